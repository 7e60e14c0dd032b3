"""LinkFailureSweep with enableNodeSegmentLabel: the node-label MPLS half of
every scenario's update against the oracle's literal answer
(tests/whatif_labels.py: the oracle's solver with node segment labels on;
mutate, buildRouteDb, calculateUpdate against the base, restore). Per scenario:
mplsRoutesToUpdate, mplsRoutesToDelete, the base RouteDb with the update
applied, mplsCounts and changedLabels, and the unicast half unchanged
(whatif.check_sweep); with full records also the scenario's whole RouteDb.

The worlds are those of the restore tests with labels that exercise every rule
of SpfSolver.cpp:352-445: an unset label, one with a top-12 bit, a duplicate
between two nodes, one shared with the source. The mix of outcomes is asserted
on the oracle's side, so the selection cannot go vacuous.

A unit refused on the device (a 2^31 override) never comes out of a sweep --
the constructor sends such a weight to topology copies -- so that rule is
checked on the raw entry in tests/test_gpu_spf_node_diff.py."""
import functools
import random

import pytest

import test_gpu_scenarios as S
import test_gpu_whatif_restore as TR
import whatif as W
import whatif_labels as WL
import whatif_restore as WR

pytestmark = pytest.mark.gpu

ME = TR.ME  # "12", the centre of the 5x5 grid
INVALID_TOP = (1 << 20) | 9  # a top-12 bit set: no route (SpfSolver.cpp:360-368)
DUP, DUP_OWNERS = 500, ("6", "8")  # "6" < "8": 6 holds it while it has a route
SHARED = 112  # the source's, also node 10's: "10" < "12" holds it while it has a route


def label_grid(world):
    """label 100 + n on node n of the grid world, except: node 3 none, node 9 an
    invalid one, 6 and 8 the same, 10 the source's"""
    for n, d in world.adjdbs.items():
        d["nodeLabel"] = 100 + int(n)
    world.adjdbs["3"]["nodeLabel"] = 0
    world.adjdbs["9"]["nodeLabel"] = INVALID_TOP
    for n in DUP_OWNERS:
        world.adjdbs[n]["nodeLabel"] = DUP
    world.adjdbs["10"]["nodeLabel"] = SHARED
    assert world.adjdbs[ME]["nodeLabel"] == SHARED
    return world


def grid_world(seeded, zero_link=False):
    return label_grid(TR.grid_world(seeded, zero_link))


def grid_scenarios(seeded):
    """one of every kind on the restore tests' drained grid"""
    m = {(n, i): x for n, i, x in TR.TM.adjacencies(TR.grid_world(seeded))}
    up = max(m[TR.link_up(12, 13)], m[TR.link_up(13, 12)])
    return [
        {"links": [TR.link_up(12, 13)]},
        {"nodesDown": ["13"]},
        {"nodesDrained": ["8"]},
        {"linkMetrics": [TR.link_up(12, 13) + (4 * up,), TR.link_up(13, 12) + (4 * up,)]},
        # 11 is soft-drained by 50 at baseline: its link to the source, lowered
        {"linkMetrics": [TR.link_up(11, 12) + (1,), TR.link_up(12, 11) + (1,)]},
        {"nodesSoftDrained": [("13", 50)]},
        {"nodesUndrained": ["7"]},
        {"linksUndrained": [TR.link_up(6, 11)]},
        {"nodesSoftUndrained": ["11"]},
        {"nodesDown": [DUP_OWNERS[0]]},  # the other owner takes the label
        {"nodesDown": ["10"]},           # the source's POP_AND_LOOKUP takes it
        {"nodesUndrained": ["3"]},       # 3 is not drained: changes nothing
        {},
    ]


DOWN_DUP, DOWN_SHARED, NOTHING = 9, 10, (11, 12)


@functools.lru_cache(maxsize=None)
def grid_answers(oracle, seeded, brs):
    o = WL.LabelOracle(oracle, grid_world(seeded), ME, True, brs)
    return [o.answer(sc) for sc in grid_scenarios(seeded)]


def check_grid_pattern(answers):
    kinds = [WL.mpls_kind(u) for u, _ in answers]
    assert sum(k != "empty" for k in kinds) * 2 >= len(kinds), kinds
    assert any(k in ("delete", "mixed") for k in kinds), kinds
    assert all(kinds[i] == "empty" for i in NOTHING), kinds
    # the duplicate passes to its other owner, the shared one to the source
    upd = answers[DOWN_DUP][0]
    assert DUP in upd["mplsRoutesToUpdate"] and DUP not in upd["mplsRoutesToDelete"]
    upd = answers[DOWN_SHARED][0]
    assert SHARED in upd["mplsRoutesToUpdate"] and SHARED not in upd["mplsRoutesToDelete"]
    # no scenario ever reports the unset or the invalid label
    for u, _ in answers:
        assert not {0, INVALID_TOP} & (set(u["mplsRoutesToUpdate"]) | set(u["mplsRoutesToDelete"]))


def run(sw, mode, answers, label, form=None):
    """S.run with the label half: launch, fetch, compare; the whole RouteDbs
    when the launch wrote every record"""
    sw.setMode(mode)
    sw.launch()
    sw.fetchUpdates()
    if form is not None:
        assert sw.form() == form, (label, sw.form())
    WL.check_labels(sw, answers, label)
    if mode != 2 or sw.form() == 2:
        sw.fetchRecords()
        for v, (want, canon) in enumerate(answers):
            assert sw.routeDbCanonical(v) == canon, (label, v)
            n = (len(want["mplsRoutesToUpdate"]), len(want["mplsRoutesToDelete"]))
            assert tuple(sw.mplsCounts(v)) == n, (label, v, "after fetchRecords")


def labelled(product, ls, ps, scs, brs=False, me=ME):
    return product.LinkFailureSweep(me, ls, ps, scs, True, brs, enableNodeSegmentLabel=True)


@pytest.mark.parametrize("seeded", [False, True], ids=["unit", "seeded"])
@pytest.mark.parametrize("brs", [False, True], ids=["plain", "brs"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_grid(product, oracle, mode, brs, seeded):
    """natural form (the what-if entry's repair; topology copies in mode 0,
    where node bits are not built), the bitset form forced, the global form"""
    answers = grid_answers(oracle, seeded, brs)
    check_grid_pattern(answers)
    scs = grid_scenarios(seeded)
    als, ls, ps = grid_world(seeded).load(product, ME)
    sw = labelled(product, ls, ps, scs, brs)
    assert sw.numVariants() == len(scs) and sw.nhWords() == 1
    label = (mode, brs, seeded)
    run(sw, mode, answers, label + ("natural",),
        product.kTopologyCopies if mode == 0 else product.kEdgeBitset)
    sw.setListForm(True)
    run(sw, mode, answers, label + ("list",))
    sw.setListForm(False)
    sw.setGlobalForm(True)
    run(sw, mode, answers, label + ("global",), product.kGlobalState)


def test_register_list_form(product, oracle):
    """link failures only: ogs_spf_routes_variants writes the rows"""
    answers = grid_answers(oracle, True, False)
    scs = grid_scenarios(True)
    pick = [0, 12]
    more = [{"links": [TR.link_up(13, 14)]}, {"links": [TR.link_up(12, 11), TR.link_up(12, 17)]}]
    o = WL.LabelOracle(oracle, grid_world(True), ME)
    answers = [answers[i] for i in pick] + [o.answer(sc) for sc in more]
    assert sum(WL.mpls_kind(u) != "empty" for u, _ in answers) >= 2
    als, ls, ps = grid_world(True).load(product, ME)
    sw = labelled(product, ls, ps, [scs[i] for i in pick] + more)
    for mode in (0, 1, 2):
        run(sw, mode, answers, ("register", mode), product.kRegisterList)


def test_option_off_is_the_sweep_as_it_was(product, oracle):
    """the default and enableNodeSegmentLabel=False: same form and flags, empty
    MPLS halves, the label-free oracle's answers"""
    scs = grid_scenarios(True)
    o = W.Oracle(oracle, grid_world(True), ME)
    answers = [o.answer(sc) for sc in scs]
    als, ls, ps = grid_world(True).load(product, ME)
    plain = product.LinkFailureSweep(ME, ls, ps, scs, True, False)
    off = product.LinkFailureSweep(ME, ls, ps, scs, True, False, enableNodeSegmentLabel=False)
    on = labelled(product, ls, ps, scs)
    assert (plain.form(), plain.flags()) == (off.form(), off.flags()) == (on.form(), on.flags())
    S.run(off, 1, answers, "off", product.kEdgeBitset)
    for v in range(len(scs)):
        upd = off.routeUpdate(v)
        assert upd["mplsRoutesToUpdate"] == {} and upd["mplsRoutesToDelete"] == []
        assert tuple(off.mplsCounts(v)) == (0, 0) and off.changedLabels(v) == []


def test_wide_source(product, oracle):
    """the hub of a 40-node ring: next-hop sets of two words"""
    w = S.hub_ring_world(ring=40, parallel=False, prefixes=2)
    scs = [{"links": [("hub", "hub-r5/0")]}, {"links": [("r3", "r3-r4/0")]}, S.HUB_GROUP,
           {"nodesDown": ["r7"]}, {}]
    o = WL.LabelOracle(oracle, w, "hub")
    answers = [o.answer(sc) for sc in scs]
    kinds = [WL.mpls_kind(u) for u, _ in answers]
    assert kinds[3] in ("delete", "mixed") and kinds[4] == "empty", kinds
    assert sum(k != "empty" for k in kinds) >= 3, kinds
    als, ls, ps = w.load(product, "hub")
    sw = labelled(product, ls, ps, scs, me="hub")
    assert sw.nhWords() == 2
    for mode in (0, 1):
        run(sw, mode, answers, ("wide", mode), product.kEdgeBitset)
    for mode in (0, 1):
        sw.setGlobalForm(True)
        run(sw, mode, answers, ("wide global", mode), product.kGlobalState)


def test_exact_domain(product, oracle):
    """a zero-metric link: topology copies, each copy's labels from its own rows"""
    w = grid_world(False, zero_link=True)
    scs = [{"nodesUndrained": ["7"]}, {"linksUndrained": [TR.link_up(6, 11)]},
           {"nodesDown": [DUP_OWNERS[0]]}, {"nodesDown": ["13"]}, {}]
    o = WL.LabelOracle(oracle, w, ME)
    answers = [o.answer(sc) for sc in scs]
    kinds = [WL.mpls_kind(u) for u, _ in answers]
    assert all(k != "empty" for k in kinds[:4]) and kinds[3] in ("delete", "mixed"), kinds
    als, ls, ps = w.load(product, ME)
    sw = labelled(product, ls, ps, scs)
    assert sw.form() == product.kTopologyCopies
    run(sw, 1, answers, "exact", product.kTopologyCopies)


@functools.lru_cache(maxsize=None)
def wan_case(product, oracle):
    """the restore tests' 2,400-node WAN and drained baseline, label 100000 + id
    on every node, its first 8 scenarios (scenario 0 undrains 60 nodes at once)"""
    w = WR.as_restore_world(W.generated_world(product, "wan", S.WAN))
    rng = random.Random(TR.WAN_SEED)
    hard, over, softs = WR.drain_baseline(w, rng, "0")
    scs = TR.restoring_scenarios(w, rng, hard, over, softs, "0", 40)[:8]
    for n, d in w.adjdbs.items():
        d["nodeLabel"] = 100000 + int(n)
    o = WL.LabelOracle(oracle, w, "0")
    return w, scs, [o.answer(sc) for sc in scs]


@pytest.mark.parametrize("mode", [1, 2])
def test_natural_size(product, oracle, mode):
    w, scs, answers = wan_case(product, oracle)
    kinds = [WL.mpls_kind(u) for u, _ in answers]
    assert sum(k != "empty" for k in kinds) >= 4, kinds
    als, ls, ps = w.load(product, "0")
    sw = labelled(product, ls, ps, scs, me="0")
    run(sw, mode, answers, ("wan", mode), product.kEdgeBitset)
