"""LinkFailureSweep over the restoring scenario kinds -- linksUndrained,
nodesUndrained, nodesSoftUndrained -- alone and mixed with the kinds that take
things away, against the oracle's literal answer (tests/whatif_restore.py:
re-send the adjacency or the database with the overload bit off, or with
nodeMetricIncrementVal = 0 and lowered metrics; buildRouteDb; calculateUpdate
against the base; restore). Per scenario: unicastRoutesToUpdate /
unicastRoutesToDelete, the base RouteDb with the update applied, the counts and
the changed prefixes (whatif.check_sweep); with full records (modes 0 and 1)
also the scenario's whole RouteDb.

Every test aimed at the kernels asserts the form after the launch, so a
fall-back to topology copies cannot pass for them, and the mix of outcomes on
the oracle side, so it cannot go vacuous. The raw-ABI tests drive
ogs_spf_routes_whatif and ogs_spf_routes_whatif_global with torch-owned
buffers; their round trip needs no oracle: a graph with links marked down and
nodes overloaded, and one unit that revives and clears all of them, must give
the bytes ogs_spf_routes gives on the graph without the marks."""
import copy
import ctypes
import functools
import random

import pytest

import lsdb as L
import test_gpu_rebuild_routes as T
import test_gpu_scenarios as S
import test_gpu_whatif_global as TG
import test_gpu_whatif_metric as TM
import whatif as W
import whatif_restore as WR

pytestmark = pytest.mark.gpu

A = L.kTestingAreaName
ME = "12"

# ---- the 5x5 grid with a drained baseline -----------------------------------
NODE_OVER = (7, 17, 12)
ADJ_OVER = ((2, 3), (6, 11), (8, 13), (16, 21), (13, 18), (18, 13))
SOFT = {11: 50, 23: 50}


class GridWorld(WR.RestoreWorld):
    """test_gpu_whatif_metric's grid world (20 prefixes a node) over a RestoreWorld"""

    def __init__(self, grid):
        super().__init__([grid.adjdb(n) for n in range(T.N * T.N)], [], A)

    def load(self, M, me):
        als, ls, _ = W.World.load(self, M, me)
        return als, ls, T._prefixes(M, TM.PER_NODE, A)


def ifname(node, nb):
    return next(i for n, i, _ in T.Grid().neighbours(node) if n == nb)


def grid_world(seeded, zero_link=False):
    g = T.Grid()
    if seeded:  # test_gpu_scenarios' seeded metrics
        rng = random.Random(0x5CE)
        for node in range(T.N * T.N):
            for nb, _, _ in g.neighbours(node):
                g.metric[(node, nb)] = rng.randint(1, 9)
    if zero_link:
        g.metric[(0, 1)] = g.metric[(1, 0)] = 0
    g.node_over, g.adj_over = set(NODE_OVER), set(ADJ_OVER)
    for node, inc in SOFT.items():
        for nb, _, _ in g.neighbours(node):
            g.metric[(node, nb)] = g.metric.get((node, nb), 1) + inc
    w = GridWorld(g)
    for node, inc in SOFT.items():
        w.adjdbs[str(node)]["nodeMetricIncrementVal"] = inc
    return w


def link_up(a, b):
    return (str(a), ifname(a, b))


SINGLES = (
    [{"nodesUndrained": ["7"]}, {"nodesUndrained": ["17"]}, {"nodesUndrained": ["12"]},
     {"nodesUndrained": ["3"]}, {"nodesUndrained": ["7", "17"]}] +
    [{"linksUndrained": [link_up(a, b)]} for a, b in sorted(ADJ_OVER)] +
    [{"linksUndrained": [link_up(13, 18), link_up(18, 13)]}] +
    [{"nodesSoftUndrained": ["11"]}, {"nodesSoftUndrained": ["23"]},
     {"nodesSoftUndrained": ["0"]}])
# (updates, deletions) of SINGLES on unit metrics, plain selection: the oracle
# alone, on the CPU
UNIT_COUNTS = [(308, 2), (308, 2), (0, 1), (0, 0), (407, 1),
               (210, 2), (57, 1), (38, 0), (0, 0), (38, 2), (0, 0),
               (77, 2), (230, 2), (229, 2), (0, 0)]
EMPTY = {3, 8, 10, 14}  # on unit and on seeded metrics
MIXES = [
    {"nodesUndrained": ["7"], "nodesDrained": ["8"], "links": [link_up(12, 11)]},
    {"linksUndrained": [link_up(6, 11)],
     "linkMetrics": [link_up(6, 11) + (7,), link_up(11, 6) + (7,)]},
    {"nodesSoftUndrained": ["11"], "nodesSoftDrained": [("13", 30)], "nodesDown": ["7"]},
    {"nodesUndrained": ["17"], "linksUndrained": [link_up(16, 21)], "nodesSoftUndrained": ["23"]},
]
GRID = SINGLES + MIXES
# the scenarios without a cleared node bit: what a full recompute (mode 0) takes
# through the full frontier form
LINK_ONLY = [i for i, sc in enumerate(GRID)
             if not ("nodesUndrained" in sc or "nodesSoftUndrained" in sc or
                     "nodesDrained" in sc or "nodesSoftDrained" in sc)]


@functools.lru_cache(maxsize=None)
def grid_answers(oracle, seeded, brs):
    o = W.Oracle(oracle, grid_world(seeded), ME, True, brs)
    return [o.answer(sc) for sc in GRID]


def check_grid_pattern(answers, seeded, brs):
    n = [(len(u["unicastRoutesToUpdate"]), len(u["unicastRoutesToDelete"])) for u, _ in answers]
    singles = n[:len(SINGLES)]
    assert {i for i, c in enumerate(singles) if c == (0, 0)} == EMPTY, singles
    assert singles[2][0] == 0 and singles[2][1] >= 1  # the source undrained: SPF as it was
    assert all(c != (0, 0) for c in n[len(SINGLES):]), n[len(SINGLES):]
    if not seeded and not brs:
        assert singles == UNIT_COUNTS, singles


@pytest.mark.parametrize("seeded", [False, True], ids=["unit", "seeded"])
@pytest.mark.parametrize("brs", [False, True], ids=["plain", "brs"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_grid(product, oracle, mode, brs, seeded):
    answers = grid_answers(oracle, seeded, brs)
    check_grid_pattern(answers, seeded, brs)
    als, ls, ps = grid_world(seeded).load(product, ME)
    label = (mode, brs, seeded)
    assert len(LINK_ONLY) == 8
    if mode == 0:
        # link revivals ride in the metric slice: the full frontier form takes
        # them; cleared bits are node bits, which it does not build
        sw = product.LinkFailureSweep(ME, ls, ps, [GRID[i] for i in LINK_ONLY], True, brs)
        S.run(sw, 0, [answers[i] for i in LINK_ONLY], label + ("links",), product.kEdgeBitset)
        clears = [i for i in range(len(GRID)) if i not in LINK_ONLY]
        sw = product.LinkFailureSweep(ME, ls, ps, [GRID[i] for i in clears], True, brs)
        S.run(sw, 0, [answers[i] for i in clears], label + ("clears",), product.kTopologyCopies)
    else:
        sw = product.LinkFailureSweep(ME, ls, ps, GRID, True, brs)
        assert sw.numVariants() == 19 and sw.nhWords() == 1
        S.run(sw, mode, answers, label, product.kEdgeBitset)


@pytest.mark.parametrize("seeded", [False, True], ids=["unit", "seeded"])
@pytest.mark.parametrize("brs", [False, True], ids=["plain", "brs"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_grid_forced_global(product, oracle, mode, brs, seeded):
    import openr_amd.capi as capi
    answers = grid_answers(oracle, seeded, brs)
    check_grid_pattern(answers, seeded, brs)
    als, ls, ps = grid_world(seeded).load(product, ME)
    sw = product.LinkFailureSweep(ME, ls, ps, GRID, True, brs)
    assert sw.form() == product.kEdgeBitset
    for k in TG.STATE_FORMS:
        with capi.scoped_options(capi.load(), spf_global_lds=k):
            TG.run_global(product, sw, mode, answers, ("grid", mode, brs, seeded, k))


def test_a_sweep_without_restorations_keeps_its_entry(product, oracle):
    """no-op restorations fold away: the sweep is the register-list sweep it
    would be without them"""
    als, ls, ps = grid_world(False).load(product, ME)
    scs = [{"links": [("13", "0/1")], "nodesUndrained": ["3"], "nodesSoftUndrained": ["0"],
            "linksUndrained": [("12", "0/1")]}]
    sw = product.LinkFailureSweep(ME, ls, ps, scs, True, False)
    assert sw.form() == product.kRegisterList
    o = W.Oracle(oracle, grid_world(False), ME)
    S.run(sw, 2, [o.answer(scs[0])], "folded", product.kRegisterList)


# ---- hub and ring: a source with next-hop sets of two words --------------------
def wide_world():
    w = WR.as_restore_world(S.hub_ring_world(ring=40, parallel=False, prefixes=2))

    def over(node, ifn):
        next(a for a in w.adjdbs[node]["adjacencies"] if a["ifName"] == ifn)["isOverloaded"] = True

    over("hub", "hub-r5/0")
    over("r9", "r9-hub/0")
    over("hub", "hub-r14/0")
    over("r14", "r14-hub/0")
    over("r30", "r30-r31/0")
    w.adjdbs["r20"]["isOverloaded"] = True
    return w


def test_wide_source(product, oracle):
    """The hub of a 40-node ring as source, some spokes overloaded at baseline:
    link revivals go through the full frontier form in modes 0 and 1 (the
    repair stops at one next-hop word); a node undrain runs as topology copies;
    both run in the global form."""
    w = wide_world()
    links = [{"linksUndrained": [("hub", "hub-r5/0")]}, {"linksUndrained": [("r9", "r9-hub/0")]},
             {"linksUndrained": [("hub", "hub-r14/0"), ("r14", "r14-hub/0")]},
             {"linksUndrained": [("hub", "hub-r14/0")]},
             {"linksUndrained": [("r30", "r30-r31/0")],
              "linkMetrics": [("r30", "r30-r31/0", 1), ("r31", "r31-r30/0", 1)]},
             {"linksUndrained": [("hub", "hub-r5/0"), ("r9", "r9-hub/0")],
              "links": [("hub", "hub-r6/0")]}]
    scs = links + [{"nodesUndrained": ["r20"]}]
    o = W.Oracle(oracle, w, "hub")
    answers = [o.answer(sc) for sc in scs]
    kinds = [W.kind_of(u) for u, _ in answers]
    # r9's spoke comes up and is on no shortest path; hub - r14 stays down
    assert [i for i, k in enumerate(kinds) if k == "empty"] == [1, 3], kinds
    als, ls, ps = w.load(product, "hub")
    sw = product.LinkFailureSweep("hub", ls, ps, links, True, False)
    assert sw.nhWords() == 2
    for mode in (0, 1):
        S.run(sw, mode, answers[:6], ("wide links", mode), product.kEdgeBitset)
    for mode in (0, 1):
        TG.run_global(product, sw, mode, answers[:6], ("wide links global", mode))
    sw = product.LinkFailureSweep("hub", ls, ps, scs, True, False)
    S.run(sw, 1, answers, "wide undrain", product.kTopologyCopies)
    for mode in (0, 1):
        TG.run_global(product, sw, mode, answers, ("wide undrain global", mode))


# ---- large edge set ---------------------------------------------------------
WAN_SEED = 0x2E57


def restoring_scenarios(w, rng, hard, over, softs, me, count, group=60):
    """`count` scenarios over a drained baseline: scenario 0 undrains `group`
    nodes, brings every overloaded adjacency back and soft-undrains every
    soft-drained node; then single undrains, link revivals, soft-undrains and
    mixes with the kinds that take away"""
    adjs = [x for x in TM.adjacencies(w) if x[0] != me]
    names = sorted(n for n in w.adjdbs if n != me and w.adjdbs[n]["adjacencies"])
    scs = [{"nodesUndrained": rng.sample(hard, min(group, len(hard))), "linksUndrained": list(over),
            "nodesSoftUndrained": list(softs)}]
    k = (count - 1) // 4
    scs += [{"nodesUndrained": [n]} for n in rng.sample(hard, k)]
    scs += [{"linksUndrained": rng.sample(over, 4)} for _ in range(k)]
    scs += [{"nodesSoftUndrained": [n]} for n in rng.sample(softs, k)]
    while len(scs) < count:
        scs.append({"nodesUndrained": rng.sample(hard, 2), "linksUndrained": rng.sample(over, 3),
                    "links": [x[:2] for x in rng.sample(adjs, 3)],
                    "linkMetrics": [(n, i, 8 * m) for n, i, m in rng.sample(adjs, 3)],
                    "nodesDrained": [rng.choice([n for n in names if n not in hard])]})
    return scs


@functools.lru_cache(maxsize=None)
def wan_case(product, oracle):
    """40 restoring scenarios on test_gpu_scenarios' 2,400-node WAN with about
    5 % of the nodes hard-drained, 3 % of the adjacencies overloaded at one end
    and 30 nodes soft-drained (seed WAN_SEED = 0x2E57: the oracle alone finds at
    least half of the scenarios non-empty). Scenario 0 undrains 60 nodes at once
    and brings every overloaded adjacency back: its metric slice runs past 256
    entries."""
    w = WR.as_restore_world(W.generated_world(product, "wan", S.WAN))
    rng = random.Random(WAN_SEED)
    hard, over, softs = WR.drain_baseline(w, rng, "0")
    scs = restoring_scenarios(w, rng, hard, over, softs, "0", 40)
    assert len(scs) == 40 and len(scs[0]["nodesUndrained"]) == 60
    o = W.Oracle(oracle, w, "0")
    return w, scs, [o.answer(sc) for sc in scs]


@pytest.mark.parametrize("desc", [1, 0])
@pytest.mark.parametrize("mode", [1, 2])
def test_large_edge_set(product, oracle, mode, desc):
    import openr_amd.capi as capi
    w, scs, answers = wan_case(product, oracle)
    assert w.directed_edges() > 8192
    kinds = [W.kind_of(u) for u, _ in answers]
    assert sum(k != "empty" for k in kinds) >= 20, kinds
    als, ls, ps = w.load(product, "0")
    x = product.expand_whatif(ls, "0", scs[0])
    assert len(x["revivedEdges"]) + len(x["metricEdges"]) > 256 and len(x["cleared"]) == 90
    with capi.scoped_options(capi.load(), c4_desc=desc):
        sw = product.LinkFailureSweep("0", ls, ps, scs, True, False)
        S.run(sw, mode, answers, ("wan", mode, desc), product.kEdgeBitset)


# ---- natural size: past the LDS forms' limit ------------------------------------
@functools.lru_cache(maxsize=None)
def wan17k_case(product, oracle):
    """test_gpu_whatif_global's 17,000-node WAN with the baseline drains of the
    2,400-node case and 8 restoring scenarios near the source; prefix databases
    of 1,000 nodes, as there."""
    w = WR.as_restore_world(W.generated_world(product, "wan", TG.WAN17K))
    rng = random.Random(0x17001)
    nbrs = lambda n: [a["otherNodeName"] for a in w.adjdbs[n]["adjacencies"]]  # noqa: E731
    first = nbrs("0")
    second = sorted({m for n in first for m in nbrs(n)} - {"0"} - set(first))
    assert len(first) >= 3 and len(second) >= 3
    near = {"0"}  # the source's neighbourhood: whole hops until it holds 40 nodes
    while len(near) < 41:
        near |= {m for n in near for m in nbrs(n)}
    near = sorted(near - {"0"} - set(first) - set(second))
    # (the first two hops' own drains are the ones below)
    hard, over, softs = WR.drain_baseline(w, rng, "0", spare=first + second)
    # drains where the source's routes run: one of its neighbours and a node two
    # hops out hard-drained, its link to another neighbour and a link to the
    # second hop overloaded, another second-hop node soft-drained
    near_hard = [first[1], second[0]] + rng.sample([n for n in near if n not in softs], 4)
    for n in near_hard:
        w.adjdbs[n]["isOverloaded"] = True

    def adjacency(a, b):
        return next(x for x in w.adjdbs[a]["adjacencies"] if x["otherNodeName"] == b)

    ends = [("0", first[2]), (first[0], next(m for m in nbrs(first[0]) if m in second[1:]))]
    ends += [(n, nbrs(n)[0]) for n in rng.sample([n for n in near if n not in near_hard], 4)]
    near_over = []
    for a, b in ends:
        adjacency(a, b)["isOverloaded"] = True
        near_over.append((a, adjacency(a, b)["ifName"]))
    near_soft = [second[-1]] + [n for n in near if n not in near_hard and n not in softs][:1]
    for n in near_soft:
        w.adjdbs[n]["nodeMetricIncrementVal"] = 40
        for a in w.adjdbs[n]["adjacencies"]:
            a["metric"] += 40
    scs = ([{"nodesUndrained": [n]} for n in near_hard[:2]] + [{"nodesUndrained": near_hard}] +
           [{"linksUndrained": [x]} for x in near_over[:2]] +
           [{"nodesSoftUndrained": [near_soft[0]]},
            {"nodesUndrained": near_hard[2:4], "linksUndrained": near_over[2:],
             "nodesSoftUndrained": near_soft, "nodesDrained": [near_hard[0]]},
            {"nodesUndrained": rng.sample(hard, 60), "linksUndrained": rng.sample(over, 100)}])
    assert len(scs) == 8
    touched = set(near) | set(first) | set(second) | set(near_hard) | {n for n, _ in near_over} | set(near_soft)
    behind = {m for n in touched for m in nbrs(n)}
    keep = (["0"] + sorted((touched | behind) - {"0"}))[:900]
    keep += rng.sample(sorted(set(w.adjdbs) - set(keep)), 1000 - len(keep))
    keep = set(keep)
    w.prefix_dbs = [d for d in w.prefix_dbs if d["thisNodeName"] in keep]
    o = W.Oracle(oracle, w, "0")
    return w, scs, [o.answer(sc) for sc in scs]


@pytest.mark.parametrize("mode", [1, 2])
def test_natural_size(product, oracle, mode):
    w, scs, answers = wan17k_case(product, oracle)
    kinds = [W.kind_of(u) for u, _ in answers]
    assert sum(k != "empty" for k in kinds) >= 6, kinds
    als, ls, ps = w.load(product, "0")
    sw = product.LinkFailureSweep("0", ls, ps, scs, True, False)
    assert sw.nhWords() == 1 and sw.form() == product.kGlobalState
    TG.run_global(product, sw, mode, answers, ("17k restore", mode), forced=False)


# ---- the exact domain ----------------------------------------------------------
def test_exact_domain(product, oracle):
    """A zero-metric link in the grid: one scenario of each new kind runs as
    topology copies and equals the oracle. So does a revived link whose own
    weight is past the 32-bit path-sum guard."""
    wz = grid_world(False, zero_link=True)
    scs = [{"nodesUndrained": ["7"]}, {"linksUndrained": [link_up(6, 11)]},
           {"nodesSoftUndrained": ["11"]}]
    oz = W.Oracle(oracle, wz, ME)
    answers = [oz.answer(sc) for sc in scs]
    assert all(W.kind_of(u) != "empty" for u, _ in answers)
    als, ls, ps = wz.load(product, ME)
    sw = product.LinkFailureSweep(ME, ls, ps, scs, True, False)
    assert sw.form() == product.kTopologyCopies
    S.run(sw, 1, answers, "exact topology", product.kTopologyCopies)
    w = grid_world(True)
    o = W.Oracle(oracle, w, ME)
    als, ls, ps = w.load(product, ME)
    for name, metric in (("wide", 1 << 30), ("zero", 0)):
        scs = [{"linksUndrained": [link_up(6, 11)],
                "linkMetrics": [link_up(6, 11) + (metric,), link_up(11, 6) + (metric,)]},
               {"nodesUndrained": ["7"]}]
        answers = [o.answer(sc) for sc in scs]
        # (a link of weight 2^30 is on no shortest path: that update is empty)
        assert [W.kind_of(u) != "empty" for u, _ in answers] == [name == "zero", True]
        sw = product.LinkFailureSweep(ME, ls, ps, scs, True, False)
        assert sw.form() == product.kTopologyCopies
        S.run(sw, 2, answers, name, product.kTopologyCopies)


# ---- the raw ABI on the device ------------------------------------------------
INCREMENTAL, CHANGED_ONLY, HOP = TM.INCREMENTAL, TM.CHANGED_ONLY, 0x08
RESTORE, EDGE_UP, CLEAR_SHIFT = 0x100, 1 << 31, 4
EDGE_DOWN, DST_MASK, DST_OVERLOADED = 1 << 31, 0x1FFFFF, 1 << 21
RSLOT_SHIFT, RSLOT_MASK = 22, 0x1FF
WHATIF, GLOBAL = TG.WHATIF, TG.GLOBAL
FLAGS = [INCREMENTAL, INCREMENTAL | CHANGED_ONLY, 0]
FLAG_IDS = ["repair", "changed-only", "full"]


def up(v):
    """weight v with OGS_WHATIF_EDGE_UP, as the signed 32-bit value the tensors hold"""
    return (v | EDGE_UP) - 2**32


@pytest.fixture(scope="module")
def abi(product):
    return TM.Abi(product)


def weights(abi):
    return [int(x) >> 32 for x in abi.h["edges"].view("uint64")]


@pytest.mark.parametrize("entry", [WHATIF, GLOBAL])
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_abi_flag_alone_changes_nothing(abi, entry, flags):
    """OGS_F_RESTORE with no up flag and no clear nibble, EDGE_UP on edges that
    are up, a clear of a bit the node lacks, and ids past E with an up flag:
    byte for byte the call without any of them."""
    rng = random.Random(0x2E5)
    dead, nodes = TM._wan_lists(abi)
    metrics = [[], TM._overrides(abi, rng, 30, 8), TM._overrides(abi, rng, 300, 8),
               TM._overrides(abi, rng, 30, 0.001), TM._overrides(abi, rng, 5, 8), []]
    if not flags and entry == WHATIF:
        nodes = None  # node bits are not built in the LDS full form
    bits = None if nodes is None else [[TM.OVERLOADED if i % 2 == 0 else 6 for i in range(len(n))]
                                       for n in nodes]
    ref = abi.call(entry, flags, dead, nodes, bits, metrics)
    counts = ref["counts"].view(-1, 2).sum(1).tolist()
    assert sum(c > 0 for c in counts) >= 4, counts
    TM._same(abi.torch, abi.call(entry, flags | RESTORE, dead, nodes, bits, metrics), ref,
             label="flag alone")
    # every override with the up flag: the edges are up, so plain overrides
    ups = [[(e, up(v)) for e, v in m] for m in metrics]
    TM._same(abi.torch, abi.call(entry, flags | RESTORE, dead, nodes, bits, ups), ref,
             label="up on up edges")
    # ids past E carry values that would refuse the unit, or revive
    past = [m + [(abi.E, up(0)), (abi.E + 7, up(5)), (0xFFFFFFFF - 2**32, up(5))] for m in ups]
    TM._same(abi.torch, abi.call(entry, flags | RESTORE, dead, nodes, bits, past), ref,
             label="ids past E")
    if nodes is None:
        return
    # the WAN carries no node flag: clearing every bit of other nodes is no entry
    # at all for the units whose node slice was empty, and changes nothing else
    flagged = abi.h["node_flags"].view("uint8")
    assert not flagged.any()
    more = [n + [v for v in (5, 9, 11) if v not in n] for n in nodes]
    mbits = [b + [7 << CLEAR_SHIFT] * (len(m) - len(b)) for b, m in zip(bits, more)]
    TM._same(abi.torch, abi.call(entry, flags | RESTORE, dead, more, mbits, metrics), ref,
             label="clear of absent bits")


@pytest.mark.parametrize("entry", [WHATIF, GLOBAL])
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_abi_up_with_weight_zero_refuses_the_unit(abi, entry, flags):
    torch = abi.torch
    rng = random.Random(0xBAD)
    U = 4
    dead = [[] for _ in range(U)]
    good = [TM._overrides(abi, rng, 30, 8), [], TM._overrides(abi, rng, 30, 0.001),
            TM._overrides(abi, rng, 5, 8)]
    ref = abi.call(entry, flags | RESTORE, dead, metrics=good)
    bad = [list(m) for m in good]
    bad[1] = [(5, 7), (9, up(0)), (11, 3)]
    bad[3] = bad[3][:2] + [(bad[3][2][0], up(0))] + bad[3][3:]
    got = abi.call(entry, flags | RESTORE, dead, metrics=bad)
    TM._same(torch, got, ref, rows=(U, [0, 2]), label="neighbours")
    for u in (1, 3):
        assert got["counts"].view(U, 2)[u].tolist() == [-1, -1]  # OGS_WHATIF_REFUSED
        assert not got["changed"].view(U, -1)[u].any()
        for k in ("meta", "metric", "mask", "sel", "dist", "nh"):
            assert (got[k].view(U, -1)[u] == TM.FILL).all(), (u, k)
    # without the flag 2^31 | w is a weight past the domain: refused as before
    got = abi.call(entry, flags, dead, metrics=[[(5, up(7))], [], [], []])
    assert got["counts"].view(U, 2)[0].tolist() == [-1, -1]


def marked_graph(abi, rng, links, nodes, extra_flags=0):
    """Graph B: the Abi's graph A with `links` links marked OGS_EDGE_DOWN (both
    directions) and `nodes` nodes OGS_NODE_OVERLOADED with
    OGS_EDGE_DST_OVERLOADED on every edge into them; its base unit's records.
    Returns (B as an Abi, the marked directed edges ascending, the marked nodes)."""
    torch, capi = abi.torch, abi.capi
    h = abi.h
    edges = h["edges"].view("uint64").copy()
    row = h["row_ptr"].view("uint32")
    nflags = h["node_flags"].view("uint8").copy()
    s = int(h["units"].view("uint32")[1])
    marked = set()
    for e in rng.sample(range(abi.E), links):
        x = int(edges[e])
        v = x & DST_MASK
        r = int(row[v]) + ((x >> RSLOT_SHIFT) & RSLOT_MASK)
        assert int(edges[r]) & DST_MASK == int(h["edge_src"].view("uint32")[e])
        marked |= {e, r}
    for e in marked:
        edges[e] = int(edges[e]) | EDGE_DOWN
    over = rng.sample([v for v in range(abi.Sn) if v != s], nodes)
    for v in over:
        nflags[v] |= TM.OVERLOADED
    for e in range(abi.E):
        if int(edges[e]) & DST_MASK in over:
            edges[e] = int(edges[e]) | DST_OVERLOADED
    b = copy.copy(abi)
    b.t = dict(abi.t)
    b.t["edges"] = torch.from_numpy(edges.view("int64")).to(abi.dev)
    b.t["node_flags"] = torch.from_numpy(nflags).to(abi.dev)
    t = b.t
    b.g = capi.Graph(h["num_topos"], abi.Sn, abi.E, h["max_degree"], t["node_base"].data_ptr(),
                     t["row_ptr"].data_ptr(), t["edges"].data_ptr(), t["node_flags"].data_ptr(),
                     t["topo_desc"].data_ptr())
    b.g.edge_src = t["edge_src"].data_ptr()
    b.flags = abi.flags | extra_flags
    b.base = base_records(b)
    return b, sorted(marked), sorted(over)


def base_records(a, extra_flags=0):
    """ogs_spf_routes of a's base unit on a's graph"""
    out, so = a.outs(1)
    u = a.unit.view(-1).to(a.dev)
    a.capi.check(a.lib, a.lib.ogs_spf_routes(ctypes.byref(a.g), ctypes.byref(a.pt),
                                             ctypes.c_void_p(u.data_ptr()), 1,
                                             a.flags | extra_flags, 1, ctypes.byref(so), a.stream),
                 "ogs_spf_routes")
    a.torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("hop", [0, HOP], ids=["metric", "hops"])
@pytest.mark.parametrize("entry", [WHATIF, GLOBAL])
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_abi_round_trip(abi, entry, flags, hop):
    """One unit on graph B that revives every marked link and clears every
    marked node: dist, nh and the records of ogs_spf_routes on graph A. A second
    unit also lists two of the revived links dead (dead beats up): the bytes of
    a unit on B that revives the others only. The full LDS form builds no node
    bits: its B carries marked links alone."""
    torch = abi.torch
    rng = random.Random(0x707)
    with_nodes = not (entry == WHATIF and not flags)
    b, marked, over = marked_graph(abi, rng, 40, 6 if with_nodes else 0, hop)
    want = base_records(abi, hop)  # graph A
    assert not torch.equal(want["dist"], b.base["dist"])  # the marks moved shortest paths
    w = weights(abi)
    revive = [(e, up(w[e])) for e in marked]
    # the first marked link, both directions
    x = int(abi.h["edges"].view("uint64")[marked[0]])
    rev = int(abi.h["row_ptr"].view("uint32")[x & DST_MASK]) + ((x >> RSLOT_SHIFT) & RSLOT_MASK)
    killed = sorted({marked[0], rev})
    others = [(e, v) for e, v in revive if e not in killed]
    nodes = [over, over, over] if with_nodes else None
    bits = [[TM.OVERLOADED << CLEAR_SHIFT] * len(over)] * 3 if with_nodes else None
    got = b.call(entry, flags | RESTORE, [[], killed, []], nodes, bits, [revive, revive, others])
    U = 3
    changed_only = bool(flags & CHANGED_ONLY)
    for k in ("dist", "nh"):
        assert torch.equal(got[k].view(U, -1)[0], want[k]), (k, "round trip")
        assert torch.equal(got[k].view(U, -1)[1], got[k].view(U, -1)[2]), (k, "dead beats up")
    bit = lambda row, p: (int(row[p // 32]) >> (p % 32)) & 1  # noqa: E731
    ch = got["changed"].view(U, -1).cpu()
    n_changed = 0
    for k in ("meta", "metric", "mask", "sel"):
        g0, wk, bk = got[k].view(U, -1)[0].cpu(), want[k].cpu(), b.base[k].cpu()
        if not changed_only:
            assert torch.equal(g0, wk), (k, "round trip")
            continue
        for p in range(abi.Sp):  # records of the changed routes only
            if bit(ch[0], p):
                n_changed += 1
                assert g0[p] == wk[p], (k, p)
            elif k != "sel":
                assert bk[p] == wk[p], (k, p, "unchanged route differs between A and B")
    if changed_only:
        assert n_changed > 0
    assert got["counts"].view(U, 2)[0].sum() > 0
    for k in ("changed", "counts", "meta", "metric", "mask", "sel"):
        assert torch.equal(got[k].view(U, -1)[1], got[k].view(U, -1)[2]), (k, "dead beats up")
