"""LinkFailureSweep over what-if scenarios of any size -- nodes down, nodes
drained, link groups -- against the oracle's literal answer (tests/whatif.py:
mutate the oracle's LinkState, buildRouteDb, calculateUpdate against the base,
restore). Per scenario: unicastRoutesToUpdate / unicastRoutesToDelete, the base
RouteDb with the update applied, the counts and the changed prefixes; with
full records (modes 0 and 1) also the scenario's whole RouteDb.

Each test asserts the mix of outcomes on the oracle side, so it cannot go
vacuous. A link is two-way, so a dead list always has an even length: the
first size past the eight-register list is 10 directed edges."""
import functools
import random

import pytest

import lsdb as L
import test_gpu_rebuild_routes as T
import whatif as W

pytestmark = pytest.mark.gpu

A = L.kTestingAreaName
ME = "12"


class GridWorld(W.World):
    """test_gpu_rebuild_routes' 5x5 grid and its 2,503 prefixes (100 a node
    + the anycast extras)."""

    def __init__(self, grid):
        super().__init__([grid.adjdb(n) for n in range(T.N * T.N)], [], A)

    def load(self, M, me):
        als, ls, _ = super().load(M, me)
        return als, ls, T._prefixes(M, 100, A)


def grid_world(seeded=False, zero_link=False):
    g = T.Grid()
    if seeded:
        rng = random.Random(0x5CE)
        for node in range(T.N * T.N):
            for nb, _, _ in g.neighbours(node):
                g.metric[(node, nb)] = rng.randint(1, 9)
    if zero_link:
        g.metric[(6, 7)] = g.metric[(7, 6)] = 0
    return GridWorld(g)


def row_cut(r):
    """all 5 links between rows r and r + 1: 10 directed edges"""
    return {"links": [(str(r * T.N + c), "0/4") for c in range(T.N)]}


def grid_scenarios():
    others = [str(n) for n in range(T.N * T.N) if str(n) != ME]
    return ([{"nodesDown": [n]} for n in others] + [{"nodesDrained": [n]} for n in others] +
            [row_cut(r) for r in range(T.N - 1)] + [{}])


@functools.lru_cache(maxsize=None)
def grid_answers(oracle, seeded, brs):
    o = W.Oracle(oracle, grid_world(seeded), ME, True, brs)
    return [o.answer(sc) for sc in grid_scenarios()]


def run(sw, mode, answers, label, form=None):
    sw.setMode(mode)
    sw.launch()
    sw.fetchUpdates()
    if form is not None:
        assert sw.form() == form, (label, sw.form())
    W.check_sweep(sw, answers, label)
    if mode != 2 or sw.form() == 2:  # every record was written
        sw.fetchRecords()
        for v, (_, canon) in enumerate(answers):
            assert sw.routeDbCanonical(v) == canon, (label, v)


@pytest.mark.parametrize("seeded", [False, True], ids=["unit", "seeded"])
@pytest.mark.parametrize("brs", [False, True], ids=["plain", "brs"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_grid(product, oracle, mode, brs, seeded):
    answers = grid_answers(oracle, seeded, brs)
    kinds = [W.kind_of(u) for u, _ in answers]
    downs, drains, cuts = kinds[:24], kinds[24:48], kinds[48:52]
    assert set(downs) <= {"delete", "mixed"} and len(set(downs)) == 2
    assert set(drains) <= {"update", "mixed"}  # a drain is never empty
    assert set(cuts) == {"mixed"} and kinds[52] == "empty"
    if not seeded:
        assert (downs.count("delete"), downs.count("mixed")) == (13, 11)
        assert (drains.count("update"), drains.count("mixed")) == (15, 9)
    als, ls, ps = grid_world(seeded).load(product, ME)
    scs = grid_scenarios()
    sw = product.LinkFailureSweep(ME, ls, ps, scs, True, brs)
    assert sw.numVariants() == 53 and sw.nhWords() == 1
    # the repair (modes 1, 2) takes lists and drains. A full recompute (mode
    # 0) takes dead lists through the full frontier form; drains are not
    # built there, so a sweep that drains runs one patched topology a scenario
    run(sw, mode, answers, (mode, brs, seeded),
        product.kTopologyCopies if mode == 0 else product.kEdgeBitset)
    if mode == 0:
        lists = [i for i, sc in enumerate(scs) if "nodesDrained" not in sc]
        sw = product.LinkFailureSweep(ME, ls, ps, [scs[i] for i in lists], True, brs)
        run(sw, 0, [answers[i] for i in lists], (mode, brs, seeded, "lists"),
            product.kEdgeBitset)


# ---- hub and ring -----------------------------------------------------------
def hub_ring_world(ring=12, parallel=True, prefixes=3):
    rng = random.Random(0xB0B)
    adjs = {f"r{i}": [] for i in range(ring)}
    adjs["hub"] = []
    idx = {n: i + 1 for i, n in enumerate(sorted(adjs))}

    def link(a, b, metric, k=0):
        for x, y in ((a, b), (b, a)):
            adjs[x].append(L.createAdjacency(y, f"{x}-{y}/{k}", f"{y}-{x}/{k}", f"fe80::{idx[y]:x}",
                                             f"192.168.0.{idx[y]}", metric, 100000 + idx[y]))

    for i in range(ring):
        link(f"r{i}", f"r{(i + 1) % ring}", rng.randint(1, 9))
        link("hub", f"r{i}", rng.randint(3, 6))
    if parallel:
        link("r3", "r4", 2, 1)
    names = sorted(adjs)
    dbs = [L.createAdjDb(n, adjs[n], 1 + names.index(n)) for n in names]
    pdbs = []
    for i, n in enumerate(names):
        ents = [L.createPrefixEntry(f"fc00:{i:x}::{k:x}/128") for k in range(prefixes)]
        if n in ("hub", "r6"):
            ents.append(L.createPrefixEntry("fd00::aa/128"))
        pdbs.append(L.createPrefixDb(n, ents))
    return W.World(dbs, pdbs, A)


HUB_GROUP = {"links": [("hub", f"hub-r{i}/0") for i in range(6)]}


def test_hub_and_ring(product, oracle):
    w = hub_ring_world()
    scs = [{"nodesDown": ["hub"]}, {"nodesDrained": ["hub"]}, HUB_GROUP,
           {"links": [("r3", "r3-r4/1")]}, {"links": [("r3", "r3-r4/1"), ("r4", "r4-r3/0")]}]
    o = W.Oracle(oracle, w, "r0")
    answers = [o.answer(sc) for sc in scs]
    down, drain = answers[0][0], answers[1][0]
    # the hub's own 3 prefixes go, the anycast stays through r6
    assert len(down["unicastRoutesToDelete"]) == 3 and down["unicastRoutesToUpdate"]
    assert not drain["unicastRoutesToDelete"] and len(drain["unicastRoutesToUpdate"]) >= 4
    als, ls, ps = w.load(product, "r0")
    dead, drained = product.expand_scenario(ls, "r0", scs[0])
    assert len(dead) == 24 and drained == []
    sw = product.LinkFailureSweep("r0", ls, ps, scs, True, False)
    for mode in (1, 2):
        run(sw, mode, answers, ("hub", mode), product.kEdgeBitset)


def test_register_and_bitset_forms(product, oracle):
    """r3 has four links (the parallel one): r3 down is exactly 8 dead
    directed edges, the register list's limit; with one more link, 10."""
    w = hub_ring_world()
    small = [{"nodesDown": ["r3"]}, {"links": [("r7", "r7-r8/0")]}, {"links": HUB_GROUP["links"][:4]}]
    big = small + [{"nodesDown": ["r3"], "links": [("r7", "r7-r8/0")]}]
    o = W.Oracle(oracle, w, "r0")
    answers = [o.answer(sc) for sc in big]
    assert any(W.kind_of(u) != "empty" for u, _ in answers)
    als, ls, ps = w.load(product, "r0")
    assert len(product.expand_scenario(ls, "r0", big[0])[0]) == 8
    assert len(product.expand_scenario(ls, "r0", big[3])[0]) == 10
    sw = product.LinkFailureSweep("r0", ls, ps, big, True, False)
    run(sw, 2, answers, "8 and 10", product.kEdgeBitset)
    sw = product.LinkFailureSweep("r0", ls, ps, small, True, False)
    for mode in (0, 1, 2):
        run(sw, mode, answers[:3], ("<= 8", mode), product.kRegisterList)
    sw.setListForm(True)
    for mode in (0, 1, 2):
        run(sw, mode, answers[:3], ("<= 8 forced", mode), product.kEdgeBitset)
    sw.setListForm(False)
    run(sw, 2, answers[:3], "<= 8 again", product.kRegisterList)


def test_wide_source(product, oracle):
    """The hub of a 40-node ring as source: next-hop sets of two words, past
    the repair. Dead lists go through the full frontier form; a sweep with a
    drain runs as topology copies."""
    w = hub_ring_world(ring=40, parallel=False, prefixes=2)
    scs = [{"links": [("hub", f"hub-r{i}/0") for i in range(3, 9)]}, {"nodesDown": ["r9"]},
           {"nodesDrained": ["r20"]}]
    o = W.Oracle(oracle, w, "hub")
    answers = [o.answer(sc) for sc in scs]
    assert all(W.kind_of(u) != "empty" for u, _ in answers)
    als, ls, ps = w.load(product, "hub")
    sw = product.LinkFailureSweep("hub", ls, ps, scs[:2], True, False)
    assert sw.nhWords() == 2
    for mode in (0, 1):
        run(sw, mode, answers[:2], ("wide lists", mode), product.kEdgeBitset)
    sw = product.LinkFailureSweep("hub", ls, ps, scs, True, False)
    run(sw, 1, answers, "wide drain", product.kTopologyCopies)


# ---- large edge set ---------------------------------------------------------
WAN = dict(nodes=2400, seed=0xC4, prefixesPerNode=1)


@functools.lru_cache(maxsize=None)
def wan_case(product, oracle):
    w = W.generated_world(product, "wan", WAN)
    rng = random.Random(0x1A6E)
    names = sorted(n for n in w.adjdbs if n != "0" and w.adjdbs[n]["adjacencies"])
    picks = rng.sample(names, 48)
    links = [(n, a["ifName"]) for n in names for a in w.adjdbs[n]["adjacencies"]]
    scs = ([{"nodesDown": [n]} for n in picks[:24]] + [{"nodesDrained": [n]} for n in picks[24:]] +
           [{"links": rng.sample(links, 12)} for _ in range(8)])
    o = W.Oracle(oracle, w, "0")
    return w, scs, [o.answer(sc) for sc in scs]


@pytest.mark.parametrize("desc", [1, 0])
@pytest.mark.parametrize("mode", [1, 2])
def test_large_edge_set(product, oracle, mode, desc):
    """More than 8,192 directed edges: the bitset's zeroing and fill take
    more than one pass of the workgroup's 256 threads x 32 edges."""
    import openr_amd.capi as capi
    w, scs, answers = wan_case(product, oracle)
    assert w.directed_edges() > 8192
    kinds = [W.kind_of(u) for u, _ in answers]
    assert "empty" not in kinds[:24] and sum(k != "empty" for k in kinds[24:48]) >= 12
    assert sum(k != "empty" for k in kinds[48:]) >= 4
    als, ls, ps = w.load(product, "0")
    with capi.scoped_options(capi.load(), c4_desc=desc):
        sw = product.LinkFailureSweep("0", ls, ps, scs, True, False)
        run(sw, mode, answers, ("wan", mode, desc), product.kEdgeBitset)


def test_large_edge_set_full_form(product, oracle):
    """The same lists (no drains) through the full frontier form, whose
    workgroups each fill the bitset in more than one pass."""
    w, scs, answers = wan_case(product, oracle)
    lists = list(range(24)) + list(range(48, 56))
    als, ls, ps = w.load(product, "0")
    sw = product.LinkFailureSweep("0", ls, ps, [scs[i] for i in lists], True, False)
    run(sw, 0, [answers[i] for i in lists], "wan full", product.kEdgeBitset)


def test_setters_drop_fetched_results(product, oracle):
    """setMode / setListForm select the form again: what a launch of another
    form left fetched must not be read through the new one."""
    answers = grid_answers(oracle, False, False)
    als, ls, ps = grid_world(False).load(product, ME)
    sw = product.LinkFailureSweep(ME, ls, ps, grid_scenarios(), True, False)
    run(sw, 0, answers, "copies", product.kTopologyCopies)
    sw.setMode(1)
    assert sw.form() == product.kEdgeBitset
    for read in (lambda: sw.routeUpdate(0), lambda: sw.changedPrefixes(0), lambda: sw.counts(0)):
        with pytest.raises((IndexError, RuntimeError)):
            read()
    run(sw, 1, answers, "after copies", product.kEdgeBitset)
    sw.setMode(0)
    with pytest.raises((IndexError, RuntimeError)):
        sw.routeUpdate(0)
    run(sw, 0, answers, "copies again", product.kTopologyCopies)


# ---- exact domain, relaunch, empty sweep --------------------------------------
def test_exact_domain(product, oracle):
    """One zero-metric link: every scenario as a patched topology copy."""
    w = grid_world(zero_link=True)
    scs = [{"nodesDown": ["7"]}, {"nodesDrained": ["7"]}, {"nodesDrained": ["6", "13"]}, row_cut(1),
           {"nodesDown": ["11"], "nodesDrained": ["13"], "links": [("12", "0/2")]}, {}]
    o = W.Oracle(oracle, w, ME)
    answers = [o.answer(sc) for sc in scs]
    assert [W.kind_of(u) for u, _ in answers][5] == "empty"
    assert sum(W.kind_of(u) == "mixed" for u, _ in answers) >= 2
    als, ls, ps = w.load(product, ME)
    sw = product.LinkFailureSweep(ME, ls, ps, scs, True, False)
    run(sw, 2, answers, "exact", product.kTopologyCopies)


def test_second_launch_and_empty_sweep(product, oracle):
    """Two launches on one sweep (the descendant rows reused), and a sweep of
    no scenarios."""
    answers = grid_answers(oracle, True, False)
    als, ls, ps = grid_world(True).load(product, ME)
    sw = product.LinkFailureSweep(ME, ls, ps, grid_scenarios(), True, False)
    run(sw, 2, answers, "first", product.kEdgeBitset)
    run(sw, 2, answers, "second", product.kEdgeBitset)
    run(sw, 1, answers, "third", product.kEdgeBitset)
    empty = product.LinkFailureSweep(ME, ls, ps, [], True, False)
    empty.launch()
    empty.fetchUpdates()
    assert empty.numVariants() == 0 and empty.totalChanges() == 0
