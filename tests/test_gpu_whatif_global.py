"""LinkFailureSweep's global-state form (kGlobalState,
ogs_spf_routes_whatif_global): every scenario kind -- links down, nodes down,
hard drains, metric overrides, soft drains -- through one workgroup a scenario
on the global-state SPF with the route diff on the device, against the
oracle's literal answer (tests/whatif.py / tests/whatif_metric.py). Per
scenario: unicastRoutesToUpdate / unicastRoutesToDelete, the base RouteDb with
the update applied, the counts and the changed prefixes (whatif.check_sweep);
where records are written also the scenario's whole RouteDb.

Small areas reach the form through setGlobalForm(True), under each of the
four state forms ("spf_global_lds" 1, 3, 2, 0); a 17,000-node WAN reaches it
unforced -- the LDS forms stop at 16,384 nodes -- and is the case that throws
on a plain link-failure sweep without this form. Every test asserts the form
after the launch and the mix of outcomes on the oracle side. The raw-ABI tests
compare ogs_spf_routes_whatif_global byte for byte with ogs_spf_routes_whatif
on a topology both take."""
import functools
import random

import pytest

import test_gpu_scenarios as S
import test_gpu_whatif_metric as TM
import whatif as W
import whatif_metric as WM

pytestmark = pytest.mark.gpu

ME = S.ME
INCREMENTAL, CHANGED_ONLY = TM.INCREMENTAL, TM.CHANGED_ONLY
# "spf_global_lds": 1 one-phase packed words (W = 1; else the best two-phase
# form), 3 distances and next hops in LDS, 2 distances in LDS, 0 all in HBM
STATE_FORMS = (1, 3, 2, 0)


def run_global(product, sw, mode, answers, label, forced=True):
    """S.run under the global form: launch, fetch, compare; records when the
    mode wrote them"""
    if forced:
        sw.setGlobalForm(True)
    sw.setMode(mode)
    assert sw.form() == product.kGlobalState, label
    S.run(sw, mode, answers, label, product.kGlobalState)


# ---- the 5x5 grid (test_gpu_whatif_metric's: 20 prefixes a node, a v4 and a
# minNexthop entry among them): test_gpu_scenarios' 53 scenarios + one of each
# kind that moves a metric
def grid_extra(seeded):
    """on the source's own links: 11 - 12 cost out x4, 12 - 13 set to 1; a soft drain"""
    m = {(n, i): x for n, i, x in TM.adjacencies(TM.grid_world(seeded))}
    out4 = 4 * max(m[("11", "0/1")], m[("12", "0/3")])
    return [{"linkMetrics": [("11", "0/1", out4), ("12", "0/3", out4)]},
            {"linkMetrics": [("12", "0/1", 1), ("13", "0/3", 1)]},
            {"nodesSoftDrained": [("13", 50)]}]


@functools.lru_cache(maxsize=None)
def grid_answers(oracle, seeded, brs):
    o = W.Oracle(oracle, TM.grid_world(seeded), ME, True, brs)
    return [o.answer(sc) for sc in S.grid_scenarios() + grid_extra(seeded)]


def grid_sweep(product, seeded, brs):
    """the sweep and what must outlive it"""
    als, ls, ps = TM.grid_world(seeded).load(product, ME)
    sw = product.LinkFailureSweep(ME, ls, ps, S.grid_scenarios() + grid_extra(seeded), True, brs)
    assert sw.numVariants() == 56 and sw.nhWords() == 1
    return (als, ls, ps), sw


@pytest.mark.parametrize("seeded", [False, True], ids=["unit", "seeded"])
@pytest.mark.parametrize("brs", [False, True], ids=["plain", "brs"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_grid_forced(product, oracle, mode, brs, seeded):
    import openr_amd.capi as capi
    answers = grid_answers(oracle, seeded, brs)
    kinds = [W.kind_of(u) for u, _ in answers]
    assert set(kinds[:24]) <= {"delete", "mixed"} and set(kinds[24:48]) <= {"update", "mixed"}
    assert set(kinds[48:52]) == {"mixed"} and kinds[52] == "empty"
    assert kinds[53] != "empty" and kinds[55] != "empty"  # cost-out, soft drain
    assert (kinds[54] != "empty") == seeded  # to 1: a no-op on unit metrics
    keep, sw = grid_sweep(product, seeded, brs)
    assert sw.form() != product.kGlobalState  # a 25-node area needs no global form
    for k in STATE_FORMS:
        with capi.scoped_options(capi.load(), spf_global_lds=k):
            run_global(product, sw, mode, answers, ("grid", mode, brs, seeded, k))


# ---- hub and ring with the parallel link --------------------------------------
def test_hub_and_ring_mixed(product, oracle):
    """Raising units, a unit that lowers and units with node bits in one
    launch; the parallel r3 - r4 links; every mode and state form."""
    import openr_amd.capi as capi
    w = WM.as_metric_world(S.hub_ring_world())
    scs = [TM.MIXED, {"linkMetrics": TM.COST_OUT}, {"nodesDrained": ["hub"]},
           {"links": [("r7", "r7-r8/0")]}, {"nodesSoftDrained": [("r6", 20)]}, TM.SPOKES_TO_1,
           {"nodesSoftDrained": [("hub", 20)]}, {}, {"nodesDown": ["hub"]}, S.HUB_GROUP,
           {"links": [("r3", "r3-r4/1")]}, {"links": [("r3", "r3-r4/1"), ("r4", "r4-r3/0")]}]
    o = W.Oracle(oracle, w, "r0")
    answers = [o.answer(sc) for sc in scs]
    n = [len(u["unicastRoutesToUpdate"]) + len(u["unicastRoutesToDelete"]) for u, _ in answers]
    assert (n[0], n[5], n[6], n[7]) == (34, 37, 25, 0), n
    assert n[1] and n[2] and n[4] and not n[3] and n[8] and n[9], n
    als, ls, ps = w.load(product, "r0")
    sw = product.LinkFailureSweep("r0", ls, ps, scs, True, False)
    for k in STATE_FORMS:
        with capi.scoped_options(capi.load(), spf_global_lds=k):
            for mode in (0, 1, 2):
                run_global(product, sw, mode, answers, ("hub", mode, k))


# ---- two-word next-hop sets -----------------------------------------------------
def test_wide_source_with_drain(product, oracle):
    """The hub of a 40-node ring as source (W = 2) with a drain and a soft
    drain in the sweep: topology copies unforced, the global form when forced."""
    import openr_amd.capi as capi
    w = WM.as_metric_world(S.hub_ring_world(ring=40, parallel=False, prefixes=2))
    scs = [{"links": [("hub", f"hub-r{i}/0") for i in range(3, 9)]}, {"nodesDown": ["r9"]},
           {"nodesDrained": ["r20"]}, {"nodesSoftDrained": [("r20", 30)]},
           {"linkMetrics": [(a, i, 100) for k in range(3, 9)
                            for a, i in (("hub", f"hub-r{k}/0"), (f"r{k}", f"r{k}-hub/0"))]}]
    o = W.Oracle(oracle, w, "hub")
    answers = [o.answer(sc) for sc in scs]
    assert all(W.kind_of(u) != "empty" for u, _ in answers)
    als, ls, ps = w.load(product, "hub")
    sw = product.LinkFailureSweep("hub", ls, ps, scs[:3], True, False)
    assert sw.nhWords() == 2
    S.run(sw, 1, answers[:3], "unforced", product.kTopologyCopies)
    sw = product.LinkFailureSweep("hub", ls, ps, scs, True, False)
    for k in STATE_FORMS:
        with capi.scoped_options(capi.load(), spf_global_lds=k):
            for mode in (0, 1, 2):  # mode 2 at W = 2 writes every record, as elsewhere
                run_global(product, sw, mode, answers, ("wide", mode, k))
    sw.setGlobalForm(False)
    assert sw.form() == product.kEdgeBitset  # selected from the lists again
    S.run(sw, 1, answers, "unforced again", product.kTopologyCopies)


# ---- chunks ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_chunked_launch(product, oracle, mode):
    """56 scenarios in calls of 7 and of 9 (an uneven last chunk): the same
    updates, counts and records as one call."""
    answers = grid_answers(oracle, True, False)
    keep, sw = grid_sweep(product, True, False)
    run_global(product, sw, mode, answers, ("one call", mode))
    whole = [(sw.counts(v), sw.changedPrefixes(v), sw.routeUpdate(v)) for v in range(56)]
    for chunk in (7, 9):
        sw.setGlobalChunk(chunk)
        with pytest.raises((IndexError, RuntimeError)):
            sw.routeUpdate(0)  # the setter dropped what was fetched
        run_global(product, sw, mode, answers, ("chunks", chunk, mode))
        assert [(sw.counts(v), sw.changedPrefixes(v), sw.routeUpdate(v))
                for v in range(56)] == whole


def test_second_launch_and_setters(product, oracle):
    """Two launches on one sweep, the modes in turn, and the setters dropping
    what a launch of another form left fetched."""
    answers = grid_answers(oracle, True, False)
    keep, sw = grid_sweep(product, True, False)
    run_global(product, sw, 2, answers, "first")
    run_global(product, sw, 2, answers, "second")
    run_global(product, sw, 1, answers, "third")
    run_global(product, sw, 0, answers, "fourth")
    sw.setGlobalForm(False)
    assert sw.form() == product.kEdgeBitset
    for read in (lambda: sw.routeUpdate(0), lambda: sw.changedPrefixes(0), lambda: sw.counts(0)):
        with pytest.raises((IndexError, RuntimeError)):
            read()
    S.run(sw, 1, answers, "repair", product.kEdgeBitset)
    sw.setGlobalForm(True)
    with pytest.raises((IndexError, RuntimeError)):
        sw.routeUpdate(0)
    run_global(product, sw, 2, answers, "global again")
    # an area in the exact domain is never forced out of topology copies
    gz = S.grid_world(zero_link=True)
    als, ls, ps = gz.load(product, ME)
    exact = product.LinkFailureSweep(ME, ls, ps, [{"nodesDown": ["7"]}], True, False)
    exact.setGlobalForm(True)
    assert exact.form() == product.kTopologyCopies


# ---- the raw ABI on the device --------------------------------------------------
GLOBAL, WHATIF = "ogs_spf_routes_whatif_global", "ogs_spf_routes_whatif"


@pytest.fixture(scope="module")
def abi(product):
    return TM.Abi(product)


EDGE_DOWN, DST_MASK = 1 << 31, 0x1FFFFF  # OGS_EDGE_DOWN, OGS_EDGE_DST_MASK


def _base_tight(abi):
    """per directed edge of the 300-node WAN: is it tight in the base SPF (up,
    tail reached, tail the source or not overloaded, dist[tail] + w == dist[head])?"""
    h = abi.h
    edges, src = h["edges"].view("uint64"), h["edge_src"].view("uint32")
    dist = abi.base["dist"].cpu().numpy().view("uint32")
    flags = h["node_flags"].view("uint8")
    s = int(h["units"].view("uint32")[1])
    out = []
    for e in range(abi.E):
        x = int(edges[e])
        u, v, w = int(src[e]), x & DST_MASK, x >> 32
        out.append(bool(not x & EDGE_DOWN and int(dist[u]) != 0xFFFFFFFF and
                        (u == s or not flags[u] & TM.OVERLOADED) and
                        int(dist[u]) + w == int(dist[v])))
    return out


@pytest.mark.parametrize("flags", [INCREMENTAL | CHANGED_ONLY, INCREMENTAL, 0],
                         ids=["changed-only", "repair", "full"])
def test_abi_equals_the_whatif_entry(abi, flags):
    """dead lists, node bits and metric lists: `changed`, counts, records and
    SPF rows byte for byte what ogs_spf_routes_whatif writes; edge_src NULL
    (no exit-only units) gives the same bytes."""
    rng = random.Random(0x610B)
    dead, nodes = TM._wan_lists(abi)
    metrics = [[], TM._overrides(abi, rng, 30, 8), TM._overrides(abi, rng, 300, 8),
               TM._overrides(abi, rng, 30, 0.001), TM._overrides(abi, rng, 5, 8), []]
    # an edge both dead and overridden (to a lower weight) is dead
    metrics[1] = sorted({**dict(metrics[1]), dead[1][0]: 1}.items())
    if not flags:
        nodes = None  # node bits are not built in the LDS full form
    bits = None if nodes is None else [[TM.OVERLOADED if i % 2 == 0 else 6 for i in range(len(n))]
                                       for n in nodes]
    ref = abi.call(WHATIF, flags, dead, nodes, bits, metrics)
    got = abi.call(GLOBAL, flags, dead, nodes, bits, metrics)
    TM._same(abi.torch, got, ref, label=flags)
    counts = ref["counts"].view(-1, 2).sum(1).tolist()
    assert sum(c > 0 for c in counts) >= 4, counts
    src, abi.g.edge_src = abi.g.edge_src, None
    try:
        TM._same(abi.torch, abi.call(GLOBAL, flags, dead, nodes, bits, metrics), ref,
                 label=(flags, "edge_src NULL"))
    finally:
        abi.g.edge_src = src
    # node bits in the full mode, which the LDS entry does not build: the
    # records of the incremental call (a full recompute here either way)
    if not flags:
        _, nodes = TM._wan_lists(abi)
        bits = [[TM.OVERLOADED] * len(n) for n in nodes]
        want = abi.call(WHATIF, INCREMENTAL, dead, nodes, bits, metrics)
        TM._same(abi.torch, abi.call(GLOBAL, 0, dead, nodes, bits, metrics), want, label="nodes")


@pytest.mark.parametrize("flags", [INCREMENTAL | CHANGED_ONLY, 0], ids=["changed-only", "full"])
def test_abi_refused_unit_and_skipped_ids(abi, flags):
    torch = abi.torch
    rng = random.Random(0xBAD)
    E, U = abi.E, 6
    dead = [[] for _ in range(U)]
    good = [TM._overrides(abi, rng, 30, 8), TM._overrides(abi, rng, 300, 8), [],
            TM._overrides(abi, rng, 30, 0.001), TM._overrides(abi, rng, 5, 8), []]
    ref = abi.call(WHATIF, flags, dead, metrics=good)
    TM._same(torch, abi.call(GLOBAL, flags, dead, metrics=good), ref, label="good")
    # ids >= E (with values that would refuse a unit) and node ids >= N change nothing
    past = [m + [(E, 0), (E + 7, 5), (0xFFFFFFFF - 2**32, 5)] for m in good]
    TM._same(torch, abi.call(GLOBAL, flags, dead, metrics=past), ref, label="edge ids")
    if flags:
        nodes = [[abi.Sn, 0xFFFFFFFF - 2**32] if u == 3 else [] for u in range(U)]
        got = abi.call(GLOBAL, flags, [[E, 0xFFFFFFFF - 2**32]] * U, nodes,
                       [[1] * len(n) for n in nodes], good)
        # (unit 3's node slice is not empty, so it takes no exit: same bytes)
        TM._same(torch, got, ref, label="node ids")
    # a 0 in unit 2's slice, 2^31 in unit 4's, a slice longer than the call sized in unit 1's
    bad = [list(m) for m in good]
    bad[2] = [(5, 7), (9, 0), (11, 3)]
    bad[4] = bad[4][:2] + [(bad[4][2][0], (1 << 31) - 2**32)] + bad[4][3:]
    for case, longest, refused in ((bad, None, (2, 4)), (good, 200, (1,))):
        got = abi.call(GLOBAL, flags, dead, metrics=case, longest=longest)
        keep = [u for u in range(U) if u not in refused]
        TM._same(torch, got, ref, rows=(U, keep), label=("neighbours", refused))
        for u in refused:
            assert got["counts"].view(U, 2)[u].tolist() == [-1, -1]  # OGS_WHATIF_REFUSED
            assert not got["changed"].view(U, -1)[u].any()
            for k in ("meta", "metric", "mask", "sel", "dist", "nh"):
                assert (got[k].view(U, -1)[u] == TM.FILL).all(), (u, k)


def test_abi_exit_only_units(abi):
    """A unit whose only dead link is on no base shortest path runs nothing:
    a zero `changed` row, counts {0, 0}, no record; the same link list with one
    base-tight link added computes and changes routes. The exit is taken only
    with both flags, and never hides a change: every unit equals the full
    recompute's diff."""
    torch = abi.torch
    tight = _base_tight(abi)
    slack = [e for e, t in enumerate(tight) if not t]
    used = [e for e, t in enumerate(tight) if t]
    assert len(slack) > 40 and len(used) > 40
    rng = random.Random(0xE117)
    dead = [[e] for e in rng.sample(slack, 8)] + [[e] for e in rng.sample(used, 8)]
    dead += [rng.sample(slack, 20), rng.sample(slack, 20) + [used[0]]]
    U = len(dead)
    full = abi.call(GLOBAL, 0, dead)
    co = abi.call(GLOBAL, INCREMENTAL | CHANGED_ONLY, dead)
    for k in ("changed", "counts"):
        assert torch.equal(full[k], co[k]), k
    counts = co["counts"].view(U, 2).sum(1).tolist()
    slack_units, tight_units = list(range(8)) + [16], list(range(8, 16)) + [17]
    assert all(counts[u] == 0 for u in slack_units), counts
    assert sum(counts[u] > 0 for u in tight_units) >= 6, counts  # the opposite case
    for u in slack_units:  # ran nothing: no record; the base's SPF rows
        assert not co["changed"].view(U, -1)[u].any()
        for k in ("meta", "metric", "mask", "sel"):
            assert (co[k].view(U, -1)[u] == TM.FILL).all(), (u, k)
        assert torch.equal(co["dist"].view(U, -1)[u], abi.base["dist"])
        assert torch.equal(co["nh"].view(U, -1)[u], abi.base["nh"])
    # and what ogs_spf_routes_whatif's repair writes for the same lists
    TM._same(torch, co, abi.call(WHATIF, INCREMENTAL | CHANGED_ONLY, dead), label="repair")
    # a raised slack edge exits, a lowered one and a node bit never do
    e = slack[3]
    w = int(abi.h["edges"].view("uint64")[e]) >> 32
    metrics = [[(e, w + 5)], [(e, max(1, w - 1))] if w > 1 else [(e, w + 5)], []]
    nodes, bits = [[], [], [7]], [[], [], [6]]
    got = abi.call(GLOBAL, INCREMENTAL | CHANGED_ONLY, [[], [], []], nodes, bits, metrics)
    want = abi.call(GLOBAL, 0, [[], [], []], nodes, bits, metrics)
    for k in ("changed", "counts"):
        assert torch.equal(got[k], want[k]), k
    assert (got["dist"].view(3, -1)[0] == abi.base["dist"]).all()


class WideAbi(TM.Abi):
    """TM.Abi's WAN at nh_words = W > 1: W next-hop rows a unit (word w of unit
    u at nh[(u * W + w) * Sn]), W mask rows, and the base unit built at that
    width. Calls of the global entry over dead lists."""

    def __init__(self, product, W):
        self.W = W
        super().__init__(product)  # the base at one word, then at W
        import ctypes
        self.base, so = self.outs(1)
        u = self.unit.view(-1).to(self.dev)
        self.capi.check(self.lib, self.lib.ogs_spf_routes(
            ctypes.byref(self.g), ctypes.byref(self.pt), ctypes.c_void_p(u.data_ptr()), 1,
            self.flags, W, ctypes.byref(so), self.stream), "ogs_spf_routes")
        self.torch.cuda.synchronize()

    def outs(self, U):
        torch, W = self.torch, self.W
        o = {k: torch.full((U * n,), TM.FILL, dtype=torch.int32, device=self.dev)
             for k, n in (("dist", self.Sn), ("nh", W * self.Sn), ("meta", self.Sp),
                          ("metric", self.Sp), ("mask", W * self.Sp), ("sel", self.Sp))}
        so = self.capi.SpfOut(o["dist"].data_ptr(), o["nh"].data_ptr(), o["meta"].data_ptr(),
                              o["metric"].data_ptr(), o["mask"].data_ptr(), o["sel"].data_ptr())
        return o, so

    def run(self, flags, dead):
        """(status, every output) of ogs_spf_routes_whatif_global at W words"""
        import ctypes
        torch, capi = self.torch, self.capi
        U = len(dead)
        o, so = self.outs(U)
        o["changed"] = torch.full((U * ((self.Sp + 31) // 32),), TM.FILL, dtype=torch.int32,
                                  device=self.dev)
        o["counts"] = torch.full((U * 2,), TM.FILL, dtype=torch.int32, device=self.dev)
        b = self.base
        diff = capi.RouteDiff(b["meta"].data_ptr(), b["metric"].data_ptr(), b["mask"].data_ptr(),
                              o["changed"].data_ptr(), o["counts"].data_ptr(),
                              b["dist"].data_ptr(), b["nh"].data_ptr(), None, None, 0)
        units = self.unit.repeat(U, 1).contiguous().view(-1).to(self.dev)
        d_off, d_list = self.csr(dead)
        mods = capi.WhatifMods(d_off.data_ptr(), d_list.data_ptr(), None, None, None, None, None,
                               None, 0)
        rc = self.lib.ogs_spf_routes_whatif_global(
            ctypes.byref(self.g), ctypes.byref(self.pt), ctypes.c_void_p(units.data_ptr()), U,
            ctypes.byref(mods), ctypes.byref(diff), self.flags | flags, self.W, ctypes.byref(so),
            self.stream)
        torch.cuda.synchronize()
        return rc, o


@pytest.mark.parametrize("W", [2, 4])
def test_abi_wide_sets_take_no_exit(product, W):
    """OGS_F_CHANGED_ONLY is an nh_words 1 mode, so there is no exit-only unit
    at two or four next-hop words: the entry refuses the flag before any
    launch, and with OGS_F_INCREMENTAL alone a unit whose dead links are on no
    base shortest path computes its own rows -- every unit's W next-hop rows,
    its neighbours' included, and records byte for byte the full recompute's."""
    wabi = WideAbi(product, W)
    torch = wabi.torch
    tight = _base_tight(wabi)
    slack = [e for e, t in enumerate(tight) if not t]
    used = [e for e, t in enumerate(tight) if t]
    rng = random.Random(0x2E17)
    # slack and tight units alternate: a wrong row offset would land in a neighbour
    dead = [[e] for pair in zip(rng.sample(slack, 6), rng.sample(used, 6)) for e in pair]
    dead += [rng.sample(slack, 20), rng.sample(slack, 20) + [used[0]]]
    U = len(dead)
    rc, out = wabi.run(INCREMENTAL | CHANGED_ONLY, dead)
    assert rc == -1 and b"nh_words 1" in wabi.lib.ogs_last_error()  # OGS_E_INVALID
    for k, t in out.items():
        assert (t == TM.FILL).all(), k  # nothing was launched
    rc, full = wabi.run(0, dead)
    assert rc == 0
    rc, inc = wabi.run(INCREMENTAL, dead)
    assert rc == 0
    TM._same(torch, inc, full, label=("incremental", W))
    counts = full["counts"].view(U, 2).sum(1).tolist()
    slack_units = list(range(0, 12, 2)) + [12]
    assert all(counts[u] == 0 for u in slack_units), counts
    assert sum(counts[u] > 0 for u in range(U) if u not in slack_units) >= 5, counts
    for u in slack_units:  # computed, and equal to the base's W-word rows
        assert torch.equal(full["dist"].view(U, -1)[u], wabi.base["dist"])
        assert torch.equal(full["nh"].view(U, -1)[u], wabi.base["nh"])
        assert torch.equal(full["mask"].view(U, -1)[u], wabi.base["mask"])
    assert not (full["nh"] == TM.FILL).any() and not (full["mask"] == TM.FILL).any()


# ---- natural size: past the LDS forms' limit --------------------------------------
WAN17K = dict(nodes=17000, seed=0xC4, prefixesPerNode=1)


@functools.lru_cache(maxsize=None)
def wan17k_case(product, oracle):
    """The wan generator at 17,000 nodes from source "0": 63,964 directed
    edges, so a unit's bitset fill takes more than one pass of 1,024 x 32
    edges. 20 scenarios of every kind; prefix databases of 1,000 nodes -- the
    source's neighbourhood, the nodes the scenarios touch and their
    neighbours, random others (loading all 17,000 takes minutes in Python)."""
    w = WM.as_metric_world(W.generated_world(product, "wan", WAN17K))
    assert len(w.adjdbs) == 17000 and w.directed_edges() == 63964
    assert w.directed_edges() > 1024 * 32
    rng = random.Random(0x17000)
    nbrs = lambda n: [a["otherNodeName"] for a in w.adjdbs[n]["adjacencies"]]  # noqa: E731
    names = sorted(n for n in w.adjdbs if n != "0" and len(nbrs(n)) >= 2)
    near = sorted({m for n in nbrs("0") for m in nbrs(n)} - {"0"})  # two hops from the source
    down = rng.sample(near, 2) + rng.sample(names, 2)
    drained = rng.sample(near, 2) + rng.sample(names, 2)
    soft = rng.sample(near, 1) + rng.sample(names, 1)
    src_links = [("0", a["ifName"], a["metric"]) for a in w.adjdbs["0"]["adjacencies"]]
    near_links = [(n, a["ifName"], a["metric"]) for n in near for a in w.adjdbs[n]["adjacencies"]]
    single = rng.sample(src_links, 2) + rng.sample(near_links, 2)
    cost_out = rng.sample(src_links, 1) + rng.sample(near_links, 1)
    to_one = rng.sample([x for x in near_links if x[2] > 1], 2)
    scs = ([{"nodesDown": [n]} for n in down] + [{"nodesDrained": [n]} for n in drained] +
           [{"links": [(n, i)]} for n, i, _ in single] +
           [{"linkMetrics": [(n, i, 8 * m)]} for n, i, m in cost_out] +
           [{"linkMetrics": [(n, i, 1)]} for n, i, _ in to_one] +
           [{"nodesSoftDrained": [(n, 1000)]} for n in soft] +
           [{"links": [x[:2] for x in rng.sample(near_links, 6)], "nodesDown": [rng.choice(near)]},
            {}])
    assert len(scs) == 20
    touched = set(down + drained + soft + near + [x[0] for x in single + cost_out + to_one])
    behind = {m for n in touched for m in nbrs(n)} | {m for n in down + drained for k in nbrs(n)
                                                      for m in nbrs(k)}
    keep = ["0"] + sorted((touched | behind) - {"0"})
    keep = keep[:900]
    rest = sorted(set(w.adjdbs) - set(keep))
    keep += rng.sample(rest, 1000 - len(keep))
    for n in down + drained + soft:
        assert n in keep
    keep = set(keep)
    w.prefix_dbs = [d for d in w.prefix_dbs if d["thisNodeName"] in keep]
    assert len(w.prefix_dbs) == 1000
    o = W.Oracle(oracle, w, "0")
    return w, scs, [o.answer(sc) for sc in scs]


@pytest.mark.parametrize("mode", [1, 2])
def test_natural_size(product, oracle, mode):
    """17,000 nodes at one next-hop word: the form is selected with nothing
    forced, single-link failures included (without the form that sweep
    throws: the register form reports the area unsupported)."""
    w, scs, answers = wan17k_case(product, oracle)
    kinds = [W.kind_of(u) for u, _ in answers]
    assert sum(k != "empty" for k in kinds) >= 10, kinds
    assert sum(bool(u["unicastRoutesToUpdate"]) for u, _ in answers) >= 10
    assert kinds[19] == "empty"
    als, ls, ps = w.load(product, "0")
    sw = product.LinkFailureSweep("0", ls, ps, scs, True, False)
    assert sw.nhWords() == 1 and sw.form() == product.kGlobalState
    run_global(product, sw, mode, answers, ("17k", mode), forced=False)
    # the plain link-failure sweep alone: lists of two directed edges
    links = list(range(8, 12))
    sw = product.LinkFailureSweep("0", ls, ps, [scs[i] for i in links], True, False)
    assert sw.form() == product.kGlobalState
    run_global(product, sw, mode, [answers[i] for i in links], ("17k links", mode), forced=False)
