"""SpfSolver::rebuildRoutes against the oracle: Decision::rebuildRoutes' full
branch (Decision.cpp:912-927) = buildRouteDb + DecisionRouteDb::calculateUpdate
(SpfSolver.cpp:21-56) against the held RouteDb, which the oracle side runs
literally on its own replica. After every call the product's update, its held
RouteDb (routeDb()) and its best-route selection cache must equal the
oracle's; attribute-only flaps must take the device delta path
(ogs_route_delta: deltaBuilds grows, deltaFallbacks does not) and every change
of the path's key must fall back, once.

The 5x5 grid (source "12", the centre) carries 100 prefixes per node plus 3
anycast extras: 2,503 prefixes, more than one 2048-prefix tile and not a
multiple of 32. The flap sequence was checked with the oracle alone to hold a
flap with an empty update, one with updates only and one with deletions."""
import random

import pytest

import lsdb as L

pytestmark = pytest.mark.gpu

A = L.kTestingAreaName
N = 5
ME = "12"


class Grid:
    """The attribute state of the grid's adjacency databases, replayed into
    any number of LinkStates (product and oracle replicas)."""

    def __init__(self, n=N, area=A):
        self.n, self.area = n, area
        self.metric, self.adj_over, self.node_over, self.v6, self.gone = {}, set(), set(), {}, set()

    def neighbours(self, node):
        i, j = divmod(node, self.n)
        for (ii, jj, ifn, oifn) in ((i, j + 1, "0/1", "0/3"), (i - 1, j, "0/2", "0/4"),
                                    (i, j - 1, "0/3", "0/1"), (i + 1, j, "0/4", "0/2")):
            if 0 <= ii < self.n and 0 <= jj < self.n:
                yield ii * self.n + jj, ifn, oifn

    def adjdb(self, node):
        adjs = []
        for nb, ifn, oifn in self.neighbours(node):
            if (node, nb) in self.gone:
                continue
            a = L.createAdjacency(str(nb), ifn, oifn, self.v6.get((node, nb), f"fe80::{nb:x}"),
                                  f"192.168.0.{nb}", self.metric.get((node, nb), 1), 100001 + nb)
            a["isOverloaded"] = (node, nb) in self.adj_over
            adjs.append(a)
        return L.createAdjDb(str(node), adjs, node + 1, overLoadBit=node in self.node_over,
                             area=self.area)

    def load(self, M, als=None):
        als = als if als is not None else M.AreaLinkStates()
        ls = als.add(self.area, ME)
        for node in range(self.n * self.n):
            ls.updateAdjacencyDatabase(self.adjdb(node), self.area)
        return als, ls


def _prefixes(M, per_node=100, area=A, n=N):
    ps = M.PrefixState()
    for node in range(n * n):
        ents = []
        for i in range(per_node):
            if i % 25 == 7:
                e = L.createPrefixEntry(f"10.{node + 25 * (i // 256)}.{i % 256}.0/24")
            else:
                e = L.createPrefixEntry(f"fc00:{node:x}::{i:x}/128",
                                        minNexthop=2 if i % 25 == 13 else None)
            ents.append(e)
        if node in (4, 20):  # anycast
            ents.append(L.createPrefixEntry("fd00::aa/128"))
        if node in (0, 12):  # also advertised by the source: selected, no route
            ents.append(L.createPrefixEntry("fd00::10c/128"))
        if node in (2, 22):
            ents.append(L.createPrefixEntry("fd00::bb/128", minNexthop=2 if node == 2 else None))
        L.updatePrefixDatabase(ps, L.createPrefixDb(str(node), ents), area)
    return ps


class Twin:
    """Product and oracle replicas of one domain, the product's solver under
    test and the oracle's held RouteDb."""

    def __init__(self, product, oracle, grid, me=ME, v4=True, sr=False, brs=False, per_node=100,
                 worlds=None):
        self.P, self.O, self.grid, self.me = product, oracle, grid, me
        if worlds is None:
            worlds = [(grid.load(M) + (_prefixes(M, per_node),)) for M in (product, oracle)]
        (self.pa, self.pls, self.pps), (self.oa, self.ols, self.ops) = worlds
        self.ps = product.SpfSolver(me, v4, sr, brs)
        self.os = oracle.SpfSolver(me, v4, sr, brs)
        self.held = oracle.DecisionRouteDb()
        self.opol = None

    def set_policy(self, statements):
        self.ppol = self.P.RibPolicy(statements)
        self.opol = self.O.RibPolicy(statements)
        self.ps.setRibPolicy(self.ppol)

    def update(self, node):
        """replays the grid's database of `node` into both replicas"""
        for ls in (self.pls, self.ols):
            ls.updateAdjacencyDatabase(self.grid.adjdb(node), self.grid.area)

    def oracle_step(self, me=None):
        new = self.os.buildRouteDb(me or self.me, self.oa, self.ops)
        if self.opol is not None:
            self.opol.applyPolicy(new)
        upd = self.held.calculateUpdate(new)
        self.held = new
        return upd

    def step(self, label, fast, me=None):
        """one rebuildRoutes; returns the update"""
        b0, f0 = self.ps.deltaBuilds(), self.ps.deltaFallbacks()
        got = self.ps.rebuildRoutes(me or self.me, self.pa, self.pps)
        want = self.oracle_step(me)
        for k in ("unicastRoutesToUpdate", "unicastRoutesToDelete", "mplsRoutesToUpdate",
                  "mplsRoutesToDelete"):
            assert got[k] == want[k], (label, k)
        assert self.ps.routeDb().canonical() == self.held.canonical(), label
        assert self.ps.getBestRoutesCache() == self.os.getBestRoutesCache(), label
        db, df = self.ps.deltaBuilds() - b0, self.ps.deltaFallbacks() - f0
        assert (db, df) == ((1, 0) if fast else (0, 1)), (label, db, df)
        return got


def flap_sequence(seed=0xF1A9, count=20):
    """(kind, node, neighbour, value): attribute-only flaps. The first three
    are placed by hand (an empty update, a large one, deletions only); the
    rest are drawn, flaps with updates only among them."""
    rng = random.Random(seed)
    flaps = [("metric", 0, 1, 5),          # leaves 12's ECMP sets untouched
             ("metric", 12, 13, 3),        # a source link: updates, and the
                                           # minNexthop prefixes' deletions
             ("adj_over_all", 24, None, True)]  # 24 unreachable: deletions
    g = Grid()
    while len(flaps) < count:
        node = rng.randrange(N * N)
        nb = rng.choice([x for x, _, _ in g.neighbours(node)])
        kind = rng.choice(["metric", "metric", "adj_over", "node_over"])
        if kind == "metric":
            flaps.append((kind, node, nb, rng.choice([1, 2, 5, 9])))
        elif kind == "adj_over":
            flaps.append((kind, node, nb, None))  # toggles
        else:
            flaps.append((kind, node, None, None))  # toggles
    return flaps


def apply_flap(grid, flap):
    kind, node, nb, value = flap
    if kind == "metric":
        grid.metric[(node, nb)] = value
    elif kind == "adj_over":
        grid.adj_over ^= {(node, nb)}
    elif kind == "adj_over_all":
        grid.adj_over |= {(node, x) for x, _, _ in grid.neighbours(node)}
    else:
        grid.node_over ^= {node}
    return node


@pytest.mark.parametrize("brs", [False, True], ids=["plain", "best_route_selection"])
def test_flaps_take_the_delta_path(product, oracle, brs):
    grid = Grid()
    t = Twin(product, oracle, grid, brs=brs)
    assert len(t.pps.prefixes()) == 2503
    first = t.step("first call", fast=False)
    assert len(first["unicastRoutesToUpdate"]) > 2000
    seen = set()
    for i, flap in enumerate(flap_sequence()):
        t.update(apply_flap(grid, flap))
        u = t.step((i, flap), fast=True)
        nu, nd = len(u["unicastRoutesToUpdate"]), len(u["unicastRoutesToDelete"])
        seen.add("empty" if nu + nd == 0 else "deletions" if nd else "updates only")
    assert seen == {"empty", "updates only", "deletions"}
    # a call with nothing changed: the delta path, an empty update
    u = t.step("no change", fast=True)
    assert not u["unicastRoutesToUpdate"] and not u["unicastRoutesToDelete"]


@pytest.mark.parametrize("per_node,zero,policy,floor", [(300, True, False, 2048),
                                                        (500, False, True, 4700),
                                                        (500, True, True, 4700)],
                         ids=["u64_past_the_floor", "policy_past_one_copy",
                              "u64_policy_past_one_copy"])
def test_large_changes_grow_the_record_block(product, oracle, per_node, zero, policy, floor):
    """Flaps on the source's own links move about 40 % of the routes: more
    changed records than the 2,048-record block holds (the gather runs again
    into a grown block) and, at 500 prefixes per node, a block past 128 kB
    (16-byte header first, then `total` elements per column, mask rows
    strided by the capacity) -- with u32 and u64 metrics and with the policy
    columns. Still the delta path: no fallback."""
    grid = Grid()
    if zero:
        grid.metric[(0, 1)] = grid.metric[(1, 0)] = 0  # exact order, u64 metrics
    t = Twin(product, oracle, grid, per_node=per_node)
    if policy:
        t.set_policy([dict(name="w", prefixes=[f"fc00:{n:x}::{i:x}/128" for n in range(25)
                                               for i in range(0, per_node, 3)],
                           set_weight=dict(default_weight=1, area_to_weight={},
                                           neighbor_to_weight={"13": 0, "7": 4}),
                           counterID="cw")])
    t.step("first", fast=False)
    sizes = []
    for i, (nb, m) in enumerate([(13, 3), (13, 1), (11, 5), (7, 2), (11, 1)]):
        grid.metric[(12, nb)] = m
        t.update(12)
        u = t.step(("large", i), fast=True)
        sizes.append(len(u["unicastRoutesToUpdate"]) + len(u["unicastRoutesToDelete"]))
    # the first flap outgrows the 2,048-record block and the largest one a
    # block of `floor` records (4,700 records of 28 bytes pass 128 kB); every
    # later flap is copied from the grown block
    assert sizes[0] > 2048 and max(sizes) > floor and min(sizes) > 2048, sizes
    # a small change after the large ones: `total` well below the capacity
    grid.metric[(0, 5)] = 3
    t.update(0)
    t.step("small after large", fast=True)


def test_source_in_no_area(product):
    grid = Grid()
    als, _ = grid.load(product)
    ps = _prefixes(product, 1)
    s = product.SpfSolver(ME, True, False)
    assert s.rebuildRoutes(ME, als, ps) is not None
    held = s.routeDb().canonical()
    assert s.rebuildRoutes("nobody", als, ps) is None
    assert s.routeDb().canonical() == held
    assert (s.deltaBuilds(), s.deltaFallbacks()) == (0, 1)


def test_key_changes_fall_back(product, oracle):
    grid = Grid()
    t = Twin(product, oracle, grid, brs=True, per_node=20)
    t.step("first call", fast=False)
    grid.metric[(12, 13)] = 4
    t.update(12)
    t.step("flap", fast=True)
    # structural: the adjacency 6 -> 7 withdrawn (the link goes)
    grid.gone.add((6, 7))
    t.update(6)
    t.step("adjacency removed", fast=False)
    grid.metric[(12, 13)] = 1
    t.update(12)
    t.step("flap after re-flatten", fast=True)
    # a prefix advertisement change
    for ps in (t.pps, t.ops):
        L.updatePrefixDatabase(ps, L.createPrefixDb("6", [L.createPrefixEntry("fd00::aa/128")]))
    u = t.step("prefix change", fast=False)
    assert u["unicastRoutesToDelete"]  # 6's own prefixes went
    t.step("after prefix change", fast=True)
    # a next-hop address on one of the source's links: no record changes,
    # every v6 route over that link does (the attribute epoch)
    over = {p for p, r in t.ps.routeDb().unicastRoutes().items()
            if ":" in p and any(nh[1] == "0/1" for nh in r["nexthops"])}
    assert over
    grid.v6[(12, 13)] = "fe80::beef"
    t.update(12)
    u = t.step("next-hop address", fast=False)
    assert set(u["unicastRoutesToUpdate"]) >= over
    assert any(nh[0] == "fe80::beef" for p in over
               for nh in u["unicastRoutesToUpdate"][p]["nexthops"])
    t.step("after address change", fast=True)
    # another source, and back
    t.step("other source", fast=False, me="0")
    t.step("other source again", fast=True, me="0")
    t.step("back", fast=False)
    # a RibPolicy set
    t.set_policy([dict(name="ucmp", prefixes=[f"fc00:{n:x}::3/128" for n in range(25)],
                       set_weight=dict(default_weight=2, area_to_weight={},
                                       neighbor_to_weight={"13": 0, "7": 5}),
                       counterID="c1")])
    u = t.step("policy set", fast=False)
    assert any(r.get("counterID") == "c1" for r in u["unicastRoutesToUpdate"].values())
    # static routes changed
    t.step("before statics", fast=True)
    static = {"fd00::dead/128": dict(prefix="fd00::dead/128",
                                     nexthops=[L.createNextHop("fe80::99", "eth9", 0)])}
    for s in (t.ps, t.os):
        s.updateStaticUnicastRoutes(static, [])
    t.step("statics", fast=False)
    # a buildRouteDb of the same solver in between rebuilt the selection cache
    t.ps.buildRouteDb("3", t.pa, t.pps)
    t.os.buildRouteDb("3", t.oa, t.ops)
    t.step("after another entry point", fast=False)
    t.step("and again", fast=True)


def test_two_areas_fall_back(product, oracle):
    grid = Grid()
    worlds = []
    for M in (product, oracle):
        als, ls = grid.load(M)
        ls2 = als.add("area2", ME)
        ls2.updateAdjacencyDatabase(L.createAdjDb(ME, [L.createAdjacency(
            "x1", "e1", "f1", "fe80::e1", "10.7.0.1", 3, 200001)], 13, area="area2"), "area2")
        ls2.updateAdjacencyDatabase(L.createAdjDb("x1", [L.createAdjacency(
            ME, "f1", "e1", "fe80::c", "10.7.0.2", 3, 200002)], 300, area="area2"), "area2")
        ps = _prefixes(M, 4)
        L.updatePrefixDatabase(ps, L.createPrefixDb("x1", [L.createPrefixEntry("fd00::aa/128")]),
                               "area2")
        worlds.append((als, ls, ps))
    t = Twin(product, oracle, grid, worlds=worlds)
    t.step("first", fast=False)
    grid.metric[(12, 13)] = 7
    t.update(12)
    t.step("flap, two areas", fast=False)
    t.step("no change, two areas", fast=False)
    # the compiled policy is cached on the topology layout: a multi-area
    # build across attribute-only patches keeps using it
    t.set_policy([dict(name="w", prefixes=[f"fc00:{n:x}::{i:x}/128" for n in range(25)
                                           for i in (1, 2)] + ["fd00::aa/128"],
                       set_weight=dict(default_weight=1, area_to_weight={"area2": 3},
                                       neighbor_to_weight={"13": 0, "11": 2}),
                       counterID="cm")])
    t.step("policy, two areas", fast=False)
    for i, (nb, m) in enumerate([(13, 1), (11, 4), (7, 2)]):
        grid.metric[(12, nb)] = m
        t.update(12)
        t.step(("policy flap, two areas", i), fast=False)
    assert b"cid=cm" in t.ps.routeDb().canonical()


def test_policy_columns_across_flaps(product, oracle):
    """An active RibPolicy: the statement choice of a route is part of the
    diff (weights and counterID), and zero-weight next hops are dropped."""
    grid = Grid()
    t = Twin(product, oracle, grid, per_node=30)
    t.set_policy([
        dict(name="a", prefixes=[f"fc00:{n:x}::{i:x}/128" for n in range(25) for i in (1, 2, 3)],
             set_weight=dict(default_weight=1, area_to_weight={},
                             neighbor_to_weight={"13": 0, "11": 3}), counterID="ca"),
        dict(name="b", prefixes=[f"fc00:{n:x}::{i:x}/128" for n in range(25) for i in (3, 4)],
             set_weight=dict(default_weight=0, area_to_weight={A: 2}, neighbor_to_weight={}),
             counterID="cb")])
    t.step("first", fast=False)
    changed = 0
    for i, flap in enumerate(flap_sequence(seed=0xB01, count=10)):
        t.update(apply_flap(grid, flap))
        u = t.step(("policy", i, flap), fast=True)
        changed += len(u["unicastRoutesToUpdate"])
    assert changed
    assert b"cid=ca" in t.ps.routeDb().canonical()


class _RecordingAls:
    """AreaLinkStates stand-in handed to a topology generator: keeps the
    adjacency databases it loads, so a test can replay one with changes."""

    def __init__(self, als):
        self.als, self.dbs = als, {}

    def add(self, area, node):
        ls, dbs = self.als.add(area, node), self.dbs

        class _Ls:
            def updateAdjacencyDatabase(self, db, area):
                dbs[db["thisNodeName"]] = db
                return ls.updateAdjacencyDatabase(db, area)
        self.ls = ls
        return _Ls()


def test_wide_source_two_mask_words(product, oracle):
    """A hub of 40 links: next-hop sets of two words (W = 2)."""
    import test_gpu_high_degree as HD
    worlds = []
    for M in (product, oracle):
        rec = _RecordingAls(M.AreaLinkStates())
        _, _, ps = HD._hub(M, 40, seed=5, als=rec)
        worlds.append((rec.als, rec.ls, ps, rec.dbs[HD.HUB]))
    (pa, pls, pps, hub_db), (oa, ols, ops, _) = worlds
    ps_, os_ = product.SpfSolver(HD.HUB, True, False), oracle.SpfSolver(HD.HUB, True, False)
    held = oracle.DecisionRouteDb()

    def step(fast):
        nonlocal held
        b0, f0 = ps_.deltaBuilds(), ps_.deltaFallbacks()
        got = ps_.rebuildRoutes(HD.HUB, pa, pps)
        new = os_.buildRouteDb(HD.HUB, oa, ops)
        want = held.calculateUpdate(new)
        held = new
        assert got == want
        assert ps_.routeDb().canonical() == held.canonical()
        assert (ps_.deltaBuilds() - b0, ps_.deltaFallbacks() - f0) == ((1, 0) if fast else (0, 1))
        return got

    step(False)
    # the hub's own database, as the generator loaded it, with other metrics
    # on links of both mask words
    hub = [dict(a) for a in hub_db["adjacencies"]]
    assert len(hub) == 40
    total = 0
    for round_ in range(3):
        for k in (1, 17, 33, 38):
            hub[k]["metric"] = 1 + (hub[k]["metric"] + round_) % 3
        for ls in (pls, ols):
            ls.updateAdjacencyDatabase(dict(hub_db, adjacencies=hub), A)
        u = step(True)
        total += len(u["unicastRoutesToUpdate"]) + len(u["unicastRoutesToDelete"])
    assert total


def test_zero_metric_area_exact_order(product, oracle):
    """A zero link metric: the exact extraction order, u64 metrics."""
    grid = Grid()
    grid.metric[(7, 8)] = grid.metric[(8, 7)] = 0
    t = Twin(product, oracle, grid, per_node=8)
    t.step("first", fast=False)
    changed = 0
    for i, flap in enumerate([("metric", 12, 7, 4), ("metric", 12, 7, 1), ("node_over", 8, None, None),
                              ("metric", 2, 7, 3), ("node_over", 8, None, None)]):
        t.update(apply_flap(grid, flap))
        u = t.step(("exact", i), fast=True)
        changed += len(u["unicastRoutesToUpdate"]) + len(u["unicastRoutesToDelete"])
    assert changed


def test_segment_routing_mpls_part(product, oracle):
    grid = Grid()
    t = Twin(product, oracle, grid, sr=True, per_node=8)
    first = t.step("first", fast=False)
    assert len(first["mplsRoutesToUpdate"]) == N * N
    mpls = 0
    for i, flap in enumerate(flap_sequence(seed=0x5E6, count=8)):
        t.update(apply_flap(grid, flap))
        u = t.step(("sr", i, flap), fast=True)
        mpls += len(u["mplsRoutesToUpdate"]) + len(u["mplsRoutesToDelete"])
    assert mpls


COUNTERS = ["decision.route_build_runs.count", "decision.get_route_for_prefix.count",
            "decision.no_route_to_prefix.count", "decision.route_build_ms.count"]


def test_counters_move_as_one_build(product):
    """rebuildRoutes on one solver, buildRouteDb on its twin, same state."""
    M = product
    grid = Grid()
    grid.adj_over |= {(24, 19), (24, 23)}  # 24 unreachable: no_route_to_prefix moves
    (a_als, a_ls), (b_als, b_ls) = grid.load(M), grid.load(M)
    a_ps, b_ps = _prefixes(M, 6), _prefixes(M, 6)
    a, b = M.SpfSolver(ME, True, False), M.SpfSolver(ME, True, False)

    def deltas(fn):
        M.reset_decision_counters()
        fn()
        c = M.decision_counters()
        return {k: c.get(k, 0) for k in COUNTERS}

    first_a = deltas(lambda: a.rebuildRoutes(ME, a_als, a_ps))
    first_b = deltas(lambda: b.buildRouteDb(ME, b_als, b_ps))
    assert first_a == first_b  # the fallback is one build
    grid.metric[(12, 13)] = 6
    for ls in (a_ls, b_ls):
        ls.updateAdjacencyDatabase(grid.adjdb(12), A)
    fast_a = deltas(lambda: a.rebuildRoutes(ME, a_als, a_ps))
    fast_b = deltas(lambda: b.buildRouteDb(ME, b_als, b_ps))
    assert a.deltaBuilds() == 1
    assert fast_a == fast_b
    assert fast_a["decision.route_build_runs.count"] == 1
    assert fast_a["decision.get_route_for_prefix.count"] == len(a_ps.prefixes())
    assert fast_a["decision.no_route_to_prefix.count"] >= 6
