"""NetworkWhatifSweep against the oracle: every (source, scenario) pair's
update is what the oracle computes from that source's own Decision
(whatif.Oracle per source: mutate the LinkState the way the reference would,
buildRouteDb(source), calculateUpdate against that source's base, restore).
Per computed pair whatif.check_sweep's assertions; per scenario the set of
affected sources. The grid case is test_gpu_whatif_restore's seeded 5x5 grid
(a drained baseline, so the restoring kinds have something to put back) with
all 25 nodes as sources; the hub-ring case has a source the batch cannot take.
The oracle's answers are computed once and shared."""
import functools

import pytest

import test_gpu_scenarios as S
import test_gpu_whatif_restore as TR
import whatif as W
import whatif_restore as WR

pytestmark = pytest.mark.gpu

SOURCES = [str(n) for n in range(25)]


def _scenarios():
    up = TR.link_up  # (node, ifName) of a grid link
    scs = [{"links": [up(a, b)]} for a, b in ((12, 13), (12, 7), (0, 1), (6, 7), (18, 19),
                                              (21, 22), (3, 8), (10, 15))]
    scs += [{"links": [up(0, 5), up(1, 6), up(2, 7)]}, {"links": [up(12, 11), up(12, 17)]}]
    scs += [{"nodesDown": [n]} for n in ("6", "12", "24", "0")] + [{"nodesDown": ["8", "16"]}]
    scs += [{"nodesDrained": [n]} for n in ("6", "13", "0", "22", "11")]
    scs += [{"linkMetrics": [up(a, b) + (36,), up(b, a) + (36,)]}
            for a, b in ((12, 13), (1, 2), (15, 20), (8, 9), (16, 17), (5, 10), (23, 24))]
    scs += [{"linkMetrics": [up(a, b) + (1,), up(b, a) + (1,)]}
            for a, b in ((12, 13), (0, 5), (19, 24), (6, 7), (14, 19), (3, 4))]
    scs += [{"nodesSoftDrained": [(n, 50)]} for n in ("12", "6", "18", "4", "20")]
    scs += TR.GRID  # the restoring kinds, singly and mixed
    scs += [{}]
    return scs


@functools.lru_cache(maxsize=None)
def grid_case(oracle):
    """(world, scenarios, answers[s][k] or None for a source that is down)"""
    w, scs = TR.grid_world(True), _scenarios()
    assert 55 <= len(scs) <= 65
    answers = []
    for s in SOURCES:
        o = W.Oracle(oracle, w, s, True, False)
        answers.append([None if s in sc.get("nodesDown", ()) else o.answer(sc) for sc in scs])
    return w, scs, answers


class Source:
    """one source of a NetworkWhatifSweep behind LinkFailureSweep's accessors"""

    def __init__(self, net, s):
        self.net, self.s = net, s

    def routeUpdate(self, k):
        return self.net.routeUpdate(self.s, k)

    def updatedCanonical(self, k):
        return self.net.updatedCanonical(self.s, k)

    def counts(self, k):
        return self.net.counts(self.s, k)

    def changedPrefixes(self, k):
        return self.net.changedPrefixes(self.s, k)


def nonempty(a):
    return bool(a[0]["unicastRoutesToUpdate"] or a[0]["unicastRoutesToDelete"])


def check_network(product, net, answers, label):
    """after launch + fetchUpdates"""
    S_, K = len(answers), len(answers[0])
    assert (net.numSources(), net.numScenarios()) == (S_, K)
    for s in range(S_):
        live = [k for k in range(K) if answers[s][k] is not None]
        assert [net.state(s, k) for k in range(K)] == [
            product.kComputed if k in live else product.kSourceDown for k in range(K)]
        W.check_sweep(Source(net, s), [answers[s][k] for k in live], (label, s), live)
        for k in set(range(K)) - set(live):  # that node runs no Decision
            assert tuple(net.counts(s, k)) == (0, 0)
            with pytest.raises(ValueError, match="runs no Decision"):
                net.routeUpdate(s, k)
    check_impact(net, answers, label)


def check_impact(net, answers, label):
    """after any fetch: the counts and who is affected"""
    S_, K = len(answers), len(answers[0])
    for k in range(K):
        for s in range(S_):
            a = answers[s][k]
            want = (0, 0) if a is None else (len(a[0]["unicastRoutesToUpdate"]),
                                             len(a[0]["unicastRoutesToDelete"]))
            assert tuple(net.counts(s, k)) == want, (label, s, k)
        assert net.affectedSources(k) == [s for s in range(S_) if answers[s][k] is not None and
                                          nonempty(answers[s][k])], (label, k)


def test_grid_mix(oracle):
    """the oracle's side alone: the case cannot go vacuous"""
    w, scs, answers = grid_case(oracle)
    kinds = {W.kind_of(a[0]) for row in answers for a in row if a is not None}
    assert kinds == {"empty", "update", "delete", "mixed"}
    partial = 0
    for k in range(len(scs)):
        live = [row[k] for row in answers if row[k] is not None]
        partial += 0 < sum(nonempty(a) for a in live) < len(live)
    assert partial >= 10, partial
    down = sum(a is None for row in answers for a in row)
    assert down == 7  # each downed node as its own source (one of TR.MIXES downs "7")
    # the source itself hard-drained, soft-drained, undrained; a dead link at it
    me = SOURCES.index("12")
    for sc in ({"nodesDrained": ["13"]}, {"nodesSoftDrained": [("12", 50)]},
               {"nodesUndrained": ["12"]}, {"links": [TR.link_up(12, 13)]}):
        assert sc in scs
    # (a hard drain of the source itself moves nothing in its own RouteDb)
    assert not nonempty(answers[SOURCES.index("13")][scs.index({"nodesDrained": ["13"]})])
    assert nonempty(answers[me][scs.index({"nodesSoftDrained": [("12", 50)]})])
    assert nonempty(answers[me][scs.index({"nodesUndrained": ["12"]})])


@pytest.mark.parametrize("chunks", ["default", "small", "unit"])
def test_grid(product, oracle, chunks):
    w, scs, answers = grid_case(oracle)
    als, ls, ps = w.load(product, "12")
    net = product.NetworkWhatifSweep(ls, ps, SOURCES, scs, True, False)
    assert net.batchedSources() == 25
    if chunks == "small":
        plan = product.network_whatif_plan(ls, ps, SOURCES, scs)
        net.setChunkBytes(plan["unitBytes"] * (len(plan["pairs"]) // 5))
        assert net.numChunks() >= 4
    elif chunks == "unit":
        # one pair a chunk: chunks without a changed route among those with some
        plan = product.network_whatif_plan(ls, ps, SOURCES, scs)
        net.setChunkBytes(plan["unitBytes"])
        assert net.numChunks() == len(plan["pairs"]) >= 3
        flat = [a for row in answers for a in row if a is not None]
        assert 0 < sum(nonempty(a) for a in flat) < len(flat)
    else:
        assert net.numChunks() == 1
    net.launch()
    net.fetchUpdates()
    assert net.batchedSources() == 25  # the entry took the call
    check_network(product, net, answers, chunks)
    # the base served per source is that source's own RouteDb
    for s in (0, 4, 24):
        o = W.Oracle(oracle, w, SOURCES[s], True, False)
        assert net.baseCanonical(s) == o.base.canonical()


def test_grid_impact_only(product, oracle):
    w, scs, answers = grid_case(oracle)
    als, ls, ps = w.load(product, "12")
    net = product.NetworkWhatifSweep(ls, ps, SOURCES, scs, True, False)
    plan = product.network_whatif_plan(ls, ps, SOURCES, scs)
    net.setChunkBytes(plan["impactUnitBytes"] * (len(plan["pairs"]) // 4))
    assert net.numChunks(False) >= 4
    net.launch(records=False)
    with pytest.raises(RuntimeError):  # no records were written
        net.fetchUpdates()
    net.fetchImpact()
    check_impact(net, answers, "impact")
    with pytest.raises(RuntimeError):
        net.routeUpdate(0, 0)
    # and with records afterwards, from the same object
    net.launch()
    net.fetchUpdates()
    check_impact(net, answers, "records after impact")
    W.check_sweep(Source(net, 3), [answers[3][k] for k in (0, 30, 45)], "after impact",
                  [0, 30, 45])


def test_hub_and_ring(product, oracle):
    """a 40-spoke hub keeps two next-hop words: served by its own
    LinkFailureSweep, the spokes by the batch, both behind the same accessors"""
    w = WR.as_restore_world(S.hub_ring_world(ring=40, parallel=False, prefixes=2))
    sources = ["r0", "hub", "r7", "r20", "r39"]
    scs = [{"links": [("r0", "r0-r1/0")]}, {"nodesDown": ["hub"]}, {"nodesDrained": ["hub"]},
           {"links": [("hub", f"hub-r{i}/0") for i in range(6)]}, {"nodesDown": ["r7", "r8"]},
           {"linkMetrics": [("r20", "r20-hub/0", 90), ("hub", "hub-r20/0", 90)]},
           {"nodesSoftDrained": [("r39", 30)]}, {}]
    answers = []
    for s in sources:
        o = W.Oracle(oracle, w, s, True, False)
        answers.append([None if s in sc.get("nodesDown", ()) else o.answer(sc) for sc in scs])
    assert sum(a is None for row in answers for a in row) == 2
    assert sum(nonempty(a) for a in answers[1] if a is not None) >= 4  # the hub's own
    als, ls, ps = w.load(product, "hub")
    net = product.NetworkWhatifSweep(ls, ps, sources, scs, True, False)
    assert net.batchedSources() == 4
    net.launch()
    net.fetchUpdates()
    assert net.batchedSources() == 4
    check_network(product, net, answers, "hub-ring")
    o = W.Oracle(oracle, w, "hub", True, False)
    assert net.baseCanonical(1) == o.base.canonical()
