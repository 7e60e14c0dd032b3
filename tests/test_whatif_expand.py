"""expand_whatif (LinkFailureSweep::expandScenario with linkMetrics and
nodesSoftDrained) on a hand-built world, host only: the directed edges whose
weight moves, as (node, neighbour, ifName, weight) in edge-id order, and the
flag bits a scenario adds per node.

The world: a square a - b - c - d - a with a parallel link beside a - b, a
link c - e that is down already (overloaded at one end) and a node f, already
overloaded, hanging off c. Every adjacency sends metric 5 but b -> a on the
first a - b link, which sends 9 (that link's weight is 9), and d, which
carries nodeMetricIncrementVal 2 and so sends 7."""
import pytest

import lsdb as L

A = L.kTestingAreaName
OVERLOADED, SOFTDRAIN, METRICINC = 1, 2, 4

LINKS = [("a", "b", 0), ("a", "b", 1), ("b", "c", 0), ("c", "d", 0), ("d", "a", 0), ("c", "e", 0),
         ("c", "f", 0)]


def _adj(a, b, k):
    metric = 9 if (a, b, k) == ("b", "a", 0) else 7 if a == "d" else 5
    adj = L.createAdjacency(b, f"{a}-{b}/{k}", f"{b}-{a}/{k}", "fe80::1", "192.168.0.1", metric, 7)
    adj["isOverloaded"] = (a, b) == ("c", "e")
    return adj


@pytest.fixture(scope="module")
def world(host_module):
    M = host_module
    als = M.AreaLinkStates()
    ls = als.add(A, "a")
    for i, n in enumerate("abcdef"):
        adjs = [_adj(n, y if n == x else x, k) for x, y, k in LINKS if n in (x, y)]
        ls.updateAdjacencyDatabase(
            L.createAdjDb(n, adjs, i + 1, overLoadBit=n == "f",
                          nodeMetricIncrementVal=2 if n == "d" else 0), A)
    return M, als, ls


def both(a, b, w, k=0):
    return [(a, b, f"{a}-{b}/{k}", w), (b, a, f"{b}-{a}/{k}", w)]


def expand(world, **sc):
    M, _, ls = world
    return M.expand_whatif(ls, "a", sc)


def test_weight_is_the_max_of_both_directions(world):
    # the lower direction raised past the higher one: both directed edges move
    x = expand(world, linkMetrics=[("a", "a-b/0", 12)])
    assert sorted(x["metrics"]) == sorted(both("a", "b", 12))
    assert x["dead"] == [] and x["flags"] == [] and x["drained"] == []
    # the higher direction lowered: the other direction holds the weight at 5
    assert sorted(expand(world, linkMetrics=[("b", "b-a/0", 1)])["metrics"]) == sorted(
        both("a", "b", 5))
    # both lowered
    x = expand(world, linkMetrics=[("b", "b-a/0", 1), ("a", "a-b/0", 2)])
    assert sorted(x["metrics"]) == sorted(both("a", "b", 2))
    # the parallel link is a link of its own
    assert sorted(expand(world, linkMetrics=[("b", "b-a/1", 6)])["metrics"]) == sorted(
        both("a", "b", 6, 1))


def test_no_ops_fold(world):
    for lm in ([("a", "a-b/0", 7)],      # raised below the higher direction
               [("a", "a-b/0", 9)],      # ... up to it
               [("b", "b-a/0", 9)],      # the metric it sends already
               [("c", "c-e/0", 50)],     # a link that is down
               [("e", "e-c/0", 50)],     # ... named from its other end
               []):
        x = expand(world, linkMetrics=lm)
        assert x["metrics"] == [] and x["metricEdges"] == [], lm
    # named twice: the last value of an adjacency stands
    assert expand(world, linkMetrics=[("a", "a-b/0", 50), ("a", "a-b/0", 5)])["metrics"] == []


def test_dead_wins(world):
    x = expand(world, links=[("b", "b-a/0")], linkMetrics=[("a", "a-b/0", 50), ("b", "b-c/0", 8)])
    assert len(x["dead"]) == 2
    assert sorted(x["metrics"]) == sorted(both("b", "c", 8))
    x = expand(world, nodesDown=["b"], linkMetrics=[("a", "a-b/0", 50), ("c", "c-d/0", 8)])
    assert len(x["dead"]) == 6
    assert sorted(x["metrics"]) == sorted(both("c", "d", 8))


def test_sorted_without_duplicates(world):
    x = expand(world, linkMetrics=[("d", "d-a/0", 30), ("c", "c-b/0", 20), ("a", "a-d/0", 31),
                                   ("b", "b-a/1", 6), ("a", "a-b/0", 12)])
    ids = x["metricEdges"]
    assert len(ids) == 8 and ids == sorted(set(ids))
    assert sorted(x["metrics"]) == sorted(both("a", "b", 12) + both("a", "b", 6, 1) +
                                          both("b", "c", 20) + both("a", "d", 31))
    # "metrics" comes in edge-id order: rows by node name
    assert [m[0] for m in x["metrics"]] == sorted(m[0] for m in x["metrics"])


def test_soft_drain_edges_and_flags(world):
    # every up link of the node, the max of both directions, and the two bits
    x = expand(world, nodesSoftDrained=[("b", 100)])
    assert sorted(x["metrics"]) == sorted(both("a", "b", 109) + both("a", "b", 105, 1) +
                                          both("b", "c", 105))
    assert x["flags"] == [("b", SOFTDRAIN | METRICINC)] and x["drained"] == []
    # c: its link to e is down and stays out; the source itself may be
    # soft-drained, and its links whose other direction is higher stay (no-ops)
    x = expand(world, nodesSoftDrained=[("c", 10), ("a", 1)])
    assert sorted(x["metrics"]) == sorted(both("b", "c", 15) + both("c", "d", 15) +
                                          both("c", "f", 15) + both("a", "b", 6, 1))
    assert x["flags"] == [("a", SOFTDRAIN | METRICINC), ("c", SOFTDRAIN | METRICINC)]
    # d carries 2 already: published - 2 + increment; its bits are set already
    x = expand(world, nodesSoftDrained=[("d", 2)])
    assert x["metrics"] == [] and x["flags"] == []
    x = expand(world, nodesSoftDrained=[("d", 10)])
    assert sorted(x["metrics"]) == sorted(both("c", "d", 15) + both("a", "d", 15))
    assert x["flags"] == []
    # the scenario's own override first, the increment on top; a hard drain beside it
    x = expand(world, nodesSoftDrained=[("b", 3), ("b", 3)], linkMetrics=[("b", "b-c/0", 20)],
               nodesDrained=["b", "f"])
    assert sorted(x["metrics"]) == sorted(both("a", "b", 12) + both("a", "b", 8, 1) +
                                          both("b", "c", 23))
    assert x["flags"] == [("b", OVERLOADED | SOFTDRAIN | METRICINC)] and x["drained"] == ["b"]
    # expand_scenario keeps its two lists
    M, _, ls = world
    assert M.expand_scenario(ls, "a", {"nodesSoftDrained": [("b", 3)]}) == ([], [])


@pytest.mark.parametrize("sc", [
    {"linkMetrics": [("zz", "zz-a/0", 5)]},
    {"linkMetrics": [("a", "a-c/0", 5)]},
    {"linkMetrics": [("a", "a-b/0", 1 << 31)]},
    {"nodesSoftDrained": [("zz", 5)]},
    {"nodesSoftDrained": [("b", 0)]},
    {"nodesSoftDrained": [("b", -4)]},
    {"nodesSoftDrained": [("b", 1 << 31)]},
    {"nodesSoftDrained": [("b", 5), ("b", 6)]},
    {"nodesSoftDrained": [("b", 5)], "nodesDown": ["b"]},
], ids=["unknown node", "unknown link", "metric past i32", "soft: unknown node", "increment 0",
        "increment < 0", "increment past i32", "two increments", "down and soft-drained"])
def test_invalid_arguments(world, sc):
    M, _, ls = world
    with pytest.raises(ValueError):
        M.expand_whatif(ls, "a", sc)
