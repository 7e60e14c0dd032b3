"""expand_whatif (LinkFailureSweep::expandScenario) over the restoring kinds --
linksUndrained, nodesUndrained, nodesSoftUndrained -- on a hand-built world,
host only: the revived directed edges as (node, neighbour, ifName, weight) in
edge-id order and the flag bits a scenario takes off per node.

The world is test_whatif_expand's with one more link: a square a - b - c - d - a
with a parallel link beside a - b, a link c - e that is down (overloaded at c's
end only), a link d - e that is down (overloaded at BOTH ends) and a node f,
already overloaded, hanging off c. Every adjacency sends metric 5 but b -> a on
the first a - b link, which sends 9, and d, which carries
nodeMetricIncrementVal 2 and so sends 7."""
import pytest

import lsdb as L

A = L.kTestingAreaName
OVERLOADED, SOFTDRAIN, METRICINC = 1, 2, 4

LINKS = [("a", "b", 0), ("a", "b", 1), ("b", "c", 0), ("c", "d", 0), ("d", "a", 0), ("c", "e", 0),
         ("c", "f", 0), ("d", "e", 0)]
ADJ_OVER = {("c", "e"), ("d", "e"), ("e", "d")}


def _adj(a, b, k):
    metric = 9 if (a, b, k) == ("b", "a", 0) else 7 if a == "d" else 5
    adj = L.createAdjacency(b, f"{a}-{b}/{k}", f"{b}-{a}/{k}", "fe80::1", "192.168.0.1", metric, 7)
    adj["isOverloaded"] = (a, b) in ADJ_OVER
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


def nothing(x):
    return (x["revived"] == [] and x["revivedEdges"] == [] and x["cleared"] == [] and
            x["metrics"] == [] and x["flags"] == [] and x["dead"] == [] and x["drained"] == [])


def test_one_end_overloaded(world):
    x = expand(world, linksUndrained=[("c", "c-e/0")])
    assert sorted(x["revived"]) == sorted(both("c", "e", 5))
    assert len(x["revivedEdges"]) == 2 and x["revivedEdges"] == sorted(x["revivedEdges"])
    assert x["metrics"] == [] and x["cleared"] == [] and x["flags"] == [] and x["dead"] == []
    # named twice: once
    assert expand(world, linksUndrained=[("c", "c-e/0"), ("c", "c-e/0")]) == x
    # named from the end that is not overloaded: c's bit stays, the link stays down
    assert nothing(expand(world, linksUndrained=[("e", "e-c/0")]))
    # ... from both ends: as from c's
    assert expand(world, linksUndrained=[("e", "e-c/0"), ("c", "c-e/0")])["revived"] == x["revived"]


def test_both_ends_overloaded(world):
    assert nothing(expand(world, linksUndrained=[("d", "d-e/0")]))
    assert nothing(expand(world, linksUndrained=[("e", "e-d/0")]))
    # d sends 7, e sends 5: the link's weight is their max
    x = expand(world, linksUndrained=[("d", "d-e/0"), ("e", "e-d/0")])
    assert sorted(x["revived"]) == sorted(both("d", "e", 7))
    both_links = expand(world, linksUndrained=[("d", "d-e/0"), ("e", "e-d/0"), ("c", "c-e/0")])
    assert sorted(both_links["revived"]) == sorted(both("d", "e", 7) + both("c", "e", 5))
    ids = both_links["revivedEdges"]
    assert len(ids) == 4 and ids == sorted(set(ids))
    assert [m[0] for m in both_links["revived"]] == sorted(m[0] for m in both_links["revived"])


def test_revived_link_with_a_metric(world):
    x = expand(world, linksUndrained=[("c", "c-e/0")], linkMetrics=[("e", "e-c/0", 11)])
    assert sorted(x["revived"]) == sorted(both("c", "e", 11)) and x["metrics"] == []
    # a metric alone leaves a down link out, as before
    assert nothing(expand(world, linkMetrics=[("e", "e-c/0", 11)]))
    # the lower direction moved below the other: the weight stays their max
    x = expand(world, linksUndrained=[("c", "c-e/0")], linkMetrics=[("e", "e-c/0", 2)])
    assert sorted(x["revived"]) == sorted(both("c", "e", 5))
    # an up link's override rides beside a revival
    x = expand(world, linksUndrained=[("c", "c-e/0")], linkMetrics=[("b", "b-c/0", 8)])
    assert sorted(x["revived"]) == sorted(both("c", "e", 5))
    assert sorted(x["metrics"]) == sorted(both("b", "c", 8))


def test_no_ops(world):
    for sc in (dict(linksUndrained=[("a", "a-b/0")]),      # up already
               dict(linksUndrained=[("b", "b-a/1")]),
               dict(nodesUndrained=["b"]),                 # not overloaded
               dict(nodesUndrained=["a"]),                 # the source may be named
               dict(nodesSoftUndrained=["b"]),             # increment 0
               dict(nodesSoftUndrained=["a", "c"]),
               dict(linksUndrained=[], nodesUndrained=[], nodesSoftUndrained=[])):
        assert nothing(expand(world, **sc)), sc


def test_node_undrain(world):
    x = expand(world, nodesUndrained=["f"])
    assert x["cleared"] == [("f", OVERLOADED)]
    assert x["revived"] == [] and x["metrics"] == [] and x["flags"] == [] and x["drained"] == []
    assert expand(world, nodesUndrained=["f", "b", "f"])["cleared"] == [("f", OVERLOADED)]
    # beside a drain and a soft drain of other nodes
    x = expand(world, nodesUndrained=["f"], nodesDrained=["b"], nodesSoftDrained=[("c", 10)])
    assert x["cleared"] == [("f", OVERLOADED)] and x["drained"] == ["b"]
    assert x["flags"] == [("b", OVERLOADED), ("c", SOFTDRAIN | METRICINC)]


def test_soft_undrain(world):
    # d sends 7 = 5 + its increment of 2: both its up links fall back to 5
    x = expand(world, nodesSoftUndrained=["d"])
    assert sorted(x["metrics"]) == sorted(both("c", "d", 5) + both("a", "d", 5))
    assert x["cleared"] == [("d", SOFTDRAIN | METRICINC)]
    assert x["revived"] == [] and x["flags"] == []
    assert expand(world, nodesSoftUndrained=["d", "d"]) == x
    # the scenario's own override first, the increment taken off after it
    x = expand(world, nodesSoftUndrained=["d"], linkMetrics=[("d", "d-c/0", 20)])
    assert sorted(x["metrics"]) == sorted(both("c", "d", 18) + both("a", "d", 5))
    # with its down link revived: that link's weight is lowered too
    x = expand(world, nodesSoftUndrained=["d"], linksUndrained=[("d", "d-e/0"), ("e", "e-d/0")])
    assert sorted(x["revived"]) == sorted(both("d", "e", 5))
    assert sorted(x["metrics"]) == sorted(both("c", "d", 5) + both("a", "d", 5))
    # a cleared and a set bit of different nodes; a node undrained and soft-undrained
    x = expand(world, nodesSoftUndrained=["d"], nodesSoftDrained=[("b", 3)], nodesUndrained=["f"])
    assert x["cleared"] == [("d", SOFTDRAIN | METRICINC), ("f", OVERLOADED)]
    assert x["flags"] == [("b", SOFTDRAIN | METRICINC)]


def test_downed_node_keeps_its_links_withdrawn(world):
    # c - e is revived from c's end; with e down it stays withdrawn (it was not
    # up, so it is not in the dead list either)
    x = expand(world, linksUndrained=[("c", "c-e/0")], nodesDown=["e"])
    assert x["revived"] == [] and x["dead"] == []


@pytest.mark.parametrize("sc", [
    {"linksUndrained": [("zz", "zz-a/0")]},
    {"linksUndrained": [("a", "a-c/0")]},
    {"nodesUndrained": ["zz"]},
    {"nodesSoftUndrained": ["zz"]},
    {"nodesDown": ["c"], "linksUndrained": [("c", "c-e/0")]},
    {"nodesDown": ["f"], "nodesUndrained": ["f"]},
    {"nodesDown": ["d"], "nodesSoftUndrained": ["d"]},
    {"nodesDrained": ["f"], "nodesUndrained": ["f"]},
    {"nodesDrained": ["b"], "nodesUndrained": ["b"]},
    {"nodesSoftDrained": [("d", 9)], "nodesSoftUndrained": ["d"]},
    {"links": [("c", "c-e/0")], "linksUndrained": [("c", "c-e/0")]},
    {"links": [("e", "e-c/0")], "linksUndrained": [("c", "c-e/0")]},
    {"links": [("a", "a-b/0")], "linksUndrained": [("b", "b-a/0")]},
], ids=["link: unknown node", "unknown link", "undrain: unknown node", "soft: unknown node",
        "down and link undrained", "down and undrained", "down and soft-undrained",
        "drained and undrained", "drained and undrained (no-op pair)",
        "soft-drained and soft-undrained", "link down and undrained", "... by the other end",
        "... an up link"])
def test_invalid_arguments(world, sc):
    M, _, ls = world
    with pytest.raises(ValueError):
        M.expand_whatif(ls, "a", sc)
