"""expand_scenario (LinkFailureSweep::expandScenario) on a hand-built world,
host only: what a scenario removes as sorted dead directed edges
(node, neighbour, ifName) and drained node names.

The world: a square a - b - c - d - a with a parallel link beside a - b, a
spur d - e, a link c - e that is down already (overloaded at one end) and a
node f, already overloaded, hanging off c."""
import pytest

import lsdb as L

A = L.kTestingAreaName


def _adj(a, b, k=0, over=False):
    adj = L.createAdjacency(b, f"{a}-{b}/{k}", f"{b}-{a}/{k}", "fe80::1", "192.168.0.1", 5, 7)
    adj["isOverloaded"] = over
    return adj


LINKS = [("a", "b", 0), ("a", "b", 1), ("b", "c", 0), ("c", "d", 0), ("d", "a", 0), ("d", "e", 0),
         ("c", "e", 0), ("c", "f", 0)]


@pytest.fixture(scope="module")
def world(host_module):
    M = host_module
    als = M.AreaLinkStates()
    ls = als.add(A, "a")
    for i, n in enumerate("abcdef"):
        adjs = []
        for x, y, k in LINKS:
            if n in (x, y):
                other = y if n == x else x
                adjs.append(_adj(n, other, k, over=(n, other) == ("c", "e")))
        ls.updateAdjacencyDatabase(L.createAdjDb(n, adjs, i + 1, overLoadBit=n == "f"), A)
    return M, als, ls


def both(a, b, k=0):
    return [(a, b, f"{a}-{b}/{k}"), (b, a, f"{b}-{a}/{k}")]


def test_node_down_is_every_edge_out_and_in(world):
    M, _, ls = world
    dead, drained = M.expand_scenario(ls, "a", {"nodesDown": ["d"]})
    assert drained == []
    assert len(dead) == 2 * 3  # degree 3
    assert dead == sorted(both("d", "c") + both("d", "a") + both("d", "e"))
    # c has four links, one of them down already: a no-op, left out
    dead, _ = M.expand_scenario(ls, "a", {"nodesDown": ["c"]})
    assert dead == sorted(both("c", "b") + both("c", "d") + both("c", "f"))


def test_duplicates_fold(world):
    M, _, ls = world
    one, _ = M.expand_scenario(ls, "a", {"links": [("c", "c-d/0")]})
    assert one == sorted(both("c", "d"))
    # the same link from either end, twice, and as a link of a downed node
    for sc in ({"links": [("c", "c-d/0"), ("d", "d-c/0")]},
               {"links": [("c", "c-d/0"), ("c", "c-d/0")]}):
        assert M.expand_scenario(ls, "a", sc)[0] == one
    dead, _ = M.expand_scenario(ls, "a", {"links": [("c", "c-d/0")], "nodesDown": ["d"]})
    assert dead == M.expand_scenario(ls, "a", {"nodesDown": ["d"]})[0]
    _, drained = M.expand_scenario(ls, "a", {"nodesDrained": ["b", "e", "b"]})
    assert drained == ["b", "e"]


def test_parallel_link_is_taken_alone(world):
    M, _, ls = world
    dead, _ = M.expand_scenario(ls, "a", {"links": [("a", "a-b/1")]})
    assert dead == sorted(both("a", "b", 1))
    dead, _ = M.expand_scenario(ls, "a", {"links": [("b", "b-a/0")]})
    assert dead == sorted(both("a", "b", 0))
    dead, _ = M.expand_scenario(ls, "a", {"links": [("a", "a-b/1"), ("a", "a-b/0")]})
    assert dead == sorted(both("a", "b", 0) + both("a", "b", 1))


def test_no_ops(world):
    M, _, ls = world
    # a link already down, a node already overloaded, the empty scenario
    assert M.expand_scenario(ls, "a", {"links": [("e", "e-c/0")]}) == ([], [])
    assert M.expand_scenario(ls, "a", {"nodesDrained": ["f"]}) == ([], [])
    assert M.expand_scenario(ls, "a", {}) == ([], [])
    # the source may be drained, and may lose links
    assert M.expand_scenario(ls, "a", {"nodesDrained": ["a"]}) == ([], ["a"])


@pytest.mark.parametrize("sc", [
    {"links": [("zz", "zz-a/0")]}, {"links": [("a", "a-c/0")]}, {"nodesDown": ["zz"]},
    {"nodesDrained": ["zz"]}, {"nodesDown": ["a"]}, {"nodesDown": ["d"], "nodesDrained": ["d"]},
], ids=["unknown link node", "unknown link", "unknown node down", "unknown node drained",
        "me down", "down and drained"])
def test_invalid_arguments(world, sc):
    M, _, ls = world
    with pytest.raises(ValueError):
        M.expand_scenario(ls, "a", sc)
