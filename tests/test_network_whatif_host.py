"""NetworkWhatifSweep's host side through network_whatif_plan, without a
device: the batched / fallback split, the pair order, the pairs whose source is
down, the chunk boundaries and the validation errors."""
import pytest

import test_gpu_scenarios as S
import test_gpu_whatif_metric as TM

SCS = [{"nodesSoftDrained": [("12", 50)]}, {"nodesDown": ["7"]}, {"nodesDrained": ["12"]},
       {"nodesDown": ["3", "7"]}, {}]


def _grid(host_module, zero_link=False):
    w = TM.grid_world(True, zero_link)
    als, ls, ps = w.load(host_module, "12")
    return w, als, ls, ps


def test_pair_order_and_source_down(host_module):
    w, als, ls, ps = _grid(host_module)
    sources = ["12", "7", "0", "3"]
    plan = host_module.network_whatif_plan(ls, ps, sources, SCS)
    assert plan["batched"] == [0, 1, 2, 3] and plan["fallback"] == []
    # exactly the pairs whose source is in the scenario's nodesDown
    assert sorted(plan["sourceDown"]) == [(1, 1), (1, 3), (3, 3)]
    want = [(s, k) for s in range(4) for k in range(len(SCS)) if (s, k) not in plan["sourceDown"]]
    assert plan["pairs"] == want  # source-major, scenario ascending, no unit for a down source
    assert plan["chunks"] == [0, len(want)] and plan["impactChunks"] == [0, len(want)]
    # a source named twice is two sources
    twice = host_module.network_whatif_plan(ls, ps, ["12", "12"], SCS)
    assert twice["batched"] == [0, 1] and len(twice["pairs"]) == 2 * len(SCS)
    # no scenario, no source
    assert host_module.network_whatif_plan(ls, ps, sources, [])["pairs"] == []
    none = host_module.network_whatif_plan(ls, ps, [], SCS)
    assert none["pairs"] == [] and none["chunks"] == [0]


def test_wide_hub_falls_back(host_module):
    """a 40-spoke hub keeps two next-hop words: its own sweep; the spokes batch"""
    w = S.hub_ring_world(ring=40, parallel=False, prefixes=2)
    als, ls, ps = w.load(host_module, "hub")
    sources = ["r0", "hub", "r5", "r39"]
    scs = [{"nodesDown": ["hub"]}, {"links": [("r0", "r0-r1/0")]}]
    plan = host_module.network_whatif_plan(ls, ps, sources, scs)
    assert plan["batched"] == [0, 2, 3] and plan["fallback"] == [1]
    assert plan["sourceDown"] == [(1, 0)]  # listed for a fallback source too
    assert plan["pairs"] == [(s, k) for s in (0, 2, 3) for k in (0, 1)]


def test_zero_metric_area_is_all_fallback(host_module):
    w, als, ls, ps = _grid(host_module, zero_link=True)
    plan = host_module.network_whatif_plan(ls, ps, ["12", "0"], SCS)
    assert plan["batched"] == [] and plan["fallback"] == [0, 1] and plan["pairs"] == []
    # and so is an area whose scenarios carry a weight of the exact domain
    w, als, ls, ps = _grid(host_module)
    ifn = [a["ifName"] for a in w.adjdbs["12"]["adjacencies"] if a["otherNodeName"] == "13"][0]
    ofn = [a["ifName"] for a in w.adjdbs["13"]["adjacencies"] if a["otherNodeName"] == "12"][0]
    zero = [{"linkMetrics": [("12", ifn, 0), ("13", ofn, 0)]}]
    plan = host_module.network_whatif_plan(ls, ps, ["12", "0"], zero)
    assert plan["batched"] == []
    assert host_module.network_whatif_plan(ls, ps, ["12", "0"], SCS)["batched"] == [0, 1]


def test_chunks(host_module):
    w, als, ls, ps = _grid(host_module)
    sources = [str(n) for n in range(25)]
    plan = host_module.network_whatif_plan(ls, ps, sources, SCS)
    U = len(plan["pairs"])
    assert U == 25 * len(SCS) - 3
    Sp = 25 * TM.PER_NODE  # + the anycast extras
    assert plan["unitBytes"] >= 12 * Sp and plan["impactUnitBytes"] < plan["unitBytes"] // 50
    for units in (1, 3, 7):
        p = host_module.network_whatif_plan(ls, ps, sources, SCS,
                                            units * plan["unitBytes"] + 5)
        c = p["chunks"]
        assert c[0] == 0 and c[-1] == U and c == sorted(set(c))  # every unit once
        assert all(b - a == units for a, b in zip(c[:-2], c[1:-1]))
        assert 0 < c[-1] - c[-2] <= units
        # impact-only units are smaller: a chunk holds correspondingly more
        per = (units * plan["unitBytes"] + 5) // plan["impactUnitBytes"]
        ic = p["impactChunks"]
        assert ic[0] == 0 and ic[-1] == U and all(b - a <= per for a, b in zip(ic, ic[1:]))
        assert len(ic) < len(c)
    # a bound below one unit still makes progress: one unit a chunk
    assert host_module.network_whatif_plan(ls, ps, sources, SCS, 1)["chunks"] == list(range(U + 1))


def test_validation(host_module):
    w, als, ls, ps = _grid(host_module)
    plan = host_module.network_whatif_plan
    with pytest.raises(ValueError, match="not in area"):
        plan(ls, ps, ["12", "nobody"], SCS)
    with pytest.raises(ValueError, match="unknown node"):
        plan(ls, ps, ["12"], [{"nodesDown": ["nobody"]}])
    with pytest.raises(ValueError, match="no link"):
        plan(ls, ps, ["12"], [{"links": [("12", "no-such-if")]}])
    with pytest.raises(ValueError, match="both down and drained"):
        plan(ls, ps, ["12"], [{"nodesDown": ["7"], "nodesDrained": ["7"]}])
