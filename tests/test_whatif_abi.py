"""ogs_spf_routes_whatif (include/openr_gpu.h) at the boundary, without a
device: the header declares the entry, its context twin, ogs_whatif_mods and
OGS_WHATIF_REFUSED, the library exports them, the ABI version is still 8 (the
entry is additive, ogs_scenario_mods keeps its layout) and every bad-argument
call fails before any launch. The rules the entry shares with
ogs_spf_routes_scenarios are made as the same broken call on both entries and
must return the same status (the pointers below are never followed: X is just
"not NULL")."""
import ctypes
import re

import pytest

import test_scenarios_abi as S

X, OK, E_INVALID, E_UNSUPPORTED = S.X, S.OK, S.E_INVALID, S.E_UNSUPPORTED


def _mods(capi, dead=(X, X), nodes=(None, None, None), metrics=(None, None, None), longest=0):
    return capi.WhatifMods(*dead, *nodes, *metrics, longest)


def test_header_declares_and_library_exports():
    capi, lib = S._lib()
    with open(S.os.path.join(S.ROOT, "include", "openr_gpu.h")) as f:
        header = f.read()
    for name in ("ogs_spf_routes_whatif", "ogs_ctx_spf_routes_whatif"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS
        assert hasattr(lib, name)
    assert re.search(r"typedef struct ogs_whatif_mods \{[^}]*dead_off[^}]*dead_edges[^}]*"
                     r"node_off[^}]*node_ids[^}]*node_bits[^}]*metric_off[^}]*metric_edges[^}]*"
                     r"metric_vals[^}]*max_metric_per_unit[^}]*\} ogs_whatif_mods;", header)
    assert re.search(r"#define\s+OGS_WHATIF_REFUSED\s+0xFFFFFFFFu", header)
    assert capi.OGS_WHATIF_REFUSED == 0xFFFFFFFF
    assert re.search(r"#define\s+OGS_ABI_VERSION\s+8\b", header)
    assert capi.OGS_ABI_VERSION == 8 and lib.ogs_abi_version() == 8
    # the entry cites what each new scenario kind stands for in the reference
    for cite in ("LinkMonitor.cpp:1003-1006", "LinkMonitor.cpp:971-1001", "SpfSolver.cpp:511-551",
                 "LinkState.h:171-174"):
        assert cite in header
    # ogs_scenario_mods keeps its four fields, in order
    assert re.search(r"typedef struct ogs_scenario_mods \{\s*const uint32_t\* dead_off;[^;]*"
                     r"const uint32_t\* dead_edges;[^;]*const uint32_t\* drain_off;[^;]*"
                     r"const uint32_t\* drain_nodes;[^;}]*\} ogs_scenario_mods;", header)
    # the ctypes struct mirrors the C layout: 8 pointers and a u32
    assert ctypes.sizeof(capi.WhatifMods) == 8 * ctypes.sizeof(ctypes.c_void_p) + 8
    assert capi.WhatifMods.max_metric_per_unit.offset == 8 * ctypes.sizeof(ctypes.c_void_p)


@pytest.mark.parametrize("label,status,over", S.SHARED, ids=[c[0] for c in S.SHARED])
def test_shared_rules_return_the_scenarios_status(label, status, over):
    capi, lib = S._lib()
    got = S._call(lib, "ogs_spf_routes_whatif", _mods(capi), S._args(capi, **over))
    ref = S._call(lib, "ogs_spf_routes_scenarios", capi.ScenarioMods(X, X, None, None),
                  S._args(capi, **over))
    assert (got, ref) == (status, status)


def test_whatif_rules():
    capi, lib = S._lib()

    def call(mods, **over):
        return S._call(lib, "ogs_spf_routes_whatif", mods, S._args(capi, **over))

    assert call(None) == E_INVALID
    assert b"NULL" in lib.ogs_last_error()
    assert call(_mods(capi, dead=(None, X))) == E_INVALID
    assert call(_mods(capi, dead=(X, None))) == E_INVALID
    # the node and the metric lists come as whole triples
    for k in range(3):
        for full in (False, True):
            part = tuple((X if full else None) if i != k else (None if full else X)
                         for i in range(3))
            assert call(_mods(capi, nodes=part)) == E_INVALID, part
            assert b"node_off" in lib.ogs_last_error()
            assert call(_mods(capi, metrics=part, longest=4)) == E_INVALID, part
            assert b"metric_off" in lib.ogs_last_error()
    # n_units == 0 with nothing else set
    assert call(None, n=0, units=None, diff=None) == OK
    # node bits run in the base SPF's repair only: a call with node bits that
    # it cannot take (a full recompute, two-word sets, its LDS budget) is
    # refused with nothing launched, as the scenarios entry refuses drains
    nodes = _mods(capi, nodes=(X, X, X))
    drains = capi.ScenarioMods(X, X, X, X)
    for over in (dict(flags=0), dict(W=2), {"graph.max_nodes": 12000}):
        assert call(nodes, **over) == E_UNSUPPORTED, over
        assert b"node bits" in lib.ogs_last_error()
        assert S._call(lib, "ogs_spf_routes_scenarios", drains,
                       S._args(capi, **over)) == E_UNSUPPORTED
    # bitsets no form's LDS holds (2^22 edges), and a metric slice that does
    # not fit beside them (slices past 2^14 entries, 128 kB, are never sized)
    assert call(_mods(capi), **{"graph.max_edges": 1 << 22}) == E_UNSUPPORTED
    assert b"bitsets" in lib.ogs_last_error()
    for longest in ((1 << 14) + 1, 0xFFFFFFFF):
        assert call(_mods(capi, metrics=(X, X, X), longest=longest)) == E_UNSUPPORTED, longest
        assert call(_mods(capi, metrics=(X, X, X), longest=longest), flags=0) == E_UNSUPPORTED
    # the context twin reaches the same checks (a NULL context is refused)
    assert lib.ogs_ctx_spf_routes_whatif(None, None, None, None, 4, None, None, 0, 1, None,
                                         None) == E_INVALID
