"""ogs_spf_routes_whatif_pairs (include/openr_gpu.h) at the boundary, without
a device: the header declares the entry, its context twin and ogs_whatif_pairs,
the library exports them, the ABI version is still 8 (the entry is additive)
and every bad-argument call fails before any launch. The rules the entry shares
with ogs_spf_routes_whatif are made as the same broken call on both entries and
must return the same status (the pointers below are never followed: X is just
"not NULL")."""
import ctypes
import re

import pytest

import test_scenarios_abi as S
import test_whatif_abi as WA

X, OK, E_INVALID, E_UNSUPPORTED = S.X, S.OK, S.E_INVALID, S.E_UNSUPPORTED
ENTRY = "ogs_spf_routes_whatif_pairs"


def _pairs(capi, base=X, scenario=X, n_bases=3, n_scenarios=5):
    return capi.WhatifPairs(base, scenario, n_bases, n_scenarios)


def _call(lib, pairs, mods, a):
    return getattr(lib, ENTRY)(S._ref(a["graph"]), S._ref(a["table"]), a["units"], a["n"],
                               S._ref(pairs), S._ref(mods), S._ref(a["diff"]), a["flags"], a["W"],
                               S._ref(a["out"]), None)


def test_header_declares_and_library_exports():
    capi, lib = S._lib()
    with open(S.os.path.join(S.ROOT, "include", "openr_gpu.h")) as f:
        header = f.read()
    for name in (ENTRY, "ogs_ctx_spf_routes_whatif_pairs"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS
        assert hasattr(lib, name)
    # the struct's four fields, in order
    assert re.search(r"typedef struct ogs_whatif_pairs \{\s*const uint32_t\* base;[^;]*"
                     r"const uint32_t\* scenario;[^;]*int32_t n_bases;[^;]*"
                     r"int32_t n_scenarios;[^;}]*\} ogs_whatif_pairs;", header)
    assert re.search(r"#define\s+OGS_ABI_VERSION\s+8\b", header)
    assert capi.OGS_ABI_VERSION == 8 and lib.ogs_abi_version() == 8
    assert ctypes.sizeof(capi.WhatifPairs) == 2 * ctypes.sizeof(ctypes.c_void_p) + 8
    assert [f[0] for f in capi.WhatifPairs._fields_] == ["base", "scenario", "n_bases",
                                                         "n_scenarios"]
    # the comment of the entry cites what the per-node answer stands for
    comment = header[header.index("ogs_spf_routes_whatif over (source, scenario) PAIRS"):
                     header.index("typedef struct ogs_whatif_pairs")]
    for cite in ("Decision.cpp:341-360", "SpfSolver.cpp:21-56", "LinkState.cpp:491-634",
                 "LinkMonitor.cpp:1003-1006", "SpfSolver.cpp:511-551"):
        assert cite in comment, cite
    for word in ("OGS_F_INCREMENTAL", "nh_words == 1", "base_desc", "OGS_E_UNSUPPORTED",
                 "OGS_E_INVALID", "REFUSED"):
        assert word in comment, word


@pytest.mark.parametrize("label,status,over", S.SHARED, ids=[c[0] for c in S.SHARED])
def test_shared_rules_return_the_whatif_status(label, status, over):
    capi, lib = S._lib()
    got = _call(lib, _pairs(capi), WA._mods(capi), S._args(capi, **over))
    ref = S._call(lib, "ogs_spf_routes_whatif", WA._mods(capi), S._args(capi, **over))
    assert (got, ref) == (status, status)


def test_shared_mods_rules():
    """mods NULL and incomplete triples: the same status on both entries"""
    capi, lib = S._lib()
    cases = [None, WA._mods(capi, dead=(None, X)), WA._mods(capi, dead=(X, None)),
             WA._mods(capi, nodes=(X, None, X)), WA._mods(capi, metrics=(X, X, None), longest=4)]
    for mods in cases:
        got = _call(lib, _pairs(capi), mods, S._args(capi))
        ref = S._call(lib, "ogs_spf_routes_whatif", mods, S._args(capi))
        assert (got, ref) == (E_INVALID, E_INVALID)


def test_pairs_rules():
    capi, lib = S._lib()

    def call(pairs, mods=None, **over):
        return _call(lib, pairs, mods or WA._mods(capi), S._args(capi, **over))

    assert call(None) == E_INVALID
    assert b"pairs" in lib.ogs_last_error()
    assert call(_pairs(capi, base=None)) == E_INVALID
    assert call(_pairs(capi, scenario=None)) == E_INVALID
    assert call(_pairs(capi, n_bases=0)) == E_INVALID
    assert b"n_bases" in lib.ogs_last_error()
    assert call(_pairs(capi, n_bases=-1)) == E_INVALID
    assert call(_pairs(capi, n_scenarios=-1)) == E_INVALID
    # the entry runs only as the repair: no full-frontier form behind it
    nodes = WA._mods(capi, nodes=(X, X, X))
    for over in (dict(flags=0), dict(W=2), {"graph.max_nodes": 70000},
                 {"graph.max_edges": 1 << 22}):
        for mods in (None, nodes):
            assert call(_pairs(capi), mods, **over) == E_UNSUPPORTED, over
    assert call(_pairs(capi), **{"graph.max_nodes": 12000}) == E_UNSUPPORTED  # the LDS budget
    assert b"repair only" in lib.ogs_last_error()
    assert call(_pairs(capi), WA._mods(capi, metrics=(X, X, X), longest=(1 << 14) + 1)) \
        == E_UNSUPPORTED
    # n_units == 0 with nothing else set
    assert call(None, n=0, units=None, diff=None) == OK
    assert _call(lib, None, None, S._args(capi, n=0, units=None, diff=None)) == OK
    # the context twin reaches the same checks (a NULL context is refused)
    assert lib.ogs_ctx_spf_routes_whatif_pairs(None, None, None, None, 4, None, None, None, 0, 1,
                                               None, None) == E_INVALID
