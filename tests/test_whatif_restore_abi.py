"""OGS_F_RESTORE at the boundary, without a device: the header declares the
flag and its two encodings beside the entries that read them, the ABI version
is still 8 (additive: no new entry point, ogs_whatif_mods keeps its layout), and
every argument rule of ogs_spf_routes_whatif and ogs_spf_routes_whatif_global
returns with the flag set the status it returns without it (the pointers below
are never followed: X is just "not NULL")."""
import ctypes
import re

import pytest

import test_scenarios_abi as S
import test_whatif_abi as WA

X, OK, E_INVALID, E_UNSUPPORTED = S.X, S.OK, S.E_INVALID, S.E_UNSUPPORTED
ENTRIES = ("ogs_spf_routes_whatif", "ogs_spf_routes_whatif_global")


def test_header_and_bindings():
    capi, lib = S._lib()
    with open(S.os.path.join(S.ROOT, "include", "openr_gpu.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+OGS_F_RESTORE\s+0x100u", header)
    assert re.search(r"#define\s+OGS_WHATIF_EDGE_UP\s+0x80000000u", header)
    assert re.search(r"#define\s+OGS_NODE_CLEAR_SHIFT\s+4\b", header)
    assert (capi.OGS_F_RESTORE, capi.OGS_WHATIF_EDGE_UP, capi.OGS_NODE_CLEAR_SHIFT) == (
        0x100, 0x80000000, 4)
    # no other public flag shares the bit
    flags = dict(re.findall(r"#define\s+(OGS_F_\w+)\s+(0x[0-9A-Fa-f]+)u", header))
    assert [n for n, v in flags.items() if int(v, 16) & 0x100] == ["OGS_F_RESTORE"]
    assert re.search(r"#define\s+OGS_ABI_VERSION\s+8\b", header)
    assert capi.OGS_ABI_VERSION == 8 and lib.ogs_abi_version() == 8
    # ogs_whatif_mods keeps its layout: 8 pointers and a u32
    assert ctypes.sizeof(capi.WhatifMods) == 8 * ctypes.sizeof(ctypes.c_void_p) + 8
    # what the restoring kinds stand for in the reference, and the sizing rule
    for cite in ("LinkState.cpp:574", "LinkState.cpp:480", "LinkMonitor.cpp:971-1001",
                 "SpfSolver.cpp:526-551", "max_metric_per_unit counts the revived edges"):
        assert cite in header, cite


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("label,status,over", S.SHARED, ids=[c[0] for c in S.SHARED])
def test_shared_rules_keep_their_status(entry, label, status, over):
    capi, lib = S._lib()
    if entry.endswith("_global") and label == "edge_src NULL":
        return  # graph->edge_src may be NULL there: the call would reach a launch
    for restore in (0, capi.OGS_F_RESTORE):
        a = S._args(capi, **over)
        a["flags"] |= restore
        assert S._call(lib, entry, WA._mods(capi), a) == status, (label, restore)


def test_whatif_rules_keep_their_status():
    capi, lib = S._lib()
    R = capi.OGS_F_RESTORE

    def call(entry, mods, **over):
        a = S._args(capi, **over)
        got = []
        for restore in (0, R):
            b = dict(a)
            b["flags"] = a["flags"] | restore
            got.append(S._call(lib, entry, mods, b))
        assert got[0] == got[1], (entry, over, got)
        return got[1]

    for entry in ENTRIES:
        assert call(entry, None) == E_INVALID
        assert call(entry, WA._mods(capi, dead=(None, X))) == E_INVALID
        assert call(entry, WA._mods(capi, dead=(X, None))) == E_INVALID
        for k in range(3):
            for full in (False, True):
                part = tuple((X if full else None) if i != k else (None if full else X)
                             for i in range(3))
                assert call(entry, WA._mods(capi, nodes=part)) == E_INVALID, part
                assert call(entry, WA._mods(capi, metrics=part, longest=4)) == E_INVALID, part
        assert call(entry, None, n=0, units=None, diff=None) == OK
    # clear nibbles are node bits: where the repair cannot take the call the
    # LDS entry refuses it with nothing launched, flag or no flag
    nodes = WA._mods(capi, nodes=(X, X, X))
    for over in (dict(flags=0), dict(W=2), {"graph.max_nodes": 12000}):
        assert call("ogs_spf_routes_whatif", nodes, **over) == E_UNSUPPORTED, over
        assert b"node bits" in lib.ogs_last_error()
    # revived edges ride in the metric slice: its sizing rules are the slice's
    assert call("ogs_spf_routes_whatif", WA._mods(capi),
                **{"graph.max_edges": 1 << 22}) == E_UNSUPPORTED
    for longest in ((1 << 14) + 1, 0xFFFFFFFF):
        m = WA._mods(capi, metrics=(X, X, X), longest=longest)
        assert call("ogs_spf_routes_whatif", m) == E_UNSUPPORTED, longest
        assert call("ogs_spf_routes_whatif", m, flags=0) == E_UNSUPPORTED
    # the global entry's own rule
    assert call("ogs_spf_routes_whatif_global", WA._mods(capi), W=8) == E_UNSUPPORTED
    assert call("ogs_spf_routes_whatif_global", WA._mods(capi), W=3) == E_UNSUPPORTED
