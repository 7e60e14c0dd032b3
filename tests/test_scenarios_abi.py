"""ogs_spf_routes_scenarios (include/openr_gpu.h) at the boundary, without a
device: the header declares the entry and its context twin, the library
exports them, the ABI version is still 8 (the entry is additive) and every
bad-argument call fails before any launch. The rules the entry shares with
ogs_spf_routes_variants are made as the same broken call on both entries and
must return the same status (the pointers below are never followed: X is just
"not NULL")."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = 0x1000
OK, E_INVALID, E_UNSUPPORTED = 0, -1, -4
INCREMENTAL, CHANGED_ONLY, WIDE = 0x40, 0x80, 0x10


def _lib():
    import openr_amd.capi as capi
    return capi, capi.load()


class UnitMods(ctypes.Structure):
    _fields_ = [("dead_edges", ctypes.c_void_p), ("dead_per_unit", ctypes.c_int32)]


def test_header_declares_and_library_exports():
    capi, lib = _lib()
    with open(os.path.join(ROOT, "include", "openr_gpu.h")) as f:
        header = f.read()
    for name in ("ogs_spf_routes_scenarios", "ogs_ctx_spf_routes_scenarios"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS
        assert hasattr(lib, name)
    assert re.search(r"typedef struct ogs_scenario_mods \{[^}]*dead_off[^}]*dead_edges[^}]*"
                     r"drain_off[^}]*drain_nodes[^}]*\} ogs_scenario_mods;", header)
    assert re.search(r"#define\s+OGS_ABI_VERSION\s+8\b", header)
    assert capi.OGS_ABI_VERSION == 8 and lib.ogs_abi_version() == 8
    # the entry cites what each scenario kind stands for in the reference
    for cite in ("LinkState.cpp:643", "LinkState.cpp:441", "LinkState.cpp:741-752"):
        assert cite in header
    # ogs_unit_mods keeps its two fields
    assert re.search(r"typedef struct ogs_unit_mods \{\s*const uint32_t\* dead_edges;[^;]*"
                     r"int32_t dead_per_unit;[^;}]*\} ogs_unit_mods;", header)


def _args(capi, **kw):
    """a call's arguments that pass every check; kw overrides"""
    graph = capi.Graph(1, 100, 400, 4, X, X, X, X, None, None, 0, None, 0, X, None)
    table = capi.PrefixTable(10, 10, X, X, X, X, X, X)
    out = capi.SpfOut(None, None, X, X, X, X, None)
    diff = capi.RouteDiff(X, X, X, X, X, X, X, None, None, 0)
    a = dict(graph=graph, table=table, units=X, n=4, diff=diff, flags=INCREMENTAL, W=1, out=out)
    for k, v in kw.items():
        if "." in k:
            obj, field = k.split(".")
            setattr(a[obj], field, v)
        else:
            a[k] = v
    return a


def _ref(x):
    return None if x is None else (x if isinstance(x, int) else ctypes.byref(x))


def _call(lib, entry, mods, a):
    fn = getattr(lib, entry)
    return fn(_ref(a["graph"]), _ref(a["table"]), a["units"], a["n"], _ref(mods), _ref(a["diff"]),
              a["flags"], a["W"], _ref(a["out"]), None)


# rules both entries state: (label, status, overrides)
SHARED = [
    ("graph NULL", E_INVALID, dict(graph=None)),
    ("prefixes NULL", E_INVALID, dict(table=None)),
    ("out NULL", E_INVALID, dict(out=None)),
    ("n_units < 0", E_INVALID, dict(n=-1)),
    ("units NULL", E_INVALID, dict(units=None)),
    ("row_ptr NULL", E_INVALID, {"graph.row_ptr": None}),
    ("node_flags NULL", E_INVALID, {"graph.node_flags": None}),
    ("adv_off NULL", E_INVALID, {"table.adv_off": None}),
    ("diff arrays NULL", E_INVALID, {"diff.changed": None}),
    ("incremental without diff", E_INVALID, dict(diff=None)),
    ("incremental without base_dist", E_INVALID, {"diff.base_dist": None}),
    ("changed-only without incremental", E_INVALID, dict(flags=CHANGED_ONLY)),
    ("changed-only with nh_words 2", E_INVALID, dict(flags=INCREMENTAL | CHANGED_ONLY, W=2)),
    ("max_nodes 0", E_UNSUPPORTED, {"graph.max_nodes": 0}),
    ("max_nodes past 2^21", E_UNSUPPORTED, {"graph.max_nodes": (1 << 21) + 1}),
    ("nh_words 0", E_INVALID, dict(W=0)),
    ("edge_src NULL", E_UNSUPPORTED, {"graph.edge_src": None}),
    ("wide metric", E_UNSUPPORTED, dict(flags=INCREMENTAL | WIDE)),
    ("nh_words 8", E_UNSUPPORTED, dict(W=8)),
    ("n_units 0, NULL arrays", OK, dict(n=0, units=None, diff=None)),
]


@pytest.mark.parametrize("label,status,over", SHARED, ids=[c[0] for c in SHARED])
def test_shared_rules_return_the_variants_status(label, status, over):
    capi, lib = _lib()
    got = _call(lib, "ogs_spf_routes_scenarios", capi.ScenarioMods(X, X, None, None),
                _args(capi, **over))
    ref = _call(lib, "ogs_spf_routes_variants", UnitMods(X, 4), _args(capi, **over))
    assert (got, ref) == (status, status)


def test_scenario_rules():
    capi, lib = _lib()

    def call(mods, **over):
        return _call(lib, "ogs_spf_routes_scenarios", mods, _args(capi, **over))

    assert call(None) == E_INVALID
    assert b"NULL" in lib.ogs_last_error()
    assert call(capi.ScenarioMods(None, X, None, None)) == E_INVALID
    assert call(capi.ScenarioMods(X, None, None, None)) == E_INVALID
    assert call(capi.ScenarioMods(X, X, X, None)) == E_INVALID
    assert call(capi.ScenarioMods(X, X, None, X)) == E_INVALID
    # n_units == 0 with nothing else set
    assert call(None, n=0, units=None, diff=None) == OK
    # drains run in the base SPF's repair only: a call with drains that it
    # cannot take (a full recompute, two-word sets, its LDS budget) is refused
    # with nothing launched; dead lists alone take the full frontier form
    assert call(capi.ScenarioMods(X, X, X, X), flags=0) == E_UNSUPPORTED
    assert b"drains" in lib.ogs_last_error()
    assert call(capi.ScenarioMods(X, X, X, X), W=2) == E_UNSUPPORTED
    assert call(capi.ScenarioMods(X, X, X, X), **{"graph.max_nodes": 12000}) == E_UNSUPPORTED
    # a bitset no form's LDS holds (2^22 edges: 512 kB)
    assert call(capi.ScenarioMods(X, X, None, None),
                **{"graph.max_edges": 1 << 22}) == E_UNSUPPORTED
    assert b"bitset" in lib.ogs_last_error()
    # the context twin reaches the same checks (a NULL context is refused)
    assert lib.ogs_ctx_spf_routes_scenarios(None, None, None, None, 4, None, None, 0, 1, None,
                                            None) == E_INVALID
    # ogs_unit_mods' limit stands
    assert _call(lib, "ogs_spf_routes_variants", UnitMods(X, 9), _args(capi)) == E_INVALID
