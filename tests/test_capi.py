"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports
every entry point include/openr_gpu.h declares, and the product fails loudly
(no CPU fallback) when no HIP device is visible."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "openr_gpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ogs_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_entry_points():
    syms = declared_symbols()
    assert "ogs_spf_routes" in syms and len(syms) >= 10


def test_library_exports_every_declared_symbol():
    import openr_amd
    import openr_amd.capi as capi
    lib = ctypes.CDLL(openr_amd.LIB_PATH)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, missing
    assert sorted(capi.EXPORTS) == declared_symbols()


def test_pure_entry_points_without_device():
    import openr_amd.capi as capi
    lib = capi.load()
    assert b"gfx950" in lib.ogs_version()
    assert [lib.ogs_nh_words_for_degree(d) for d in (0, 1, 32, 33, 65, 200, 511)] == \
        [1, 1, 1, 2, 4, 8, 16]
    # past 512 links: the exact width (runtime-width kernels), never an error
    assert [lib.ogs_nh_words_for_degree(d) for d in (512, 513, 700, 4096)] == [16, 17, 22, 128]
    assert lib.ogs_nh_words_for_degree(-1) < 0
    assert lib.ogs_abi_version() == capi.OGS_ABI_VERSION


def option_names(lib):
    names, i = [], 0
    while lib.ogs_option_name(i) is not None:
        names.append(lib.ogs_option_name(i).decode())
        i += 1
    return names


def test_engine_options_documented_and_validated():
    """Every ogs_set_option knob the library parses is documented in the
    header; unknown names and out-of-range values are rejected (no device
    needed: options are process-wide settings)."""
    import openr_amd.capi as capi
    lib = capi.load()
    names = option_names(lib)
    header = open(os.path.join(ROOT, "include", "openr_gpu.h")).read()
    assert len(names) >= 20
    undocumented = [n for n in names if f'"{n}"' not in header]
    assert not undocumented, undocumented
    assert lib.ogs_set_option(b"no_such_option", 1) != 0
    assert lib.ogs_set_option(b"route_store_nt", 4) != 0
    assert lib.ogs_set_option(b"route_store_nt", -1) != 0
    assert lib.ogs_set_option(b"route_store_nt", 3) == 0
    assert lib.ogs_set_option(b"route_store_nt", 2) == 0


# tests/golden/engine_options.json: each knob's default (kernels/engine.h) and
# which of the probe values ogs_set_option accepted before the knobs became one
# table. The 2^32 + k probes catch a table that narrows before it validates.
OPTION_PROBES = list(range(-3, 1027)) + [
    4095, 4096, 4097, 65535, 65536, 65537, 163839, 163840, 163841,
    2**31 - 1, 2**31, -2**31, 2**32, 2**32 + 1, 2**32 + 5, -2**32]
OGS_E_INVALID = -1


def golden_options():
    with open(os.path.join(ROOT, "tests", "golden", "engine_options.json")) as f:
        return json.load(f)["options"]


def _get(lib, name):
    value = ctypes.c_int64(-12345)
    assert lib.ogs_get_option(name.encode(), ctypes.byref(value)) == 0, name
    return value.value


def test_option_names_match_the_recorded_table():
    import openr_amd.capi as capi
    names = option_names(capi.load())
    assert len(names) == len(set(names)) == 34
    assert set(names) == set(golden_options())
    lib = capi.load()
    assert lib.ogs_option_name(len(names)) is None and lib.ogs_option_name(-1) is None


def test_option_defaults_match_the_recorded_table():
    """Read in a fresh process: no test before this one can have left a knob set."""
    code = ("import json, sys; sys.path.insert(0, sys.argv[1]); import openr_amd.capi as c; "
            "lib = c.load(); names = [lib.ogs_option_name(i).decode() for i in range(34)]; "
            "print(json.dumps({n: c.get_option(lib, n) for n in names}))")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    want = {n: o["default"] for n, o in golden_options().items()}
    if "OGS_UNIT_WIDTH" in os.environ:
        del got["unit_width"], want["unit_width"]
    assert got == want


def test_set_option_accepts_what_it_accepted_before():
    """Per knob and probe: the setter's status is the recorded one; the getter
    then returns the value (accepted) or the previous value (rejected)."""
    import openr_amd.capi as capi
    lib = capi.load()
    for name, opt in golden_options().items():
        start = current = _get(lib, name)
        for v in OPTION_PROBES:
            want = any(lo <= v <= hi for lo, hi in opt["accepted"])
            rc = lib.ogs_set_option(name.encode(), v)
            assert (rc == 0) == want and rc in (0, OGS_E_INVALID), (name, v, rc)
            if want:
                current = v
            assert _get(lib, name) == current, (name, v)
        assert lib.ogs_set_option(name.encode(), start) == 0
        # a rejected value is named in the error with what is accepted
        assert lib.ogs_set_option(name.encode(), 2**32 + 5) == OGS_E_INVALID
        err = lib.ogs_last_error().decode()
        assert name in err and str(opt["accepted"][0][0]) in err, err


def test_option_calls_reject_unknown_and_null():
    import openr_amd.capi as capi
    lib = capi.load()
    value = ctypes.c_int64(77)
    assert lib.ogs_set_option(b"no_such_option", 1) == OGS_E_INVALID
    assert lib.ogs_set_option(None, 1) == OGS_E_INVALID
    assert lib.ogs_get_option(b"no_such_option", ctypes.byref(value)) == OGS_E_INVALID
    assert lib.ogs_get_option(None, ctypes.byref(value)) == OGS_E_INVALID
    assert lib.ogs_get_option(b"route_stream", None) == OGS_E_INVALID
    assert value.value == 77
    assert lib.ogs_ctx_get_option(None, b"route_stream", ctypes.byref(value)) == OGS_E_INVALID
    assert lib.ogs_ctx_set_option(None, b"route_stream", 5) == OGS_E_INVALID


def test_scoped_options_restore():
    import openr_amd.capi as capi
    lib = capi.load()
    names = ("route_stream", "lds_pull", "spf_queue")
    before = {n: _get(lib, n) for n in names}
    with capi.scoped_options(lib, route_stream=2, lds_pull=9):
        assert (_get(lib, "route_stream"), _get(lib, "lds_pull")) == (2, 9)
        with capi.scoped_options(lib, route_stream=4, spf_queue=0):
            assert (_get(lib, "route_stream"), _get(lib, "spf_queue")) == (4, 0)
            assert _get(lib, "lds_pull") == 9
        assert (_get(lib, "route_stream"), _get(lib, "lds_pull")) == (2, 9)
        assert _get(lib, "spf_queue") == before["spf_queue"]
    assert {n: _get(lib, n) for n in names} == before
    # the body raises
    with pytest.raises(KeyError):
        with capi.scoped_options(lib, route_stream=1, lds_pull=0):
            raise KeyError("body")
    assert {n: _get(lib, n) for n in names} == before
    # a later option is rejected: the ones already applied go back
    with pytest.raises(RuntimeError, match="lds_pull"):
        with capi.scoped_options(lib, route_stream=1, lds_pull=99, spf_queue=0):
            pytest.fail("the body must not run")
    assert {n: _get(lib, n) for n in names} == before
    with pytest.raises(RuntimeError):
        with capi.scoped_options(lib, no_such_option=1):
            pytest.fail("the body must not run")


# ---- argument checks of the compute entry points ---------------------------
# Every call below breaks one or two rules and must fail before any launch, so
# the pointers are never followed (X is just "not NULL"). The statuses were
# recorded from the library before the shared checks were factored out; where
# two rules are broken the status shows which check comes first
# (OGS_E_UNSUPPORTED for max_nodes wins only over the checks after it).
X = 0x1000
OGS_E_UNSUPPORTED = -4
F_EXACT, F_INCREMENTAL, F_CHANGED_ONLY = 0x20, 0x40, 0x80
TOO_MANY_NODES = (1 << 21) + 1


class PathOut(ctypes.Structure):
    _fields_ = [("path_count", ctypes.c_void_p), ("path_len", ctypes.c_void_p),
                ("path_edges", ctypes.c_void_p), ("max_paths", ctypes.c_uint32),
                ("max_edges", ctypes.c_uint32)]


class UnitMods(ctypes.Structure):
    _fields_ = [("dead_edges", ctypes.c_void_p), ("dead_per_unit", ctypes.c_int32)]


# ogs_area_table, ogs_route_diff and ogs_rib_policy: openr_amd.capi's
# AreaTable, RouteDiff and RibPolicy


def _struct(cls, base, **over):
    o = cls()
    for k, v in {**base, **over}.items():
        setattr(o, k, v)
    return o


def bad_argument_cases(lib, capi):
    """[(label, recorded status, call)]"""
    P = ctypes.c_void_p

    def graph(**kw):
        return ctypes.byref(_struct(capi.Graph, dict(
            num_topos=1, max_nodes=10, max_edges=40, max_degree=4, node_base=X, row_ptr=X,
            edges=X, node_flags=X), **kw))

    def table(**kw):
        return ctypes.byref(_struct(capi.PrefixTable, dict(
            max_prefixes=4, max_advertisements=4, pfx_base=X, adv_off=X, adv_node=X,
            adv_metrics=X, adv_min_nh=X, pfx_flags=X), **kw))

    def paths(**kw):
        return ctypes.byref(_struct(PathOut, dict(path_count=X, path_len=X, path_edges=X,
                                                  max_paths=4, max_edges=40), **kw))

    def areas(**kw):
        return ctypes.byref(_struct(capi.AreaTable, dict(num_areas=1, num_names=10, name_local=X,
                                                    adv_area=X, adv_name=X), **kw))

    def mods(**kw):
        return ctypes.byref(_struct(UnitMods, dict(dead_edges=X, dead_per_unit=2), **kw))

    def diff(**kw):
        return ctypes.byref(_struct(capi.RouteDiff, dict(base_meta=X, base_metric=X, base_mask=X,
                                                    changed=X, counts=X), **kw))

    def policy(**kw):
        return ctypes.byref(_struct(capi.RibPolicy, dict(num_statements=2, active=3, pfx_match=X,
                                                    adv_tag_match=X, slot_nonzero=X), **kw))

    def groups(*specs):
        arr = (capi.RouteGroup * len(specs))()
        for g, (units, n, w) in zip(arr, specs):
            g.units, g.n_units, g.nh_words = units, n, w
        return arr

    out = ctypes.byref(capi.SpfOut())
    I, U = OGS_E_INVALID, OGS_E_UNSUPPORTED

    def routes(g, pt=None, units=X, n=4, flags=0, w=1, o=out):
        return lambda: lib.ogs_spf_routes(g, pt, P(units), n, flags, w, o, None)

    def grouped(g, pt, arr, n, flags=0):
        return lambda: lib.ogs_spf_routes_groups(g, pt, arr, n, flags, None)

    def from_spf(g, pt, units=X, n=4, dist=X, nh=X, w=1):
        return lambda: lib.ogs_routes_from_spf(g, pt, P(units), n, P(dist), P(nh), None, 0, w,
                                               out, None)

    def ksp(g, units=X, n=4, masks=None, mask_words=0, o=None):
        return lambda: lib.ogs_ksp_paths(g, P(units), n, P(masks), mask_words, 0,
                                         o or paths(), None)

    def ksp2(g, sources=X, ns=2, units=X, n=4, k2=-1):
        return lambda: lib.ogs_ksp2_paths(g, P(sources), ns, P(units), n, 0, paths(),
                                          paths() if k2 == -1 else k2, None)

    def variants(g, pt, units=X, n=4, m=None, d=None, flags=0, w=1):
        return lambda: lib.ogs_spf_routes_variants(g, pt, P(units), n, m, d, flags, w, out, None)

    def multiarea(g, pt, at, units=X, n=4, row=X, dist=X, nh=X, w=1):
        return lambda: lib.ogs_routes_multiarea(g, pt, at, P(units), n, P(row), P(dist), P(nh),
                                                0, w, out, None)

    def rib(pt, pol, a=1, n=4, w=1, meta=X, mask=X, applied=None, counter=None):
        return lambda: lib.ogs_rib_policy_apply(pt, pol, a, n, w, P(meta), P(mask), P(applied),
                                                P(counter), None)

    return [
        ("routes: graph NULL", I, routes(None)),
        ("routes: out NULL", I, routes(graph(), o=None)),
        ("routes: n_units < 0", I, routes(graph(), n=-1)),
        ("routes: no units, bad graph", 0, routes(graph(max_nodes=0, row_ptr=None), n=0)),
        ("routes: units NULL before max_nodes", I, routes(graph(max_nodes=0), units=None)),
        ("routes: node_flags NULL before max_nodes", I,
         routes(graph(max_nodes=TOO_MANY_NODES, node_flags=None))),
        ("routes: max_nodes 0", U, routes(graph(max_nodes=0))),
        ("routes: max_nodes before slot_stride", U,
         routes(graph(max_nodes=TOO_MANY_NODES, slot_node=X, slot_stride=100))),
        ("routes: max_nodes before prefix arrays", U,
         routes(graph(max_nodes=-5), table(adv_node=None))),
        ("routes: max_nodes before nh_words", U, routes(graph(max_nodes=0), w=0)),
        ("routes: slot_stride 100", I, routes(graph(slot_node=X, slot_stride=100))),
        ("routes: slot_stride < max_nodes", I,
         routes(graph(max_nodes=100, slot_node=X, slot_stride=64))),
        ("routes: slot_edges without slot_node", I, routes(graph(slot_edges=X, slot_degree=4))),
        ("routes: slot_degree 5", I,
         routes(graph(slot_node=X, slot_stride=64, slot_edges=X, slot_degree=5))),
        ("routes: adv_min_nh NULL", I, routes(graph(), table(adv_min_nh=None))),
        ("routes: pfx_base NULL", I, routes(graph(), table(pfx_base=None))),
        ("routes: nh_words 0", I, routes(graph(), w=0)),
        ("routes: exact order without wide metric", I, routes(graph(), flags=F_EXACT)),
        ("groups: groups NULL", I, grouped(graph(), None, None, 1)),
        ("groups: n_groups < 0", I, grouped(graph(), None, groups((X, 1, 1)), -1)),
        ("groups: n_units < 0", I, grouped(graph(), None, groups((X, -1, 1)), 1)),
        ("groups: group units NULL", I, grouped(graph(), None, groups((None, 2, 1)), 1)),
        ("groups: nh_words 0 before max_nodes", I,
         grouped(graph(max_nodes=0), None, groups((X, 2, 0)), 1)),
        ("groups: no live group, bad graph", 0,
         grouped(graph(max_nodes=0, row_ptr=None), None, groups((None, 0, 0), (X, 0, 1)), 2)),
        ("groups: row_ptr NULL before max_nodes", I,
         grouped(graph(max_nodes=0, row_ptr=None), None, groups((X, 2, 1)), 1)),
        ("groups: max_nodes before prefix arrays", U,
         grouped(graph(max_nodes=TOO_MANY_NODES), table(pfx_flags=None), groups((X, 2, 1)), 1)),
        ("groups: adv_off NULL", I,
         grouped(graph(), table(adv_off=None), groups((X, 0, 1), (X, 2, 1)), 2)),
        ("groups: slot_degree 3", I,
         grouped(graph(slot_node=X, slot_stride=64, slot_edges=X, slot_degree=3), None,
                 groups((X, 2, 1)), 1)),
        ("groups: exact order without wide metric", I,
         grouped(graph(), None, groups((X, 2, 1)), 1, F_EXACT)),
        ("from_spf: prefixes NULL", I, from_spf(graph(), None)),
        ("from_spf: n_units < 0", I, from_spf(graph(), table(), n=-2)),
        ("from_spf: no prefixes, NULL arrays", 0,
         from_spf(graph(), table(max_prefixes=0, adv_off=None), dist=None)),
        ("from_spf: adv_metrics NULL", I, from_spf(graph(), table(adv_metrics=None))),
        ("from_spf: pfx_flags NULL, nh_words 0", I, from_spf(graph(), table(pfx_flags=None), w=0)),
        ("from_spf: spf_dist NULL", I, from_spf(graph(), table(), dist=None)),
        ("from_spf: node_base NULL", I, from_spf(graph(node_base=None), table())),
        ("from_spf: nh_words 0", I, from_spf(graph(), table(), w=0)),
        ("ksp: out NULL", I, lambda: lib.ogs_ksp_paths(graph(), P(X), 4, None, 0, 0, None, None)),
        ("ksp: path_len NULL before max_nodes", I,
         ksp(graph(max_nodes=0), o=paths(path_len=None))),
        ("ksp: row_ptr NULL", I, ksp(graph(row_ptr=None))),
        ("ksp: max_nodes before mask_words", U,
         ksp(graph(max_nodes=0), masks=X, mask_words=0)),
        ("ksp: max_nodes before rslot_ext", U,
         ksp(graph(max_nodes=TOO_MANY_NODES, max_degree=512))),
        ("ksp: mask_words too small", I, ksp(graph(), masks=X, mask_words=1)),
        ("ksp: 512 edges without rslot_ext", I, ksp(graph(max_degree=512))),
        ("ksp2: k2 NULL", I, ksp2(graph(), k2=None)),
        ("ksp2: n_sources < 0", I, ksp2(graph(), ns=-1)),
        ("ksp2: no units, bad graph", 0, ksp2(graph(max_nodes=0, edges=None), n=0)),
        ("ksp2: n_sources 0", I, ksp2(graph(), ns=0)),
        ("ksp2: edges NULL before max_nodes", I, ksp2(graph(max_nodes=0, edges=None))),
        ("ksp2: k2 path_edges NULL before max_nodes", I,
         ksp2(graph(max_nodes=0), k2=paths(path_edges=None))),
        ("ksp2: max_nodes before rslot_ext", U, ksp2(graph(max_nodes=0, max_degree=600))),
        ("ksp2: 600 edges without rslot_ext", I, ksp2(graph(max_degree=600))),
        ("variants: prefixes NULL", I, variants(graph(), None)),
        ("variants: adv_off NULL before max_nodes", I,
         variants(graph(max_nodes=0), table(adv_off=None))),
        ("variants: edges NULL", I, variants(graph(edges=None), table())),
        ("variants: dead_per_unit 9 before max_nodes", I,
         variants(graph(max_nodes=0), table(), m=mods(dead_per_unit=9))),
        ("variants: diff counts NULL", I, variants(graph(), table(), d=diff(counts=None))),
        ("variants: incremental without mods", I,
         variants(graph(), table(), d=diff(base_dist=X, base_nh=X), flags=F_INCREMENTAL)),
        ("variants: changed-only without incremental, max_nodes 0", I,
         variants(graph(max_nodes=0), table(), flags=F_CHANGED_ONLY)),
        ("variants: max_nodes before nh_words", U, variants(graph(max_nodes=0), table(), w=0)),
        ("variants: max_nodes too large", U, variants(graph(max_nodes=TOO_MANY_NODES), table())),
        ("variants: nh_words 0", I, variants(graph(), table(), w=0)),
        ("multiarea: areas NULL", I, multiarea(graph(), table(), None)),
        ("multiarea: pfx_base NULL", I, multiarea(graph(), table(pfx_base=None), areas())),
        ("multiarea: adv_name NULL", I, multiarea(graph(), table(), areas(adv_name=None))),
        ("multiarea: spf_row NULL", I, multiarea(graph(), table(), areas(), row=None)),
        ("multiarea: num_areas 0", I, multiarea(graph(), table(), areas(num_areas=0))),
        ("multiarea: num_areas > num_topos", I, multiarea(graph(), table(), areas(num_areas=2))),
        ("multiarea: nh_words 0", I, multiarea(graph(), table(), areas(), w=0)),
        ("rib: policy NULL", I, rib(table(), None)),
        ("rib: num_areas 0", I, rib(table(), policy(), a=0)),
        ("rib: no statements", 0, rib(table(adv_off=None), policy(num_statements=0))),
        ("rib: 33 statements", I, rib(table(), policy(num_statements=33))),
        ("rib: adv_off NULL", I, rib(table(adv_off=None), policy())),
        ("rib: continuation without applied", I, rib(table(), policy(statement_base=32))),
        ("rib: nh_words 0", I, rib(table(), policy(), w=0)),
    ]


def test_spf_routes_rejects_bad_arguments():
    import openr_amd.capi as capi
    lib = capi.load()
    out = capi.SpfOut()
    assert lib.ogs_spf_routes(None, None, None, 1, 0, 1, ctypes.byref(out), None) == -1
    g = capi.Graph()
    assert lib.ogs_spf_routes(ctypes.byref(g), None, None, 0, 0, 1, ctypes.byref(out), None) == 0
    g.max_nodes = 10
    assert lib.ogs_spf_routes(ctypes.byref(g), None, None, 4, 0, 1, ctypes.byref(out), None) == -1
    cases = bad_argument_cases(lib, capi)
    assert {label: call() for label, _, call in cases} == \
        {label: status for label, status, _ in cases}


def test_product_fails_loudly_without_gpu():
    import openr_amd
    if openr_amd.decision.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(RuntimeError):
        openr_amd.require_gpu()
    import lsdb as L
    M = openr_amd.decision
    als = M.AreaLinkStates()
    ls = als.add(L.kTestingAreaName, "1")
    ls.updateAdjacencyDatabase(L.createAdjDb("1", [L.adj12], 1), L.kTestingAreaName)
    ls.updateAdjacencyDatabase(L.createAdjDb("2", [L.adj21], 2), L.kTestingAreaName)
    with pytest.raises(RuntimeError):
        ls.getSpfResult("1")
    with pytest.raises(RuntimeError):
        M.SpfSolver("1", False, False).buildRouteDb("1", als, M.PrefixState())


def test_product_ingestion_matches_oracle_on_cpu(oracle):
    """Link formation / LinkStateChange are host-side ingestion in the
    product; they must agree with the oracle call-for-call."""
    import openr_amd
    import kat_cases
    M = openr_amd.decision
    kat_cases.kat_linkstate_basic(M)
    kat_cases.kat_linkstate_link_usable(M)


C_CONSUMER = os.path.join(ROOT, "tests", "c_consumer", "spf_square")


def test_c_consumer_builds_and_links():
    """The header compiles as C11 and a C program links against the library
    alone (no C++ runtime types in the ABI): built by `make`."""
    import subprocess
    assert os.path.exists(C_CONSUMER), "run make (builds tests/c_consumer/spf_square)"
    r = subprocess.run([C_CONSUMER], capture_output=True, text=True, timeout=60)
    # no device here -> 77; on a GPU box the gpu test below runs it for real
    assert r.returncode in (0, 77), r.stdout + r.stderr


@pytest.mark.gpu
def test_c_consumer_spf_on_device():
    """Plain-C ogs_spf_routes on a 4-node topology: distances and ECMP
    next-hop link slots (tests/c_consumer/spf_square.c)."""
    import subprocess
    r = subprocess.run([C_CONSUMER], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
