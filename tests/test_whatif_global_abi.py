"""ogs_spf_routes_whatif_global and ogs_whatif_needs_global
(include/openr_gpu.h) at the boundary, without a device: the header declares
both, the library exports them, the ABI version is still 8 (both are
additive), every bad-argument call fails before any launch with the status
ogs_spf_routes_whatif gives the same broken call, and the host-only question
"does this area need the global form" flips exactly where the LDS forms stop
fitting (the pointers below are never followed: X is just "not NULL")."""
import re

import pytest

import test_scenarios_abi as S
from test_whatif_abi import _mods

X, OK, E_INVALID, E_UNSUPPORTED = S.X, S.OK, S.E_INVALID, S.E_UNSUPPORTED
ENTRY = "ogs_spf_routes_whatif_global"


def test_header_declares_and_library_exports():
    capi, lib = S._lib()
    with open(S.os.path.join(S.ROOT, "include", "openr_gpu.h")) as f:
        header = f.read()
    for name in (ENTRY, "ogs_whatif_needs_global"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS
        assert hasattr(lib, name)
    assert re.search(r"int ogs_whatif_needs_global\(const ogs_graph\*[^,)]*,\s*uint32_t flags,\s*"
                     r"int32_t nh_words\);", header)
    # every declared entry point is listed, and nothing else
    declared = set(re.findall(r"^(?:int|const char\*|uint32_t|void)\s+(ogs_\w+)\s*\(", header,
                              re.M))
    assert {ENTRY, "ogs_whatif_needs_global"} <= declared
    assert declared <= set(capi.EXPORTS)
    assert re.search(r"#define\s+OGS_ABI_VERSION\s+8\b", header)
    assert capi.OGS_ABI_VERSION == 8 and lib.ogs_abi_version() == 8
    # the header states the workspace a unit takes
    assert "Workspace, proportional to n_units" in header


# the rules shared with ogs_spf_routes_whatif that hold for this entry too:
# everything up to the shape rules (this form needs no edge_src and takes any
# max_nodes up to 2^21, so those two rows differ and are stated below)
SHARED = [c for c in S.SHARED if c[0] != "edge_src NULL"]


@pytest.mark.parametrize("label,status,over", SHARED, ids=[c[0] for c in SHARED])
def test_shared_rules_return_the_whatif_status(label, status, over):
    capi, lib = S._lib()
    got = S._call(lib, ENTRY, _mods(capi), S._args(capi, **over))
    ref = S._call(lib, "ogs_spf_routes_whatif", _mods(capi), S._args(capi, **over))
    assert (got, ref) == (status, status)


def test_shared_order():
    """A call broken twice fails on the rule ogs_spf_routes_whatif states
    first: OGS_E_UNSUPPORTED (max_nodes) wins over the nh_words < 1 check
    after it and loses to the NULL checks before it."""
    capi, lib = S._lib()
    for over, status in (({"graph.max_nodes": 0, "W": 0}, E_UNSUPPORTED),
                         ({"graph.max_nodes": 0, "diff.changed": None}, E_INVALID),
                         (dict(W=0, flags=S.INCREMENTAL | S.WIDE), E_INVALID),
                         (dict(units=None, flags=S.CHANGED_ONLY), E_INVALID)):
        got = S._call(lib, ENTRY, _mods(capi), S._args(capi, **over))
        ref = S._call(lib, "ogs_spf_routes_whatif", _mods(capi), S._args(capi, **over))
        assert (got, ref) == (status, status), over


def test_global_rules():
    capi, lib = S._lib()

    def call(mods, **over):
        return S._call(lib, ENTRY, mods, S._args(capi, **over))

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
    # what this form does not take, node bits or not
    for mods in (_mods(capi), _mods(capi, nodes=(X, X, X))):
        assert call(mods, flags=S.INCREMENTAL | S.WIDE) == E_UNSUPPORTED
        assert b"32-bit" in lib.ogs_last_error()
        assert call(mods, flags=S.WIDE) == E_UNSUPPORTED
        for W in (3, 8, 16):
            assert call(mods, W=W) == E_UNSUPPORTED, W
        assert call(mods, **{"graph.max_nodes": 0}) == E_UNSUPPORTED
        assert call(mods, **{"graph.max_nodes": (1 << 21) + 1}) == E_UNSUPPORTED
    # changed-only, and with it the exit-only units, exists at one next-hop
    # word alone: with everything the exit needs (base_dist, base_nh, edge_src,
    # out->nh) the flag is refused at 2 and 4 words before any launch
    for W in (2, 4):
        assert call(_mods(capi), flags=S.INCREMENTAL | S.CHANGED_ONLY, W=W,
                    **{"out.nh": X, "out.dist": X}) == E_INVALID, W
        assert b"nh_words 1" in lib.ogs_last_error()
    # n_units == 0 with nothing else set
    assert call(None, n=0, units=None, diff=None) == OK
    assert call(_mods(capi, nodes=(X, X, X)), n=0) == OK


def frontier_bytes(n, W):
    """LDS of the frontier kernel's unit: u32 dist [n], W next-hop words a
    node, u16 stamps (frontier_lds_bytes of spf_frontier.hip, chunk-scan form)"""
    up4 = lambda x: (x + 3) & ~3
    return 4 * (up4(n) + up4(n * W)) + 2 * ((n + 1) & ~1)


def first_not_fitting(W):
    n = 1
    while frontier_bytes(n + 1, W) <= 160 * 1024:
        n += 1
    return n + 1


def test_needs_global_at_the_frontier_limit():
    capi, lib = S._lib()

    def needs(n, W=1, flags=0, degree=4):
        g = capi.Graph(1, n, 4 * n, degree, None, None, None, None, None, None, 0, None, 0, None,
                       None)
        return lib.ogs_whatif_needs_global(g, flags, W)

    assert first_not_fitting(1) == 16385
    assert (needs(16384), needs(16385)) == (0, 1)
    for W in (2, 4):
        n = first_not_fitting(W)
        assert frontier_bytes(n - 1, W) <= 160 * 1024 < frontier_bytes(n, W)
        assert (needs(n - 1, W), needs(n, W)) == (0, 1), (W, n)
    assert 11000 < first_not_fitting(2) < 12000 and 7000 < first_not_fitting(4) < 7500
    # the project's large-area workload, and the id limit of the edge encoding
    assert needs(20000) == 1 and needs(1 << 21) == 1
    # what the global form does not take either
    assert needs(20000, flags=S.WIDE) == 0
    assert needs(20000, W=8) == 0 and needs(20000, W=3) == 0 and needs(20000, W=0) == 0
    assert needs(0) == 0 and needs((1 << 21) + 1) == 0
    assert lib.ogs_whatif_needs_global(None, 0, 1) == 0
    # small areas never need it
    assert needs(25) == 0 and needs(2000, W=4) == 0
