"""ogs_route_delta (include/openr_gpu.h, ABI 8) at the boundary, without a
device: the header declares it, the library exports it, the ABI version is 8
and every bad-argument call fails before any launch with the status the
header states (the pointers below are never followed: X is just "not NULL")."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = 0x1000
OK, E_INVALID, E_UNSUPPORTED = 0, -1, -4


def _lib():
    import openr_amd.capi as capi
    return capi, capi.load()


def test_header_declares_and_library_exports():
    capi, lib = _lib()
    with open(os.path.join(ROOT, "include", "openr_gpu.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+ogs_route_delta\s*\(", header)
    assert re.search(r"#define\s+OGS_ABI_VERSION\s+8\b", header)
    assert "8: ogs_route_delta" in header
    assert "ogs_route_delta" in capi.EXPORTS
    assert hasattr(lib, "ogs_route_delta")
    assert capi.OGS_ABI_VERSION == 8
    assert lib.ogs_abi_version() == 8
    # the ctypes workspace formula is the header's macro
    m = re.search(r"#define\s+OGS_ROUTE_DELTA_TILE\s+(\d+)", header)
    assert int(m.group(1)) == capi.OGS_ROUTE_DELTA_TILE
    assert "* (size_t)528)" in header
    for p, want in ((0, 0), (1, 528), (2048, 528), (2049, 1056), (70001, 35 * 528)):
        assert capi.route_delta_workspace_bytes(p) == want


def _cases(capi, lib):
    def records(**kw):
        o = capi.SpfOut(None, None, X, X, X, X, None)
        for k, v in kw.items():
            setattr(o, k, v)
        return ctypes.byref(o)

    def outs(**kw):
        o = capi.RouteDeltaOut(16, X, X, X, X, X, X, X, X, X)
        for k, v in kw.items():
            setattr(o, k, v)
        return ctypes.byref(o)

    def policy(*cols):
        return ctypes.byref(capi.RouteDeltaPolicy(*cols))

    def call(prev=None, nxt=None, P=8, adv_off=None, adv_class=None, pol=None, flags=0, W=1,
             out=None, ws=X, default=True):
        if default:
            prev = prev if prev is not None else records()
            nxt = nxt if nxt is not None else records()
            out = out if out is not None else outs()
        return lambda: lib.ogs_route_delta(prev, nxt, P, adv_off, adv_class, pol, flags, W, out,
                                           ws, None)

    return [
        ("prev NULL", E_INVALID, call(prev=None, nxt=records(), out=outs(), default=False)),
        ("next NULL", E_INVALID, call(prev=records(), nxt=None, out=outs(), default=False)),
        ("out NULL", E_INVALID, call(prev=records(), nxt=records(), out=None, default=False)),
        ("workspace NULL", E_INVALID, call(ws=None)),
        ("prev meta NULL", E_INVALID, call(prev=records(meta=None))),
        ("next mask NULL", E_INVALID, call(nxt=records(mask=None))),
        ("next sel NULL", E_INVALID, call(nxt=records(sel=None))),
        ("record arrays NULL", E_INVALID, call(out=outs(prefix=None))),
        ("kind NULL", E_INVALID, call(out=outs(kind=None))),
        ("header NULL", E_INVALID, call(out=outs(header=None))),
        ("num_prefixes < 0", E_INVALID, call(P=-1)),
        ("num_prefixes 0, NULL arrays", OK,
         call(prev=None, nxt=None, P=0, out=None, ws=None, default=False)),
        ("nh_words 3", E_UNSUPPORTED, call(W=3)),
        ("nh_words 8", E_UNSUPPORTED, call(W=8)),
        ("nh_words 0", E_UNSUPPORTED, call(W=0)),
        ("policy: prev side only", E_INVALID, call(pol=policy(X, X, None, None))),
        ("policy: next side only", E_INVALID, call(pol=policy(None, None, X, X))),
        ("policy: applied without counter", E_INVALID, call(pol=policy(X, None, X, None))),
        ("policy given, out columns NULL", E_INVALID,
         call(pol=policy(X, X, X, X), out=outs(applied=None))),
        ("adv_class without adv_off", E_INVALID, call(adv_class=X)),
        ("adv_off without adv_class", E_INVALID, call(adv_off=X)),
        ("unknown flag", E_INVALID, call(flags=0x20)),
    ]


def test_bad_arguments_fail_before_any_launch():
    capi, lib = _lib()
    cases = _cases(capi, lib)
    assert {label: fn() for label, _, fn in cases} == {label: st for label, st, _ in cases}
    # a failed call leaves its message
    lib.ogs_route_delta(None, None, 8, None, None, None, 0, 1, None, None, None)
    assert b"NULL" in lib.ogs_last_error()
