"""The node-label sweep at the boundary, without a device: the two new C-ABI
entries are declared, exported and bound with the documented signatures, their
argument checks answer before anything is launched, and the sweep's
constructor takes enableNodeSegmentLabel (off: the sweep it was)."""
import ctypes
import os
import re

import pytest

import lsdb as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = 0x1000  # "not NULL": every call below fails before a pointer is followed
I, U = -1, -4  # OGS_E_INVALID, OGS_E_UNSUPPORTED
WIDE = 0x10


def test_entries_are_declared_exported_and_bound():
    import openr_amd.capi as capi
    header = open(os.path.join(ROOT, "include", "openr_gpu.h")).read()
    lib = capi.load()
    for name in ("ogs_spf_node_diff", "ogs_spf_node_changes_gather"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
        assert name in capi.EXPORTS and hasattr(lib, name)
        assert not hasattr(lib, "ogs_ctx_" + name[4:])  # as the sibling gather: no ctx form
    P, I32, U32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    assert lib.ogs_spf_node_diff.argtypes == [
        ctypes.POINTER(capi.Graph), P, I32, ctypes.POINTER(capi.SpfOut),
        ctypes.POINTER(capi.NodeDiff), U32, I32, P]
    assert lib.ogs_spf_node_changes_gather.argtypes == [
        P, I32, I32, ctypes.POINTER(capi.SpfOut), I32, ctypes.POINTER(capi.NodeChanges), P]
    assert [f for f, _ in capi.NodeDiff._fields_] == [
        "base_dist", "base_nh", "interest", "unit_counts", "changed", "counts"]
    assert [f for f, _ in capi.NodeChanges._fields_] == ["offsets", "total", "node", "dist", "nh"]
    # additive: the version number existing consumers check stays
    assert capi.OGS_ABI_VERSION == lib.ogs_abi_version() == 8


def test_argument_errors_need_no_device():
    import openr_amd.capi as capi
    lib = capi.load()

    def graph(**kw):
        return ctypes.byref(capi.Graph(**{**dict(num_topos=1, max_nodes=10, node_base=X), **kw}))

    def rows(**kw):
        return ctypes.byref(capi.SpfOut(**{**dict(dist=X, nh=X), **kw}))

    def nd(**kw):
        return ctypes.byref(capi.NodeDiff(**{**dict(base_dist=X, base_nh=X, changed=X, counts=X),
                                             **kw}))

    def diff(g=None, units=X, n=4, r=None, d=None, flags=0, w=1):
        return lib.ogs_spf_node_diff(g or graph(), units, n, r or rows(), d or nd(), flags, w, None)

    assert diff(n=0) == 0 and diff(n=-1) == I
    assert lib.ogs_spf_node_diff(None, X, 4, rows(), nd(), 0, 1, None) == I
    assert lib.ogs_spf_node_diff(graph(), X, 4, None, nd(), 0, 1, None) == I
    assert lib.ogs_spf_node_diff(graph(), X, 4, rows(), None, 0, 1, None) == I
    assert diff(units=None) == I
    assert diff(r=rows(dist=None)) == I and diff(r=rows(nh=None)) == I  # NULL rows
    assert diff(g=graph(node_base=None)) == I
    for field in ("base_dist", "base_nh", "changed", "counts"):
        assert diff(d=nd(**{field: None})) == I, field
    assert diff(w=3) == U and diff(w=0) == U and diff(w=8) == U
    assert diff(flags=WIDE) == U
    assert b"32-bit" in lib.ogs_last_error()
    assert diff(g=graph(max_nodes=0)) == U and diff(g=graph(max_nodes=(1 << 21) + 1)) == U

    def changes(**kw):
        return ctypes.byref(capi.NodeChanges(**{**dict(offsets=X, total=5, node=X, dist=X, nh=X),
                                                **kw}))

    def gather(changed=X, n=4, sn=10, r=None, w=1, c=None):
        return lib.ogs_spf_node_changes_gather(changed, n, sn, r or rows(), w, c or changes(), None)

    assert gather(n=0) == 0 and gather(sn=0) == 0 and gather(n=-1) == I
    assert gather(changed=None) == I and gather(c=changes(offsets=None)) == I
    assert gather(r=rows(dist=None)) == I and gather(r=rows(nh=None)) == I
    assert gather(w=3) == U
    assert gather(c=changes(total=0, node=None, dist=None, nh=None)) == 0  # nothing to write
    for field in ("node", "dist", "nh"):
        assert gather(c=changes(**{field: None})) == I, field


def test_constructor_takes_the_flag(host_module):
    """enableNodeSegmentLabel is a keyword of the constructor, default False;
    where a device is visible, off gives the form and flags of the sweep
    without the argument (the constructor uploads, so it needs one)."""
    import openr_amd
    M = host_module
    assert "enableNodeSegmentLabel: bool = False" in M.LinkFailureSweep.__init__.__doc__
    for name in ("mplsCounts", "changedLabels", "flags"):
        assert hasattr(M.LinkFailureSweep, name)
    als = M.AreaLinkStates()
    ls = als.add(L.kTestingAreaName, "1")
    ls.updateAdjacencyDatabase(L.createAdjDb("1", [L.adj12], 1), L.kTestingAreaName)
    ls.updateAdjacencyDatabase(L.createAdjDb("2", [L.adj21], 2), L.kTestingAreaName)
    ps = M.PrefixState()
    args = ("1", ls, ps, [{}], True, False)
    if openr_amd.decision.device_count() == 0:
        with pytest.raises(RuntimeError):  # no device, not a TypeError for the keyword
            M.LinkFailureSweep(*args, enableNodeSegmentLabel=False)
        return
    plain, off = M.LinkFailureSweep(*args), M.LinkFailureSweep(*args, enableNodeSegmentLabel=False)
    assert (plain.form(), plain.flags()) == (off.form(), off.flags())
