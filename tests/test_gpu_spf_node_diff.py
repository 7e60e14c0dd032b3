"""ogs_spf_node_diff and ogs_spf_node_changes_gather on the device, through
the C ABI with torch-owned buffers, against a numpy restatement of the rule in
include/openr_gpu.h: node v of a unit is changed when its reachedness differs
from the base's, or both are reached and the distance or any next-hop word
differs; never the source, never a node at or past the topology's count, never
a node outside the interest mask, never anything of a refused unit."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INF = 0xFFFFFFFF
POISON = 0xDEADBEEF
SIZES = [31, 32, 33, 64, 65, 2049]


def make_rows(rng, U, W, Sn, src):
    """a random base and U units that copy it with a seeded 10 % of the nodes
    perturbed, one kind a node: 0 distance only, 1 one next-hop word only (the
    last word for every second one), 2 reached -> unreached, 3 unreached ->
    reached, 4 next-hop garbage under an unreached row (NOT a change)"""
    bd = rng.integers(1, 1000, Sn, dtype=np.uint32)
    bd[rng.random(Sn) < 0.15] = INF
    bnh = rng.integers(0, 2**32, (W, Sn), dtype=np.uint32)
    d = np.repeat(bd[None], U, 0).copy()
    nh = np.repeat(bnh[None], U, 0).copy()
    for u in range(U):
        for v in np.flatnonzero(rng.random(Sn) < 0.10):
            kind = int(rng.integers(0, 5))
            reached = bd[v] != INF
            if kind == 0 and reached:
                d[u, v] += 1
            elif kind == 1 and reached:
                w = W - 1 if v % 2 else int(rng.integers(0, W))
                nh[u, w, v] ^= np.uint32(1 << int(rng.integers(0, 32)))
            elif kind == 2 and reached:
                d[u, v] = INF
            elif kind == 3 and not reached:
                d[u, v] = 7
            elif not reached:
                nh[u, :, v] = rng.integers(0, 2**32, W, dtype=np.uint32)
        d[u, src] = 12345  # the source's own row: never reported
        nh[u, 0, src] ^= np.uint32(1)
    return bd, bnh, d, nh


def reference(bd, bnh, d, nh, N, src, interest, refused):
    """changed [U, Sn] bool"""
    ra, rb = d != INF, (bd != INF)[None]
    ch = (ra != rb) | (ra & rb & ((d != bd[None]) | (nh != bnh[None]).any(1)))
    ch[:, N:] = False
    ch[:, src] = False
    if interest is not None:
        ch &= interest[None]
    for u in refused:
        ch[u] = False
    return ch


def pack(bits, words):
    """[..., Sn] bool -> [..., words] uint32, bit v % 32 of word v / 32"""
    pad = np.zeros(bits.shape[:-1] + (words * 32,), dtype=np.uint8)
    pad[..., :bits.shape[-1]] = bits
    return np.packbits(pad, axis=-1, bitorder="little").view(np.uint32)


class Dev:
    def __init__(self):
        import torch
        import openr_amd.capi as capi
        self.torch, self.capi, self.lib = torch, capi, capi.load()
        self.dev = torch.device("cuda:0")

    def put(self, a, offset=0):
        """a on the device as int32 words, `offset` elements into a larger buffer
        (offset 1: 4-byte aligned only, so the element loads run)"""
        flat = np.ascontiguousarray(a).view(np.int32).reshape(-1)
        buf = self.torch.empty(flat.size + offset + 3, dtype=self.torch.int32, device=self.dev)
        view = buf[offset:offset + flat.size]
        view.copy_(self.torch.from_numpy(flat))
        assert view.data_ptr() % 16 == (4 * offset) % 16
        return view

    def get(self, t):
        return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def dev(product):
    return Dev()


def run_case(dev, rng, U, W, Sn, N, offset, masked):
    capi, lib, torch = dev.capi, dev.lib, dev.torch
    words = (Sn + 31) // 32
    src = int(rng.integers(0, N))
    bd, bnh, d, nh = make_rows(rng, U, W, Sn, src)
    refused = [2] if U > 2 else []
    counts_in = np.zeros(2 * U, dtype=np.uint32)
    for u in refused:  # wrote no rows: whatever is there must not be read into the answer
        counts_in[2 * u] = counts_in[2 * u + 1] = INF
        d[u], nh[u] = POISON, POISON
    interest = None
    if masked:
        interest = rng.random(Sn) < 0.7
        for v in (30, 31, 32, 33):  # both sides of a word edge, on and off
            if v < Sn:
                interest[v] = v in (31, 32)
    want = reference(bd, bnh, d, nh, N, src, interest, refused)

    t_bd, t_bnh = dev.put(bd, offset), dev.put(bnh, offset)
    t_d, t_nh = dev.put(d, offset), dev.put(nh, offset)
    t_units = dev.put(np.array([[0, src]] * U, dtype=np.uint32))
    t_base = dev.put(np.array([0, N], dtype=np.uint32))
    t_interest = dev.put(pack(interest, words)) if masked else None
    t_counts_in = dev.put(counts_in)
    t_changed = torch.full((U * words,), -1, dtype=torch.int32, device=dev.dev)  # written whole
    t_counts = torch.full((U,), -1, dtype=torch.int32, device=dev.dev)
    g = capi.Graph(num_topos=1, max_nodes=Sn, node_base=t_base.data_ptr())
    rows = capi.SpfOut(dist=t_d.data_ptr(), nh=t_nh.data_ptr())
    nd = capi.NodeDiff(t_bd.data_ptr(), t_bnh.data_ptr(),
                       t_interest.data_ptr() if masked else None, t_counts_in.data_ptr(),
                       t_changed.data_ptr(), t_counts.data_ptr())
    capi.check(lib, lib.ogs_spf_node_diff(ctypes.byref(g), t_units.data_ptr(), U,
                                          ctypes.byref(rows), ctypes.byref(nd), 0, W, None),
               "ogs_spf_node_diff")
    torch.cuda.synchronize()
    label = (U, W, Sn, N, offset, masked)
    got = dev.get(t_changed).reshape(U, words)
    assert (got == pack(want, words)).all(), label
    counts = dev.get(t_counts)
    assert counts.tolist() == want.sum(1).tolist(), label
    for u in refused:
        assert counts[u] == 0 and not got[u].any(), label

    # the gather: unit-major, node ascending
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    total = int(offsets[-1])
    t_off = dev.put(offsets)
    t_node = torch.full((max(total, 1),), -1, dtype=torch.int32, device=dev.dev)
    t_dist = torch.full((max(total, 1),), -1, dtype=torch.int32, device=dev.dev)
    t_cnh = torch.full((W * max(total, 1),), -1, dtype=torch.int32, device=dev.dev)
    ch = capi.NodeChanges(t_off.data_ptr(), total, t_node.data_ptr(), t_dist.data_ptr(),
                          t_cnh.data_ptr())
    capi.check(lib, lib.ogs_spf_node_changes_gather(t_changed.data_ptr(), U, Sn,
                                                    ctypes.byref(rows), W, ctypes.byref(ch), None),
               "ogs_spf_node_changes_gather")
    torch.cuda.synchronize()
    us, vs = np.nonzero(want)  # row-major: unit-major, node ascending
    assert len(us) == total
    assert dev.get(t_node)[:total].tolist() == vs.tolist(), label
    assert dev.get(t_dist)[:total].tolist() == d[us, vs].tolist(), label
    gnh = dev.get(t_cnh)[:W * total].reshape(W, total) if total else np.zeros((W, 0))
    for w in range(W):
        assert gnh[w].tolist() == nh[us, w, vs].tolist(), label + (w,)
    return total


@pytest.mark.parametrize("W", [1, 2, 4])
@pytest.mark.parametrize("Sn", SIZES)
def test_diff_and_gather(dev, Sn, W):
    rng = np.random.default_rng(0x5EED0 + 8 * Sn + W)
    total = 0
    for N in (Sn, Sn - 3):
        for U in (1, 5):
            for offset, masked in ((0, False), (1, False), (0, True), (1, True)):
                total += run_case(dev, rng, U, W, Sn, N, offset, masked)
    assert total > 0  # the perturbations reach the comparison


def test_equal_rows_report_nothing(dev):
    """units equal to the base: zero counts, a zero bitmap over the ones it held,
    and a gather of no record with NULL record arrays"""
    capi, lib, torch = dev.capi, dev.lib, dev.torch
    rng = np.random.default_rng(7)
    U, W, Sn = 3, 2, 65
    words = 3
    bd, bnh, _, _ = make_rows(rng, U, W, Sn, 0)
    d, nh = np.repeat(bd[None], U, 0), np.repeat(bnh[None], U, 0)
    t_bd, t_bnh, t_d, t_nh = dev.put(bd), dev.put(bnh), dev.put(d), dev.put(nh)
    t_units = dev.put(np.array([[0, 4]] * U, dtype=np.uint32))
    t_base = dev.put(np.array([0, Sn], dtype=np.uint32))
    t_changed = torch.full((U * words,), -1, dtype=torch.int32, device=dev.dev)
    t_counts = torch.full((U,), -1, dtype=torch.int32, device=dev.dev)
    g = capi.Graph(num_topos=1, max_nodes=Sn, node_base=t_base.data_ptr())
    rows = capi.SpfOut(dist=t_d.data_ptr(), nh=t_nh.data_ptr())
    nd = capi.NodeDiff(t_bd.data_ptr(), t_bnh.data_ptr(), None, None, t_changed.data_ptr(),
                       t_counts.data_ptr())
    capi.check(lib, lib.ogs_spf_node_diff(ctypes.byref(g), t_units.data_ptr(), U,
                                          ctypes.byref(rows), ctypes.byref(nd), 0, W, None),
               "ogs_spf_node_diff")
    torch.cuda.synchronize()
    assert not dev.get(t_changed).any() and not dev.get(t_counts).any()
    t_off = dev.put(np.zeros(U + 1, dtype=np.uint32))
    ch = capi.NodeChanges(t_off.data_ptr(), 0, None, None, None)
    assert lib.ogs_spf_node_changes_gather(t_changed.data_ptr(), U, Sn, ctypes.byref(rows), W,
                                           ctypes.byref(ch), None) == 0
    torch.cuda.synchronize()
