"""ogs_route_delta (include/openr_gpu.h, ABI 8) through the raw C-ABI with
torch-owned device buffers, against a numpy restatement of its rule
(RibUnicastEntry::operator==, RibEntry.h:81-87, as ogs_route_diff states it,
plus the selection kind). Synthetic records, no SPF: a seeded random `prev`,
`next` = `prev` with one mutation per chosen prefix. Every output column and
the header must be equal, in ascending prefix order; nothing may be written
past the capacity."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VALID, DRAINED, LOCAL, SELECTED = 0x1, 0x2, 0x4, 0x8
REASON_SHIFT, BEST_SHIFT = 4, 8
ROUTE, SELECTION = 0x1, 0x2
F_WIDE = 0x10
NONE16 = 0xFFFF
# word, tile and multi-tile edges of the 2048-prefix tile
SIZES = [1, 31, 32, 33, 2047, 2048, 2049, 70001]
FILL = 0x5A5A5A5A


def _table(rng, P):
    """adv_off [P+1] and adv_class [2A]: advertisers 0 and 1 of a prefix with
    two or more are the same class (as is, and drained)."""
    k = rng.integers(1, 5, size=P)
    adv_off = np.concatenate([[0], np.cumsum(k)]).astype(np.uint32)
    cls = np.zeros(2 * int(adv_off[-1]), dtype=np.uint32)
    for p in range(P):
        a0, n = int(adv_off[p]), int(k[p])
        vals = list(rng.integers(0, 3, size=n)) + list(rng.integers(3, 6, size=n))
        if n >= 2:
            vals[1], vals[n + 1] = vals[0], vals[n]
        for j in range(2 * n):
            c = vals.index(vals[j])
            cls[2 * (a0 + j % n) + j // n] = c
    return k, adv_off, cls


def _prev(rng, P, W, wide, k):
    valid = rng.random(P) < 0.7
    meta = np.where(valid, VALID, rng.integers(1, 6, size=P) << REASON_SHIFT).astype(np.uint32)
    meta |= (rng.integers(0, 2, size=P) * DRAINED).astype(np.uint32)
    meta |= (rng.integers(0, 2, size=P) * LOCAL).astype(np.uint32)
    meta |= (rng.integers(0, 2, size=P) * SELECTED).astype(np.uint32)
    meta |= ((rng.integers(0, 4, size=P) % k) << BEST_SHIFT).astype(np.uint32)
    hi = (1 << 40) if wide else (1 << 31)
    return dict(
        meta=meta,
        metric=rng.integers(0, hi, size=P).astype(np.uint64 if wide else np.uint32),
        mask=rng.integers(0, 1 << 32, size=W * P, dtype=np.uint64).astype(np.uint32),
        sel=rng.integers(0, 16, size=P).astype(np.uint32),
        applied=rng.integers(0, 3, size=P).astype(np.uint16),
        counter=np.where(rng.random(P) < 0.5, NONE16, rng.integers(0, 3, size=P)).astype(np.uint16))


def _mutate(rng, prev, P, W, k, density, policy):
    nxt = {n: a.copy() for n, a in prev.items()}
    chosen = np.nonzero(rng.random(P) < density)[0] if density < 1 else np.arange(P)
    kinds = rng.integers(0, 11, size=len(chosen))
    seen = set()
    for p, m in zip(chosen, kinds):
        v = bool(prev["meta"][p] & VALID)
        if m == 5 and v:
            m = 1  # the reason field exists on invalid records only
        if m == 4 and k[p] < 2:
            m = 2
        if m in (8, 9) and not policy:
            m = 7
        seen.add(int(m))
        if m == 0:  # valid <-> invalid
            nxt["meta"][p] = (prev["meta"][p] & ~np.uint32(VALID | 0xF0)) | np.uint32(
                (0 if v else VALID) | ((rng.integers(1, 6) << REASON_SHIFT) if v else 0))
        elif m == 1:  # metric only
            nxt["metric"][p] = prev["metric"][p] + 1
        elif m == 2:  # one mask word in the last W row
            nxt["mask"][(W - 1) * P + p] ^= np.uint32(1 << int(rng.integers(0, 32)))
        elif m == 3:  # sel only: SELECTION without ROUTE
            nxt["sel"][p] ^= np.uint32(1 << int(rng.integers(0, 4)))
        elif m == 4:  # best -> an advertiser of the same class
            best = int(prev["meta"][p] >> BEST_SHIFT)
            other = 1 - best if best < 2 else 0
            # from 2+ the class may differ: both outcomes are in the reference
            nxt["meta"][p] = (prev["meta"][p] & np.uint32(0xFF)) | np.uint32(other << BEST_SHIFT)
        elif m == 5:  # igp-irrelevant: the reason of an invalid record
            r = int(prev["meta"][p] >> REASON_SHIFT) & 0xF
            nxt["meta"][p] = (prev["meta"][p] & ~np.uint32(0xF0)) | np.uint32(
                (r % 5 + 1) << REASON_SHIFT)
        elif m == 6:
            nxt["meta"][p] ^= np.uint32(LOCAL)
        elif m == 7:
            nxt["meta"][p] ^= np.uint32(DRAINED)
        elif m == 8:
            nxt["applied"][p] ^= np.uint16(1)
        elif m == 9:
            nxt["counter"][p] ^= np.uint16(1)
        else:
            nxt["meta"][p] ^= np.uint32(SELECTED)
    return nxt, seen


def _reference(prev, nxt, P, W, adv_off, adv_class, policy):
    a, b = nxt["meta"], prev["meta"]
    va, vb = (a & VALID) != 0, (b & VALID) != 0
    if adv_class is not None:
        def cls(m):
            return adv_class[2 * (adv_off[:-1] + (m >> BEST_SHIFT)) + ((m & DRAINED) != 0)]
        # the class lookup is read for valid records only
        best = (((a ^ b) & LOCAL) != 0) | (cls(np.where(va, a, 0)) != cls(np.where(vb, b, 0)))
    else:
        best = ((a ^ b) & np.uint32(DRAINED | LOCAL | (0xFFFFFF << BEST_SHIFT))) != 0
    diff = best | (nxt["metric"] != prev["metric"])
    for w in range(W):
        diff |= nxt["mask"][w * P:(w + 1) * P] != prev["mask"][w * P:(w + 1) * P]
    if policy:
        diff |= (nxt["applied"] != prev["applied"]) | (nxt["counter"] != prev["counter"])
    route = (va != vb) | (va & vb & diff)
    sel = (((a ^ b) & np.uint32(SELECTED | DRAINED | (0xFFFFFF << BEST_SHIFT))) != 0) | \
        (nxt["sel"] != prev["sel"])
    idx = np.nonzero(route | sel)[0].astype(np.uint32)
    reason = (a >> REASON_SHIFT) & 0xF
    header = [len(idx), int((va & route).sum()), int((vb & ~va).sum()),
              int((~va & ((reason == 2) | (reason == 4))).sum())]
    cols = dict(prefix=idx, kind=(route * ROUTE + sel * SELECTION).astype(np.uint32)[idx],
                meta=a[idx], metric=nxt["metric"][idx], sel=nxt["sel"][idx],
                mask=[nxt["mask"][w * P:(w + 1) * P][idx] for w in range(W)])
    if policy:
        cols["applied"], cols["counter"] = nxt["applied"][idx], nxt["counter"][idx]
    return header, cols, route, sel


class _Device:
    def __init__(self):
        import torch

        import openr_amd.capi as capi
        self.torch, self.capi = torch, capi
        self.lib = capi.load()
        self.dev = torch.device("cuda:0")

    def up(self, a, shift=0):
        """device copy of a numpy array (viewed as signed for torch), optionally
        `shift` elements into a larger allocation (a misaligned base)"""
        t = self.torch
        signed = {np.dtype("uint16"): np.int16, np.dtype("uint32"): np.int32,
                  np.dtype("uint64"): np.int64}[a.dtype]
        src = t.from_numpy(np.ascontiguousarray(a).view(signed))
        buf = t.empty(len(a) + shift, dtype=src.dtype, device=self.dev)
        buf[shift:] = src.to(self.dev)
        return buf[shift:]

    def run(self, prev, nxt, P, W, wide, adv_off, adv_class, policy, cap, shift=0):
        t, capi = self.torch, self.capi
        keep = []

        def side(r):
            d = {n: self.up(r[n], shift) for n in ("meta", "metric", "mask", "sel", "applied",
                                                   "counter")}
            keep.append(d)
            return d, capi.SpfOut(None, None, d["meta"].data_ptr(), d["metric"].data_ptr(),
                                  d["mask"].data_ptr(), d["sel"].data_ptr(), None)
        dp, sp = side(prev)
        dn, sn = side(nxt)
        pad = 64  # past the capacity: must stay FILL
        fill32 = np.int32(FILL)

        def out(n, dtype=t.int32):
            v = {t.int32: int(fill32), t.int64: int(fill32), t.int16: 0x5A5A}[dtype]
            return t.full((n + pad,), v, dtype=dtype, device=self.dev)
        o = dict(prefix=out(cap), kind=out(cap), meta=out(cap),
                 metric=out(cap, t.int64 if wide else t.int32), mask=out(W * cap), sel=out(cap),
                 applied=out(cap, t.int16), counter=out(cap, t.int16), header=out(4))
        do = capi.RouteDeltaOut(cap, o["prefix"].data_ptr(), o["kind"].data_ptr(),
                                o["meta"].data_ptr(), o["metric"].data_ptr(),
                                o["mask"].data_ptr(), o["sel"].data_ptr(),
                                o["applied"].data_ptr(), o["counter"].data_ptr(),
                                o["header"].data_ptr())
        pol = None
        if policy:
            pol = ctypes.byref(capi.RouteDeltaPolicy(
                dp["applied"].data_ptr(), dp["counter"].data_ptr(), dn["applied"].data_ptr(),
                dn["counter"].data_ptr()))
        off = cls = None
        if adv_class is not None:
            off, cls = self.up(adv_off), self.up(adv_class)
        # garbage in the workspace: the call zeroes nothing it relies on
        ws = t.full((capi.route_delta_workspace_bytes(P) // 4,), -1, dtype=t.int32,
                    device=self.dev)
        stream = t.cuda.current_stream()
        capi.check(self.lib, self.lib.ogs_route_delta(
            ctypes.byref(sp), ctypes.byref(sn), P, off.data_ptr() if off is not None else None,
            cls.data_ptr() if cls is not None else None, pol, F_WIDE if wide else 0, W,
            ctypes.byref(do), ws.data_ptr(), ctypes.c_void_p(stream.cuda_stream)),
            "ogs_route_delta")
        t.cuda.synchronize()
        unsigned = {t.int16: np.uint16, t.int32: np.uint32, t.int64: np.uint64}
        return {n: v.cpu().numpy().view(unsigned[v.dtype]) for n, v in o.items()}


@pytest.fixture(scope="module")
def device(product):
    return _Device()


def _compare(got, header, cols, W, cap, policy, label):
    total = header[0]
    assert list(got["header"][:4]) == header, (label, "header")
    n = min(total, cap)
    assert np.all(np.diff(got["prefix"][:n].astype(np.int64)) > 0), (label, "order")
    names = ["prefix", "kind", "meta", "metric", "sel"] + (["applied", "counter"] if policy else [])
    for name in names:
        assert np.array_equal(got[name][:n], cols[name][:n]), (label, name)
        fill = got[name][n:]
        assert np.all(fill == fill[-1]) and len(fill) >= 64, (label, name, "past the records")
    for w in range(W):
        assert np.array_equal(got["mask"][w * cap:w * cap + n], cols["mask"][w][:n]), \
            (label, "mask", w)
        assert np.all(got["mask"][w * cap + n:(w + 1) * cap] == np.uint32(FILL)), (label, w)
    assert np.all(got["mask"][W * cap:] == np.uint32(FILL)), (label, "mask tail")
    assert np.all(got["header"][4:] == np.uint32(FILL)), (label, "header tail")
    if not policy:  # columns left alone without a policy
        assert np.all(got["applied"] == 0x5A5A) and np.all(got["counter"] == 0x5A5A), label


@pytest.mark.parametrize("wide", [False, True], ids=["u32", "u64"])
@pytest.mark.parametrize("W", [1, 2, 4])
def test_delta_matches_numpy_rule(device, W, wide):
    seen_all = set()
    for P in SIZES:
        rng = np.random.default_rng(0xD17A0000 + P * 8 + W * 2 + wide)
        k, adv_off, adv_class = _table(rng, P)
        prev = _prev(rng, P, W, wide, k)
        for density in (0.0, 0.01, 1.0):
            nxt, seen = _mutate(rng, prev, P, W, k, density, True)
            seen_all |= seen
            for policy in (False, True):
                for classes in (None, adv_class):
                    header, cols, route, sel = _reference(prev, nxt, P, W, adv_off, classes,
                                                          policy)
                    label = (P, W, wide, density, policy, classes is not None)
                    if density == 0.0:
                        assert header[:3] == [0, 0, 0], label
                    got = device.run(prev, nxt, P, W, wide, adv_off, classes, policy, cap=P)
                    _compare(got, header, cols, W, P, policy, label)
    assert seen_all == set(range(11))  # every mutation kind was drawn


def test_mutation_kinds_report_as_stated(device):
    """One prefix per property the issue names, checked by kind."""
    P, W = 64, 2
    rng = np.random.default_rng(7)
    k = np.full(P, 2)
    adv_off = (np.arange(P + 1) * 2).astype(np.uint32)
    adv_class = np.tile(np.array([0, 2, 0, 2], dtype=np.uint32), P)  # advertisers 0 == 1
    prev = _prev(rng, P, W, False, k)
    prev["meta"][:] = VALID | SELECTED
    prev["meta"][40:] = 2 << REASON_SHIFT  # invalid, unreachable
    nxt = {n: a.copy() for n, a in prev.items()}
    nxt["sel"][3] ^= 1                                  # sel only
    nxt["meta"][5] |= 1 << BEST_SHIFT                   # same-class advertiser
    nxt["meta"][41] = 4 << REASON_SHIFT                 # reason of an invalid record
    nxt["metric"][7] += 1                               # metric only
    nxt["mask"][(W - 1) * P + 9] ^= 1                   # last mask row
    nxt["meta"][11] = 2 << REASON_SHIFT                 # valid -> invalid
    nxt["meta"][42] = VALID                             # invalid -> valid
    want = {3: SELECTION, 5: SELECTION, 7: ROUTE, 9: ROUTE, 11: ROUTE | SELECTION, 42: ROUTE}
    got = device.run(prev, nxt, P, W, False, adv_off, adv_class, False, cap=P)
    n = int(got["header"][0])
    assert dict(zip(got["prefix"][:n].tolist(), got["kind"][:n].tolist())) == want
    # to_update {7, 9, 42}, to_delete {11}; no_route: 40..63 minus 42 (valid)
    # with reason 2 or 4, plus 11
    assert list(got["header"][:4]) == [6, 3, 1, 24]
    # without classes the same-class advertiser is a ROUTE change too
    want[5] = ROUTE | SELECTION
    got = device.run(prev, nxt, P, W, False, adv_off, None, False, cap=P)
    n = int(got["header"][0])
    assert dict(zip(got["prefix"][:n].tolist(), got["kind"][:n].tolist())) == want


@pytest.mark.parametrize("P,shift", [(2049, 0), (4096, 0), (4096, 1)])
def test_capacity_below_total_and_misaligned_rows(device, P, shift):
    """Nothing past the capacity is written and the header keeps the true
    total; rows whose base is not 16-byte aligned take the element loads."""
    W = 2
    rng = np.random.default_rng(P + shift)
    k, adv_off, adv_class = _table(rng, P)
    prev = _prev(rng, P, W, True, k)
    nxt, _ = _mutate(rng, prev, P, W, k, 0.5, True)
    header, cols, _, _ = _reference(prev, nxt, P, W, adv_off, adv_class, True)
    assert header[0] > 600
    for cap in (header[0], header[0] // 2, 1, 0):
        got = device.run(prev, nxt, P, W, True, adv_off, adv_class, True, cap=cap, shift=shift)
        _compare(got, header, cols, W, cap, True, (P, shift, cap))
