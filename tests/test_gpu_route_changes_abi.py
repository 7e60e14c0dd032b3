"""ogs_route_changes_gather on the device, through the C ABI with torch-owned
buffers, against abi_refs.route_changes_ref: one wavefront per unit and four
units per workgroup (unit counts off a multiple of 4), 64 bitmap words per
step (S_p on both sides of 2,048), a last word with bits at or past S_p, a
slice shorter than the unit's set bits. All comparisons are exact."""
import ctypes

import numpy as np
import pytest

import abi_refs as R
from abi_dev import Dev, ptr

pytestmark = pytest.mark.gpu

POISON = 0xDEADBEEF
# per unit: a full unit, an empty one, a full one, then sparse and half-set ones
DENSITIES = [1.0, 0.0, 1.0, 0.01, 0.5, 0.01, 1.0, 0.0, 0.5]


def make_case(seed, U, Sp, W, densities=None, tail_bits=False):
    rng = np.random.default_rng(seed)
    words = (Sp + 31) // 32
    dens = np.array((densities or DENSITIES)[:U])
    bits = rng.random((U, words * 32)) < dens[:, None]
    bits[:, Sp:] = tail_bits  # bits at or past max_prefixes: ignored
    changed = np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(-1)
    meta = rng.integers(0, 2**32, U * Sp, dtype=np.uint32)
    meta[rng.random(U * Sp) < 0.3] &= ~np.uint32(R.ROUTE_VALID)  # deletions
    metric = rng.integers(0, 2**32, U * Sp, dtype=np.uint32)
    mask = rng.integers(0, 2**32, U * W * Sp, dtype=np.uint32)    # [(u*W+w)*S_p+p]
    return dict(U=U, Sp=Sp, W=W, changed=changed, meta=meta, metric=metric, mask=mask)


def gather(dev, c, offsets, total, offset=0, null_records=False, slack=0):
    """one call on poisoned record arrays of total + slack records; -> (status, dict)"""
    capi, lib = dev.capi, dev.lib
    keep = [dev.put(c[k], offset) for k in ("changed", "meta", "metric", "mask")]
    t_off = dev.put(np.asarray(offsets, np.uint32), offset)
    n = total + slack
    out = {k: dev.put(np.full(max(m, 1), POISON, np.uint32), offset)
           for k, m in (("prefix", n), ("meta", n), ("metric", n), ("mask", c["W"] * total + slack))}
    rec = capi.SpfOut(meta=ptr(keep[1]), metric=ptr(keep[2]), mask=ptr(keep[3]))
    ch = capi.RouteChanges(ptr(t_off), total, *(
        [None] * 4 if null_records else [ptr(out[k]) for k in ("prefix", "meta", "metric", "mask")]))
    dev.sync()
    rc = lib.ogs_route_changes_gather(ptr(keep[0]), c["U"], c["Sp"], ctypes.byref(rec), c["W"],
                                      ctypes.byref(ch), None)
    dev.sync()
    return rc, {k: dev.get(v) for k, v in out.items()}


def want_records(c, offsets, total):
    out = {k: np.full(n, POISON, np.uint32) for k, n in
           (("prefix", total), ("meta", total), ("metric", total), ("mask", c["W"] * total))}
    return R.route_changes_ref(c["changed"], c["U"], c["Sp"], c["meta"], c["metric"], c["mask"],
                               c["W"], offsets, total, out)


def compare(c, got, want, total, label):
    W = c["W"]
    for k in ("prefix", "meta", "metric"):
        assert (got[k][:total] == want[k]).all(), label + (k,)
        assert (got[k][total:] == POISON).all(), label + (k, "past the records")
    for w in range(W):
        assert (got["mask"][w * total:(w + 1) * total] ==
                want["mask"][w * total:(w + 1) * total]).all(), label + ("mask", w)
    assert (got["mask"][W * total:] == POISON).all(), label + ("mask", "past the records")


def offsets_of(c):
    counts = R.route_changes_counts(c["changed"], c["U"], c["Sp"])
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)


@pytest.fixture(scope="module")
def dev(product):
    return Dev()


@pytest.mark.parametrize("W", [1, 2, 4])
@pytest.mark.parametrize("U", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("Sp", [31, 32, 33, 2047, 2048, 2049, 4097])
def test_gather(dev, Sp, U, W):
    seed = 0x6A7E00 + 64 * Sp + 8 * U + W
    # a single unit cannot mix densities in one call: one call per density
    mixes = [[d] for d in (0.0, 0.01, 0.5, 1.0)] if U == 1 else [DENSITIES]
    seen = 0
    for i, dens in enumerate(mixes):
        c = make_case(seed + 1000 * i, U, Sp, W, dens)
        offsets = offsets_of(c)
        total = int(offsets[-1])
        want = want_records(c, offsets, total)
        for offset in (0, 1):  # 16-byte aligned buffers, then views one element in
            rc, got = gather(dev, c, offsets, total, offset, slack=3)
            assert rc == 0
            compare(c, got, want, total, (Sp, U, W, i, offset))
        seen += total
    assert seen > 0
    if U >= 3:  # the empty unit between two full ones
        assert offsets[1] == Sp and offsets[2] == offsets[1] and offsets[3] - offsets[2] == Sp


@pytest.mark.parametrize("Sp", [33, 2049, 4097])
def test_bits_at_or_past_max_prefixes_are_ignored(dev, Sp):
    """every bit of the last word past S_p set, in every unit: no record for
    them and no shift of the later units' records"""
    c = make_case(0x6A7E01 + Sp, 5, Sp, 2, tail_bits=True)
    words = (Sp + 31) // 32
    last = c["changed"].reshape(5, words)[:, -1]
    assert ((last >> np.uint32(Sp % 32)) == (1 << (32 - Sp % 32)) - 1).all()
    offsets = offsets_of(c)
    total = int(offsets[-1])
    assert total == R.changed_bits(c["changed"], 5, Sp).sum()
    rc, got = gather(dev, c, offsets, total, slack=3)
    assert rc == 0
    compare(c, got, want_records(c, offsets, total), total, (Sp,))


@pytest.mark.parametrize("Sp", [33, 2049])
def test_short_slice(dev, Sp):
    """offsets[u + 1] - offsets[u] smaller than unit u's set bits (units 0 and
    2 are full): nothing at or past offsets[u + 1], the next unit's records
    intact, the records that fit are the unit's first ones"""
    c = make_case(0x6A7E02 + Sp, 5, Sp, 2)
    counts = R.route_changes_counts(c["changed"], 5, Sp).astype(np.int64)
    counts[0] -= 3
    counts[2] -= Sp - 1  # room for one record
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    total = int(offsets[-1])
    want = want_records(c, offsets, total)
    first = np.flatnonzero(R.changed_bits(c["changed"], 5, Sp)[0])
    assert want["prefix"][:offsets[1]].tolist() == first[:-3].tolist()
    rc, got = gather(dev, c, offsets, total, slack=3)
    assert rc == 0
    compare(c, got, want, total, (Sp,))


def test_no_records_and_null_arrays(dev):
    """total = 0 with NULL record arrays: OGS_OK, nothing written"""
    c = make_case(0x6A7E03, 3, 65, 2, [0.0, 0.0, 0.0])
    rc, got = gather(dev, c, np.zeros(4, np.uint32), 0, null_records=True)
    assert rc == 0
    assert all((v == POISON).all() for v in got.values())


def test_three_words_unsupported(dev):
    """a host-side check: no kernel runs"""
    c = make_case(0x6A7E04, 3, 65, 3)
    offsets = offsets_of(c)
    total = int(offsets[-1])
    rc, got = gather(dev, c, offsets, total)
    assert rc == dev.capi.OGS_E_UNSUPPORTED
    assert all((v == POISON).all() for v in got.values())
