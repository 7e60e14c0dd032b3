"""ogs_rib_policy_apply (and its ogs_ctx_ form) on the device, through the C
ABI with torch-owned buffers, against abi_refs.rib_policy_ref: several units
with their own slot_nonzero slices and records, several areas, every next-hop
width instantiation (1, 2, 4, 8, 16) and the runtime-width form (3, 17), a
prefix table that starts at global prefix 7, slack columns past the table's
prefixes, chunked policies. All comparisons are exact."""
import ctypes

import numpy as np
import pytest

import abi_refs as R
from abi_dev import Dev, ptr

pytestmark = pytest.mark.gpu

POISON16, POISON32 = 0xA5A5, 0xDEADBEEF


def make_case(seed, U, A, W, P, slack, p0, K):
    """a seeded random prefix table of one topology, records of U units and a
    K-statement policy (K may pass 32: match tables are [rows, K] bool)"""
    rng = np.random.default_rng(seed)
    Sp, PT = P + slack, p0 + P
    seg = rng.integers(1, 5, PT)
    adv_off = np.concatenate([[0], np.cumsum(seg)]).astype(np.uint32)
    T = int(adv_off[-1])
    # records: about a fifth not valid, the best index anywhere in the segment
    valid = rng.random((U, Sp)) < 0.8
    best = (rng.random((U, Sp)) * np.concatenate([seg[p0:], np.ones(slack, int)])[None]).astype(
        np.uint32)
    meta = np.where(valid, R.ROUTE_VALID | (rng.integers(0, 8, (U, Sp)) << 1),
                    rng.integers(1, 6, (U, Sp)) << R.REASON_SHIFT).astype(np.uint32)
    meta |= best << R.BEST_SHIFT
    meta[:, P:] = POISON32
    # one to three next hops anywhere in the areas' words
    mask = np.zeros((U, A, W, Sp), np.uint32)
    for _ in range(3):
        on = rng.random((U, Sp)) < (1.0 if _ == 0 else 0.5)
        a, w = rng.integers(0, A, (U, Sp)), rng.integers(0, W, (U, Sp))
        bit = (np.uint32(1) << rng.integers(0, 32, (U, Sp)).astype(np.uint32))
        uu, pp = np.nonzero(on)
        mask[uu, a[uu, pp], w[uu, pp], pp] |= bit[uu, pp]
    mask[:, :, :, P:] = POISON32
    # the K = 1 policy must still transform a tenth of the routes
    dense = K == 1
    active_bits = rng.random(K) < 0.85
    active_bits[0] = True
    pfx_bits = rng.random((PT, K)) < (0.8 if dense else 0.45)
    tag_bits = rng.random((T, K)) < (0.8 if dense else 0.6)
    # each unit its own weights; a quarter of its link slots weigh 0 under every
    # statement, so some routes match and are never transformed
    nz = rng.integers(0, 2**32, (U, K, A, W), dtype=np.uint32)
    nz &= ~(rng.integers(0, 2**32, (U, 1, A, W), dtype=np.uint32) &
            rng.integers(0, 2**32, (U, 1, A, W), dtype=np.uint32))
    return dict(U=U, A=A, W=W, P=P, Sp=Sp, p0=p0, K=K, T=T,
                pfx_base=np.array([p0, PT], np.uint32), adv_off=adv_off, meta=meta.reshape(-1),
                mask=mask.reshape(-1), active_bits=active_bits, pfx_bits=pfx_bits,
                tag_bits=tag_bits, nz=nz)


def pack_bits(bits):
    """[rows, <= 32] bool -> [rows] uint32"""
    k = bits.shape[1]
    return (bits.astype(np.uint64) << np.arange(k, dtype=np.uint64)[None]).sum(1).astype(np.uint32)


def chunk(c, lo, hi):
    """statements lo..hi-1 of the case's policy as one ogs_rib_policy chunk"""
    active = int(pack_bits(c["active_bits"][None, lo:hi])[0])
    return dict(num_statements=hi - lo, statement_base=lo, active=active,
                pfx_match=pack_bits(c["pfx_bits"][:, lo:hi]),
                adv_tag_match=pack_bits(c["tag_bits"][:, lo:hi]),
                slot_nonzero=np.ascontiguousarray(c["nz"][:, lo:hi]).reshape(-1))


def whole(c):
    active = sum(1 << k for k in range(c["K"]) if c["active_bits"][k])
    return dict(num_statements=c["K"], statement_base=0, active=active, pfx_match=c["pfx_bits"],
                adv_tag_match=c["tag_bits"], slot_nonzero=c["nz"].reshape(-1))


def reference(c):
    """one pass over the whole policy, from poisoned applied / counter columns"""
    n = c["U"] * c["Sp"]
    return R.rib_policy_ref(c["pfx_base"], c["adv_off"], c["Sp"], whole(c), c["A"], c["U"],
                            c["W"], c["meta"], c["mask"], np.full(n, POISON16, np.uint16),
                            np.full(n, POISON16, np.uint16))


def check_not_vacuous(c, want):
    """on the reference's side: every outcome of the walk occurs"""
    U, Sp, P, K = c["U"], c["Sp"], c["P"], c["K"]
    meta = c["meta"].reshape(U, Sp)[:, :P]
    app = want[1].reshape(U, Sp)[:, :P].astype(np.int64)
    cnt = want[2].reshape(U, Sp)[:, :P].astype(np.int64)
    valid = (meta & R.ROUTE_VALID) != 0
    took = app != R.POLICY_NONE
    assert not took[~valid].any() and (cnt[~valid] == R.POLICY_NONE).all()
    assert took.sum() * 10 >= valid.sum(), (took.sum(), valid.sum())
    assert (cnt != app).any()  # matched, every next hop dropped, not transformed
    if K > 1:  # (with one statement a route's first match is its only one)
        gp = c["p0"] + np.arange(P)
        bestent = c["adv_off"][gp][None].astype(np.int64) + (meta >> R.BEST_SHIFT)
        match = (c["pfx_bits"][gp][None] & c["tag_bits"][np.where(valid, bestent, 0)] &
                 c["active_bits"][None, None])          # [U, P, K]
        first = np.where(match.any(2), match.argmax(2), R.POLICY_NONE)
        assert (took & (app != first)).any()  # transformed by a later match than its first


def apply(dev, c, pol, t_meta, t_mask, t_app, t_cnt, ctx=None, stream=None):
    capi, lib = dev.capi, dev.lib
    keep = [dev.put(c["pfx_base"]), dev.put(c["adv_off"]), dev.put(pol["pfx_match"]),
            dev.put(pol["adv_tag_match"]), dev.put(pol["slot_nonzero"])]
    pt = capi.PrefixTable(max_prefixes=c["Sp"], max_advertisements=c["T"],
                          pfx_base=ptr(keep[0]), adv_off=ptr(keep[1]))
    rp = capi.RibPolicy(pol["num_statements"], pol["active"], ptr(keep[2]), ptr(keep[3]),
                        ptr(keep[4]), pol["statement_base"])
    args = (ctypes.byref(pt), ctypes.byref(rp), c["A"], c["U"], c["W"], ptr(t_meta), ptr(t_mask),
            ptr(t_app), ptr(t_cnt), stream)
    dev.sync()  # the uploads, before a launch on any stream
    if ctx is None:
        capi.check(lib, lib.ogs_rib_policy_apply(*args), "ogs_rib_policy_apply")
    else:
        capi.check(lib, lib.ogs_ctx_rib_policy_apply(ctx, *args), "ogs_ctx_rib_policy_apply")
    dev.sync()
    return keep


def run_case(dev, c, chunks=None, with_columns=True, ctx=None, stream=None):
    want = reference(c)
    check_not_vacuous(c, want)
    U, Sp, P = c["U"], c["Sp"], c["P"]
    n = U * Sp
    t_meta, t_mask = dev.put(c["meta"]), dev.put(c["mask"])
    t_app = dev.put(np.full(n, POISON16, np.uint16)) if with_columns else None
    t_cnt = dev.put(np.full(n, POISON16, np.uint16)) if with_columns else None
    for lo, hi in chunks or [(0, c["K"])]:
        apply(dev, c, chunk(c, lo, hi), t_meta, t_mask, t_app, t_cnt, ctx, stream)
    label = {k: c[k] for k in ("U", "A", "W", "P", "Sp", "p0", "K")}
    got_mask = dev.get(t_mask)
    assert (dev.get(t_meta) == c["meta"]).all(), label  # meta is never written
    assert (got_mask == want[0]).all(), label
    m4, in4 = got_mask.reshape(U, c["A"], c["W"], Sp), c["mask"].reshape(U, c["A"], c["W"], Sp)
    assert (m4[:, :, :, P:] == POISON32).all(), label   # slack columns
    invalid = (c["meta"].reshape(U, Sp) & R.ROUTE_VALID) == 0
    assert (m4.transpose(0, 3, 1, 2)[invalid] == in4.transpose(0, 3, 1, 2)[invalid]).all(), label
    if with_columns:
        got_app, got_cnt = dev.get(t_app, np.uint16), dev.get(t_cnt, np.uint16)
        assert (got_app == want[1]).all(), label
        assert (got_cnt == want[2]).all(), label
        assert (got_app.reshape(U, Sp)[:, P:] == POISON16).all(), label
        assert (got_cnt.reshape(U, Sp)[:, P:] == POISON16).all(), label


@pytest.fixture(scope="module")
def dev(product):
    return Dev()


CASES = (
    # (U, A, W, P, slack, p0, K): units x areas
    [(U, A, 2, 257, 5, 7, 32) for U in (1, 3, 5) for A in (1, 2, 3)] +
    # every width instantiation and the runtime-width form, one and three areas
    [(3, A, W, 255, 0, 0, 31) for W in (1, 2, 3, 4, 8, 16, 17) for A in (1, 3)] +
    # the table's size around the block of 256 threads, slack, the table's base
    [(3, 2, 3, P, slack, p0, 31) for P in (255, 256, 257) for slack in (0, 5) for p0 in (0, 7)] +
    [(3, 2, 4, 257, 5, 7, K) for K in (1, 31, 32)])


def case_seed(i):
    return 0xAB1E00 + i


@pytest.mark.parametrize("i", range(len(CASES)), ids=[
    "U%d-A%d-W%d-P%d+%d-base%d-K%d" % c for c in CASES])
def test_policy_apply(dev, i):
    run_case(dev, make_case(case_seed(i), *CASES[i]))


def test_seventy_statements_in_three_chunks(dev):
    """statement_base 0, 32, 64 with K = 32, 32, 6, chaining applied / counter,
    equals one walk over the 70 statements"""
    run_case(dev, make_case(0xAB1E70, 3, 2, 2, 257, 5, 7, 70), chunks=[(0, 32), (32, 64), (64, 70)])


def test_first_chunk_without_applied_and_counter(dev):
    run_case(dev, make_case(0xAB1E71, 3, 2, 2, 257, 5, 7, 32), with_columns=False)


def test_context_form_on_a_side_stream(dev):
    """ogs_ctx_rib_policy_apply on a second context and a side stream"""
    capi, lib, torch = dev.capi, dev.lib, dev.torch
    ctx = ctypes.c_void_p()
    capi.check(lib, lib.ogs_ctx_create(0, ctypes.byref(ctx)), "ogs_ctx_create")
    try:
        stream = torch.cuda.Stream(dev.dev)
        run_case(dev, make_case(0xAB1E72, 3, 2, 3, 257, 5, 7, 32), ctx=ctx,
                 stream=ctypes.c_void_p(stream.cuda_stream))
    finally:
        lib.ogs_ctx_destroy(ctx)
