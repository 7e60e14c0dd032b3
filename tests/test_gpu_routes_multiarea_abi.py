"""ogs_routes_multiarea (and its ogs_ctx_ form) on the device, through the C
ABI with torch-owned buffers, against abi_refs.routes_multiarea_ref on a
hand-packed random domain: several units with their own SPF rows (one with
OGS_NODE_NONE in an area), one to three areas, every next-hop width
instantiation and the runtime-width form, every v4 / best-route-selection
flag set, 32- and 64-bit distances (with the settled bitsets and a reached
node at the all-ones distance), a prefix table that starts at global prefix
7 and slack columns. All comparisons are exact."""
import ctypes

import numpy as np
import pytest

import abi_refs as R
from abi_dev import Dev, ptr

pytestmark = pytest.mark.gpu

G = 40  # node names of the domain
POISON32, POISON64 = 0xDEADBEEF, 0xDEADBEEFDEADBEEF
V4, V4O6, BRS, WIDE = R.F_ENABLE_V4, R.F_V4_OVER_V6, R.F_BEST_ROUTE_SELECTION, R.F_WIDE_METRIC
FLAG_SETS = [v | o | b for b in (0, BRS) for v in (0, V4) for o in (0, V4O6)]


def make_case(seed, U, A, W, flags, P=255, slack=5, p0=7, reached=False):
    rng = np.random.default_rng(seed)
    wide = bool(flags & WIDE)
    # names x areas with holes; a node's id is the rank of its name in its area
    present = rng.random((G, A)) < 0.75
    sources = rng.choice(G, U, replace=False)
    present[sources[0], :] = True
    if U > 1:  # one unit's source has no adjacency database in an area
        present[sources[1], A - 1] = False
    name_local = np.where(present, np.cumsum(present, 0) - 1, R.NONE).astype(np.uint32)
    nodes = present.sum(0)
    node_base = np.concatenate([[0], np.cumsum(nodes)]).astype(np.uint32)
    Sn = int(nodes.max()) + 3
    kind = rng.random(int(node_base[-1]))
    node_flags = np.select(
        [kind < 0.15, kind < 0.22, kind < 0.27],
        [R.NODE_OVERLOADED, R.NODE_SOFTDRAIN | R.NODE_METRICINC, R.NODE_METRICINC], 0).astype(np.uint8)
    # SPF rows of the (source, area) pairs that have one, in shuffled order
    pairs = [(u, a) for u in range(U) for a in range(A) if present[sources[u], a]]
    order = rng.permutation(len(pairs))
    spf_row = np.full(U * A, R.NONE, np.uint32)
    for r, i in enumerate(order):
        spf_row[pairs[i][0] * A + pairs[i][1]] = r
    rows = len(pairs)
    inf = 2**64 - 1 if wide else 2**32 - 1
    dist = rng.integers(1, 3, (rows, Sn)).astype(np.uint64 if wide else np.uint32)  # many ties
    if wide:
        dist += rng.integers(0, 2, (rows, Sn)).astype(np.uint64) << np.uint64(33)
    nh = np.zeros((rows, W, Sn), np.uint32)
    linked = rng.random((rows, Sn)) < 0.88  # the rest: reached over no link slot
    for on in (linked, linked & (rng.random((rows, Sn)) < 0.5)):  # one or two slots, any word
        rr, vv = np.nonzero(on)
        nh[rr, rng.integers(0, W, len(rr)), vv] |= np.uint32(1) << rng.integers(
            0, 32, len(rr)).astype(np.uint32)
    unreached = rng.random((rows, Sn)) < 0.15
    garbage = rng.integers(0, 2**32, (rows, W, Sn), dtype=np.uint32)
    nh = np.where(unreached[:, None, :], garbage, nh)
    rw = (Sn + 31) // 32
    settled = None
    if reached:  # the bitset decides: unreached distances are garbage, a reached one all ones
        settled_bits = np.zeros((rows, rw * 32), bool)
        settled_bits[:, :Sn] = ~unreached
        dist[~unreached & (rng.random((rows, Sn)) < 0.08)] = inf
        settled = np.packbits(settled_bits, axis=1, bitorder="little").view(np.uint32).reshape(-1)
    else:
        dist[unreached] = inf
    for r, i in enumerate(order):  # the source's own node: 0, no next hop
        u, a = pairs[i]
        v = name_local[sources[u], a]
        row = int(spf_row[u * A + a])
        dist[row, v], nh[row, :, v] = 0, 0
        if settled is not None:
            settled.reshape(rows, rw)[row, int(v) // 32] |= np.uint32(1 << (int(v) % 32))
    # the prefix table: p0 leading prefixes of another topology, then P of this one
    PT = p0 + P
    keys = [n * A + a for n in range(G) for a in range(A) if present[n, a]]
    absent = [n * A + a for n in range(G) for a in range(A) if not present[n, a]]
    segs, v4, minnh = [], [], []
    for gp in range(PT):
        roll = rng.random()
        size = int(rng.integers(33, 41)) if roll < 0.04 else int(rng.choice([1, 1, 2, 2, 3, 3, 4]))
        size = min(size, len(keys))
        pick = set(rng.choice(keys, size, replace=False).tolist())
        if absent and rng.random() < 0.1:  # an advertiser with no adjacency database
            pick.add(int(rng.choice(absent)))
        if rng.random() < 0.08:  # a source advertises it
            pick.add(int(sources[rng.integers(0, U)]) * A + int(rng.integers(0, A)))
        segs.append(sorted(pick))  # (name, area) key order
        v4.append(rng.random() < 0.1)
        minnh.append(rng.random() < 0.12)
    adv_off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint32)
    flat = np.array([k for s in segs for k in s])
    T = len(flat)
    adv_name, adv_area = (flat // A).astype(np.uint32), (flat % A).astype(np.uint32)
    adv_node = name_local[adv_name, adv_area]  # OGS_NODE_NONE: no adjacency database there
    # mostly equal, so best-route selection often keeps several entries
    adv_metrics = np.stack([rng.random(T) < 0.08, 100 + 100 * (rng.random(T) < 0.07),
                            100 + 100 * (rng.random(T) < 0.07), 1 + (rng.random(T) < 0.1)],
                           1).astype(np.int32)
    adv_min_nh = np.full(T, R.MIN_NH_UNSET, np.int64)
    pfx_flags = np.zeros(PT, np.uint8)
    for gp in range(PT):
        lo, hi = int(adv_off[gp]), int(adv_off[gp + 1])
        if v4[gp]:
            pfx_flags[gp] |= R.PFX_V4
        if minnh[gp]:
            some = np.flatnonzero(rng.random(hi - lo) < 0.6)
            if len(some):
                adv_min_nh[lo + some] = rng.integers(1, 4, len(some))
                pfx_flags[gp] |= R.PFX_HAS_MIN_NH
    Sp = P + slack
    return dict(
        U=U, A=A, W=W, flags=flags, P=P, Sp=Sp, p0=p0, Sn=Sn, wide=wide, T=T,
        graph=dict(max_nodes=Sn, node_base=node_base, node_flags=node_flags),
        table=dict(max_prefixes=Sp, pfx_base=np.array([p0, PT], np.uint32), adv_off=adv_off,
                   adv_node=adv_node, adv_metrics=adv_metrics.reshape(-1), adv_min_nh=adv_min_nh,
                   pfx_flags=pfx_flags),
        areas=dict(num_areas=A, name_local=name_local.reshape(-1), adv_area=adv_area,
                   adv_name=adv_name, reached=settled),
        units=sources.astype(np.uint32), spf_row=spf_row, dist=dist.reshape(-1),
        nh=nh.reshape(-1))


def poison(c):
    n = c["U"] * c["Sp"]
    return dict(meta=np.full(n, POISON32, np.uint32),
                metric=np.full(n, POISON64 if c["wide"] else POISON32,
                               np.uint64 if c["wide"] else np.uint32),
                sel=np.full(n, POISON32, np.uint32),
                mask=np.full(n * c["A"] * c["W"], POISON32, np.uint32))


def reference(c):
    return R.routes_multiarea_ref(c["graph"], c["table"], c["areas"], c["units"], c["U"],
                                  c["spf_row"], c["dist"], c["nh"], c["flags"], c["W"], poison(c))


def check_not_vacuous(c, want):
    """on the reference's side: every outcome this flag set can produce occurs"""
    U, Sp, P, A, W = c["U"], c["Sp"], c["P"], c["A"], c["W"]
    meta = want["meta"].reshape(U, Sp)[:, :P]
    valid = (meta & R.ROUTE_VALID) != 0
    reasons = set(R.reason_of(meta[~valid]).tolist())
    expect = {R.REASON_UNREACHABLE, R.REASON_SELF, R.REASON_NO_NEXTHOP, R.REASON_MIN_NEXTHOP}
    if not c["flags"] & (V4 | V4O6):  # the only flag set the v4 gate closes
        expect.add(R.REASON_V4_DISABLED)
    assert reasons == expect, (reasons, expect)
    assert valid.sum() * 3 >= valid.size, (valid.sum(), valid.size)
    if A > 1:
        per_area = want["mask"].reshape(U, A, W, Sp)[:, :, :, :P].any(2)  # [U, A, P]
        assert (valid & (per_area.sum(1) >= 2)).any()
    if U > 1:
        assert (c["spf_row"] == R.NONE).any()


def launch(dev, c, skip=None, ctx=None, stream=None):
    """-> the four outputs as numpy arrays (None for the one passed as NULL)"""
    capi, lib = dev.capi, dev.lib
    g, t, a = c["graph"], c["table"], c["areas"]
    d = {k: dev.put(v) for k, v in (
        ("node_base", g["node_base"]), ("node_flags", g["node_flags"]), ("pfx_base", t["pfx_base"]),
        ("adv_off", t["adv_off"]), ("adv_node", t["adv_node"]), ("adv_metrics", t["adv_metrics"]),
        ("adv_min_nh", t["adv_min_nh"]), ("pfx_flags", t["pfx_flags"]),
        ("name_local", a["name_local"]), ("adv_area", a["adv_area"]), ("adv_name", a["adv_name"]),
        ("units", c["units"]), ("spf_row", c["spf_row"]), ("dist", c["dist"]), ("nh", c["nh"]))}
    t_reached = dev.put(a["reached"]) if a["reached"] is not None else None
    outs = {k: (None if k == skip else dev.put(v)) for k, v in poison(c).items()}
    graph = capi.Graph(num_topos=c["A"], max_nodes=c["Sn"], node_base=ptr(d["node_base"]),
                       node_flags=ptr(d["node_flags"]))
    table = capi.PrefixTable(c["Sp"], c["T"], ptr(d["pfx_base"]), ptr(d["adv_off"]),
                             ptr(d["adv_node"]), ptr(d["adv_metrics"]), ptr(d["adv_min_nh"]),
                             ptr(d["pfx_flags"]))
    areas = capi.AreaTable(c["A"], G, ptr(d["name_local"]), ptr(d["adv_area"]), ptr(d["adv_name"]),
                           ptr(t_reached))
    out = capi.SpfOut(meta=ptr(outs["meta"]), metric=ptr(outs["metric"]), mask=ptr(outs["mask"]),
                      sel=ptr(outs["sel"]))
    args = (ctypes.byref(graph), ctypes.byref(table), ctypes.byref(areas), ptr(d["units"]), c["U"],
            ptr(d["spf_row"]), ptr(d["dist"]), ptr(d["nh"]), c["flags"], c["W"], ctypes.byref(out),
            stream)
    dev.sync()  # the uploads, before a launch on any stream
    if ctx is None:
        capi.check(lib, lib.ogs_routes_multiarea(*args), "ogs_routes_multiarea")
    else:
        capi.check(lib, lib.ogs_ctx_routes_multiarea(ctx, *args), "ogs_ctx_routes_multiarea")
    dev.sync()
    return {k: None if v is None else dev.get(v, np.uint64 if k == "metric" and c["wide"]
                                              else np.uint32) for k, v in outs.items()}


def run_case(dev, c, skip=None, ctx=None, stream=None):
    want = reference(c)
    check_not_vacuous(c, want)
    got = launch(dev, c, skip, ctx, stream)
    label = {k: c[k] for k in ("U", "A", "W", "flags", "P", "Sp", "p0")}
    U, Sp, P = c["U"], c["Sp"], c["P"]
    for k in ("meta", "metric", "sel", "mask"):
        if k == skip:
            continue
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (label, k, bad[:8].tolist(), got[k][bad[:8]].tolist(),
                               want[k][bad[:8]].tolist())
        cols = got[k].reshape(-1, Sp)[:, P:]  # slack columns keep their poison
        assert (cols == (POISON64 if k == "metric" and c["wide"] else POISON32)).all(), (label, k)


@pytest.fixture(scope="module")
def dev(product):
    return Dev()


# (U, A, W, flags, P, slack, p0, reached)
SHAPES = [(U, A, W, FLAG_SETS[(3 * i + j + k) % 8] | (WIDE if (i + j + k) % 2 else 0),
           (255, 257)[(i + k) % 2], (5, 0)[(j + k) % 2], (7, 0)[(i + j) % 2], False)
          for k, U in enumerate((1, 4)) for i, A in enumerate((1, 2, 3))
          for j, W in enumerate((1, 2, 3, 4, 8, 16))]
FLAGS = [(4, 3, 2, f | w, 257, 5, 7, r) for f in FLAG_SETS
         for w, r in ((0, False), (WIDE, False), (WIDE, True))]
CASES = SHAPES + FLAGS


def case_seed(i):
    return 0x3A7EA00 + i


def case_id(c):
    return "U%d-A%d-W%d-f%02x-P%d+%d-base%d%s" % (c[:7] + ("-reached" if c[7] else "",))


@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_routes_multiarea(dev, i):
    U, A, W, flags, P, slack, p0, reached = CASES[i]
    run_case(dev, make_case(case_seed(i), U, A, W, flags, P, slack, p0, reached))


@pytest.mark.parametrize("skip", ["meta", "metric", "sel", "mask"])
def test_one_output_null(dev, skip):
    """each output NULL in turn: the others are still right"""
    run_case(dev, make_case(0x3A7EB00, 4, 3, 3, BRS | WIDE, 257, 5, 7, True), skip=skip)


def test_context_form_on_a_side_stream(dev):
    """ogs_ctx_routes_multiarea on a second context and a side stream"""
    capi, lib, torch = dev.capi, dev.lib, dev.torch
    ctx = ctypes.c_void_p()
    capi.check(lib, lib.ogs_ctx_create(0, ctypes.byref(ctx)), "ogs_ctx_create")
    try:
        stream = torch.cuda.Stream(dev.dev)
        run_case(dev, make_case(0x3A7EB01, 3, 3, 4, BRS | V4, 257, 5, 7), ctx=ctx,
                 stream=ctypes.c_void_p(stream.cuda_stream))
    finally:
        lib.ogs_ctx_destroy(ctx)
