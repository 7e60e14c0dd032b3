"""ogs_spf_routes_whatif_pairs on the device with torch-owned buffers: the
seeded 5x5 grid with a drained baseline (test_gpu_whatif_restore's world: 25
nodes, 20 prefixes a node + the anycast extras), every node's base records from
ONE ogs_spf_routes launch, ~60 scenario rows of every kind as raw id lists, and
a shuffled subset of (source, scenario) pairs as units -- so unit index, base
row and scenario row all differ. Every output row must equal, byte for byte,
what ogs_spf_routes_whatif writes for that source over that source's pairs
(its own base, per-unit lists), with and without OGS_F_CHANGED_ONLY. The mix
of outcomes is asserted on the per-source reference side."""
import ctypes
import random

import numpy as np
import pytest

import test_gpu_whatif_restore as TR

pytestmark = pytest.mark.gpu

ENABLE_V4, INCREMENTAL, CHANGED_ONLY, RESTORE = 0x01, 0x40, 0x80, 0x100
EDGE_UP, CLEAR_SHIFT = 0x80000000, 4
OVERLOADED, SOFT_BITS = 1, 2 | 4
FILL = -7
REFUSED = [-1, -1]  # OGS_WHATIF_REFUSED as int32


class Grid:
    def __init__(self, product):
        import torch

        import openr_amd.capi as capi
        self.torch, self.capi, self.lib = torch, capi, capi.load()
        self.dev = torch.device("cuda:0")
        als, ls, ps = TR.grid_world(True).load(product, TR.ME)
        h = self.h = product.area_host_arrays(ls, ps)
        up = lambda key, dt: torch.from_numpy(h[key].view(dt)).to(self.dev)  # noqa: E731
        t = self.t = {k: up(k, dt) for k, dt in (
            ("node_base", "int32"), ("row_ptr", "int32"), ("edges", "int64"),
            ("node_flags", "uint8"), ("topo_desc", "int32"), ("pfx_base", "int32"),
            ("adv_off", "int32"), ("adv_node", "int32"), ("adv_metrics", "int32"),
            ("adv_min_nh", "int64"), ("pfx_flags", "uint8"), ("edge_src", "int32"))}
        self.Sn, self.Sp, self.E = h["max_nodes"], h["max_prefixes"], h["max_edges"]
        self.N = len(h["names"])
        assert (self.N, self.Sn) == (25, 25) and self.Sp >= 500
        self.words = (self.Sp + 31) // 32
        self.g = capi.Graph(1, self.Sn, self.E, h["max_degree"], t["node_base"].data_ptr(),
                            t["row_ptr"].data_ptr(), t["edges"].data_ptr(),
                            t["node_flags"].data_ptr(), t["topo_desc"].data_ptr())
        self.g.edge_src = t["edge_src"].data_ptr()
        self.pt = capi.PrefixTable(self.Sp, h["max_advertisements"], t["pfx_base"].data_ptr(),
                                   t["adv_off"].data_ptr(), t["adv_node"].data_ptr(),
                                   t["adv_metrics"].data_ptr(), t["adv_min_nh"].data_ptr(),
                                   t["pfx_flags"].data_ptr())
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        # every node's base: one launch, unit-major rows
        self.base, so = self.outs(self.N)
        units = self.u32([x for s in range(self.N) for x in (0, s)])
        capi.check(self.lib, self.lib.ogs_spf_routes(
            ctypes.byref(self.g), ctypes.byref(self.pt), ctypes.c_void_p(units.data_ptr()), self.N,
            ENABLE_V4, 1, ctypes.byref(so), self.stream), "ogs_spf_routes")
        torch.cuda.synchronize()
        self.rows = scenario_rows(h)

    def u32(self, values, dtype=np.uint32):
        a = np.asarray(list(values) or [0], dtype=np.int64).astype(dtype)
        view = a.view(np.int32) if dtype == np.uint32 else a
        return self.torch.from_numpy(view.copy()).to(self.dev)

    def outs(self, U):
        torch = self.torch
        o = {k: torch.full((U * n,), FILL, dtype=torch.int32, device=self.dev)
             for k, n in (("dist", self.Sn), ("nh", self.Sn), ("meta", self.Sp),
                          ("metric", self.Sp), ("mask", self.Sp), ("sel", self.Sp))}
        so = self.capi.SpfOut(o["dist"].data_ptr(), o["nh"].data_ptr(), o["meta"].data_ptr(),
                              o["metric"].data_ptr(), o["mask"].data_ptr(), o["sel"].data_ptr())
        return o, so

    def mods(self, rows, keep):
        """ogs_whatif_mods over `rows` (one CSR row each), always with the node
        and the metric triple"""
        def csr(lists, dtype=np.uint32):
            off, flat = [0], []
            for l in lists:
                flat += list(l)
                off.append(len(flat))
            t = (self.u32(off), self.u32(flat, dtype))
            keep.extend(t)
            return t
        d_off, d_list = csr([r["dead"] for r in rows])
        n_off, n_list = csr([r["nodes"] for r in rows])
        _, n_bits = csr([r["bits"] for r in rows], np.uint8)
        m_off, m_edge = csr([[e for e, _ in r["metrics"]] for r in rows])
        _, m_val = csr([[v for _, v in r["metrics"]] for r in rows])
        longest = max([len(r["metrics"]) for r in rows] + [1])
        return self.capi.WhatifMods(d_off.data_ptr(), d_list.data_ptr(), n_off.data_ptr(),
                                    n_list.data_ptr(), n_bits.data_ptr(), m_off.data_ptr(),
                                    m_edge.data_ptr(), m_val.data_ptr(), longest)

    def diff(self, o, U, base_row=0):
        torch, b = self.torch, self.base
        o["changed"] = torch.full((U * self.words,), FILL, dtype=torch.int32, device=self.dev)
        o["counts"] = torch.full((U * 2,), FILL, dtype=torch.int32, device=self.dev)
        at = lambda k, n: b[k].data_ptr() + 4 * base_row * n  # noqa: E731
        return self.capi.RouteDiff(at("meta", self.Sp), at("metric", self.Sp), at("mask", self.Sp),
                                   o["changed"].data_ptr(), o["counts"].data_ptr(),
                                   at("dist", self.Sn), at("nh", self.Sn), None, None, 0)

    def whatif(self, flags, src, ks):
        """ogs_spf_routes_whatif from `src` over scenario rows `ks`, against
        src's base row"""
        U, keep = len(ks), []
        o, so = self.outs(U)
        diff = self.diff(o, U, src)
        units = self.u32([x for _ in ks for x in (0, src)])
        mods = self.mods([self.rows[k] for k in ks], keep)
        rc = self.lib.ogs_spf_routes_whatif(
            ctypes.byref(self.g), ctypes.byref(self.pt), ctypes.c_void_p(units.data_ptr()), U,
            ctypes.byref(mods), ctypes.byref(diff), ENABLE_V4 | RESTORE | flags, 1,
            ctypes.byref(so), self.stream)
        self.capi.check(self.lib, rc, "ogs_spf_routes_whatif")
        self.torch.cuda.synchronize()
        return o

    def pairs(self, flags, units, n_bases=None, n_scenarios=None):
        """ogs_spf_routes_whatif_pairs over units [(source, base row, scenario row)]"""
        U, keep = len(units), []
        o, so = self.outs(U)
        diff = self.diff(o, U)
        du = self.u32([x for s, _, _ in units for x in (0, s)])
        base, scen = self.u32([b for _, b, _ in units]), self.u32([k for _, _, k in units])
        mods = self.mods(self.rows, keep)
        p = self.capi.WhatifPairs(base.data_ptr(), scen.data_ptr(),
                                  self.N if n_bases is None else n_bases,
                                  len(self.rows) if n_scenarios is None else n_scenarios)
        rc = self.lib.ogs_spf_routes_whatif_pairs(
            ctypes.byref(self.g), ctypes.byref(self.pt), ctypes.c_void_p(du.data_ptr()), U,
            ctypes.byref(p), ctypes.byref(mods), ctypes.byref(diff), ENABLE_V4 | RESTORE | flags,
            1, ctypes.byref(so), self.stream)
        self.capi.check(self.lib, rc, "ogs_spf_routes_whatif_pairs")
        self.torch.cuda.synchronize()
        return o


def scenario_rows(h):
    """~60 rows of raw id lists over the grid's CSR: dead links, hard and soft
    drains, raised and lowered metrics, the restorations, an empty row, a row
    of ids past the topology and a row with a metric value of 0"""
    rng = random.Random(0x9A125)
    edges = h["edges"].view(np.uint64)
    lo = (edges & np.uint64(0xFFFFFFFF)).astype(np.int64)
    dst, down, wt = lo & 0x1FFFFF, (lo >> 31) & 1, (edges >> np.uint64(32)).astype(np.int64)
    src = h["edge_src"].astype(np.int64)
    flags = h["node_flags"]
    E, N = len(edges), len(flags)
    rev = {e: next(r for r in range(E) if src[r] == dst[e] and dst[r] == src[e]) for e in range(E)}
    links = [(e, rev[e]) for e in range(E) if src[e] < dst[e]]
    up = [l for l in links if not down[l[0]]]
    dn = [l for l in links if down[l[0]]]
    hard = [n for n in range(N) if flags[n] & OVERLOADED]
    soft = [n for n in range(N) if flags[n] & 2]
    plain = [n for n in range(N) if not flags[n]]
    assert len(dn) >= 4 and len(hard) == 3 and len(soft) == 2

    def row(dead=(), nodes=(), metrics=()):
        nodes = sorted(nodes)
        return {"dead": sorted(dead), "nodes": [n for n, _ in nodes],
                "bits": [b for _, b in nodes], "metrics": sorted(metrics)}

    def moved(link, weight):
        return [(link[0], weight), (link[1], weight)]

    def node_links(n, delta):
        return [m for l in up if n in (src[l[0]], dst[l[0]])
                for m in moved(l, max(1, int(wt[l[0]]) + delta))]

    rows = []
    rows += [row(dead=l) for l in rng.sample(up, 12)]
    rows += [row(dead=[e for l in rng.sample(up, 3) for e in l]) for _ in range(4)]
    rows += [row(nodes=[(n, OVERLOADED)]) for n in rng.sample(plain, 6)]
    rows += [row(nodes=[(n, SOFT_BITS)], metrics=node_links(n, 50)) for n in rng.sample(plain, 4)]
    rows += [row(metrics=moved(l, 4 * int(wt[l[0]]))) for l in rng.sample(up, 10)]
    rows += [row(metrics=moved(l, 1)) for l in rng.sample([l for l in up if wt[l[0]] > 1], 8)]
    rows += [row(nodes=[(n, OVERLOADED << CLEAR_SHIFT)]) for n in hard + [plain[0]]]
    rows += [row(nodes=[(n, OVERLOADED << CLEAR_SHIFT) for n in hard[:2]])]
    rows += [row(metrics=moved(l, int(wt[l[0]]) | EDGE_UP)) for l in dn[:4]]
    rows += [row(nodes=[(n, SOFT_BITS << CLEAR_SHIFT)], metrics=node_links(n, -50)) for n in soft]
    rows += [row(dead=up[0], nodes=[(plain[1], OVERLOADED), (hard[0], OVERLOADED << CLEAR_SHIFT)],
                 metrics=moved(up[5], 9 * int(wt[up[5][0]])) + moved(dn[0], 3 | EDGE_UP))]
    rows += [row(), row(dead=[E, 0xFFFFFFFF], nodes=[(N + 3, OVERLOADED)],
                        metrics=[(E + 1, 0), (E + 9, 5)])]
    rows += [row(metrics=[(up[2][0], 7), (up[2][1], 0)])]  # a weight of 0: the unit is refused
    assert 55 <= len(rows) <= 65
    return rows


@pytest.fixture(scope="module")
def grid(product):
    return Grid(product)


def _units(grid):
    """a shuffled subset of the pairs of 10 sources: >= 8 base rows used, some
    unused; three units that must be refused among them"""
    rng = random.Random(0x5A1F)
    me = grid.h["names"].index(TR.ME)  # hard-drained itself
    sources = sorted(set(rng.sample(range(grid.N), 9)) | {me})
    K = len(grid.rows)
    units = [(s, s, k) for s in sources for k in range(K)]
    rng.shuffle(units)
    units = units[:int(len(units) * 0.7)]
    bad = {40: (3, grid.N, 5), 200: (3, 3, K), 333: (4, 0xFFFFFFFF, 0xFFFFFFFF)}
    for at, u in bad.items():
        units.insert(at, u)
    assert len({b for _, b, _ in units} & set(range(grid.N))) >= 8
    assert len(set(range(grid.N)) - {b for _, b, _ in units}) >= 10
    assert sum(u != b or u != k for u, (_, b, k) in enumerate(units)) > len(units) - 5
    return sources, units, set(bad)


@pytest.mark.parametrize("flags", [INCREMENTAL, INCREMENTAL | CHANGED_ONLY],
                         ids=["repair", "changed-only"])
def test_pairs_equal_the_per_source_entry(grid, flags):
    torch = grid.torch
    sources, units, bad = _units(grid)
    U, K = len(units), len(grid.rows)
    got = grid.pairs(flags, units)
    view = lambda o, k, n: o[k].view(n, -1)  # noqa: E731
    kinds, changed_of = set(), {}
    for s in sources:
        mine = [u for u, (src, _, _) in enumerate(units) if src == s and u not in bad]
        ref = grid.whatif(flags, s, [units[u][2] for u in mine])
        for key in ref:
            assert torch.equal(view(got, key, U)[mine], view(ref, key, len(mine))), (s, key)
        counts = view(ref, "counts", len(mine)).tolist()
        for i, u in enumerate(mine):
            c = counts[i]
            kinds.add("refused" if c == REFUSED else "empty" if c == [0, 0] else
                      "update" if c[1] == 0 else "delete")
            changed_of.setdefault(units[u][2], []).append(view(ref, "changed", len(mine))[i])
            if c != REFUSED and flags & CHANGED_ONLY:
                # records exactly at the changed prefixes
                bits = view(ref, "changed", len(mine))[i]
                n = sum(bin(w & 0xFFFFFFFF).count("1") for w in bits.tolist())
                assert n == c[0] + c[1]
                assert int((view(ref, "meta", len(mine))[i] != FILL).sum()) == n
    # refused: an out-of-range base row, an out-of-range scenario row, both
    for u in bad:
        assert view(got, "counts", U)[u].tolist() == REFUSED
        assert not view(got, "changed", U)[u].any()
        for key in ("meta", "metric", "mask", "sel", "dist", "nh"):
            assert (view(got, key, U)[u] == FILL).all(), (u, key)
    # the mix, on the reference side
    assert kinds == {"refused", "empty", "update", "delete"}
    differ = sum(any(not torch.equal(rows[0], r) for r in rows[1:])
                 for rows in changed_of.values())
    assert len(changed_of) == K and all(len(r) >= 2 for r in changed_of.values())
    assert differ >= K // 2, (differ, K)


def test_pair_bounds_follow_the_call(grid):
    """n_bases / n_scenarios are the call's: the same unit is computed under
    one bound and refused under a smaller one, its neighbours untouched"""
    units = [(5, 5, 3), (9, 9, 20), (5, 5, 21)]
    flags = INCREMENTAL | CHANGED_ONLY
    full = grid.pairs(flags, units)
    assert full["counts"].view(3, 2)[1].tolist() != REFUSED
    for kw, keep in ((dict(n_bases=9), [0, 2]), (dict(n_scenarios=20), [0])):  # rows 20, 21
        got = grid.pairs(flags, units, **kw)
        for u in sorted({0, 1, 2} - set(keep)):
            assert got["counts"].view(3, 2)[u].tolist() == REFUSED
            assert not got["changed"].view(3, -1)[u].any()
            assert (got["meta"].view(3, -1)[u] == FILL).all()
        for key in got:
            assert grid.torch.equal(got[key].view(3, -1)[keep], full[key].view(3, -1)[keep]), key
