// spf_repair_body.h -- the statements of the variant repair, one body for
// the kernels spf_frontier.hip defines around it (spf_variant_repair_kernel,
// spf_whatif_repair_kernel, spf_whatif_pairs_kernel). Included INSIDE a
// kernel definition, so each kernel compiles the statements against its own
// parameters: the instantiations that existed before the what-if form keep
// their code generation. A shared
// __forceinline__ template body was tried first, with the kernel arguments
// passed by reference and then by value: both times
// spf_variant_repair_kernel<false, true, false> and <false, false, false>
// went from 67 to 69 VGPRs (the restrict-qualified kernel arguments reach an
// inlined callee as scoped alias metadata, not as noalias arguments, and the
// schedule moves); included in place, every earlier instantiation keeps its
// VGPR, scratch, LDS and occupancy figures. In scope at the include:
// constexpr bools CHANGED_ONLY, LIST, DRAINS, WHATIF and the kernel parameters
// g, pt, key, units, flags, oDist, oNh, out, mods, diff, desc.
// No include guard: it is included once per kernel.
  static_assert(LIST || !DRAINS, "drains come with the list form");
  static_assert(LIST || !WHATIF, "the what-if form is a list form");
  constexpr uint32_t kInf = 0xFFFFFFFFu;
  const int tid = threadIdx.x;
  const uint32_t u0 = blockIdx.x;
  const ogs_unit unit = units[u0];
  const uint32_t s = unit.src;
  const uint32_t nb = g.node_base[unit.topo];
  const uint32_t N = g.node_base[unit.topo + 1] - nb;
  const uint32_t* __restrict__ gRow = g.row_ptr + nb;
  const uint32_t e0 = gRow[0];
  const uint64_t* __restrict__ edges = g.edges + e0;
  const uint8_t* gflags = g.node_flags + nb;  // the base's
  const uint32_t Sn = uint32_t(g.max_nodes);
  const bool hop = (flags & OGS_F_HOP_METRIC) != 0;
  const uint32_t* __restrict__ bD = diff.base_dist;
  const uint32_t* __restrict__ bN = diff.base_nh;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint64_t* dn = reinterpret_cast<uint64_t*>(smem);                      // [Sn]
  uint32_t* stamp = reinterpret_cast<uint32_t*>(dn + Sn);                // [Sn]
  uint16_t* q0 = reinterpret_cast<uint16_t*>(stamp + ((Sn + 3u) & ~3u));  // [Sn]
  uint16_t* q1 = q0 + ((Sn + 1u) & ~1u);                                 // [Sn]
  uint32_t* inA = reinterpret_cast<uint32_t*>(q1 + ((Sn + 1u) & ~1u));   // [Sn/32]
  __shared__ uint32_t qcnt[3], cnt[2];
  auto isA = [&](uint32_t v) { return (inA[v >> 5] >> (v & 31u)) & 1u; };
  // LIST: the unit's slices, the bitset [ceil(max_edges/32)] and the flag row
  uint32_t l0 = 0, l1 = 0, r0 = 0, r1 = 0, E = 0;
  uint32_t* deadBits = nullptr;
  uint8_t* lflags = nullptr;
  const uint32_t* nodeList = nullptr;  // the unit's drained / flagged nodes
  // WHATIF: {dead, overridden} words, the metric slice, the two unit flags
  uint64_t* bb = nullptr;
  uint32_t *me = nullptr, *mv = nullptr, *wf = nullptr;
  uint32_t m0 = 0, mn = 0;
  if constexpr (WHATIF) {
    __shared__ uint32_t whatifFlags[2];  // refused, lowers
    wf = whatifFlags;
    l0 = mods.dead_off[u0];
    l1 = mods.dead_off[u0 + 1];
    E = gRow[N] - e0;
    const uint32_t ew = (uint32_t(g.max_edges) + 31u) / 32u;
    bb = reinterpret_cast<uint64_t*>(inA + (((Sn + 31u) / 32u + 1u) & ~1u));  // 8-aligned
    deadBits = reinterpret_cast<uint32_t*>(bb);
    uint32_t* after = deadBits + 2u * ew;
    if constexpr (DRAINS) {
      r0 = mods.node_off[u0];
      r1 = mods.node_off[u0 + 1];
      nodeList = mods.node_ids;
      lflags = reinterpret_cast<uint8_t*>(after);
      after += ((Sn + 3u) & ~3u) / 4u;
    }
    me = after;
    mv = me + mods.max_metric_per_unit;
    // under OGS_F_HOP_METRIC the metric lists are ignored, but for the up flags
    // of OGS_F_RESTORE
    if (mods.metric_off && (!hop || (flags & OGS_F_RESTORE))) {
      m0 = mods.metric_off[u0];
      mn = mods.metric_off[u0 + 1] - m0;
    }
  } else if constexpr (LIST) {
    l0 = mods.dead_off[u0];
    l1 = mods.dead_off[u0 + 1];
    E = gRow[N] - e0;
    deadBits = inA + (Sn + 31u) / 32u;
    if constexpr (DRAINS) {
      r0 = mods.drain_off[u0];
      r1 = mods.drain_off[u0 + 1];
      nodeList = mods.drain_nodes;
      lflags = reinterpret_cast<uint8_t*>(deadBits + (uint32_t(g.max_edges) + 31u) / 32u);
    }
  }
  const bool drains = DRAINS && r1 > r0;  // unit-uniform
  // (the drained row is written above the seeds: no restrict on it)
  typedef const uint8_t* __restrict__ FlagsRestrict;
  std::conditional_t<DRAINS, const uint8_t*, FlagsRestrict> nflags = drains ? lflags : gflags;
  // the base's tight DAG (seeds, growth rounds) is told by the base's flags
  auto relaxesBase = [&](uint32_t v) { return v == s || !(gflags[v] & OGS_NODE_OVERLOADED); };
  auto relaxes = [&](uint32_t v) { return v == s || !(nflags[v] & OGS_NODE_OVERLOADED); };
  auto seed = [&](uint32_t v) {
    if (!(atomicOr(&inA[v >> 5], 1u << (v & 31u)) & (1u << (v & 31u)))) {
      q1[atomicAdd(&qcnt[1], 1u)] = uint16_t(v);
    }
  };
  // head of dead edge e when the edge is tight in the base
  auto seedOf = [&](uint32_t e) {
    const uint32_t u = g.edge_src[e0 + e];
    const uint64_t x = edges[e];
    const uint32_t lo = static_cast<uint32_t>(x);
    const uint32_t v = edge_dst(lo);
    const uint32_t w = hop ? 1u : static_cast<uint32_t>(x >> 32);
    if (!(lo & OGS_EDGE_DOWN) && relaxesBase(u) && bD[u] != kInf && bD[u] + w == bD[v]) seed(v);
  };

  std::conditional_t<WHATIF, WhatifBits, std::conditional_t<LIST, DeadBits, DeadEdges>> dead;
  if constexpr (WHATIF) {
    const bool tooLong = mn > mods.max_metric_per_unit;  // past the LDS the caller sized
    dead = WhatifBits{bb, me, mv, tooLong ? 0u : mn};
    for (uint32_t w = tid; w < (E + 31u) / 32u; w += kBlock) bb[w] = 0ull;
    if (drains) {
      for (uint32_t v = tid; v < N; v += kBlock) lflags[v] = gflags[v];
    }
    if (tid == 0) {
      wf[0] = tooLong ? 1u : 0u;
      wf[1] = 0u;
    }
    if (tooLong) mn = 0u;
  } else if constexpr (!LIST) {
#pragma unroll
    for (int k = 0; k < kMaxDead; ++k) {
      dead.e[k] = k < mods.dead_per_unit ? mods.dead_edges[size_t(u0) * mods.dead_per_unit + k]
                                         : OGS_NODE_NONE;
    }
  } else {
    dead.bits = deadBits;
    for (uint32_t w = tid; w < (E + 31u) / 32u; w += kBlock) deadBits[w] = 0u;
    if (drains) {
      for (uint32_t v = tid; v < N; v += kBlock) lflags[v] = gflags[v];
    }
  }
  for (uint32_t w = tid; w < (N + 31u) / 32u; w += kBlock) inA[w] = 0u;
  if (tid < 3) qcnt[tid] = 0u;
  if (tid < 2) cnt[tid] = 0u;
  __syncthreads();
  // ---- seeds: heads of the failed edges that are tight in the base --------
  if constexpr (!LIST) {
    // (the seed's edge straight from the list: indexing `dead` by tid would put
    // the array in scratch memory, and every edge test of the rounds with it)
    const uint32_t seedEdge = (tid < kMaxDead && tid < mods.dead_per_unit)
        ? mods.dead_edges[size_t(u0) * mods.dead_per_unit + tid]
        : OGS_NODE_NONE;
    if (seedEdge != OGS_NODE_NONE) seedOf(seedEdge);
  } else {
    for (uint32_t i = l0 + tid; i < l1; i += kBlock) {
      const uint32_t e = mods.dead_edges[i];
      if (e >= E) continue;  // OGS_NODE_NONE or a bad id: never outside the bitset
      atomicOr(&deadBits[WHATIF ? 2u * (e >> 5) : e >> 5], 1u << (e & 31u));
      seedOf(e);
    }
    // the metric slice: into LDS, the "overridden" bits, and each override
    // against the CSR weight (see above)
    if constexpr (WHATIF) {
    for (uint32_t i = tid; i < mn; i += kBlock) {
      const uint32_t e = mods.metric_edges[m0 + i], v = mods.metric_vals[m0 + i];
      me[i] = e;
      mv[i] = v;
      if (e >= E) continue;  // skipped: sets no bit, so the search never returns it
      const bool restore = (flags & OGS_F_RESTORE) != 0;
      const bool up = restore && (v & OGS_WHATIF_EDGE_UP);
      const uint32_t nw = restore ? v & ~OGS_WHATIF_EDGE_UP : v;
      if (hop) {  // weights ignored: only a revival counts
        if (!up) continue;
      } else if (nw - 1u >= 0x7FFFFFFFu) {  // 0 or >= 2^31: the exact domain's
        wf[0] = 1u;
        continue;
      }
      atomicOr(&deadBits[2u * (e >> 5) + 1u], 1u << (e & 31u));
      const uint64_t x = edges[e];
      if (static_cast<uint32_t>(x) & OGS_EDGE_DOWN) {
        // revived: nodes outside every base descendant set may get shorter
        // paths, as for a lowered metric
        if (up) wf[1] = 1u;
        continue;
      }
      if (hop) continue;
      const uint32_t w = static_cast<uint32_t>(x >> 32);
      if (nw > w) seedOf(e);
      else if (nw < w) wf[1] = 1u;
    }
    }
    // a drained node's strict descendants: heads of its base-tight out-edges
    // (not the source, which always relaxes; reached; not drained already)
    for (uint32_t i = r0 + tid; DRAINS && i < r1; i += kBlock) {
      const uint32_t x = nodeList[i];
      if (x >= N) continue;
      const uint8_t fx = gflags[x];
      uint8_t add = uint8_t(OGS_NODE_OVERLOADED);
      if constexpr (WHATIF) {
        add = mods.node_bits[i];
        if (flags & OGS_F_RESTORE) {  // clear-then-set
          const uint8_t clr = uint8_t((add >> OGS_NODE_CLEAR_SHIFT) & 0x7u);
          add &= 0x0Fu;
          // an undrained node transits again: shorter paths anywhere, as for
          // a lowered metric (cleared soft-drain bits are selection only)
          if ((fx & clr & ~add) & OGS_NODE_OVERLOADED) wf[1] = 1u;
          lflags[x] = uint8_t(fx & ~clr) | add;
        } else {
          lflags[x] = fx | add;
        }
      } else {
        lflags[x] = fx | add;
      }
      if (!(add & OGS_NODE_OVERLOADED)) continue;  // soft-drain bits: selection only
      const uint32_t dx = bD[x];
      if (x == s || (fx & OGS_NODE_OVERLOADED) || dx == kInf) continue;
      const uint32_t b = gRow[x] - e0;
      for_row(edges, b, gRow[x + 1] - e0 - b, [&](uint32_t, uint64_t y) {
        const uint32_t lo = static_cast<uint32_t>(y);
        if (lo & OGS_EDGE_DOWN) return;
        const uint32_t t = edge_dst(lo);
        if (dx + (hop ? 1u : static_cast<uint32_t>(y >> 32)) == bD[t]) seed(t);
      });
    }
  }
  __syncthreads();
  uint32_t n = qcnt[1];
  bool lowers = false;  // unit-uniform
  if constexpr (WHATIF) {
    if (wf[0]) {  // refused: no record, the zeroed `changed` row, the sentinel
      if (tid < 2) diff.counts[size_t(u0) * 2 + tid] = OGS_WHATIF_REFUSED;
      return;
    }
    lowers = wf[1] != 0u;
  }
  // (a unit that drains changes its drained nodes' own routes whatever n)
  if (CHANGED_ONLY && n == 0 && !drains && !lowers) {  // nothing on a shortest path: no change
    if (tid < 2) diff.counts[size_t(u0) * 2 + tid] = 0u;
    if (oDist || oNh) {
      for (uint32_t v = tid; v < N; v += kBlock) {
        if (oDist) oDist[size_t(u0) * Sn + v] = bD[v];
        if (oNh) oNh[size_t(u0) * Sn + v] = bN[v];
      }
    }
    return;
  }
  for (uint32_t v = tid; v < N; v += kBlock) {
    dn[v] = lowers ? (v == s ? 0ull : uint64_t(kInf))
                   : (uint64_t(bD[v]) | (uint64_t(bN[v]) << 32));
    stamp[v] = 0u;
  }
  if (lowers) {  // ---- recompute from the source: every node in A, no growth --
    __syncthreads();  // the seeds' list entries and count are dead from here
    for (uint32_t w = tid; w < (N + 31u) / 32u; w += kBlock) inA[w] = ~0u;
    n = 0;
  } else if (desc) {  // ---- A = OR of the seeds' precomputed descendant rows ------
    const uint32_t words = (N + 31u) / 32u;
    for (uint32_t w = tid; w < words; w += kBlock) {
      uint32_t a = 0u;
      for (uint32_t i = 0; i < n; ++i) a |= desc[size_t(q1[i]) * words + w];
      inA[w] = a;
    }
    n = 0;
  }
  __syncthreads();
  // ---- A: the seeds' descendants in the base tight DAG (list rounds) ------
  for (uint32_t r = 1; n; ++r) {
    if (tid == 0) qcnt[(r + 2) % 3] = 0u;
    const uint16_t* cur = (r & 1) ? q1 : q0;
    uint16_t* nxt = (r & 1) ? q0 : q1;
    for (uint32_t i = tid; i < n; i += kBlock) {
      const uint32_t x = cur[i];
      if (!relaxesBase(x)) continue;
      const uint32_t dx = static_cast<uint32_t>(dn[x]);
      const uint32_t b = gRow[x] - e0;
      for_row(edges, b, gRow[x + 1] - e0 - b, [&](uint32_t, uint64_t y) {
        const uint32_t lo = static_cast<uint32_t>(y);
        if (lo & OGS_EDGE_DOWN) return;
        const uint32_t t = edge_dst(lo);
        if (dx + (hop ? 1u : static_cast<uint32_t>(y >> 32)) != static_cast<uint32_t>(dn[t])) {
          return;
        }
        if (!(atomicOr(&inA[t >> 5], 1u << (t & 31u)) & (1u << (t & 31u)))) {
          nxt[atomicAdd(&qcnt[(r + 1) % 3], 1u)] = uint16_t(t);
        }
      });
    }
    __syncthreads();
    n = qcnt[(r + 1) % 3];
  }
  // ---- reset A, seed its boundary, re-relax --------------------------------
  __syncthreads();  // every thread has read the last (zero) count
  if (tid < 3) qcnt[tid] = 0u;
  for (uint32_t v = tid; v < N; v += kBlock) {
    if (isA(v) && !lowers) dn[v] = uint64_t(kInf);
  }
  if (lowers && tid == 1) {  // round 1's list is the source alone (tid 1 zeroed the count)
    q1[0] = uint16_t(s);
    qcnt[1] = 1u;
  }
  __syncthreads();
  for (uint32_t x = tid; !lowers && x < N; x += kBlock) {
    if (!isA(x)) continue;
    const uint32_t b = gRow[x] - e0, m = gRow[x + 1] - e0 - b;
    for (uint32_t j = 0; j < m; ++j) {  // links are two-way: out-neighbours = in-neighbours
      const uint32_t p = edge_dst(static_cast<uint32_t>(edges[b + j]));
      if (isA(p) || !relaxes(p) || static_cast<uint32_t>(dn[p]) == kInf) continue;
      if (atomicMax(&stamp[p], 1u) < 1u) q1[atomicAdd(&qcnt[1], 1u)] = uint16_t(p);
    }
  }
  __syncthreads();
  packed_rounds<true>(s, edges, gRow, e0, nflags, hop, dn, stamp, q0, q1, qcnt,
                             nullptr, dead, 1u, qcnt[1]);
  // from here inA only selects the prefixes the changed-only pass visits:
  // those of the unit's drained nodes join it
  if constexpr (DRAINS) {
    for (uint32_t i = r0 + tid; i < r1; i += kBlock) {
      const uint32_t x = nodeList[i];
      if (x < N) atomicOr(&inA[x >> 5], 1u << (x & 31u));
    }
  }
  __syncthreads();
  if (oDist || oNh) {
    for (uint32_t v = tid; v < N; v += kBlock) {
      if (oDist) oDist[size_t(u0) * Sn + v] = static_cast<uint32_t>(dn[v]);
      if (oNh) oNh[size_t(u0) * Sn + v] = static_cast<uint32_t>(dn[v] >> 32);
    }
  }

  // ---- routes --------------------------------------------------------------
  const uint32_t Sp = uint32_t(pt.max_prefixes);
  const uint32_t p0 = pt.pfx_base[unit.topo];
  const uint32_t P = pt.pfx_base[unit.topo + 1] - p0;
  const RouteCfg cfg{(flags & OGS_F_ENABLE_V4) != 0, (flags & OGS_F_V4_OVER_V6) != 0,
                     (flags & OGS_F_BEST_ROUTE_SELECTION) != 0};
  const DiffCtx dc{diff.base_meta, diff.base_metric, diff.base_mask,
                   diff.changed + size_t(u0) * ((Sp + 31u) / 32u), cnt, pt.adv_off + p0,
                   diff.adv_class};
  const uint32_t* tkey = key + size_t(unit.topo) * Sp;
  auto nodeRec = [&](uint32_t v, Rec<1>& r) {
    const uint64_t x = dn[v];
    const uint32_t d = static_cast<uint32_t>(x), nv = static_cast<uint32_t>(x >> 32);
    r.meta = node_route_meta(v, s, d != kInf, __popc(nv), nflags[v]);
    r.metric = (v == s) ? kInf : d;
    r.mask[0] = nv;
  };
  if constexpr (!CHANGED_ONLY) {
    stream_routes<1, true>(pt, tkey, p0, P, Sp, u0, s, nflags, PackedView{dn}, cfg, out,
                           nodeRec, &dc, (flags & kFlagNtStores) != 0);
  } else {
    const bool v4Gated = !cfg.enableV4 && !cfg.v4OverV6;
    uint32_t upd = 0, del = 0;
    for (uint32_t p = tid; p < P; p += kBlock) {
      const uint32_t k = tkey[p];
      bool hit = false;
      if (!(k & kKeySlow)) {
        hit = isA(k & kKeyNode);
      } else {
        for (uint32_t a = pt.adv_off[p0 + p]; a < pt.adv_off[p0 + p + 1]; ++a) {
          const uint32_t v = pt.adv_node[a];
          hit |= v != OGS_NODE_NONE && isA(v);
        }
      }
      if (!hit) continue;  // every advertiser keeps its base state
      Rec<1> r;
      if (!(k & kKeySlow)) {
        if ((k & kKeyV4) && v4Gated) continue;  // the gate's record never changes
        nodeRec(k & kKeyNode, r);
        r.sel = (r.meta & OGS_ROUTE_SELECTED) ? 1u : 0u;
      } else {
        route_one<uint32_t, 1>(pt, p0 + p, s, nflags, PackedView{dn}, cfg, r.meta, r.metric,
                               r.mask, r.sel);
      }
      if (!route_changed<1>(r, dc, Sp, p, upd, del)) continue;
      atomicOr(dc.changed + p / 32u, 1u << (p % 32u));
      const size_t o = size_t(u0) * Sp + p;
      if (out.meta) out.meta[o] = r.meta;
      if (out.metric) static_cast<uint32_t*>(out.metric)[o] = r.metric;
      if (out.sel) out.sel[o] = r.sel;
      if (out.mask) out.mask[o] = r.mask[0];
    }
    if (upd) atomicAdd(&cnt[0], upd);
    if (del) atomicAdd(&cnt[1], del);
  }
  __syncthreads();
  if (tid < 2) diff.counts[size_t(u0) * 2 + tid] = cnt[tid];
