// spf_global.hip — SPF + RouteDb for topologies past the LDS budget (SURVEY
// §8 row g1 "global frontier": WAN areas of tens of thousands of nodes, the
// reference's 99x99 GridTopology.StressTest, SpfSolverTest.cpp:2858-2873).
//
// Same fixpoint as spf_core.h / spf_frontier.hip (reference: LinkState::runSpf,
// LinkState.cpp:720-820; distances are the least solution of dist(v) = min
// over usable u of dist(u) + w(u, v), next-hop sets the least solution of
// NH(v) = U over tight u of (u == src ? {slot} : NH(u)), u relaxing iff u is
// the source or not hard-drained, 741-752). One workgroup of 1024 threads per
// unit walks the frontier list of the round, so every round touches only the
// rows of the nodes changed in the previous round; the two lists are rows in
// HBM, so there is no size limit but the 21-bit node ids of the edge
// encoding.
//
// spf_global_kernel is the two-phase form, stated once: a dist phase, then
// a next-hop phase seeded from the source's row. A state policy says where
// the unit's distances and next-hop words live and how "already in the next
// list" is remembered:
//   HbmState      all in HBM (the caller's output rows or the workspace),
//                 relaxations are L2 atomics, an HBM stamp row; any size, and
//                 any next-hop width (W == kWRuntime: a runtime word count)
//   LdsDistState  distances in LDS, next-hop words in HBM, parity bitsets
//   LdsBothState  distances and next-hop words in LDS, a per-round bitset
// spf_global_lds3_kernel is the one-phase form (packed {dist, nh} words in
// LDS, W = 1, u32 distances).
//
// A unit's workgroup runs on ONE CU, so its HBM state never leaves that
// XCD's L2 until the kernel ends: a round ends with every wave's stores
// drained and a workgroup barrier, and every read of state written in this
// launch is an L2-served `sc1` load (spf_core.h, round_sync / ld_state) -- no
// L2 write-back / L1 invalidate per round. (The first form used agent-scope
// release + acquire fences per round, ~3.5 us of cache maintenance each:
// option "spf_global_sync" 0 keeps it for A/B.)
//
// Routes: route_global.h, one thread per (unit, prefix) against the unit's
// state in HBM. u32 or u64 distances (OGS_F_WIDE_METRIC).
//
// What-if units (ogs_spf_routes_whatif_global): both kernels take a mods
// policy. WhatifRows keeps the unit's dead / overridden edge bitsets and its
// node-flag row in per-unit HBM rows of the workspace (the LDS forms have no
// room left at 20k nodes), fills them before round 1 and reads them with sc1
// loads beside the edge loads; NoMods is the plain build, compiled to the
// code these kernels had before the policy. Routes and the diff against the
// base records: route_global_diff_kernel (route_global.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "openr_gpu.h"
#include "route_core.h"
#include "route_global.h"
#include "spf_core.h"
#include "engine.h"
#include "launch.h"

namespace ogs {

constexpr int kGBlock = 1024;
constexpr int kGRow = 4;      // row edges per step of a frontier node
constexpr int kWRuntime = 0;  // W: the next-hop word count is a kernel argument

// ---- the unit: its source and its topology's CSR ---------------------------
template <typename D>
struct GUnit {
  uint32_t u0, s, N;
  size_t Sn;
  const uint32_t* gRow;
  uint32_t e0;
  const uint64_t* edges;  // edges[gRow[v] - e0 ...]: v's row
  const uint8_t* nflags;
  bool hop;

  __device__ __forceinline__ GUnit(const ogs_graph& g, const ogs_unit& unit, uint32_t flags)
      : u0(blockIdx.x), s(unit.src), Sn(size_t(g.max_nodes)),
        hop((flags & OGS_F_HOP_METRIC) != 0) {
    const uint32_t nb = g.node_base[unit.topo];
    N = g.node_base[unit.topo + 1] - nb;
    gRow = g.row_ptr + nb;
    e0 = gRow[0];
    edges = g.edges + e0;
    nflags = g.node_flags + nb;
  }
  __device__ __forceinline__ D weight(uint64_t x) const {
    return hop ? D(1) : D(static_cast<uint32_t>(x >> 32));
  }
  // a hard-drained node relaxes nothing unless it is the source (741-752)
  __device__ __forceinline__ bool drained(uint32_t v) const {
    return nflags[v] & OGS_NODE_OVERLOADED;
  }
};

// kB edges of a row from edge e on (`left` remain), decoded: target, whether
// the link is up, and the candidate distance dv + w
// (mu: the unit's mods policy, below -- a dead edge reads as down, an
// overridden one carries the unit's weight; the step's one or two bitset
// words are loaded beside its edge words)
template <typename D, int kB>
struct GEdges {
  uint32_t t[kB];
  D c[kB];
  bool up[kB];
  template <class MU>
  __device__ __forceinline__ GEdges(const GUnit<D>& u, const MU& mu, D dv, uint32_t e,
                                    uint32_t left) {
    uint64_t x[kB];
#pragma unroll
    for (int k = 0; k < kB; ++k) {
      x[k] = uint32_t(k) < left ? u.edges[e + k] : uint64_t(OGS_EDGE_DOWN);
    }
    if constexpr (MU::kOn) {
      const uint32_t last = e + (left < uint32_t(kB) ? left : uint32_t(kB)) - 1u;  // left >= 1
      const uint64_t b0 = mu.word(e >> 5), b1 = mu.word(last >> 5);
#pragma unroll
      for (int k = 0; k < kB; ++k) {
        const uint32_t lo = static_cast<uint32_t>(x[k]);
        const uint64_t bw = ((e + k) >> 5) == (e >> 5) ? b0 : b1;
        const uint32_t bit = 1u << ((e + k) & 31u);
        const bool live = uint32_t(k) < left;  // past the row: no bit is this edge's
        up[k] = live && !mu.down(e + k, lo, bw);
        t[k] = edge_dst(lo);
        c[k] = dv + ((!u.hop && live && (static_cast<uint32_t>(bw >> 32) & bit))
                         ? D(MU::weight_of(mu.search(e + k)))
                         : u.weight(x[k]));
      }
    } else {
#pragma unroll
      for (int k = 0; k < kB; ++k) {
        const uint32_t lo = static_cast<uint32_t>(x[k]);
        up[k] = !(lo & OGS_EDGE_DOWN);
        t[k] = edge_dst(lo);
        c[k] = dv + u.weight(x[k]);
      }
    }
  }
};

// ---- the unit's modifications (ogs_spf_routes_whatif_global) ----------------
// A mods policy answers, shaped like WhatifBits of spf_frontier.hip: is
// directed edge e dead in this unit, what is e's weight, is node v hard-
// drained. NoMods is the plain build: the kernels compile to what they were
// before the policy existed.
struct NoMods {
  static constexpr bool kOn = false;
};

// What the what-if launch hands every workgroup besides the plain arguments.
struct GWhatifArgs {
  ogs_whatif_mods mods;
  const uint32_t* edgeSrc;   // graph->edge_src or nullptr (no exit-only units)
  const uint32_t* baseDist;  // diff->base_dist when exit-only units are allowed, else nullptr
  const uint32_t* baseNh;
  uint32_t* exitDist;        // the caller's dist / nh rows (an exit-only unit copies the
  uint32_t* exitNh;          // base's [S_n] rows there: set at W == 1 only) or nullptr
  uint32_t* counts;          // diff->counts or nullptr
  uint64_t* bits;            // [U][ew] {dead word, overridden word << 32}
  uint8_t* frows;            // [U][SnB] the units' node-flag rows (nullptr: no node lists)
  uint32_t* skip;            // [U] 1: the unit ran no SPF (refused / exit-only)
  uint32_t ew, SnB;
  bool restore;              // OGS_F_RESTORE: up flags and clear nibbles are read
};

// Per-unit HBM rows in the workspace, filled by the unit's workgroup before
// round 1: at 20k nodes the LDS forms leave no room for an edge bitset. The
// rows are written inside the launch, so the fill ends in round_sync<true>()
// and every later read is an sc1 load (ld_state<true>), as for the SPF state.
// An overridden edge finds its weight by binary search over the unit's
// ascending (metric_edges, metric_vals) slice in global memory; the search
// stays inside [0, n) whatever the slice holds.
struct WhatifRows {
  static constexpr bool kOn = true;
  const uint64_t* bb;
  const uint32_t* me;
  const uint32_t* mv;
  uint32_t n;
  const uint8_t* nflags;  // the unit's row, or the topology's when it has no node bits

  __device__ __forceinline__ uint64_t word(uint32_t i) const { return ld_state<true>(bb + i); }
  __device__ __forceinline__ bool has(uint32_t e) const {
    return (static_cast<uint32_t>(word(e >> 5)) >> (e & 31u)) & 1u;
  }
  __device__ __forceinline__ uint32_t search(uint32_t e) const {
    uint32_t lo = 0, hi = n;  // n >= 1: a set bit came from the slice
    while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (me[mid] <= e) lo = mid; else hi = mid;
    }
    return mv[lo];
  }
  // (search() returns the slice's value: weight | OGS_WHATIF_EDGE_UP, the
  // latter only under OGS_F_RESTORE -- without the flag it refused the unit)
  static __device__ __forceinline__ uint32_t weight_of(uint32_t val) {
    return val & ~OGS_WHATIF_EDGE_UP;
  }
  __device__ __forceinline__ uint32_t weight(uint32_t e, uint64_t x) const {
    return ((static_cast<uint32_t>(word(e >> 5) >> 32) >> (e & 31u)) & 1u)
        ? weight_of(search(e)) : static_cast<uint32_t>(x >> 32);
  }
  // is edge e (lo: its CSR word's low half, bw: its {dead, overridden} word)
  // down in this unit: dead, or down in the CSR and not revived. The slice is
  // searched only for edges down in the CSR and overridden.
  __device__ __forceinline__ bool down(uint32_t e, uint32_t lo, uint64_t bw) const {
    const uint32_t bit = 1u << (e & 31u);
    if (static_cast<uint32_t>(bw) & bit) return true;
    if (!(lo & OGS_EDGE_DOWN)) return false;
    if (!(static_cast<uint32_t>(bw >> 32) & bit)) return true;
    return !(search(e) & OGS_WHATIF_EDGE_UP);
  }
  __device__ __forceinline__ bool drained(uint32_t v) const {
    return ld_state<true>(nflags + v) & OGS_NODE_OVERLOADED;
  }

  // Fills the unit's rows; false when the unit runs no SPF: refused (a bad
  // weight, a slice past max_metric_per_unit: counts = OGS_WHATIF_REFUSED) or
  // exit-only (no node bits, no lowered metric, no dead or raised edge tight
  // in the base: nothing on a shortest path moved, counts = {0, 0}). Both
  // decisions are uniform across the workgroup.
  __device__ __forceinline__ bool setup(const GWhatifArgs& a, const ogs_graph& g,
                                        const GUnit<uint32_t>& u) {
    constexpr uint32_t kInf = 0xFFFFFFFFu;
    __shared__ uint32_t wf[2];  // refused, something on a base shortest path moved
    const uint32_t tid = threadIdx.x, u0 = u.u0;
    const ogs_whatif_mods& m = a.mods;
    // (never past the row the launch sized from graph->max_edges)
    const uint32_t E = min(u.gRow[u.N] - u.e0, a.ew * 32u);
    const uint32_t words = (E + 31u) / 32u;
    uint64_t* row = a.bits + size_t(u0) * a.ew;
    uint32_t* row32 = reinterpret_cast<uint32_t*>(row);
    // ignored under OGS_F_HOP_METRIC, but for the up flags of OGS_F_RESTORE
    const bool restore = a.restore;
    const bool metrics = m.metric_off && (!u.hop || restore);
    const uint32_t m0 = metrics ? m.metric_off[u0] : 0u;
    uint32_t mn = metrics ? m.metric_off[u0 + 1] - m0 : 0u;
    const bool tooLong = mn > m.max_metric_per_unit;
    if (tooLong) mn = 0u;
    const uint32_t r0 = m.node_off ? m.node_off[u0] : 0u;
    const uint32_t r1 = m.node_off ? m.node_off[u0 + 1] : 0u;
    const bool nodes = r1 > r0;
    uint8_t* frow = nodes ? a.frows + size_t(u0) * a.SnB : nullptr;
    const uint32_t* bD = a.baseDist;
    const bool exits = bD && a.edgeSrc && !nodes;

    for (uint32_t w = tid; w < words; w += kGBlock) row[w] = 0ull;
    if (nodes) {
      for (uint32_t v = tid; v < u.N; v += kGBlock) frow[v] = u.nflags[v];
    }
    if (tid == 0) {
      wf[0] = tooLong ? 1u : 0u;
      wf[1] = 0u;
    }
    round_sync<true>();
    // is edge e (in range, weight w in the base) tight in the base?
    auto tight = [&](uint32_t e, uint64_t x) {
      const uint32_t lo = static_cast<uint32_t>(x);
      if (lo & OGS_EDGE_DOWN) return false;
      const uint32_t p = a.edgeSrc[u.e0 + e], v = edge_dst(lo);
      const uint32_t dp = bD[p];
      return (p == u.s || !(u.nflags[p] & OGS_NODE_OVERLOADED)) && dp != kInf &&
          dp + u.weight(x) == bD[v];
    };
    for (uint32_t i = m.dead_off[u0] + tid; i < m.dead_off[u0 + 1]; i += kGBlock) {
      const uint32_t e = m.dead_edges[i];
      if (e >= E) continue;  // OGS_NODE_NONE or a bad id: never outside the row
      atomicOr(&row32[2u * (e >> 5)], 1u << (e & 31u));
      if (exits && tight(e, u.edges[e])) wf[1] = 1u;
    }
    for (uint32_t i = tid; i < mn; i += kGBlock) {
      const uint32_t e = m.metric_edges[m0 + i], v = m.metric_vals[m0 + i];
      if (e >= E) continue;  // skipped: sets no bit, so the search never returns it
      const bool up = restore && (v & OGS_WHATIF_EDGE_UP);
      const uint32_t nw = restore ? v & ~OGS_WHATIF_EDGE_UP : v;
      if (u.hop) {  // weights ignored: only a revival counts
        if (!up) continue;
      } else if (nw - 1u >= 0x7FFFFFFFu) {  // 0 or >= 2^31: the exact domain's
        wf[0] = 1u;
        continue;
      }
      atomicOr(&row32[2u * (e >> 5) + 1u], 1u << (e & 31u));
      if (!exits) continue;
      const uint64_t x = u.edges[e];
      if (static_cast<uint32_t>(x) & OGS_EDGE_DOWN) {
        if (up) wf[1] = 1u;  // a revival: no exit-only path
        continue;
      }
      if (u.hop) continue;
      const uint32_t w = static_cast<uint32_t>(x >> 32);
      if (nw < w || (nw > w && tight(e, x))) wf[1] = 1u;
    }
    for (uint32_t i = r0 + tid; i < r1; i += kGBlock) {
      const uint32_t x = m.node_ids[i];
      if (x >= u.N) continue;
      const uint8_t b = m.node_bits[i];
      // OGS_F_RESTORE: clear-then-set (units with node lists take no exit)
      frow[x] = restore ? uint8_t((u.nflags[x] & ~((b >> OGS_NODE_CLEAR_SHIFT) & 0x7u)) | (b & 0x0Fu))
                        : uint8_t(u.nflags[x] | b);
    }
    round_sync<true>();
    const bool refused = wf[0] != 0u;
    const bool exit = !refused && exits && wf[1] == 0u;
    if (tid == 0) a.skip[u0] = (refused || exit) ? 1u : 0u;
    if (a.counts && tid < 2) a.counts[size_t(u0) * 2 + tid] = refused ? OGS_WHATIF_REFUSED : 0u;
    // (exits only at W == 1: the unit's next-hop row is u0 * Sn, one word a node)
    if (exit && a.exitDist) {
      for (uint32_t v = tid; v < u.N; v += kGBlock) a.exitDist[size_t(u0) * u.Sn + v] = bD[v];
    }
    if (exit && a.exitNh) {
      for (uint32_t v = tid; v < u.N; v += kGBlock) {
        a.exitNh[size_t(u0) * u.Sn + v] = a.baseNh[v];
      }
    }
    if (refused || exit) return false;
    bb = row;
    me = m.metric_edges + m0;
    mv = m.metric_vals + m0;
    n = mn;
    nflags = nodes ? frow : u.nflags;
    return true;
  }
};

// ---- the frontier lists: two HBM rows, round r's list in row r & 1 with its
// length in count slot r % 3 (LDS) -------------------------------------------
struct GLists {
  uint32_t* q;  // [2 * Sn]
  size_t Sn;
  uint32_t* qcnt;

  __device__ __forceinline__ void init(uint32_t s) {  // round 1's list: the source
    if (threadIdx.x == 0) {
      q[Sn] = s;
      qcnt[0] = 0u;
      qcnt[1] = 1u;
      qcnt[2] = 0u;
    }
  }
  __device__ __forceinline__ uint32_t* list(uint32_t r) const { return q + (r & 1) * Sn; }
  __device__ __forceinline__ void begin_round(uint32_t r) {
    if (threadIdx.x == 0) qcnt[(r + 2) % 3] = 0u;
  }
  __device__ __forceinline__ void push(uint32_t t, uint32_t r) {  // into round r + 1's list
    const uint32_t at = atomicAdd(&qcnt[(r + 1) % 3], 1u);
    list(r + 1)[at] = t;
  }
  // the length of round r + 1's list, once round r's pushes are visible
  template <bool L2SYNC>
  __device__ __forceinline__ uint32_t end_round(uint32_t r) {
    round_sync<L2SYNC>();
    const uint32_t n = qcnt[(r + 1) % 3];
    __syncthreads();  // every thread has read the count before it is reset
    return n;
  }
  __device__ __forceinline__ void reset() {  // between the phases
    if (threadIdx.x == 0) qcnt[0] = qcnt[1] = qcnt[2] = 0u;
  }
};

// ---- "t is already in the next list": first_push(t, r) is true for t's
// first push of round r + 1 ---------------------------------------------------
// An HBM row of the last round each node was pushed for (rounds count on
// through both phases, so the row is never cleared).
struct StampMember {
  static constexpr bool kPerRound = false;
  uint32_t* stamp;
  __device__ __forceinline__ void init(uint32_t N) {
    for (uint32_t v = threadIdx.x; v < N; v += kGBlock) stamp[v] = 0u;
  }
  __device__ __forceinline__ bool first_push(uint32_t t, uint32_t r) {
    return atomicMax(&stamp[t], r + 1) < r + 1;
  }
  __device__ __forceinline__ void consume(uint32_t, uint32_t) {}
  __device__ __forceinline__ void reset() {}
};

// A bitset per round parity in LDS: bit set on the first push of a round,
// cleared when the entry is consumed (round 1's entry was never pushed).
struct ParityMember {
  static constexpr bool kPerRound = false;
  uint32_t* mark;  // [2 * mw]
  uint32_t mw;
  __device__ __forceinline__ void init(uint32_t) { reset(); }
  __device__ __forceinline__ bool first_push(uint32_t t, uint32_t r) {
    const uint32_t bit = 1u << (t & 31u);
    return !(atomicOr(&mark[((r + 1) & 1) * mw + (t >> 5)], bit) & bit);
  }
  __device__ __forceinline__ void consume(uint32_t v, uint32_t r) {
    if (r > 1) atomicAnd(&mark[(r & 1) * mw + (v >> 5)], ~(1u << (v & 31u)));
  }
  // a phase's last round consumed nothing: clear both parities
  __device__ __forceinline__ void reset() {
    for (uint32_t i = threadIdx.x; i < 2 * mw; i += kGBlock) mark[i] = 0u;
  }
};

// ONE bitset in LDS, cleared in bulk at the start of every round -- behind
// the same barrier that the round's first frontier loads are already in
// flight across.
struct RoundMember {
  static constexpr bool kPerRound = true;
  uint32_t* mark;  // [mw]
  uint32_t mw;
  __device__ __forceinline__ void init(uint32_t) {}
  __device__ __forceinline__ bool first_push(uint32_t t, uint32_t) {
    const uint32_t bit = 1u << (t & 31u);
    return !(atomicOr(&mark[t >> 5], bit) & bit);
  }
  __device__ __forceinline__ void begin_round() {
    reset();
    __syncthreads();
  }
  __device__ __forceinline__ void consume(uint32_t, uint32_t) {}
  __device__ __forceinline__ void reset() {
    for (uint32_t i = threadIdx.x; i < mw; i += kGBlock) mark[i] = 0u;
  }
};

// ---- where dist[v] (D) and nh[w * Sn + v] live -------------------------------
// kStaged: a relaxation step's memory operations are issued class by class
// over the step's edges (they are L2 round trips), else edge by edge (LDS).
// Both in HBM. L2SYNC: spf_core.h.
template <typename D, int W, bool L2SYNC>
struct HbmState {
  using Dist = D;
  using Member = StampMember;
  static constexpr int kW = W;
  static constexpr bool kL2Sync = L2SYNC, kDistStaged = true, kNhStaged = W != kWRuntime;
  static constexpr int kNhStep = W == kWRuntime ? 1 : W <= 4 ? kGRow : 2;
  D* dist;
  uint32_t* nh;
  size_t Sn;
  int wn;

  __device__ __forceinline__ HbmState(const GUnit<D>& u, int Wn, D* oDist, uint32_t* oNh, char*)
      : dist(oDist + u.u0 * u.Sn), Sn(u.Sn), wn(W == kWRuntime ? Wn : W) {
    nh = oNh + size_t(u.u0) * wn * Sn;
  }
  __device__ __forceinline__ Member member(uint32_t* stampRow) const { return Member{stampRow}; }
  __device__ __forceinline__ int words() const { return W == kWRuntime ? wn : W; }
  __device__ __forceinline__ D ld_dist(uint32_t v) const { return ld_state<L2SYNC>(dist + v); }
  __device__ __forceinline__ D min_dist(uint32_t t, D c) { return atomicMin(&dist[t], c); }
  __device__ __forceinline__ uint32_t ld_nh(int w, uint32_t v) const {
    return ld_state<L2SYNC>(nh + w * Sn + v);
  }
  __device__ __forceinline__ uint32_t* nh_word(int w, uint32_t v) { return nh + w * Sn + v; }
  __device__ __forceinline__ void after_dist(const GUnit<D>&) {}
  __device__ __forceinline__ void after_nh(const GUnit<D>&) {}
};

// Distances in LDS (N * sizeof(D) + two list bitsets <= 160 kB, e.g. 20k
// nodes at u32): a dist round's chain is frontier entry -> row -> edge words
// (L2) with LDS atomics for the relaxations, instead of dist loads and
// atomics whose lines the atomics drop from L2. The next-hop words stay in
// HBM; the final distances are copied to the caller's row for the route
// kernel.
uint32_t global_lds_bytes(uint32_t Sn, uint32_t dsize) {
  return ((Sn * dsize + 15u) & ~15u) + 2u * 4u * ((Sn + 31u) / 32u);
}

template <typename D, int W>
struct LdsDistState {
  using Dist = D;
  using Member = ParityMember;
  static constexpr int kW = W;
  static constexpr bool kL2Sync = true, kDistStaged = false, kNhStaged = true;
  static constexpr int kNhStep = W <= 4 ? kGRow : 2;
  D* dist;         // LDS
  uint32_t* nh;    // HBM
  uint32_t* mark;  // LDS
  D* oD;
  size_t Sn;

  __device__ __forceinline__ LdsDistState(const GUnit<D>& u, int, D* oDist, uint32_t* oNh,
                                          char* smem)
      : dist(reinterpret_cast<D*>(smem)), nh(oNh + size_t(u.u0) * W * u.Sn),
        mark(reinterpret_cast<uint32_t*>(smem + ((u.Sn * sizeof(D) + 15u) & ~size_t(15)))),
        oD(oDist + u.u0 * u.Sn), Sn(u.Sn) {}
  __device__ __forceinline__ Member member(uint32_t*) const {
    return Member{mark, (uint32_t(Sn) + 31u) / 32u};
  }
  __device__ __forceinline__ int words() const { return W; }
  __device__ __forceinline__ D ld_dist(uint32_t v) const { return dist[v]; }
  __device__ __forceinline__ D min_dist(uint32_t t, D c) { return atomicMin(&dist[t], c); }
  __device__ __forceinline__ uint32_t ld_nh(int w, uint32_t v) const {
    return ld_state<true>(nh + w * Sn + v);
  }
  __device__ __forceinline__ uint32_t* nh_word(int w, uint32_t v) { return nh + w * Sn + v; }
  __device__ __forceinline__ void after_dist(const GUnit<D>& u) {
    for (uint32_t v = threadIdx.x; v < u.N; v += kGBlock) oD[v] = dist[v];
  }
  __device__ __forceinline__ void after_nh(const GUnit<D>&) {}
};

// Distances AND next-hop words in LDS (N * (sizeof(D) + 4W) + one list bitset
// <= 160 kB, e.g. 20k nodes at u32, W = 1): both phases relax with LDS
// atomics; only the frontier lists (HBM rows) and the CSR are read from L2.
// The final distances and next-hop words are copied to the caller's rows for
// the route kernel.
uint32_t global_lds2_bytes(uint32_t Sn, uint32_t dsize, int W) {
  return ((Sn * dsize + 15u) & ~15u) + ((Sn * 4u * uint32_t(W) + 15u) & ~15u) +
      4u * ((Sn + 31u) / 32u);
}

template <typename D, int W>
struct LdsBothState {
  using Dist = D;
  using Member = RoundMember;
  static constexpr int kW = W;
  static constexpr bool kL2Sync = true, kDistStaged = false, kNhStaged = false;
  static constexpr int kNhStep = kGRow;
  D* dist;         // LDS, all three
  uint32_t* nh;
  uint32_t* mark;
  D* oD;
  uint32_t* oN;
  size_t Sn;

  __device__ __forceinline__ LdsBothState(const GUnit<D>& u, int, D* oDist, uint32_t* oNh,
                                          char* smem)
      : dist(reinterpret_cast<D*>(smem)),
        nh(reinterpret_cast<uint32_t*>(smem + ((u.Sn * sizeof(D) + 15u) & ~size_t(15)))),
        oD(oDist + u.u0 * u.Sn), oN(oNh + size_t(u.u0) * W * u.Sn), Sn(u.Sn) {
    mark = nh + ((Sn * W + 3u) & ~size_t(3));
  }
  __device__ __forceinline__ Member member(uint32_t*) const {
    return Member{mark, (uint32_t(Sn) + 31u) / 32u};
  }
  __device__ __forceinline__ int words() const { return W; }
  __device__ __forceinline__ D ld_dist(uint32_t v) const { return dist[v]; }
  __device__ __forceinline__ D min_dist(uint32_t t, D c) { return atomicMin(&dist[t], c); }
  __device__ __forceinline__ uint32_t ld_nh(int w, uint32_t v) const { return nh[w * Sn + v]; }
  __device__ __forceinline__ uint32_t* nh_word(int w, uint32_t v) { return nh + w * Sn + v; }
  __device__ __forceinline__ void after_dist(const GUnit<D>&) {}
  __device__ __forceinline__ void after_nh(const GUnit<D>& u) {
    for (uint32_t v = threadIdx.x; v < u.N; v += kGBlock) {
      oD[v] = dist[v];
#pragma unroll
      for (int w = 0; w < W; ++w) oN[w * Sn + v] = nh[w * Sn + v];
    }
  }
};

// One unit's two-phase SPF. oDist / oNh: the units' dist [Sn] and nh
// [W * Sn] rows; scratch: stamp / q0 / q1 rows per unit (>= N entries each).
// Wn: the next-hop word count where F::kW == kWRuntime (sources of more than
// 512 links; rslot is never read: push-style relaxation, link slots from the
// source's own row).
// M: the mods policy. MA: nothing for NoMods -- the plain kernels keep the
// argument list they had --, GWhatifArgs for WhatifRows (a unit that is
// refused or exit-only leaves before its state is touched).
template <class F, class M = NoMods, class... MA>
__global__ __launch_bounds__(kGBlock) void spf_global_kernel(
    ogs_graph g, const ogs_unit* __restrict__ units, uint32_t flags, int Wn,
    typename F::Dist* __restrict__ oDist, uint32_t* __restrict__ oNh,
    uint32_t* __restrict__ scratch, MA... ma) {
  static_assert(sizeof...(MA) == (M::kOn ? 1 : 0), "the policy's arguments, or none");
  using D = typename F::Dist;
  constexpr int W = F::kW;
  constexpr int kUnrollW = W == kWRuntime ? 1 : W;  // a runtime count: no unrolling
  constexpr bool L2 = F::kL2Sync;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ uint32_t qcnt[3];
  const uint32_t tid = threadIdx.x;
  const GUnit<D> u(g, units[blockIdx.x], flags);
  M mu;
  if constexpr (M::kOn) {
    if (!mu.setup(ma..., g, u)) return;
  }
  auto drained = [&](uint32_t v) {
    if constexpr (M::kOn) return mu.drained(v); else return u.drained(v);
  };
  uint32_t* rows = scratch + u.u0 * 3 * u.Sn;
  F st(u, Wn, oDist, oNh, smem);
  auto mem = st.member(rows);
  GLists fr{rows + u.Sn, u.Sn, qcnt};

  for (uint32_t v = tid; v < u.N; v += kGBlock) {
    st.dist[v] = (v == u.s) ? D(0) : DistInf<D>::value;
#pragma unroll kUnrollW
    for (int w = 0; w < st.words(); ++w) *st.nh_word(w, v) = 0u;
  }
  mem.init(u.N);
  fr.init(u.s);
  round_sync<L2>();

  // One phase's rounds, from round r with n entries in its list: visit(v, r)
  // for every entry. Returns the first round that was not run.
  auto rounds = [&](uint32_t r, uint32_t n, auto&& visit) {
    for (; n; ++r) {
      fr.begin_round(r);
      const uint32_t* cur = fr.list(r);
      uint32_t v0 = 0u;
      if constexpr (F::Member::kPerRound) {
        // each thread's first entry is loaded, then the bitset is cleared
        // behind one barrier (the load's latency overlaps it)
        if (tid < n) v0 = ld_state<L2>(cur + tid);
        mem.begin_round();
      }
      for (uint32_t i = tid; i < n; i += kGBlock) {
        const uint32_t v = (F::Member::kPerRound && i == tid) ? v0 : ld_state<L2>(cur + i);
        mem.consume(v, r);
        visit(v, r);
      }
      n = fr.end_round<L2>(r);
    }
    return r;
  };

  // ---- dist phase: rows of the nodes whose distance dropped last round ----
  const uint32_t r0 = rounds(1u, 1u, [&](uint32_t v, uint32_t r) {
    if (v != u.s && drained(v)) return;  // 741-752
    const D dv = st.ld_dist(v);
    const uint32_t b = u.gRow[v] - u.e0, m = u.gRow[v + 1] - u.e0 - b;
    for (uint32_t j0 = 0; j0 < m; j0 += kGRow) {
      const GEdges<D, kGRow> e(u, mu, dv, b + j0, m - j0);
      if constexpr (F::kDistStaged) {
        // the targets' dist, then the atomicMins, then the membership
        // atomics: one L2 round trip per step instead of one per edge and
        // step (6.13 -> 5.65 ms on G1)
        D seen[kGRow];
        bool ok[kGRow];
#pragma unroll
        for (int k = 0; k < kGRow; ++k) seen[k] = e.up[k] ? st.ld_dist(e.t[k]) : D(0);
#pragma unroll
        for (int k = 0; k < kGRow; ++k) {
          ok[k] = e.up[k] && e.c[k] < seen[k];
          seen[k] = ok[k] ? st.min_dist(e.t[k], e.c[k]) : D(0);
        }
#pragma unroll
        for (int k = 0; k < kGRow; ++k) {
          ok[k] = ok[k] && e.c[k] < seen[k] && mem.first_push(e.t[k], r);
        }
#pragma unroll
        for (int k = 0; k < kGRow; ++k) {
          if (ok[k]) fr.push(e.t[k], r);
        }
      } else {
#pragma unroll
        for (int k = 0; k < kGRow; ++k) {
          if (e.up[k] && e.c[k] < st.ld_dist(e.t[k]) && e.c[k] < st.min_dist(e.t[k], e.c[k]) &&
              mem.first_push(e.t[k], r)) {
            fr.push(e.t[k], r);
          }
        }
      }
    }
  });
  st.after_dist(u);

  // ---- next-hop phase: the source's row seeds link slots, tight pushes ----
  fr.reset();
  mem.reset();
  round_sync<L2>();
  {
    const uint32_t b = u.gRow[u.s] - u.e0, m = u.gRow[u.s + 1] - u.e0 - b;
    for (uint32_t j = tid; j < m && j < 32u * uint32_t(st.words()); j += kGBlock) {
      const uint64_t x = u.edges[b + j];
      const uint32_t lo = static_cast<uint32_t>(x);
      const uint32_t t = edge_dst(lo);
      D w0;
      if constexpr (M::kOn) {
        if (mu.down(b + j, lo, mu.word((b + j) >> 5))) continue;
        w0 = u.hop ? D(1) : D(mu.weight(b + j, x));
      } else {
        if (lo & OGS_EDGE_DOWN) continue;
        w0 = u.weight(x);
      }
      if (w0 == st.ld_dist(t)) {
        atomicOr(st.nh_word(j >> 5, t), 1u << (j & 31u));
        if (mem.first_push(t, r0)) fr.push(t, r0);
      }
    }
  }
  rounds(r0 + 1, fr.end_round<L2>(r0), [&](uint32_t v, uint32_t r) {
    if (v == u.s || drained(v)) return;
    const D dv = st.ld_dist(v);
    uint32_t nv[kUnrollW];  // NH(v); with a runtime word count re-read per edge
    if constexpr (W != kWRuntime) {
#pragma unroll
      for (int w = 0; w < W; ++w) nv[w] = st.ld_nh(w, v);
    }
    const uint32_t b = u.gRow[v] - u.e0, m = u.gRow[v + 1] - u.e0 - b;
    constexpr int kB = F::kNhStep;
    for (uint32_t j0 = 0; j0 < m; j0 += kB) {
      const GEdges<D, kB> e(u, mu, dv, b + j0, m - j0);
      if constexpr (F::kNhStaged) {
        bool ok[kB], add[kB];
#pragma unroll
        for (int k = 0; k < kB; ++k) ok[k] = e.up[k] && e.c[k] == st.ld_dist(e.t[k]);  // tight
        uint32_t a[kB][kUnrollW];
#pragma unroll
        for (int k = 0; k < kB; ++k) {
#pragma unroll
          for (int w = 0; w < W; ++w) a[k][w] = ok[k] ? nv[w] & ~st.ld_nh(w, e.t[k]) : 0u;
        }
#pragma unroll
        for (int k = 0; k < kB; ++k) {
          add[k] = false;
#pragma unroll
          for (int w = 0; w < W; ++w) {
            if (a[k][w] && (a[k][w] & ~atomicOr(st.nh_word(w, e.t[k]), a[k][w]))) add[k] = true;
          }
        }
#pragma unroll
        for (int k = 0; k < kB; ++k) add[k] = add[k] && mem.first_push(e.t[k], r);
#pragma unroll
        for (int k = 0; k < kB; ++k) {
          if (add[k]) fr.push(e.t[k], r);
        }
      } else {
#pragma unroll
        for (int k = 0; k < kB; ++k) {
          if (!e.up[k] || e.c[k] != st.ld_dist(e.t[k])) continue;  // not tight
          bool add = false;
#pragma unroll kUnrollW
          for (int w = 0; w < st.words(); ++w) {
            uint32_t a;
            if constexpr (W == kWRuntime) a = st.ld_nh(w, v); else a = nv[w];
            a &= ~st.ld_nh(w, e.t[k]);
            if (a && (a & ~atomicOr(st.nh_word(w, e.t[k]), a))) add = true;
          }
          if (add && mem.first_push(e.t[k], r)) fr.push(e.t[k], r);
        }
      }
    }
  });
  st.after_nh(u);
}

// ---- one phase, packed {dist, next-hop word} in LDS (W = 1, u32 distances;
// N * 8 + one list bitset <= 160 kB, e.g. 20k nodes) -------------------------
// As the frontier kernel's packed form (packed_rounds): each relaxation is a
// 64-bit LDS compare-and-swap of {dist, nh}; a strictly shorter candidate
// replaces the word, an equal one ORs its next hops in, and either change
// pushes the target. Distances and next-hop sets converge in the same rounds
// (the two-phase forms run the next-hop propagation as a second sequence of
// rounds); the least fixpoint is the same (spf_core.h).
uint32_t global_lds3_bytes(uint32_t Sn) { return Sn * 8u + 4u * ((Sn + 31u) / 32u); }

// With a prefix table (pt.max_prefixes > 0) the unit's RouteDb is written by
// the same workgroup after its last round (route_one against the packed LDS
// words, one thread per prefix, coalesced record stores), as
// route_global_kernel would from the HBM rows: the launch no longer reads
// its own dist / next-hop rows back (G1: 64 x 20k x 8 B of the 44 MB the PMC
// counted per launch pair, profiles/r05_pmc_g1.json).
// M: the mods policy, as for spf_global_kernel (the what-if launch passes no
// prefix table: its route pass is route_global_diff_kernel).
template <class M = NoMods, class... MA>
__global__ __launch_bounds__(kGBlock) void spf_global_lds3_kernel(
    ogs_graph g, const ogs_unit* __restrict__ units, uint32_t flags,
    uint32_t* __restrict__ oDist, uint32_t* __restrict__ oNh, uint32_t* __restrict__ scratch,
    ogs_prefix_table pt, ogs_spf_out out, MA... ma) {
  static_assert(sizeof...(MA) == (M::kOn ? 1 : 0), "the policy's arguments, or none");
  constexpr uint32_t kInf = 0xFFFFFFFFu;
  const int tid = threadIdx.x;
  const uint32_t u0 = blockIdx.x;
  const ogs_unit unit = units[u0];
  const uint32_t s = unit.src;
  const uint32_t nb = g.node_base[unit.topo];
  const uint32_t N = g.node_base[unit.topo + 1] - nb;
  const size_t Sn = size_t(g.max_nodes);
  const uint32_t* __restrict__ gRow = g.row_ptr + nb;
  const uint32_t e0 = gRow[0];
  const uint64_t* __restrict__ edges = g.edges + e0;
  const uint8_t* __restrict__ nflags = g.node_flags + nb;
  const bool hop = (flags & OGS_F_HOP_METRIC) != 0;
  M mu;
  if constexpr (M::kOn) {
    if (!mu.setup(ma..., g, GUnit<uint32_t>(g, unit, flags))) return;
  }
  uint32_t* q0 = scratch + u0 * 3 * Sn + Sn;
  uint32_t* q1 = q0 + Sn;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint64_t* dn = reinterpret_cast<uint64_t*>(smem);              // [N] {dist, nh}
  uint32_t* mark = reinterpret_cast<uint32_t*>(dn + Sn);        // [ceil(N/32)]
  const uint32_t mw = (uint32_t(Sn) + 31u) / 32u;
  __shared__ uint32_t qcnt[3];

  for (uint32_t v = tid; v < N; v += kGBlock) dn[v] = (v == s) ? 0ull : uint64_t(kInf);
  if (tid == 0) {
    q1[0] = s;
    qcnt[0] = 0u;
    qcnt[1] = 1u;
    qcnt[2] = 0u;
  }
  round_sync<true>();
  const uint32_t sb = gRow[s] - e0;  // the source's row: its link slots
  uint32_t r = 1, n = 1;
  for (; n; ++r) {
    if (tid == 0) qcnt[(r + 2) % 3] = 0u;
    const uint32_t* cur = (r & 1) ? q1 : q0;
    uint32_t* nxt = (r & 1) ? q0 : q1;
    const uint32_t v0 = uint32_t(tid) < n ? ld_state<true>(cur + tid) : 0u;
    for (uint32_t i = tid; i < mw; i += kGBlock) mark[i] = 0u;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += kGBlock) {
      const uint32_t v = i == uint32_t(tid) ? v0 : ld_state<true>(cur + i);
      if constexpr (M::kOn) {
        if (v != s && mu.drained(v)) continue;
      } else {
        if (v != s && (nflags[v] & OGS_NODE_OVERLOADED)) continue;  // 741-752
      }
      const uint64_t xv = dn[v];
      const uint32_t dv = static_cast<uint32_t>(xv), nv = static_cast<uint32_t>(xv >> 32);
      const uint32_t b = gRow[v] - e0, m = gRow[v + 1] - e0 - b;
      for (uint32_t j0 = 0; j0 < m; j0 += kGRow) {
        uint64_t x[kGRow];
#pragma unroll
        for (int k = 0; k < kGRow; ++k) {
          x[k] = j0 + k < m ? edges[b + j0 + k] : uint64_t(OGS_EDGE_DOWN);
        }
        uint64_t b0 = 0, b1 = 0;  // the step's {dead, overridden} words
        if constexpr (M::kOn) {
          b0 = mu.word((b + j0) >> 5);
          b1 = mu.word((b + (j0 + kGRow < m ? j0 + kGRow : m) - 1u) >> 5);
        }
#pragma unroll
        for (int k = 0; k < kGRow; ++k) {
          const uint32_t lo = static_cast<uint32_t>(x[k]);
          const uint32_t t = edge_dst(lo);
          uint32_t wk = hop ? 1u : static_cast<uint32_t>(x[k] >> 32);
          if constexpr (M::kOn) {
            if (j0 + k >= m) continue;  // past the row: no bit is this edge's
            const uint32_t e = b + j0 + k, bit = 1u << (e & 31u);
            const uint64_t bw = (e >> 5) == ((b + j0) >> 5) ? b0 : b1;
            if (mu.down(e, lo, bw)) continue;  // dead, or down and not revived
            if (!hop && (static_cast<uint32_t>(bw >> 32) & bit)) wk = M::weight_of(mu.search(e));
          } else {
            if (lo & OGS_EDGE_DOWN) continue;
          }
          const uint32_t c = dv + wk;
          // the source contributes its link slot, every other node NH(v)
          // (a source slot past bit 31 is not in a one-word set: dropped, as
          // the two-phase forms drop slots >= 32 W)
          const uint32_t slot = b + j0 + k - sb;
          const uint32_t bits = (v == s) ? (slot < 32u ? 1u << slot : 0u) : nv;
          uint64_t old = dn[t];
          bool changed = false;
          for (;;) {
            const uint32_t dt = static_cast<uint32_t>(old), nt = static_cast<uint32_t>(old >> 32);
            if (c > dt || (c == dt && !(bits & ~nt))) break;
            const uint64_t nw = c < dt ? (uint64_t(c) | (uint64_t(bits) << 32))
                                       : (uint64_t(dt) | (uint64_t(nt | bits) << 32));
            const uint64_t seen = atomicCAS(reinterpret_cast<unsigned long long*>(&dn[t]),
                                            static_cast<unsigned long long>(old),
                                            static_cast<unsigned long long>(nw));
            if (seen == old) {
              changed = true;
              break;
            }
            old = seen;
          }
          if (changed) {
            const uint32_t bit = 1u << (t & 31u);
            if (!(atomicOr(&mark[t >> 5], bit) & bit)) {
              nxt[atomicAdd(&qcnt[(r + 1) % 3], 1u)] = t;
            }
          }
        }
      }
    }
    round_sync<true>();
    n = qcnt[(r + 1) % 3];
    __syncthreads();
  }
  uint32_t* oD = oDist + u0 * Sn;
  uint32_t* oN = oNh + u0 * Sn;
  for (uint32_t v = tid; v < N; v += kGBlock) {
    const uint64_t x = dn[v];
    oD[v] = static_cast<uint32_t>(x);
    oN[v] = static_cast<uint32_t>(x >> 32);
  }
  // ---- the unit's RouteDb from the final LDS words (every thread left the
  // last round through its barrier: dn is final) --------------------------
  const uint32_t Sp = uint32_t(pt.max_prefixes);
  if (Sp == 0u) return;
  const uint32_t p0 = pt.pfx_base[unit.topo];
  const uint32_t P = pt.pfx_base[unit.topo + 1] - p0;
  const RouteCfg cfg{(flags & OGS_F_ENABLE_V4) != 0, (flags & OGS_F_V4_OVER_V6) != 0,
                     (flags & OGS_F_BEST_ROUTE_SELECTION) != 0};
  const PackedView sv{dn};
  for (uint32_t p = tid; p < Sp; p += kGBlock) {
    const size_t rec = size_t(u0) * Sp + p;
    uint32_t meta = 0, metric = kInf, selBits = 0, mask[1] = {0u};
    if (p < P) route_one<uint32_t, 1>(pt, p0 + p, s, nflags, sv, cfg, meta, metric, mask, selBits);
    if (out.meta) out.meta[rec] = meta;
    if (out.metric) static_cast<uint32_t*>(out.metric)[rec] = metric;
    if (out.sel) out.sel[rec] = selBits;
    if (out.mask) out.mask[rec] = mask[0];
  }
}

// "spf_global" option: 0 (default) the global path only where the LDS paths
// cannot hold a unit, 1 every ogs_spf_routes call (A/B, parity tests).
// EngineOptions::spfGlobal (engine.h), default 0
// "spf_global_sync": 1 (default) rounds end with drained stores + barrier
// and state is read through sc1 loads; 0 agent-scope fences per round (A/B)
// EngineOptions::spfGlobalSync (engine.h), default 1
// "spf_global_lds": 1 (default) the best LDS form that fits -- one-phase
// packed {dist, nh} words (spf_global_lds3_kernel, W = 1, u32), else
// distances and next-hop words in two phases (LdsBothState), else distances
// only (LdsDistState); 3 the two-phase form, 2 distances only, 0 always the
// all-HBM form (A/B)
// EngineOptions::spfGlobalLds (engine.h), default 1

// Does the LDS-resident workgroup path fit a unit of this graph? (the last
// fallback of spf_route.hip: dist + next-hop words, CSR read from L2)
bool lds_unit_fits(const ogs_graph& g, int W, uint32_t flags) {
  const uint64_t d = (flags & OGS_F_WIDE_METRIC) ? 8 : 4;
  const uint64_t b = ((uint64_t(g.max_nodes) * d + 15) & ~15ull) +
      ((uint64_t(g.max_nodes) * W * 4 + 15) & ~15ull);
  return b <= 160u * 1024u;
}

bool use_global(const ogs_graph& g, int W, uint32_t flags) {
  if (opts().spfGlobal == 1 || !lds_unit_fits(g, W, flags)) return true;
  // past the frontier kernel's LDS budget the remaining LDS paths sweep
  // every edge every round; on such graphs (large sparse / deep: WAN areas
  // of 16k+ nodes) the HBM frontier wins -- G1, 20,000-node WAN x 64
  // sources: 12.4 ms vs 35.0 ms for the multi-source sweep
  return g.max_nodes > 256 && !(flags & OGS_F_WIDE_METRIC) &&
      frontier_lds_bytes(uint32_t(g.max_nodes), W, false, true, false) > 160u * 1024u;
}

// SPF (+ RouteDb when pt has prefixes) of every unit with W-word next-hop
// sets (W == kWRuntime: Wn words, all state in HBM). dist / nh are the
// caller's rows where given, else workspace, followed by the units' scratch.
template <typename D, int W>
hipError_t launch_global_w(const ogs_graph& g, const ogs_prefix_table* pt,
                           const ogs_unit* units, int nUnits, uint32_t flags, int Wn,
                           const ogs_spf_out& out, hipStream_t stream) {
  const size_t Sn = size_t(g.max_nodes), U = size_t(nUnits);
  const size_t distBytes = out.dist ? 0 : round256(U * Sn * sizeof(D));
  const size_t nhBytes = out.nh ? 0 : round256(U * Wn * Sn * 4);
  void* ws = nullptr;
  hipError_t e = workspace(distBytes + nhBytes + round256(U * 3 * Sn * 4), stream, &ws);
  if (e != hipSuccess) return e;
  char* base = static_cast<char*>(ws);
  D* dist = out.dist ? static_cast<D*>(out.dist) : reinterpret_cast<D*>(base);
  uint32_t* nh = out.nh ? out.nh : reinterpret_cast<uint32_t*>(base + distBytes);
  uint32_t* scratch = reinterpret_cast<uint32_t*>(base + distBytes + nhBytes);
  auto run = [&](auto k, uint32_t ldsBytes) {
    return launch_dyn_lds(k, dim3(nUnits), dim3(kGBlock), ldsBytes, stream, g, units, flags, Wn,
                          dist, nh, scratch);
  };
  if constexpr (W == kWRuntime) {
    e = run(spf_global_kernel<HbmState<D, W, true>>, 0);
    if (e != hipSuccess || !pt || pt->max_prefixes == 0) return e;
    return launch_route_global_wide<D>(g, *pt, units, nUnits, flags, Wn, dist, nh, out, stream);
  } else {
    constexpr uint32_t kLds = 160u * 1024u;
    const int form = opts().spfGlobalLds;
    const bool sync = opts().spfGlobalSync;
    const uint32_t lds = global_lds_bytes(uint32_t(Sn), sizeof(D));
    const uint32_t lds2 = global_lds2_bytes(uint32_t(Sn), sizeof(D), W);
    const uint32_t lds3 = global_lds3_bytes(uint32_t(Sn));
    if constexpr (W == 1 && sizeof(D) == 4) {
      if (form == 1 && sync && lds3 <= kLds) {
        // the route pass runs inside the launch (no separate route kernel)
        const ogs_prefix_table ptv = pt ? *pt : ogs_prefix_table{};
        return launch_dyn_lds(spf_global_lds3_kernel<NoMods>, dim3(nUnits), dim3(kGBlock), lds3,
                              stream, g, units, flags, reinterpret_cast<uint32_t*>(dist), nh,
                              scratch, ptv, out);
      }
    }
    if ((form == 1 || form == 3) && sync && lds2 <= kLds) {
      e = run(spf_global_kernel<LdsBothState<D, W>>, lds2);
    } else if ((form == 1 || form == 2) && sync && lds <= kLds) {
      e = run(spf_global_kernel<LdsDistState<D, W>>, lds);
    } else if (sync) {
      e = run(spf_global_kernel<HbmState<D, W, true>>, 0);
    } else {
      e = run(spf_global_kernel<HbmState<D, W, false>>, 0);
    }
    if (e != hipSuccess || !pt || pt->max_prefixes == 0) return e;
    return launch_route_global<D, W>(g, *pt, units, nUnits, flags, dist, nh, out, stream);
  }
}

// SPF (+ RouteDb) with next-hop sets of any width (past 16 words, or a width
// that is no power of two).
hipError_t launch_spf_routes_global_wide(const ogs_graph& g, const ogs_prefix_table* pt,
                                         const ogs_unit* units, int nUnits, uint32_t flags,
                                         int W, const ogs_spf_out& out, hipStream_t stream) {
  if (flags & OGS_F_WIDE_METRIC) {
    return launch_global_w<uint64_t, kWRuntime>(g, pt, units, nUnits, flags, W, out, stream);
  }
  return launch_global_w<uint32_t, kWRuntime>(g, pt, units, nUnits, flags, W, out, stream);
}

template <typename D>
hipError_t launch_global_d(const ogs_graph& g, const ogs_prefix_table* pt,
                           const ogs_unit* units, int nUnits, uint32_t flags, int W,
                           const ogs_spf_out& out, hipStream_t stream) {
  switch (W) {
    case 1: return launch_global_w<D, 1>(g, pt, units, nUnits, flags, W, out, stream);
    case 2: return launch_global_w<D, 2>(g, pt, units, nUnits, flags, W, out, stream);
    case 4: return launch_global_w<D, 4>(g, pt, units, nUnits, flags, W, out, stream);
    case 8: return launch_global_w<D, 8>(g, pt, units, nUnits, flags, W, out, stream);
    case 16: return launch_global_w<D, 16>(g, pt, units, nUnits, flags, W, out, stream);
    default: return launch_global_w<D, kWRuntime>(g, pt, units, nUnits, flags, W, out, stream);
  }
}

// SPF (+ RouteDb when pt is non-NULL) of every unit through the global path.
hipError_t launch_spf_routes_global(const ogs_graph& g, const ogs_prefix_table* pt,
                                    const ogs_unit* units, int nUnits, uint32_t flags,
                                    int W, const ogs_spf_out& out, hipStream_t stream) {
  if (flags & OGS_F_WIDE_METRIC) {
    return launch_global_d<uint64_t>(g, pt, units, nUnits, flags, W, out, stream);
  }
  return launch_global_d<uint32_t>(g, pt, units, nUnits, flags, W, out, stream);
}

// ---- ogs_spf_routes_whatif_global ------------------------------------------
// Can the global what-if form take this area? (u32 distances, W = 1, 2 or 4)
bool whatif_global_takes(const ogs_graph& g, uint32_t flags, int W) {
  return !(flags & OGS_F_WIDE_METRIC) && (W == 1 || W == 2 || W == 4) && g.max_nodes > 0 &&
      uint32_t(g.max_nodes) <= OGS_MAX_NODES_PER_TOPO;
}

// One launch of the global-state SPF with the mods policy over every unit (the
// state form chosen as launch_global_w chooses it), then the route and diff
// pass. Workspace per unit: openr_gpu.h states it.
template <int W>
hipError_t launch_whatif_global_w(const ogs_graph& g, const ogs_prefix_table& pt,
                                  const ogs_unit* units, int nUnits,
                                  const ogs_whatif_mods& mods, const ogs_route_diff* diff,
                                  uint32_t flags, const ogs_spf_out& out, hipStream_t stream) {
  const size_t Sn = size_t(g.max_nodes), U = size_t(nUnits), Sp = size_t(pt.max_prefixes);
  const uint32_t ew = (uint32_t(std::max(g.max_edges, 0)) + 31u) / 32u;
  const uint32_t SnB = (uint32_t(Sn) + 3u) & ~3u;
  const bool nodes = mods.node_off != nullptr;
  const size_t distBytes = out.dist ? 0 : round256(U * Sn * 4);
  const size_t nhBytes = out.nh ? 0 : round256(U * W * Sn * 4);
  const size_t listBytes = round256(U * 3 * Sn * 4);
  const size_t bitBytes = round256(U * size_t(ew) * 8);
  const size_t rowBytes = nodes ? round256(U * size_t(SnB)) : 0;
  void* ws = nullptr;
  hipError_t e = workspace(distBytes + nhBytes + listBytes + bitBytes + rowBytes + round256(U * 4),
                           stream, &ws);
  if (e != hipSuccess) return e;
  char* base = static_cast<char*>(ws);
  uint32_t* dist = out.dist ? static_cast<uint32_t*>(out.dist) : reinterpret_cast<uint32_t*>(base);
  uint32_t* nh = out.nh ? out.nh : reinterpret_cast<uint32_t*>(base + distBytes);
  char* at = base + distBytes + nhBytes;
  uint32_t* scratch = reinterpret_cast<uint32_t*>(at);
  at += listBytes;
  uint64_t* bits = reinterpret_cast<uint64_t*>(at);
  at += bitBytes;
  uint8_t* frows = nodes ? reinterpret_cast<uint8_t*>(at) : nullptr;
  at += rowBytes;
  uint32_t* skip = reinterpret_cast<uint32_t*>(at);
  if (diff) {
    e = hipMemsetAsync(diff->changed, 0, U * ((Sp + 31) / 32) * 4, stream);
    if (e != hipSuccess) return e;
  }
  const bool changedOnly = (flags & OGS_F_CHANGED_ONLY) != 0;
  // Exit-only units at one next-hop word only: OGS_F_CHANGED_ONLY is an
  // nh_words == 1 mode (the entry refuses it otherwise), diff->base_nh is one
  // [S_n] row, and the exit's copy of the base rows below is a one-word copy.
  const bool exits = W == 1 && (flags & OGS_F_INCREMENTAL) && changedOnly && diff &&
      diff->base_dist && g.edge_src;
  GWhatifArgs a{};
  a.mods = mods;
  if (!mods.metric_off) a.mods.max_metric_per_unit = 0u;
  a.edgeSrc = exits ? g.edge_src : nullptr;
  a.baseDist = exits ? diff->base_dist : nullptr;
  a.baseNh = exits ? diff->base_nh : nullptr;
  a.exitDist = exits ? static_cast<uint32_t*>(out.dist) : nullptr;
  a.exitNh = exits && diff->base_nh ? out.nh : nullptr;
  a.counts = diff ? diff->counts : nullptr;
  a.bits = bits;
  a.frows = frows;
  a.skip = skip;
  a.ew = ew;
  a.SnB = SnB;
  a.restore = (flags & OGS_F_RESTORE) != 0;
  auto run = [&](auto k, uint32_t ldsBytes) {
    return launch_dyn_lds(k, dim3(nUnits), dim3(kGBlock), ldsBytes, stream, g, units, flags, W,
                          dist, nh, scratch, a);
  };
  // "spf_global_lds" chooses the state form as in launch_global_w.
  // "spf_global_sync" does not apply: the units' bitset and flag rows are read
  // with sc1 loads after drained stores, so every form here is an L2SYNC form
  // (the fenced HbmState<.., false> of that A/B is never taken).
  constexpr uint32_t kLds = 160u * 1024u;
  const int form = opts().spfGlobalLds;
  const uint32_t lds = global_lds_bytes(uint32_t(Sn), 4);
  const uint32_t lds2 = global_lds2_bytes(uint32_t(Sn), 4, W);
  const uint32_t lds3 = global_lds3_bytes(uint32_t(Sn));
  // (the one-phase kernel gets no prefix table: the route pass is its own launch)
  if (W == 1 && form == 1 && lds3 <= kLds) {
    if constexpr (W == 1) {
      e = launch_dyn_lds(spf_global_lds3_kernel<WhatifRows, GWhatifArgs>, dim3(nUnits),
                         dim3(kGBlock), lds3, stream, g, units, flags, dist, nh, scratch,
                         ogs_prefix_table{}, ogs_spf_out{}, a);
    }
  } else if ((form == 1 || form == 3) && lds2 <= kLds) {
    e = run(spf_global_kernel<LdsBothState<uint32_t, W>, WhatifRows, GWhatifArgs>, lds2);
  } else if ((form == 1 || form == 2) && lds <= kLds) {
    e = run(spf_global_kernel<LdsDistState<uint32_t, W>, WhatifRows, GWhatifArgs>, lds);
  } else {
    e = run(spf_global_kernel<HbmState<uint32_t, W, true>, WhatifRows, GWhatifArgs>, 0);
  }
  if (e != hipSuccess || Sp == 0) return e;
  const ogs_route_diff d = diff ? *diff : ogs_route_diff{};
  const unsigned by = unsigned((Sp + kBlock - 1) / kBlock);
  auto rk = changedOnly ? route_global_diff_kernel<W, true> : route_global_diff_kernel<W, false>;
  hipLaunchKernelGGL(rk, dim3(unsigned(nUnits), by), dim3(kBlock), 0, stream, g, pt, units, flags,
                     dist, nh, skip, mods.node_off, frows, SnB, d, out);
  return hipGetLastError();
}

hipError_t launch_whatif_global(const ogs_graph& g, const ogs_prefix_table& pt,
                                const ogs_unit* units, int nUnits, const ogs_whatif_mods& mods,
                                const ogs_route_diff* diff, uint32_t flags, int W,
                                const ogs_spf_out& out, hipStream_t stream) {
  switch (W) {
    case 1: return launch_whatif_global_w<1>(g, pt, units, nUnits, mods, diff, flags, out, stream);
    case 2: return launch_whatif_global_w<2>(g, pt, units, nUnits, mods, diff, flags, out, stream);
    case 4: return launch_whatif_global_w<4>(g, pt, units, nUnits, mods, diff, flags, out, stream);
    default: return hipErrorInvalidValue;
  }
}

// ogs_routes_from_spf: route_global_kernel over caller-held SPF state.
hipError_t launch_routes_from_spf(const ogs_graph& g, const ogs_prefix_table& pt,
                                  const ogs_unit* units, int n, const void* dist,
                                  const uint32_t* nh, const uint32_t* reach, uint32_t flags,
                                  int W, const ogs_spf_out& out, hipStream_t stream) {
  const bool wide = (flags & OGS_F_WIDE_METRIC) != 0;
#define OGS_RFS(W_)                                                                         \
  return wide ? launch_route_global<uint64_t, W_>(g, pt, units, n, flags,                   \
                                                  static_cast<const uint64_t*>(dist), nh,   \
                                                  out, stream, reach)                       \
              : launch_route_global<uint32_t, W_>(g, pt, units, n, flags,                   \
                                                  static_cast<const uint32_t*>(dist), nh,   \
                                                  out, stream, reach);
  switch (W) {
    case 1: OGS_RFS(1)
    case 2: OGS_RFS(2)
    case 4: OGS_RFS(4)
    case 8: OGS_RFS(8)
    case 16: OGS_RFS(16)
    default:  // sources of more than 512 links
      return wide ? launch_route_global_wide<uint64_t>(g, pt, units, n, flags, W,
                                                       static_cast<const uint64_t*>(dist), nh,
                                                       out, stream, reach)
                  : launch_route_global_wide<uint32_t>(g, pt, units, n, flags, W,
                                                       static_cast<const uint32_t*>(dist), nh,
                                                       out, stream, reach);
  }
#undef OGS_RFS
}

}  // namespace ogs
