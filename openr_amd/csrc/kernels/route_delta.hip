// route_delta.hip — the routes that differ between two builds of ONE source
// (ogs_route_delta).
//
// Reference: Decision::rebuildRoutes' full branch (Decision.cpp:912-927)
// builds the whole RouteDb and diffs it against the held one
// (DecisionRouteDb::calculateUpdate, SpfSolver.cpp:21-56). Here the previous
// and the next build's record blocks both live on the device (same prefix
// table, same source row), so the diff runs there and the host downloads and
// materialises the changed records only.
//
// Two launches, no workgroup ever waits on another:
//   pass 1  one workgroup per tile of kDeltaTile prefixes, four prefixes per
//           lane (16-B loads): the ROUTE and SELECTION bitmaps of the tile
//           (64 words each) and its {records, updates, deletions, no-route}
//           counts, all plain stores into the caller's workspace -- every
//           word of it is written, so nothing is zeroed first;
//   pass 2  one wavefront per tile: its base = the sum of the tile counts
//           before it, the in-wave popcount scan of route_update.hip, the
//           records; the last tile sums the counts into the header.
// Byte-bound and tiny (2 x (12 + 4W) B per prefix read once); the order is
// the prefix order whatever the schedule.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openr_gpu.h"
#include "route_stream.h"
#include "spf_core.h"
#include "launch.h"

namespace ogs {

constexpr uint32_t kDeltaTile = OGS_ROUTE_DELTA_TILE;  // prefixes per tile
constexpr int kDeltaBlock = int(kDeltaTile / 4);       // pass 1: 4 per lane
constexpr uint32_t kTileWords = kDeltaTile / 32;       // 64: one per lane
static_assert(kTileWords == 64, "pass 2 reads one bitmap word per lane");

// workspace: stats [T][4] | route bits [T][64] | selection bits [T][64]
struct DeltaWs {
  uint32_t *stats, *routeBits, *selBits;
  DeltaWs(void* ws, uint32_t T) {
    stats = static_cast<uint32_t*>(ws);
    routeBits = stats + size_t(T) * 4;
    selBits = routeBits + size_t(T) * kTileWords;
  }
};

struct DeltaSide {  // one build's records (rows of P) + optional policy columns
  const uint32_t* meta;
  const void* metric;
  const uint32_t* mask;
  const uint32_t* sel;
  const uint16_t* applied;
  const uint16_t* counter;
};

__device__ __forceinline__ bool no_route_reason(uint32_t meta) {
  if (meta & OGS_ROUTE_VALID) return false;
  const uint32_t r = (meta >> OGS_ROUTE_REASON_SHIFT) & 0xFu;
  return r == OGS_REASON_UNREACHABLE || r == OGS_REASON_NO_NEXTHOP;
}

template <int W, typename M>
__global__ __launch_bounds__(kDeltaBlock) void route_delta_mark_kernel(
    DeltaSide a /* next */, DeltaSide b /* prev */, uint32_t P,
    const uint32_t* __restrict__ advOff, const uint32_t* __restrict__ advClass, bool vec,
    uint32_t* __restrict__ stats, uint32_t* __restrict__ routeBits,
    uint32_t* __restrict__ selBits) {
  __shared__ uint32_t sStats[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  if (tid < 4) sStats[tid] = 0;
  __syncthreads();
  const uint32_t q = blockIdx.x * kDeltaTile + tid * 4u;
  uint32_t nibR = 0, nibS = 0, upd = 0, del = 0, noRoute = 0;
  if (q < P) {
    uint32_t am[4], bm[4], as[4], bs[4], aw[W][4], bw[W][4];
    M ac[4], bc[4];
    uint16_t aa[4], ba[4], an[4], bn[4];
    load4(a.meta, q, P, vec, am);
    load4(b.meta, q, P, vec, bm);
    load4(static_cast<const M*>(a.metric), q, P, vec, ac);
    load4(static_cast<const M*>(b.metric), q, P, vec, bc);
    load4(a.sel, q, P, vec, as);
    load4(b.sel, q, P, vec, bs);
#pragma unroll
    for (int w = 0; w < W; ++w) {
      load4(a.mask + size_t(w) * P, q, P, vec, aw[w]);
      load4(b.mask + size_t(w) * P, q, P, vec, bw[w]);
    }
    const bool pol = a.applied != nullptr;  // both sides or neither (capi.hip)
    if (pol) {
      load4(a.applied, q, P, vec, aa);
      load4(b.applied, q, P, vec, ba);
      load4(a.counter, q, P, vec, an);
      load4(b.counter, q, P, vec, bn);
    }
    constexpr uint32_t kSel = OGS_ROUTE_SELECTED | OGS_ROUTE_DRAINED |
        (0xFFFFFFu << OGS_ROUTE_BEST_SHIFT);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (q + uint32_t(j) >= P) break;
      const bool va = am[j] & OGS_ROUTE_VALID, vb = bm[j] & OGS_ROUTE_VALID;
      bool ch = records_differ<W>(
          am[j], bm[j], advOff, advClass, q + uint32_t(j), [&] { return ac[j] != bc[j]; },
          [&](int w) { return aw[w][j] != bw[w][j]; });
      // the statement choice decides next-hop weights and counterID
      if (pol && va && vb) ch |= aa[j] != ba[j] || an[j] != bn[j];
      const bool sc = ((am[j] ^ bm[j]) & kSel) != 0u || as[j] != bs[j];
      nibR |= (ch ? 1u : 0u) << j;
      nibS |= (sc ? 1u : 0u) << j;
      upd += (va && ch) ? 1u : 0u;
      del += (vb && !va) ? 1u : 0u;
      noRoute += no_route_reason(am[j]) ? 1u : 0u;
    }
  }
  // word k of the wave = the nibbles of lanes 8k..8k+7
  uint32_t wr = nibR << (4u * (lane & 7u)), wsel = nibS << (4u * (lane & 7u));
#pragma unroll
  for (int d = 1; d < 8; d <<= 1) {
    wr |= __shfl_xor(wr, d, 64);
    wsel |= __shfl_xor(wsel, d, 64);
  }
  if ((lane & 7u) == 0u) {
    const size_t w = size_t(blockIdx.x) * kTileWords + tid / 8u;
    routeBits[w] = wr;
    selBits[w] = wsel;
  }
  const uint32_t n = uint32_t(__popc(nibR | nibS));
  if (n) atomicAdd(&sStats[0], n);
  if (upd) atomicAdd(&sStats[1], upd);
  if (del) atomicAdd(&sStats[2], del);
  if (noRoute) atomicAdd(&sStats[3], noRoute);
  __syncthreads();
  if (tid < 4) stats[size_t(blockIdx.x) * 4 + tid] = sStats[tid];
}

template <int W, typename M>
__global__ __launch_bounds__(kBlock) void route_delta_gather_kernel(
    DeltaSide a /* next */, uint32_t P, uint32_t T, const uint32_t* __restrict__ stats,
    const uint32_t* __restrict__ routeBits, const uint32_t* __restrict__ selBits,
    ogs_route_delta_out out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t t = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (t >= T) return;  // whole wave leaves together
  uint32_t before = 0;
  for (uint32_t i = lane; i < t; i += 64u) before += stats[size_t(i) * 4];
  const uint32_t base = wave_sum(before);
  const size_t w = size_t(t) * kTileWords + lane;
  const uint32_t rb = routeBits[w], sb = selBits[w];
  uint32_t bits = rb | sb;
  const uint32_t c = uint32_t(__popc(bits));
  const uint32_t incl = wave_inclusive_scan(c, lane);
  uint32_t o = base + incl - c;
  const size_t cap = out.capacity;
  M* oMetric = static_cast<M*>(out.metric);
  const M* aMetric = static_cast<const M*>(a.metric);
  for (; bits; bits &= bits - 1u) {
    const uint32_t k = uint32_t(__builtin_ctz(bits));
    const uint32_t p = uint32_t(w) * 32u + k;
    if (o < cap && p < P) {  // never past the caller's arrays
      out.prefix[o] = p;
      out.kind[o] = ((rb >> k) & 1u ? OGS_DELTA_ROUTE : 0u) |
          ((sb >> k) & 1u ? OGS_DELTA_SELECTION : 0u);
      out.meta[o] = a.meta[p];
      oMetric[o] = aMetric[p];
      out.sel[o] = a.sel[p];
#pragma unroll
      for (int j = 0; j < W; ++j) out.mask[size_t(j) * cap + o] = a.mask[size_t(j) * P + p];
      if (a.applied) {
        out.applied[o] = a.applied[p];
        out.counter[o] = a.counter[p];
      }
    }
    ++o;
  }
  if (t == T - 1u) {  // every earlier tile is in `base`: the totals
    uint32_t upd = 0, del = 0, noRoute = 0;
    for (uint32_t i = lane; i < T; i += 64u) {
      upd += stats[size_t(i) * 4 + 1];
      del += stats[size_t(i) * 4 + 2];
      noRoute += stats[size_t(i) * 4 + 3];
    }
    upd = wave_sum(upd);
    del = wave_sum(del);
    noRoute = wave_sum(noRoute);
    const uint32_t total = base + __shfl(incl, 63, 64);
    if (lane == 0) {
      out.header[0] = total;
      out.header[1] = upd;
      out.header[2] = del;
      out.header[3] = noRoute;
    }
  }
}

template <int W, typename M>
static hipError_t launch_delta(const DeltaSide& a, const DeltaSide& b, uint32_t P,
                               const uint32_t* advOff, const uint32_t* advClass, bool vec,
                               const ogs_route_delta_out& out, void* workspace,
                               hipStream_t stream) {
  const uint32_t T = (P + kDeltaTile - 1u) / kDeltaTile;
  const DeltaWs ws(workspace, T);
  hipLaunchKernelGGL((route_delta_mark_kernel<W, M>), dim3(T), dim3(kDeltaBlock), 0, stream, a,
                     b, P, advOff, advClass, vec, ws.stats, ws.routeBits, ws.selBits);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const unsigned grid = (T + kBlock / 64 - 1) / (kBlock / 64);
  hipLaunchKernelGGL((route_delta_gather_kernel<W, M>), dim3(grid), dim3(kBlock), 0, stream, a,
                     P, T, ws.stats, ws.routeBits, ws.selBits, out);
  return hipGetLastError();
}

hipError_t launch_route_delta(const ogs_spf_out& prev, const ogs_spf_out& next, int P,
                              const uint32_t* advOff, const uint32_t* advClass,
                              const ogs_route_delta_policy* policy, bool wide, int W,
                              const ogs_route_delta_out& out, void* workspace,
                              hipStream_t stream) {
  const DeltaSide a{next.meta, next.metric, next.mask, next.sel,
                    policy ? policy->next_applied : nullptr,
                    policy ? policy->next_counter : nullptr};
  const DeltaSide b{prev.meta, prev.metric, prev.mask, prev.sel,
                    policy ? policy->prev_applied : nullptr,
                    policy ? policy->prev_counter : nullptr};
  // vector loads need 16-B aligned rows (mask row w starts at w * P); the u16
  // policy columns are read 8 B at a time
  uintptr_t align = 0;
  for (const DeltaSide* s : {&a, &b}) {
    align |= reinterpret_cast<uintptr_t>(s->meta) | reinterpret_cast<uintptr_t>(s->metric) |
        reinterpret_cast<uintptr_t>(s->mask) | reinterpret_cast<uintptr_t>(s->sel) |
        (reinterpret_cast<uintptr_t>(s->applied) << 1) |
        (reinterpret_cast<uintptr_t>(s->counter) << 1);
  }
  const bool vec = (uint32_t(P) & 3u) == 0u && (align & 15u) == 0u;
  const uint32_t n = uint32_t(P);
#define OGS_DELTA_CASE(W_)                                                                  \
  case W_:                                                                                  \
    return wide ? launch_delta<W_, uint64_t>(a, b, n, advOff, advClass, vec, out, workspace, \
                                             stream)                                        \
                : launch_delta<W_, uint32_t>(a, b, n, advOff, advClass, vec, out, workspace, \
                                             stream)
  switch (W) {
    OGS_DELTA_CASE(1);
    OGS_DELTA_CASE(2);
    OGS_DELTA_CASE(4);
    default: return hipErrorInvalidValue;
  }
#undef OGS_DELTA_CASE
}

}  // namespace ogs
