// spf_node_delta.hip — the nodes whose SPF row differs from a base unit's
// (ogs_spf_node_diff, ogs_spf_node_changes_gather).
//
// Reference: SpfSolver::buildRouteDb makes one node-label MPLS route per
// labelled node from that node's SPF row alone -- reached, metric, next hops
// (SpfSolver.cpp:352-445) -- and DecisionRouteDb::calculateUpdate diffs those
// routes (SpfSolver.cpp:41-54). The what-if sweep's units all share the base
// unit's topology and source, so the label routes that can differ are those
// of the nodes whose row differs: the diff runs on the rows where they lie
// and the host downloads and re-resolves the changed ones only.
//
// Two launches, no workgroup ever waits on another:
//   diff    one workgroup per unit walks its rows in tiles of kNodeTile nodes,
//           four nodes per lane (16-B loads): the tile's 32 bitmap words from
//           an OR across each group of 8 lanes, the unit's count summed in
//           registers, across the waves through LDS and stored once -- every
//           word of the bitmap and every count is a plain store, so nothing
//           is zeroed first and there is no atomic;
//   gather  one wavefront per unit, the in-wave popcount scan of
//           route_update.hip, the records in node order.
// Byte-bound: 2 x 4 (1 + W) B per compared node read once, 4 (2 + W) B
// written per changed record.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openr_gpu.h"
#include "spf_core.h"
#include "launch.h"

namespace ogs {

constexpr uint32_t kNodeTile = uint32_t(kBlock) * 4u;  // nodes per step: 4 per lane

template <int W>
__global__ __launch_bounds__(kBlock) void spf_node_diff_kernel(
    const uint32_t* __restrict__ nodeBase, uint32_t nTopos, const ogs_unit* __restrict__ units,
    uint32_t Sn, const uint32_t* __restrict__ dist, const uint32_t* __restrict__ nh,
    ogs_node_diff d, bool vec) {
  __shared__ uint32_t sCount[kBlock / 64];
  const uint32_t u = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
  const uint32_t words = (Sn + 31u) / 32u;
  uint32_t* __restrict__ row = d.changed + size_t(u) * words;
  // a refused unit wrote no rows: none is read (the whole workgroup leaves)
  if (d.unit_counts && d.unit_counts[2 * size_t(u)] == OGS_WHATIF_REFUSED) {
    for (uint32_t w = tid; w < words; w += kBlock) row[w] = 0u;
    if (tid == 0) d.counts[u] = 0u;
    return;
  }
  const ogs_unit unit = units[u];
  // (a topology index past the batch compares nothing, before it indexes anything)
  const uint32_t n = unit.topo < nTopos ? nodeBase[unit.topo + 1] - nodeBase[unit.topo] : 0u;
  const uint32_t N = n < Sn ? n : Sn;  // nodes past it are padding of the stride
  const uint32_t* __restrict__ uDist = dist + size_t(u) * Sn;
  const uint32_t* __restrict__ uNh = nh + size_t(u) * W * Sn;
  uint32_t count = 0;
  for (uint32_t q0 = 0; q0 < words * 32u; q0 += kNodeTile) {
    const uint32_t q = q0 + tid * 4u;
    uint32_t nib = 0;
    // the lane's four nodes share one word of the interest mask (q % 4 == 0)
    const uint32_t want =
        q >= N ? 0u : d.interest ? (d.interest[q >> 5] >> (q & 31u)) & 0xFu : 0xFu;
    if (want) {
      uint32_t ad[4], bd[4], aw[W][4], bw[W][4];
      load4(uDist, q, Sn, vec, ad);
      load4(d.base_dist, q, Sn, vec, bd);
#pragma unroll
      for (int w = 0; w < W; ++w) {
        load4(uNh + size_t(w) * Sn, q, Sn, vec, aw[w]);
        load4(d.base_nh + size_t(w) * Sn, q, Sn, vec, bw[w]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t v = q + uint32_t(j);
        const bool ra = ad[j] != ~0u, rb = bd[j] != ~0u;
        bool ch = ad[j] != bd[j];  // covers reached against unreached
#pragma unroll
        for (int w = 0; w < W; ++w) ch |= ra && rb && aw[w][j] != bw[w][j];
        if (v < N && v != unit.src && ch) nib |= 1u << j;
      }
      nib &= want;
    }
    // word k of the wave = the nibbles of lanes 8k..8k+7
    uint32_t word = nib << (4u * (lane & 7u));
#pragma unroll
    for (int s = 1; s < 8; s <<= 1) word |= __shfl_xor(word, s, 64);
    const uint32_t w = q >> 5;
    if ((lane & 7u) == 0u && w < words) row[w] = word;
    count += uint32_t(__popc(nib));
  }
  count = wave_sum(count);
  if (lane == 0) sCount[tid >> 6] = count;
  __syncthreads();
  if (tid == 0) {
    uint32_t total = 0;
#pragma unroll
    for (int i = 0; i < kBlock / 64; ++i) total += sCount[i];
    d.counts[u] = total;
  }
}

template <int W>
__global__ __launch_bounds__(kBlock) void spf_node_changes_kernel(
    const uint32_t* __restrict__ changed, uint32_t nUnits, uint32_t Sn,
    const uint32_t* __restrict__ dist, const uint32_t* __restrict__ nh, ogs_node_changes out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t u = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (u >= nUnits) return;  // whole wave leaves together
  const uint32_t words = (Sn + 31u) / 32u;
  const uint32_t* row = changed + size_t(u) * words;
  uint32_t pos = out.offsets[u];
  const uint32_t end = out.offsets[u + 1];
  const size_t total = out.total;
  for (uint32_t w0 = 0; w0 < words; w0 += 64u) {
    const uint32_t w = w0 + lane;
    uint32_t bits = w < words ? row[w] : 0u;
    if (w == words - 1u && (Sn & 31u)) bits &= (1u << (Sn & 31u)) - 1u;
    const uint32_t c = uint32_t(__popc(bits));
    const uint32_t incl = wave_inclusive_scan(c, lane);  // of the popcounts
    uint32_t o = pos + incl - c;
    for (; bits; bits &= bits - 1u) {
      const uint32_t v = w * 32u + uint32_t(__builtin_ctz(bits));
      if (o < end && o < total) {  // never past the unit's slice, even on a bad scan
        out.node[o] = v;
        out.dist[o] = dist[size_t(u) * Sn + v];
#pragma unroll
        for (int k = 0; k < W; ++k) {
          out.nh[size_t(k) * total + o] = nh[(size_t(u) * W + k) * Sn + v];
        }
      }
      ++o;
    }
    pos += __shfl(incl, 63, 64);
  }
}

hipError_t launch_spf_node_diff(const ogs_graph& g, const ogs_unit* units, int nUnits,
                                const uint32_t* dist, const uint32_t* nh, int W,
                                const ogs_node_diff& diff, hipStream_t stream) {
  const uint32_t Sn = uint32_t(g.max_nodes);
  // vector loads need 16-B aligned rows: row r of any of the four arrays starts
  // r * Sn elements in
  const uintptr_t align = reinterpret_cast<uintptr_t>(dist) | reinterpret_cast<uintptr_t>(nh) |
      reinterpret_cast<uintptr_t>(diff.base_dist) | reinterpret_cast<uintptr_t>(diff.base_nh);
  const bool vec = (Sn & 3u) == 0u && (align & 15u) == 0u;
  const dim3 grid{unsigned(nUnits)};
#define OGS_NODE_DIFF_CASE(W_)                                                                \
  case W_:                                                                                    \
    hipLaunchKernelGGL(spf_node_diff_kernel<W_>, grid, dim3(kBlock), 0, stream, g.node_base, \
                       uint32_t(g.num_topos), units, Sn, dist, nh, diff, vec);                \
    break
  switch (W) {
    OGS_NODE_DIFF_CASE(1);
    OGS_NODE_DIFF_CASE(2);
    OGS_NODE_DIFF_CASE(4);
    default: return hipErrorInvalidValue;
  }
#undef OGS_NODE_DIFF_CASE
  return hipGetLastError();
}

hipError_t launch_spf_node_changes(const uint32_t* changed, int nUnits, int Sn, int W,
                                   const uint32_t* dist, const uint32_t* nh,
                                   const ogs_node_changes& out, hipStream_t stream) {
  const dim3 grid(unsigned((nUnits + kBlock / 64 - 1) / (kBlock / 64)));
  const uint32_t U = uint32_t(nUnits), S = uint32_t(Sn);
#define OGS_NODE_CHANGES_CASE(W_)                                                           \
  case W_:                                                                                  \
    hipLaunchKernelGGL(spf_node_changes_kernel<W_>, grid, dim3(kBlock), 0, stream, changed, \
                       U, S, dist, nh, out);                                                \
    break
  switch (W) {
    OGS_NODE_CHANGES_CASE(1);
    OGS_NODE_CHANGES_CASE(2);
    OGS_NODE_CHANGES_CASE(4);
    default: return hipErrorInvalidValue;
  }
#undef OGS_NODE_CHANGES_CASE
  return hipGetLastError();
}

}  // namespace ogs
