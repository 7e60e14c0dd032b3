// route_global.h — one thread per (unit, prefix) RouteDb from SPF state in
// HBM (spf_global.hip, spf_exact.hip): route_one (route_core.h) against the
// unit's dist / next-hop rows, no per-node LDS staging, coalesced record
// stores. u32 or u64 distances. route_global_diff_kernel adds the diff
// against a base unit's records (route_stream.h: route_changed).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "openr_gpu.h"
#include "route_core.h"
#include "route_stream.h"
#include "spf_core.h"

namespace ogs {

// Unit state in HBM as the route kernel reads it.
template <typename D, int W>
struct GlobalView {
  const D* d;
  const uint32_t* n;
  size_t Sn;
  const uint32_t* r;  // settled bitset (exact-order state) or nullptr
  __device__ __forceinline__ D dist(uint32_t v) const { return d[v]; }
  __device__ __forceinline__ bool reached(uint32_t v) const {
    return r ? ((r[v >> 5] >> (v & 31u)) & 1u) != 0u : d[v] != DistInf<D>::value;
  }
  __device__ __forceinline__ uint32_t nh(uint32_t v, int w) const {
    return n[size_t(w) * Sn + v];
  }
};

// One thread per (unit, prefix): route_one against the unit's HBM state
// (grid x = unit, y = prefix block of 256).
template <typename D, int W>
__global__ __launch_bounds__(kBlock) void route_global_kernel(
    ogs_graph g, ogs_prefix_table pt, const ogs_unit* __restrict__ units,
    uint32_t flags, const D* __restrict__ sDist, const uint32_t* __restrict__ sNh,
    const uint32_t* __restrict__ sReach, ogs_spf_out out) {
  const uint32_t u = blockIdx.x;
  const uint32_t p = blockIdx.y * kBlock + threadIdx.x;
  const ogs_unit unit = units[u];
  const uint32_t Sp = uint32_t(pt.max_prefixes);
  const uint32_t p0 = pt.pfx_base[unit.topo];
  const uint32_t P = pt.pfx_base[unit.topo + 1] - p0;
  if (p >= Sp) return;
  const size_t Sn = size_t(g.max_nodes);
  const size_t rec = size_t(u) * Sp + p;
  uint32_t meta = 0, selBits = 0, mask[W];
  D metric = DistInf<D>::value;
#pragma unroll
  for (int w = 0; w < W; ++w) mask[w] = 0u;
  if (p < P) {
    const RouteCfg cfg{(flags & OGS_F_ENABLE_V4) != 0, (flags & OGS_F_V4_OVER_V6) != 0,
                       (flags & OGS_F_BEST_ROUTE_SELECTION) != 0};
    const GlobalView<D, W> sv{sDist + u * Sn, sNh + size_t(u) * W * Sn, Sn,
                              sReach ? sReach + size_t(u) * ((Sn + 31) / 32) : nullptr};
    route_one<D, W>(pt, p0 + p, unit.src, g.node_flags + g.node_base[unit.topo], sv, cfg,
                    meta, metric, mask, selBits);
  }
  if (out.meta) out.meta[rec] = meta;
  if (out.metric) static_cast<D*>(out.metric)[rec] = metric;
  if (out.sel) out.sel[rec] = selBits;
  if (out.mask) {
#pragma unroll
    for (int w = 0; w < W; ++w) out.mask[(size_t(u) * W + w) * Sp + p] = mask[w];
  }
}

// route_global_kernel for next-hop sets wider than 16 words (sources of more
// than 512 links; runtime W, masks stored word by word).
template <typename D>
__global__ __launch_bounds__(kBlock) void route_global_wide_kernel(
    ogs_graph g, ogs_prefix_table pt, const ogs_unit* __restrict__ units,
    uint32_t flags, int W, const D* __restrict__ sDist, const uint32_t* __restrict__ sNh,
    const uint32_t* __restrict__ sReach, ogs_spf_out out) {
  const uint32_t u = blockIdx.x;
  const uint32_t p = blockIdx.y * kBlock + threadIdx.x;
  const ogs_unit unit = units[u];
  const uint32_t Sp = uint32_t(pt.max_prefixes);
  const uint32_t p0 = pt.pfx_base[unit.topo];
  const uint32_t P = pt.pfx_base[unit.topo + 1] - p0;
  if (p >= Sp) return;
  const size_t Sn = size_t(g.max_nodes);
  const size_t rec = size_t(u) * Sp + p;
  uint32_t meta = 0, selBits = 0;
  D metric = DistInf<D>::value;
  uint32_t* mask = out.mask ? out.mask + size_t(u) * W * Sp + p : nullptr;
  if (p < P) {
    const RouteCfg cfg{(flags & OGS_F_ENABLE_V4) != 0, (flags & OGS_F_V4_OVER_V6) != 0,
                       (flags & OGS_F_BEST_ROUTE_SELECTION) != 0};
    const GlobalView<D, 1> sv{sDist + u * Sn, sNh + size_t(u) * W * Sn, Sn,
                              sReach ? sReach + size_t(u) * ((Sn + 31) / 32) : nullptr};
    route_one_wide<D>(pt, p0 + p, unit.src, g.node_flags + g.node_base[unit.topo], sv, cfg, W,
                      meta, metric, mask, Sp, selBits);
  } else if (mask) {
    for (int w = 0; w < W; ++w) mask[size_t(w) * Sp] = 0u;
  }
  if (out.meta) out.meta[rec] = meta;
  if (out.metric) static_cast<D*>(out.metric)[rec] = metric;
  if (out.sel) out.sel[rec] = selBits;
}

// The route and diff pass of the global-state what-if form
// (ogs_spf_routes_whatif_global): one thread per (unit, prefix) runs route_one
// against the unit's dist / next-hop rows and the unit's OWN node-flag row
// (soft-drain and drain bits change selection there), then route_changed
// against the base records. The `changed` words come from wave ballots (a
// wave's 64 prefixes are two whole words of the unit's row), the update /
// delete counts are summed per wave and added to the unit's counts. Records
// are written always, or only for changed prefixes (CHANGED_ONLY), in the
// slots ogs_route_changes_gather reads. skip[u] != 0: the unit ran no SPF
// (refused or exit-only) and writes nothing. frows: the units' flag rows
// [SnB each], read for units whose node slice is not empty.
template <int W, bool CHANGED_ONLY>
__global__ __launch_bounds__(kBlock) void route_global_diff_kernel(
    ogs_graph g, ogs_prefix_table pt, const ogs_unit* __restrict__ units, uint32_t flags,
    const uint32_t* __restrict__ sDist, const uint32_t* __restrict__ sNh,
    const uint32_t* __restrict__ skip, const uint32_t* __restrict__ nodeOff,
    const uint8_t* __restrict__ frows, uint32_t SnB, ogs_route_diff diff, ogs_spf_out out) {
  const uint32_t u = blockIdx.x;
  if (skip[u]) return;  // block-uniform
  const uint32_t p = blockIdx.y * kBlock + threadIdx.x;
  const ogs_unit unit = units[u];
  const uint32_t Sp = uint32_t(pt.max_prefixes);
  const uint32_t p0 = pt.pfx_base[unit.topo];
  const uint32_t P = pt.pfx_base[unit.topo + 1] - p0;
  const size_t Sn = size_t(g.max_nodes);
  const bool live = p < P && p < Sp;
  const bool ownRow = nodeOff && nodeOff[u + 1] > nodeOff[u];
  const uint8_t* nflags =
      ownRow ? frows + size_t(u) * SnB : g.node_flags + g.node_base[unit.topo];
  Rec<W> r;
  r.meta = 0u;
  r.metric = 0xFFFFFFFFu;
  r.sel = 0u;
#pragma unroll
  for (int w = 0; w < W; ++w) r.mask[w] = 0u;
  bool ch = false;
  uint32_t upd = 0, del = 0;
  if (live) {
    const RouteCfg cfg{(flags & OGS_F_ENABLE_V4) != 0, (flags & OGS_F_V4_OVER_V6) != 0,
                       (flags & OGS_F_BEST_ROUTE_SELECTION) != 0};
    const GlobalView<uint32_t, W> sv{sDist + u * Sn, sNh + size_t(u) * W * Sn, Sn, nullptr};
    route_one<uint32_t, W>(pt, p0 + p, unit.src, nflags, sv, cfg, r.meta, r.metric, r.mask,
                           r.sel);
    if (diff.changed) {
      const DiffCtx dc{diff.base_meta, diff.base_metric, diff.base_mask, nullptr, nullptr,
                       pt.adv_off + p0, diff.adv_class};
      ch = route_changed<W>(r, dc, Sp, p, upd, del);
    }
  }
  if (diff.changed) {
    const uint64_t bc = __ballot(ch);
    const uint32_t nu = uint32_t(__popcll(__ballot(upd != 0u)));
    const uint32_t nd = uint32_t(__popcll(__ballot(del != 0u)));
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t words = (Sp + 31u) / 32u;
    // the wave's first prefix is a multiple of 64: lanes 0 and 32 own a word each
    const uint32_t w0 = (p - lane) / 32u + (lane >> 5);
    if ((lane & 31u) == 0u && w0 < words) {
      const uint32_t word = uint32_t(bc >> (lane & 32u));
      if (word) diff.changed[size_t(u) * words + w0] = word;  // the call zeroed the row
    }
    if (lane == 0u) {
      if (nu) atomicAdd(diff.counts + size_t(u) * 2, nu);
      if (nd) atomicAdd(diff.counts + size_t(u) * 2 + 1, nd);
    }
  }
  if (!live || (CHANGED_ONLY && !ch)) return;
  const size_t rec = size_t(u) * Sp + p;
  if (out.meta) out.meta[rec] = r.meta;
  if (out.metric) static_cast<uint32_t*>(out.metric)[rec] = r.metric;
  if (out.sel) out.sel[rec] = r.sel;
  if (out.mask) {
#pragma unroll
    for (int w = 0; w < W; ++w) out.mask[(size_t(u) * W + w) * Sp + p] = r.mask[w];
  }
}

template <typename D>
hipError_t launch_route_global_wide(const ogs_graph& g, const ogs_prefix_table& pt,
                                    const ogs_unit* units, int nUnits, uint32_t flags, int W,
                                    const D* dist, const uint32_t* nh, const ogs_spf_out& out,
                                    hipStream_t stream, const uint32_t* reach = nullptr) {
  const unsigned by = unsigned((pt.max_prefixes + kBlock - 1) / kBlock);
  hipLaunchKernelGGL((route_global_wide_kernel<D>), dim3(unsigned(nUnits), by), dim3(kBlock), 0,
                     stream, g, pt, units, flags, W, dist, nh, reach, out);
  return hipGetLastError();
}

template <typename D, int W>
hipError_t launch_route_global(const ogs_graph& g, const ogs_prefix_table& pt,
                               const ogs_unit* units, int nUnits, uint32_t flags,
                               const D* dist, const uint32_t* nh, const ogs_spf_out& out,
                               hipStream_t stream, const uint32_t* reach = nullptr) {
  const unsigned by = unsigned((pt.max_prefixes + kBlock - 1) / kBlock);
  hipLaunchKernelGGL((route_global_kernel<D, W>), dim3(unsigned(nUnits), by), dim3(kBlock), 0,
                     stream, g, pt, units, flags, dist, nh, reach, out);
  return hipGetLastError();
}

}  // namespace ogs
