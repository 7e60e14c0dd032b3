// launch.h -- every host function that one kernel translation unit defines
// and another calls, declared once: the defining and the calling unit both
// include this header, so a drifted signature is a compile error (and the
// library is linked with -z defs, so a missing definition is a link error).
// Default arguments live here only. spf_lds.h states spf_lds.hip's interface
// the same way.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "openr_gpu.h"
#include "engine.h"

namespace ogs {

// Workspace regions start on 256-byte boundaries.
inline size_t round256(size_t x) { return (x + 255) & ~size_t(255); }

// Launch k with `lds` bytes of dynamic LDS; past the 64 kB a kernel gets by
// default its limit is raised first.
template <typename... P, typename... A>
hipError_t launch_dyn_lds(void (*k)(P...), dim3 grid, dim3 block, size_t lds,
                          hipStream_t stream, const A&... args) {
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(
        reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k, grid, block, lds, stream, args...);
  return hipGetLastError();
}

// ---- the C-ABI's entry points (capi.hip calls them) ------------------------
// spf_route.hip
hipError_t launch_spf_routes(const ogs_graph& g, const ogs_prefix_table* pt,
                             const ogs_unit* units, int nUnits, uint32_t flags,
                             int W, const ogs_spf_out& out, hipStream_t stream,
                             int* unsupported);
// route_stream.hip
hipError_t launch_spf_routes_groups(const ogs_graph& g, const ogs_prefix_table* pt,
                                    const ogs_route_group* groups, int n, uint32_t flags,
                                    hipStream_t stream, int* unsupported);
hipError_t launch_variants(const ogs_graph& g, const ogs_prefix_table& pt,
                           const ogs_unit* units, int nUnits,
                           const ogs_unit_mods* mods, ogs_route_diff* diff,
                           uint32_t flags, int W, const ogs_spf_out& out,
                           hipStream_t stream, int* unsupported);
// *unsupported: 1 the rule launch_variants shares, 2 drains that the repair
// cannot take (no OGS_F_INCREMENTAL, W > 1, its LDS budget), 3 a dead bitset
// past every form's LDS
hipError_t launch_scenarios(const ogs_graph& g, const ogs_prefix_table& pt,
                            const ogs_unit* units, int nUnits,
                            const ogs_scenario_mods& mods, ogs_route_diff* diff,
                            uint32_t flags, int W, const ogs_spf_out& out,
                            hipStream_t stream, int* unsupported);
// *unsupported: 1 and 3 as launch_scenarios (3: the bitsets and the metric
// slice past every form's LDS), 2 node bits that the repair cannot take
hipError_t launch_whatif(const ogs_graph& g, const ogs_prefix_table& pt,
                         const ogs_unit* units, int nUnits,
                         const ogs_whatif_mods& mods, ogs_route_diff* diff,
                         uint32_t flags, int W, const ogs_spf_out& out,
                         hipStream_t stream, int* unsupported);
// ogs_spf_routes_whatif_pairs: the repair only. *unsupported: 1 as
// launch_whatif, 2 the repair cannot take the call
hipError_t launch_whatif_pairs(const ogs_graph& g, const ogs_prefix_table& pt,
                               const ogs_unit* units, int nUnits,
                               const ogs_whatif_pairs& pairs, const ogs_whatif_mods& mods,
                               ogs_route_diff* diff, uint32_t flags, int W,
                               const ogs_spf_out& out, hipStream_t stream, int* unsupported);
// route_multiarea.hip
hipError_t launch_routes_multiarea(const ogs_graph& g, const ogs_prefix_table& pt,
                                   const ogs_area_table& at,
                                   const uint32_t* units, int n,
                                   const uint32_t* spfRow, const void* dist,
                                   const uint32_t* nh, uint32_t flags, int W,
                                   const ogs_spf_out& out, hipStream_t stream);
// rib_policy.hip
hipError_t launch_rib_policy(const ogs_prefix_table& pt, const ogs_rib_policy& pol,
                             int A, int nUnits, int W, const uint32_t* meta,
                             uint32_t* mask, uint16_t* applied, uint16_t* counter,
                             hipStream_t stream);
// route_update.hip
hipError_t launch_route_changes(const uint32_t* changed, int nUnits, int Sp, int W,
                                const uint32_t* meta, const uint32_t* metric,
                                const uint32_t* mask, const ogs_route_changes& out,
                                hipStream_t stream);
// route_delta.hip
hipError_t launch_route_delta(const ogs_spf_out& prev, const ogs_spf_out& next, int P,
                              const uint32_t* advOff, const uint32_t* advClass,
                              const ogs_route_delta_policy* policy, bool wide, int W,
                              const ogs_route_delta_out& out, void* workspace,
                              hipStream_t stream);
// spf_node_delta.hip
hipError_t launch_spf_node_diff(const ogs_graph& g, const ogs_unit* units, int nUnits,
                                const uint32_t* dist, const uint32_t* nh, int W,
                                const ogs_node_diff& diff, hipStream_t stream);
hipError_t launch_spf_node_changes(const uint32_t* changed, int nUnits, int Sn, int W,
                                   const uint32_t* dist, const uint32_t* nh,
                                   const ogs_node_changes& out, hipStream_t stream);
// csr_patch.hip
hipError_t launch_csr_patch(uint64_t* edges, const uint32_t* idx, const uint64_t* val,
                            int n, hipStream_t stream);
// spf_global.hip
hipError_t launch_routes_from_spf(const ogs_graph& g, const ogs_prefix_table& pt,
                                  const ogs_unit* units, int n, const void* dist,
                                  const uint32_t* nh, const uint32_t* reach, uint32_t flags,
                                  int W, const ogs_spf_out& out, hipStream_t stream);
// ogs_spf_routes_whatif_global: what-if lists over the global-state SPF (any
// size; call when whatif_global_takes()), route diff in a second launch
bool whatif_global_takes(const ogs_graph& g, uint32_t flags, int W);
hipError_t launch_whatif_global(const ogs_graph& g, const ogs_prefix_table& pt,
                                const ogs_unit* units, int nUnits, const ogs_whatif_mods& mods,
                                const ogs_route_diff* diff, uint32_t flags, int W,
                                const ogs_spf_out& out, hipStream_t stream);
// ksp.hip
hipError_t launch_ksp(const ogs_graph& g, const ogs_path_unit* units,
                      int nUnits, const uint32_t* masks, uint32_t maskWords,
                      uint32_t flags, const ogs_path_out& out,
                      hipStream_t stream, int* unsupported);
hipError_t launch_ksp2(const ogs_graph& g, const ogs_unit* sources,
                       int nSources, const ogs_path_unit* units, int nUnits,
                       uint32_t flags, const ogs_path_out& o1,
                       const ogs_path_out& o2, hipStream_t stream,
                       int* unsupported);

// ---- the forms launch_spf_routes chooses among: each try_* returns false
// when the batch is not its to take, else true with the launch's status in
// *err ------------------------------------------------------------------------
// spf_route.hip
int small_unit_width();
// spf_route_small.hip (explicit instantiations there)
template <typename D, int W>
bool try_small(const ogs_graph& g, const ogs_prefix_table& pt, int hasPrefixes,
               const ogs_unit* units, int nUnits, uint32_t flags,
               const ogs_spf_out& out, int maxDegree, uint32_t maxA,
               int unitWidth, hipStream_t stream, hipError_t* err);
// spf_route_wave.hip
bool try_wave(const ogs_graph& g, const ogs_prefix_table& pt, int hasPrefixes,
              const ogs_unit* units, int nUnits, uint32_t flags,
              const ogs_spf_out& out, uint32_t maxA, hipStream_t stream,
              hipError_t* err);
// spf_route_ms.hip
bool try_ms(const ogs_graph& g, const ogs_prefix_table& pt, int hasPrefixes,
            const ogs_unit* units, int nUnits, uint32_t flags, int W,
            const ogs_spf_out& out, hipStream_t stream, hipError_t* err);
// route_stream.hip
bool try_frontier(const ogs_graph& g, const ogs_unit* units, int nUnits,
                  uint32_t flags, int W, uint32_t* dist, uint32_t* nh,
                  hipStream_t stream, hipError_t* err);
bool try_ms_stream(const ogs_graph& g, const ogs_prefix_table& pt,
                   const ogs_unit* units, int nUnits, uint32_t flags, int W,
                   const ogs_spf_out& out, hipStream_t stream, hipError_t* err);
// spf_exact.hip
hipError_t launch_spf_routes_exact(const ogs_graph& g, const ogs_prefix_table* pt,
                                   const ogs_unit* units, int nUnits, uint32_t flags,
                                   int W, const ogs_spf_out& out, hipStream_t stream);
// spf_global.hip
bool use_global(const ogs_graph& g, int W, uint32_t flags);
hipError_t launch_spf_routes_global(const ogs_graph& g, const ogs_prefix_table* pt,
                                    const ogs_unit* units, int nUnits, uint32_t flags,
                                    int W, const ogs_spf_out& out, hipStream_t stream);
hipError_t launch_spf_routes_global_wide(const ogs_graph& g, const ogs_prefix_table* pt,
                                         const ogs_unit* units, int nUnits, uint32_t flags,
                                         int W, const ogs_spf_out& out, hipStream_t stream);

// ---- spf_frontier.hip, for route_stream.hip and spf_global.hip -------------
uint32_t frontier_lds_bytes(uint32_t Sn, int W, bool queue = false, bool ninfo = true,
                            bool stamp8 = false);
bool frontier_fits(const ogs_graph& g, uint32_t flags, int W);
size_t chunk_scratch_bytes(const ogs_graph& g);
size_t desc_scratch_bytes(const ogs_graph& g);
void stream_parts(int nUnits, int W, int P, int* parts);
hipError_t launch_frontier_spf(const ogs_graph& g, const ogs_unit* units,
                               int nUnits, uint32_t flags, int W,
                               uint32_t* dist, uint32_t* nh, void* scratch,
                               hipStream_t stream);
hipError_t launch_frontier_routes(const ogs_graph& g, const ogs_prefix_table& pt,
                                  const uint32_t* key, const ogs_unit* units,
                                  int nUnits, uint32_t flags, int W,
                                  const ogs_spf_out& out, void* scratch,
                                  hipStream_t stream);
hipError_t launch_frontier_variants(const ogs_graph& g, const ogs_prefix_table& pt,
                                    const uint32_t* key, const ogs_unit* units,
                                    int n, uint32_t flags, int W,
                                    const ogs_spf_out& out,
                                    const ogs_unit_mods* mods,
                                    ogs_route_diff* diff, void* scratch,
                                    hipStream_t stream);
bool scenario_repair_fits(const ogs_graph& g, uint32_t flags, int W,
                          const ogs_route_diff* diff, bool drains);
bool scenario_frontier_fits(const ogs_graph& g, uint32_t flags, int W);
hipError_t launch_scenarios_repair(const ogs_graph& g, const ogs_prefix_table& pt,
                                   const uint32_t* key, const ogs_unit* units, int n,
                                   uint32_t flags, const ogs_spf_out& out,
                                   const ogs_scenario_mods& mods, ogs_route_diff* diff,
                                   void* scratch, hipStream_t stream);
hipError_t launch_frontier_lists(const ogs_graph& g, const ogs_prefix_table& pt,
                                 const uint32_t* key, const ogs_unit* units, int n,
                                 uint32_t flags, int W, const ogs_spf_out& out,
                                 const ogs_scenario_mods& mods, const ogs_route_diff* diff,
                                 void* scratch, hipStream_t stream);
bool whatif_repair_fits(const ogs_graph& g, uint32_t flags, int W, const ogs_route_diff* diff,
                        bool nodes, uint32_t maxMetric);
bool whatif_frontier_fits(const ogs_graph& g, uint32_t flags, int W, uint32_t maxMetric);
hipError_t launch_whatif_repair(const ogs_graph& g, const ogs_prefix_table& pt,
                                const uint32_t* key, const ogs_unit* units, int n,
                                uint32_t flags, const ogs_spf_out& out,
                                const ogs_whatif_mods& mods, ogs_route_diff* diff,
                                void* scratch, hipStream_t stream);
hipError_t launch_whatif_pairs_repair(const ogs_graph& g, const ogs_prefix_table& pt,
                                      const uint32_t* key, const ogs_unit* units, int n,
                                      uint32_t flags, const ogs_spf_out& out,
                                      const ogs_whatif_mods& mods, const ogs_whatif_pairs& pairs,
                                      const ogs_route_diff& diff, hipStream_t stream);
hipError_t launch_frontier_whatif(const ogs_graph& g, const ogs_prefix_table& pt,
                                  const uint32_t* key, const ogs_unit* units, int n,
                                  uint32_t flags, int W, const ogs_spf_out& out,
                                  const ogs_whatif_mods& mods, const ogs_route_diff* diff,
                                  void* scratch, hipStream_t stream);

}  // namespace ogs
