// ogs_stub_whatif_pairs.cpp — the host-only stand-in's entries for
// ogs_spf_routes_whatif_pairs and its context twin, beside ogs_stub.cpp: no
// device, so the launch reports OGS_E_NODEVICE like every other compute entry
// point of the stub.
#include "openr_gpu.h"

extern "C" int ogs_spf_routes_whatif_pairs(const ogs_graph*, const ogs_prefix_table*,
                                           const ogs_unit*, int32_t, const ogs_whatif_pairs*,
                                           const ogs_whatif_mods*, ogs_route_diff*, uint32_t,
                                           int32_t, ogs_spf_out*, void*) {
  return OGS_E_NODEVICE;
}

extern "C" int ogs_ctx_spf_routes_whatif_pairs(ogs_ctx*, const ogs_graph*,
                                               const ogs_prefix_table*, const ogs_unit*, int32_t,
                                               const ogs_whatif_pairs*, const ogs_whatif_mods*,
                                               ogs_route_diff*, uint32_t, int32_t, ogs_spf_out*,
                                               void*) {
  return OGS_E_NODEVICE;
}
