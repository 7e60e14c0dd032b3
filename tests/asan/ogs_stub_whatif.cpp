// ogs_stub_whatif.cpp — the host-only stand-in's entry for
// ogs_spf_routes_whatif, beside ogs_stub.cpp: no device, so the call reports
// OGS_E_NODEVICE like every other compute entry point of the stub.
#include "openr_gpu.h"

extern "C" int ogs_spf_routes_whatif(const ogs_graph*, const ogs_prefix_table*,
                                     const ogs_unit*, int32_t, const ogs_whatif_mods*,
                                     ogs_route_diff*, uint32_t, int32_t, ogs_spf_out*, void*) {
  return OGS_E_NODEVICE;
}
