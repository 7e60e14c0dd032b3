// ogs_stub_node_diff.cpp — the host-only stand-in's entries for
// ogs_spf_node_diff and ogs_spf_node_changes_gather, beside ogs_stub.cpp: no
// device, so both report OGS_E_NODEVICE like every other compute entry point
// of the stub.
#include "openr_gpu.h"

extern "C" int ogs_spf_node_diff(const ogs_graph*, const ogs_unit*, int32_t, const ogs_spf_out*,
                                 const ogs_node_diff*, uint32_t, int32_t, void*) {
  return OGS_E_NODEVICE;
}

extern "C" int ogs_spf_node_changes_gather(const uint32_t*, int32_t, int32_t, const ogs_spf_out*,
                                           int32_t, const ogs_node_changes*, void*) {
  return OGS_E_NODEVICE;
}
