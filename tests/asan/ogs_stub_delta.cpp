// ogs_stub_delta.cpp — the host-only stand-in's entry for ogs_route_delta
// (ABI 8), beside ogs_stub.cpp: no device, so the call reports
// OGS_E_NODEVICE like every other compute entry point of the stub.
#include "openr_gpu.h"

extern "C" int ogs_route_delta(const ogs_spf_out*, const ogs_spf_out*, int32_t, const uint32_t*,
                               const uint32_t*, const ogs_route_delta_policy*, uint32_t, int32_t,
                               const ogs_route_delta_out*, void*, void*) {
  return OGS_E_NODEVICE;
}
