// engine.h — per-context engine state of libopenr_gpu.so: the
// ogs_set_option knobs (EngineOptions) and the launch scratch (workspace).
// A context (ogs_ctx_create, include/openr_gpu.h) owns both, so two host
// threads with their own contexts never share a knob or a scratch buffer;
// the legacy entry points use the process default context. A context is
// thread-compatible, not thread-safe: one host thread at a time (the SURVEY
// §8(b) contract). Every option is read on the host, at launch time.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>
#include <map>
#include <mutex>
#include <vector>

namespace ogs {

// $OGS_UNIT_WIDTH seeds "unit_width" (un-validated) each time an
// EngineOptions is constructed
inline int unit_width_from_env() {
  const char* e = std::getenv("OGS_UNIT_WIDTH");
  return e ? std::atoi(e) : -1;
}

// Every ogs_set_option knob, stated once: X(name, EngineOptions member,
// default, accepted values), the accepted values being OGS_RANGE(lo, hi)
// (inclusive) or OGS_LIST(v, ...); whoever expands that argument defines the
// two macros. EngineOptions below and the name / validation table of
// ogs_set_option, ogs_get_option and ogs_option_name (capi.hip) are generated
// from this list, so a new knob is one line here plus its prose in
// include/openr_gpu.h. The meaning of each knob is documented where it is
// read (the "EngineOptions::<name>" comments) and in that header.
#define OGS_ENGINE_OPTIONS(X)                                              \
  X(ksp_wave_trace, kspWaveTrace, 1, OGS_LIST(0, 1))                       \
  X(ksp_hbm, kspHbm, 0, OGS_LIST(0, 1))                                    \
  X(ksp_queue, kspQueue, 1, OGS_LIST(0, 1))                                \
  X(ksp_stage, kspStage, -1, OGS_RANGE(-1, 2))                             \
  X(ksp_prune, kspPrune, 1, OGS_LIST(0, 1))                                \
  X(route_stream, routeStream, 5, OGS_LIST(1, 2, 4, 5))                    \
  X(route_store_nt, routeStoreNt, 2, OGS_RANGE(0, 3))                      \
  X(spf_lane_walk, spfLaneWalk, -1, OGS_RANGE(-1, 1))                      \
  X(spf_preload, spfPreload, 1, OGS_LIST(0, 1))                            \
  X(spf_seed_row, spfSeedRow, 1, OGS_LIST(0, 1))                           \
  X(spf_packed_scan, spfPackedScan, 1, OGS_LIST(0, 1))                     \
  X(spf_queue, spfQueue, -1, OGS_LIST(-1, 0))                              \
  X(spf_ninfo, spfNinfo, 1, OGS_RANGE(-1, 1))                              \
  X(frontier_block, frontierBlock, 0, OGS_LIST(0, 256, 512, 1024))         \
  X(frontier_parts, frontierParts, 0, OGS_RANGE(0, 16))                    \
  X(frontier_parts_wide, frontierPartsWide, 0, OGS_RANGE(0, 16))           \
  X(spf_frontier, spfFrontier, 1, OGS_LIST(0, 1))                          \
  X(c4_desc, c4Desc, 1, OGS_LIST(0, 1))                                    \
  X(spf_global, spfGlobal, 0, OGS_LIST(0, 1))                              \
  X(spf_global_sync, spfGlobalSync, 1, OGS_LIST(0, 1))                     \
  X(spf_global_lds, spfGlobalLds, 1, OGS_RANGE(0, 3))                      \
  X(lds_parts, ldsParts, 0, OGS_RANGE(0, 64))                              \
  X(lds_grid, ldsGrid, 0, OGS_RANGE(0, 4096))                              \
  X(lds_key16, ldsKey16, 1, OGS_LIST(0, 1))                                \
  X(lds_tail, ldsTail, 1, OGS_LIST(0, 1))                                  \
  X(lds_bfs_exit, ldsBfsExit, 1, OGS_LIST(0, 1))                           \
  X(lds_pull, ldsPull, 6, OGS_RANGE(0, 15))                                \
  X(lds_lead, ldsLead, 0, OGS_RANGE(-1, 65536))                            \
  X(lds_tail_parts, ldsTailParts, 0, OGS_RANGE(0, 64))                     \
  X(ms_group, msGroup, 0, OGS_LIST(0, 1, 2, 4))                            \
  X(wave_wg_lds, waveWgLds, 0, OGS_RANGE(0, 163840))                       \
  X(wave_upb, waveUpb, 4, OGS_LIST(4, 8, 16))                              \
  /* 2: OGS_WAVE_OPT_REG_ROUTES (spf_route_wave.hip) */                    \
  X(wave_opt, waveOpt, 2, OGS_RANGE(0, 3))                                 \
  X(unit_width, unitWidth, unit_width_from_env(),                          \
    OGS_LIST(-1, 0, 1, 2, 3, 64, 128, 256))

struct EngineOptions {
#define OGS_OPTION_MEMBER(name, member, def, accepted) int member = def;
  OGS_ENGINE_OPTIONS(OGS_OPTION_MEMBER)
#undef OGS_OPTION_MEMBER
};

struct Workspace {
  void* ptr = nullptr;
  size_t bytes = 0;
};

struct EngineContext {
  int device = 0;
  EngineOptions opts;
  std::map<hipStream_t, Workspace> ws;  // grow-only scratch per stream
  ~EngineContext();
};

// the process default options (ogs_set_option)
EngineOptions& default_options();
// the context bound to the calling thread for the current call (nullptr:
// the default context)
EngineContext* bound_context();
void bind_context(EngineContext* ctx);
inline const EngineOptions& opts() {
  EngineContext* c = bound_context();
  return c ? c->opts : default_options();
}

// Scratch of at least `bytes` for launches on `stream`: the bound context's
// own buffer (no lock: one host thread per context), else the default
// context's per-(device, stream) buffer under a mutex. A grown buffer's old
// block is retired, never freed while the process runs, so a pointer handed
// to another host thread stays valid (calls on ONE stream from several
// threads still share the buffer: give each thread its own context).
hipError_t workspace(size_t bytes, hipStream_t stream, void** out);

// RAII: sets the calling thread's HIP device to `device` for one scope and
// restores the thread's previous device on exit (only when it was changed)
class DeviceGuard {
 public:
  explicit DeviceGuard(int device) {
    if (device < 0) return;
    if (hipGetDevice(&prev_) != hipSuccess) {
      ok_ = false;
      return;
    }
    if (prev_ == device) return;
    set_ = hipSetDevice(device) == hipSuccess;
    ok_ = set_;
  }
  ~DeviceGuard() {
    if (set_) (void)hipSetDevice(prev_);
  }
  // false when the thread could not be switched to the device: the call
  // must not run (it would use the caller's device with the context's
  // pointers)
  bool ok() const { return ok_; }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;

 private:
  int prev_ = -1;
  bool set_ = false;
  bool ok_ = true;
};

// RAII: binds `ctx` (and its device) to the calling thread for one call; the
// thread's previous context binding AND its previous HIP device come back on
// exit, so a thread on device 1 calling a device-0 context stays on device 1
class BoundContext {
 public:
  explicit BoundContext(EngineContext* ctx)
      : prev_(bound_context()), dev_(ctx ? ctx->device : -1) {
    bind_context(ctx);
  }
  ~BoundContext() { bind_context(prev_); }
  bool ok() const { return dev_.ok(); }
  BoundContext(const BoundContext&) = delete;
  BoundContext& operator=(const BoundContext&) = delete;

 private:
  EngineContext* prev_;
  DeviceGuard dev_;
};

}  // namespace ogs
