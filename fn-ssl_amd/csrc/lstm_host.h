// Host-only side of the LSTM kernels, shared by every family: the one launch path (LDS limit, occupancy check of a cluster
// kernel, planning queries, launch — the launch_*_k templates beside the kernels keep their static_assert, LDS and grid
// formulas and the kernel's address), the cluster-then-guarded-fallback protocol, and the descriptor checks.
#pragma once

#include <cstdint>
#include <type_traits>

#include "common.h"
#include "tuning.h"

namespace fnssl_lstm {

constexpr int kNoStatic = -100;    // returned by a shape table: no specialisation for the shape
// returned by a cluster launch when the device cannot hold every member workgroup at once (occupancy query): the caller
// runs the per-wave / pair-split kernels instead, unguarded
constexpr int kNoCluster = -101;

// dry = a planning query (fnssl_lstm_plan, fnssl_lstm_backward_plan): every decision of the real call is taken, nothing
// is enqueued and the stream is never touched
struct LaunchCtx {
  hipStream_t st;
  bool dry;
};

template <class... P>
struct Kernel {
  void (*fn)(P...);
  int threads;            // per workgroup
  size_t lds;             // dynamic LDS bytes
  const char* name;       // for error messages
  bool cluster = false;   // every workgroup of the grid must be resident at once
};
template <class... P>
Kernel(void (*)(P...), int, size_t, const char*, bool = false) -> Kernel<P...>;

// runtime.hip.  dry -> FNSSL_OK at once; else raise the LDS limit (above 48 KB), launch, check.  A cluster kernel: raise the
// limit (the occupancy query needs it), kNoCluster unless `nwg` workgroups fit the device at once, then as above.
int enqueue_args(const LaunchCtx& lc, const void* fn, int threads, size_t lds, const char* name, bool cluster, int nwg, void** args);

template <class... P>
int enqueue(const LaunchCtx& lc, const Kernel<P...>& k, int nwg, const std::common_type_t<P>&... args) {
  void* argv[] = {const_cast<void*>(static_cast<const void*>(&args))...};
  return enqueue_args(lc, reinterpret_cast<const void*>(k.fn), k.threads, k.lds, k.name, k.cluster, nwg, argv);
}

// Knobs of the cluster kernels' bounded waits (fnssl_tuning): CLUSTER_SPIN_LIMIT (spins before a wave gives up),
// CLUSTER_TEST_STALL = m + 1 (fault injection: member m of cluster 0 exits at once, as if it never became resident).
inline unsigned cluster_spin_limit() {
  const int v = fnssl::tune(FNSSL_TUNE_CLUSTER_SPIN_LIMIT, 1, 1 << 30);
  return v ? (unsigned)v : (1u << 20);
}
inline int cluster_test_stall() { return fnssl::tune(FNSSL_TUNE_CLUSTER_TEST_STALL, 1, 1 << 20) - 1; }
// compute units the cluster kernels may count on: the device's minus what the caller keeps busy elsewhere (RESERVED_CUS:
// RCCL's all-reduce kernels under an overlapped backward), in whole XCD-uniform steps (a multiple of 8 CUs)
inline int cluster_cus() {
  const int ncu = fnssl::device_cus();
  int r = fnssl::tune(FNSSL_TUNE_RESERVED_CUS, 1, ncu);
  r = (r + 7) / 8 * 8;
  return r >= ncu ? 0 : ncu - r;
}
// The protocol of every cluster-resident family: the cluster kernel and, in the same call, the kernels behind it as its
// GUARDED fallback (they return at once unless the cluster kernel recorded a hand-off it gave up on).
//   cluster()        launches the family's cluster kernel, whose first workspace word is `status`: FNSSL_OK, kNoCluster or an error
//   fallback(guard)  launches what runs without it; guard != nullptr: as the guarded fallback, which reports no family
// The cluster family is reported only after the occupancy check passed (cluster() == FNSSL_OK), and a planning query stops
// there.  kNoCluster: the fallback runs unguarded, as for a shape the family does not take (handles = false).
template <class C, class F>
int cluster_then_fallback(const LaunchCtx& lc, bool handles, int cluster_family, int* family, const void* status, C&& cluster,
                          F&& fallback) {
  const unsigned* guard = nullptr;
  if (handles) {
    const int rc = cluster();
    if (rc == FNSSL_OK) {
      if (family) *family = cluster_family;
      if (lc.dry) return FNSSL_OK;
      guard = static_cast<const unsigned*>(status);
    } else if (rc != kNoCluster) {
      return rc;
    }
  }
  return fallback(guard);
}

// ---- descriptor checks ------------------------------------------------------------------------------------------------
// one region of a workspace layout (lstm.hip, lstm_train.hip), in bytes from the workspace's start
struct WsRegion {
  size_t off, bytes;
  size_t end() const { return off + bytes; }
};

template <class... T>
bool aligned16(const T*... p) {
  return (((reinterpret_cast<uintptr_t>(p) & 15) == 0) && ...);
}
inline bool mult4(long long so, long long si, long long st) { return ((so | si | st) & 3) == 0; }
inline bool mult4(const fnssl_view& v) { return mult4(v.so, v.si, v.st); }
inline bool nonneg(long long so, long long si, long long st) { return so >= 0 && si >= 0 && st >= 0; }
// buffer addressing: strides are non-negative, and per-wave lane spread + step walk + one row of `width` floats fit 32 bits
inline bool extent_ok(long long so, long long si, long long st, long long width, int nsteps) {
  return nonneg(so, si, st) && ((long double)so + 16.0L * si + (long double)nsteps * st + width) * 4.0L < 4.0e9L;
}
inline bool extent_ok(const fnssl_view& v, long long width, int nsteps) { return extent_ok(v.so, v.si, v.st, width, nsteps); }
// FNSSL_E_WORKSPACE (with the message) unless the caller's workspace holds `need` bytes
inline int check_workspace(const char* who, const void* workspace, size_t bytes, size_t need) {
  if (workspace && bytes >= need) return FNSSL_OK;
  fnssl::set_error("%s: workspace %zu < %zu bytes", who, bytes, need);
  return FNSSL_E_WORKSPACE;
}

}  // namespace fnssl_lstm
