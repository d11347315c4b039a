// Host-only side of the LSTM kernels, shared by every family: what only they need on top of the library's launch path
// (host.h, re-exported here — the launch_*_k templates beside the kernels keep their static_assert, LDS and grid formulas
// and the kernel's address): the shape-table codes, the cluster knobs, the cluster-then-guarded-fallback protocol, and the
// extent checks.
#pragma once

#include "host.h"
#include "tuning.h"

namespace fnssl_lstm {

constexpr int kNoStatic = -100;    // returned by a shape table: no specialisation for the shape
// returned by a cluster launch when the device cannot hold every member workgroup at once (occupancy query): the caller
// runs the per-wave / pair-split kernels instead, unguarded
constexpr int kNoCluster = -101;

using fnssl::aligned16;
using fnssl::check_workspace;
using fnssl::enqueue;
using fnssl::Kernel;
using fnssl::LaunchCtx;
using fnssl::WsRegion;

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
inline bool mult4(long long so, long long si, long long st) { return ((so | si | st) & 3) == 0; }
inline bool mult4(const fnssl_view& v) { return mult4(v.so, v.si, v.st); }
inline bool nonneg(long long so, long long si, long long st) { return so >= 0 && si >= 0 && st >= 0; }
// buffer addressing: strides are non-negative, and per-wave lane spread + step walk + one row of `width` floats fit 32 bits
inline bool extent_ok(long long so, long long si, long long st, long long width, int nsteps) {
  return nonneg(so, si, st) && ((long double)so + 16.0L * si + (long double)nsteps * st + width) * 4.0L < 4.0e9L;
}
inline bool extent_ok(const fnssl_view& v, long long width, int nsteps) { return extent_ok(v.so, v.si, v.st, width, nsteps); }

}  // namespace fnssl_lstm
