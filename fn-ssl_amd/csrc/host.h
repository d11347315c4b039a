// Host-only plumbing shared by every kernel family: the one launch path (LDS limit, launch, check — runtime.hip), the
// run-time value -> template argument dispatch, and the workspace checks.
#pragma once

#include <cstdint>
#include <cstring>
#include <type_traits>

#include "common.h"

namespace fnssl {

// dry = a planning query (fnssl_lstm_plan, fnssl_lstm_backward_plan): every decision of the real call is taken, nothing
// is enqueued and the stream is never touched.  A caller without a planning mode passes its stream.
struct LaunchCtx {
  hipStream_t st;
  bool dry;
  LaunchCtx(hipStream_t s, bool d = false) : st(s), dry(d) {}
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
// limit (the occupancy query needs it), fnssl_lstm::kNoCluster unless the grid's workgroups fit the device at once, then as above.
int enqueue_args(const LaunchCtx& lc, const void* fn, int threads, size_t lds, const char* name, bool cluster, dim3 grid, void** args);

template <class... P>
int enqueue(const LaunchCtx& lc, const Kernel<P...>& k, dim3 grid, const std::common_type_t<P>&... args) {
  void* argv[] = {const_cast<void*>(static_cast<const void*>(&args))...};
  return enqueue_args(lc, reinterpret_cast<const void*>(k.fn), k.threads, k.lds, k.name, k.cluster, grid, argv);
}

// Run-time value -> compile-time constant: f(std::integral_constant) for the one of Vs that equals v (the caller has
// checked that one does), f(std::bool_constant) for b.  Returns what f returns.
template <int... Vs, class F>
int with_value(int v, F&& f) {
  int rc = FNSSL_E_INVALID;
  (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
  return rc;
}
template <class F>
int with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// float -> bf16 bits, round to nearest even, and back: what every weight packer uses (lstm_bf16.hip, lstm_bf16w.hip,
// conv.hip, conv_bf16x.hip).  A NaN keeps its sign and upper payload and becomes quiet (0x40), so it cannot round to an infinity.
inline unsigned short bf16_rne(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);   // NaN
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline float bf16_to_float(unsigned short h) {
  const unsigned u = (unsigned)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// one region of a workspace layout, in bytes from the workspace's start
struct WsRegion {
  size_t off, bytes;
  size_t end() const { return off + bytes; }
  float* floats(void* base) const { return reinterpret_cast<float*>(static_cast<char*>(base) + off); }
};

template <class... T>
bool aligned16(const T*... p) {
  return (((reinterpret_cast<uintptr_t>(p) & 15) == 0) && ...);
}
// FNSSL_E_WORKSPACE (with the message) unless the caller's workspace holds `need` bytes
inline int check_workspace(const char* who, const void* workspace, size_t bytes, size_t need) {
  if (workspace && bytes >= need) return FNSSL_OK;
  fnssl::set_error("%s: workspace %zu < %zu bytes", who, bytes, need);
  return FNSSL_E_WORKSPACE;
}

}  // namespace fnssl
