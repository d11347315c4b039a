// The per-frame arithmetic of the front end, shared by the whole-signal kernels (frontend.hip) and the streamed kernel
// (frontend_stream.hip): the streamed front end promises the BITS of the whole-signal path, so both translation units
// inline these bodies (same compile flags) instead of restating them.
//   * tables, window, radix-4 transform and bin split of stft_rows_kernel (the kernel fnssl_stft_ex runs whenever the
//     magnitude sums are wanted, i.e. for every feature path);
//   * the per-frame means and the sequential recursion of ema_kernel / ema_array_kernel;
//   * the division by (mu + eps) of the pack kernels.
//
// Contraction is pinned.  The library is built with the compiler's default -ffp-contract=fast, under which WHICH product of
// a * b + c * d is fused into the fma depends on the surrounding code (the instruction order the combiner happens to
// visit), so the same source line gave different bits in two kernels.  Every function below that multiplies and adds
// therefore turns contraction off and spells its fused operations as fmaf(): the forms are the ones the compiler had
// chosen for the whole-signal kernels before they were shared (one product rounded, the other fused, as written below; the
// magnitude's two squares both rounded; the recursion one fma per frame), so those kernels' bits did not change.
#pragma once

#include "common.h"

namespace fnssl_frontend {

constexpr int kWin = FNSSL_WIN_LEN;   // 512
constexpr int kHop = FNSSL_HOP;       // 256
constexpr int kBins = FNSSL_NBIN;     // 257
constexpr int kNF = FNSSL_NF;         // 256
constexpr int kTwiddles = 384;        // exp(-2 pi i k / 512), k = 0..383 (the radix-4 stages reach 3 * 127)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// Orders this wave's LDS writes before its later LDS reads (a wave's LDS operations complete in order; this keeps the
// compiler from moving them across and waits for the outstanding ones) without stopping the other waves.
__device__ __forceinline__ void wave_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void pair_of(int p, int nch, int ch_mode, int& mi, int& mj) {
  if (ch_mode == FNSSL_CH_MODE_M) {
    mi = 0;
    mj = p + 1;
    return;
  }
  int i = 0, left = p;
  while (left >= nch - 1 - i) {   // row i holds nch-1-i pairs (Module.py:397-402)
    left -= nch - 1 - i;
    ++i;
  }
  mi = i;
  mj = i + 1 + left;
}

// ---- transform ---------------------------------------------------------------------------------------------------
// tw[0..384) = exp(-2 pi i k / 512), hann[0..512) = the periodic Hann-512 window; filled by `nthreads` threads
__device__ __forceinline__ void fill_tables(float2* tw, float* hann, int tid, int nthreads) {
  for (int k = tid; k < kTwiddles; k += nthreads) {
    float sn_, cs_;
    sincospif(-(float)k / 256.0f, &sn_, &cs_);
    tw[k] = make_float2(cs_, sn_);
  }
  for (int n = tid; n < kWin; n += nthreads) hann[n] = fmaf(-0.5f, cospif((float)n / 256.0f), 0.5f);
}

__device__ __forceinline__ unsigned digitrev4_8(unsigned m) {      // reverse the four base-4 digits of an 8-bit index
  return ((m & 3u) << 6) | ((m & 12u) << 2) | ((m & 48u) >> 2) | ((m & 192u) >> 6);
}

// z[m] = w[2m] x[2m] + i w[2m+1] x[2m+1], stored digit-reversed for fft256_radix4
__device__ __forceinline__ void window_store(float2* z, const float* hann, int m, float x0, float x1) {
#pragma clang fp contract(off)
  z[digitrev4_8(m)] = make_float2(hann[2 * m] * x0, hann[2 * m + 1] * x1);
}

__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
#pragma clang fp contract(off)
  return make_float2(fmaf(a.x, w.x, -(a.y * w.y)), fmaf(a.y, w.x, a.x * w.y));   // the products with w.y are the rounded ones
}

// 256-point complex FFT in place in z[256] (digit-reversed on entry, natural order on exit); tw[k] = exp(-2 pi i k / 512)
__device__ __forceinline__ void fft256_radix4(float2* z, const float2* tw, int lane) {
#pragma clang fp contract(off)
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int L = 1 << (2 * s);
    const int j = lane & (L - 1);
    const int base = ((lane >> (2 * s)) << (2 * s + 2)) + j;
    const int step = j * (128 >> (2 * s));                    // W_{4L}^j = tw[j * 512 / (4 L)]
    const float2 a0 = z[base];
    float2 a1 = z[base + L], a2 = z[base + 2 * L], a3 = z[base + 3 * L];
    if (s > 0) {
      a1 = cmul(a1, tw[step]);
      a2 = cmul(a2, tw[2 * step]);
      a3 = cmul(a3, tw[3 * step]);
    }
    const float2 t0 = make_float2(a0.x + a2.x, a0.y + a2.y), t1 = make_float2(a0.x - a2.x, a0.y - a2.y);
    const float2 t2 = make_float2(a1.x + a3.x, a1.y + a3.y);
    const float2 t3 = make_float2(a1.y - a3.y, a3.x - a1.x);  // -i (a1 - a3)
    z[base] = make_float2(t0.x + t2.x, t0.y + t2.y);
    z[base + L] = make_float2(t1.x + t3.x, t1.y + t3.y);
    z[base + 2 * L] = make_float2(t0.x - t2.x, t0.y - t2.y);
    z[base + 3 * L] = make_float2(t1.x - t3.x, t1.y - t3.y);   // a butterfly is in place: only the NEXT stage reads across lanes
    wave_lds_sync();
  }
}

// The 257 bins of the real frame from the packed transform z, five per lane at most:
//   X[k] = E[k] + W512^k O[k],  E = (Z[k] + conj Z[N-k])/2,  O = (Z[k] - conj Z[N-k])/(2i)
// emit(k, re, im) receives every bin; with SUM the wave's sum_k |X[k]| is returned (per-lane partial sums in bin order,
// then the xor butterfly of wave_sum), else 0.
template <bool SUM, class Emit>
__device__ __forceinline__ float split_bins(const float2* z, const float2* tw, int lane, Emit emit) {
#pragma clang fp contract(off)
  float msum = 0.f;
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const int k = lane + 64 * r;
    if (k <= 256) {
      const float2 zk = z[k & 255];
      const float2 zn = z[(256 - k) & 255];
      const float er2 = zk.x + zn.x, ei2 = zk.y - zn.y;                     // 2 E[k]
      const float dr = 0.5f * (zk.x - zn.x), di = 0.5f * (zk.y + zn.y);   // (Z[k] - conj Z[N-k]) / 2
      const float orr = di, oi = -dr;                                        // divide by i
      const float2 w = k < 256 ? tw[k] : make_float2(-1.f, 0.f);
      const float xr = fmaf(er2, 0.5f, fmaf(orr, w.x, -(oi * w.y)));
      const float xi = fmaf(ei2, 0.5f, fmaf(orr, w.y, oi * w.x));
      emit(k, xr, xi);
      if (SUM) msum += sqrtf(xr * xr + xi * xi);
    }
  }
  return SUM ? wave_sum(msum) : 0.f;
}

// ---- recursive normalisation -------------------------------------------------------------------------------------
// mean magnitude of a microphone pair's frame: (S_i + S_j) / 514
__device__ __forceinline__ float pair_mean(float si, float sj) { return __fdiv_rn(__fadd_rn(si, sj), (float)(2 * kBins)); }

// mean magnitude over ALL channels of a frame; s[c * stride] = the channel sums, added left to right like the reference
__device__ __forceinline__ float array_mean(const float* s, long long stride, int nch) {
  float acc = s[0];
  for (int c = 1; c < nch; ++c) acc = __fadd_rn(acc, s[(long long)c * stride]);
  return __fdiv_rn(acc, (float)(nch * kBins));
}

__device__ __forceinline__ float ema_term(float b_t, float mean) { return __fmul_rn(b_t, mean); }

// mu_t = a_t * mu_{t-1} + b_t * mean_t for n frames, by lane 0 on LDS operands: bm[0..n) holds b_t * mean_t on entry and
// mu_t on exit, ca_t[0..n) the a_t of the same frames, m the carried mu.  b_t * mean_t is rounded on its own; a_t * mu + it
// is one fma per frame (what the compiler made of the separately written product and sum).
__device__ __forceinline__ void ema_scan_tile(float* bm, const float* ca_t, int n, float& m, int lane) {
  wave_lds_sync();
  if (lane == 0) {
    float mm = m;
    for (int t = 0; t < n; ++t) {
      mm = fmaf(ca_t[t], mm, bm[t]);
      bm[t] = mm;
    }
    m = mm;
  }
  wave_lds_sync();
}

// ---- feature packing ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float feature_den(float mu, float eps) { return __fadd_rn(mu, eps); }

__device__ __forceinline__ float feature(float v, float den) { return __fdiv_rn(v, den); }

// [Re i, Re j, Im i, Im j] / den of one bin of a microphone pair
__device__ __forceinline__ float4 pair_feature(float2 xi, float2 xj, float den) {
  return make_float4(__fdiv_rn(xi.x, den), __fdiv_rn(xj.x, den), __fdiv_rn(xi.y, den), __fdiv_rn(xj.y, den));
}

}  // namespace fnssl_frontend
