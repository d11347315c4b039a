// What the IPDnet2 forward kernels (spatialnet.hip), the Mamba block's backward (spatialnet_train.hip), the f-conv /
// full-band backward (spatialnet_layer_train.hip) and the encoder / head backward (spatialnet_net_train.hip) share: the
// shape constants, a point's row load / store and LayerNorm statistics, the head's tanh, the matrix-pipe helpers (LDS
// weight image, MFMA tile product), the index split, the host-side view checks, the forward workspace layout and the
// ordered reduction of partial sums.
#pragma once

#include <cstdlib>
#include <type_traits>

#include "host.h"

namespace {

constexpr int H = 96;      // dim_hidden
constexpr int E = 192;     // Mamba d_inner
constexpr int NST = 16;    // Mamba d_state
constexpr int RK = 6;      // Mamba dt_rank
constexpr int KC = 4;      // Mamba d_conv
constexpr int XP = 40;     // x_proj outputs (6 + 16 + 16) padded to a float4 multiple
constexpr int HS = 8;      // dim_squeeze
constexpr int NG = 8;      // f-conv groups
constexpr int CG = 12;     // channels per group
constexpr int KF = 5;      // f-conv taps
constexpr float kEps = 1e-5f;

// one point's 96 channels, to and from the thread's registers
__device__ __forceinline__ void load_row(float (&x)[H], const float* __restrict__ p) {
  const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll
  for (int i = 0; i < H / 4; ++i) {
    const float4 v = p4[i];
    x[4 * i] = v.x;
    x[4 * i + 1] = v.y;
    x[4 * i + 2] = v.z;
    x[4 * i + 3] = v.w;
  }
}

__device__ __forceinline__ void store_row(float* __restrict__ p, const float (&x)[H]) {
  float4* p4 = reinterpret_cast<float4*>(p);
#pragma unroll
  for (int i = 0; i < H / 4; ++i) p4[i] = make_float4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]);
}

// nn.LayerNorm statistics over the thread's own 96 channels (biased variance, eps inside the root).
__device__ __forceinline__ void ln_stats(const float (&x)[H], float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < H; ++c) s += x[c];
  mean = s * (1.f / H);
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < H; ++c) {
    const float d = x[c] - mean;
    v = fmaf(d, d, v);
  }
  rstd = 1.f / sqrtf(v * (1.f / H) + kEps);
}

// x * sigmoid(x) with the reciprocal instruction (1 ulp) instead of the IEEE division sequence (10 operations): the
// unsqueeze of the full-band branch alone applies it 96 times per point
__device__ __forceinline__ float silu_f(float x) { return x * __builtin_amdgcn_rcpf(1.f + __expf(-x)); }

// the head's tanh, forward and backward: 1 - 2 / (e^2x + 1), the LSTM kernels' formulation (+-1 exactly where e^2x
// overflows or vanishes)
__device__ __forceinline__ float tanh_fast(float x) {
  return __fmaf_rn(-2.0f, __builtin_amdgcn_rcpf(__fadd_rn(__expf(2.0f * x), 1.0f)), 1.0f);
}

// q = p / d, r = p % d (p >= 0, d > 0) in 32-bit arithmetic whenever p fits: a 64-bit division by a run-time value is
// ~150 VALU instructions, and the three per point of the index split were most of the instruction stream of the
// matrix-pipe kernels (counters, profiles/r02/m_: 1 200 VALU instructions per 16-point tile of the encoder).
__device__ __forceinline__ long long divmod(long long p, int d, int& r) {
  if (p < (1ll << 31)) {
    const unsigned pu = (unsigned)p, q = pu / (unsigned)d;
    r = (int)(pu - q * (unsigned)d);
    return (long long)q;
  }
  const long long q = p / d;
  r = (int)(p - q * d);
  return q;
}

typedef float v2f_t __attribute__((ext_vector_type(2)));
typedef float v4f_t __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf_t __attribute__((ext_vector_type(8)));
typedef __bf16 v4bf_t __attribute__((ext_vector_type(4)));

// FNSSL_PRECISION_BF16 (BF = true): the same kernels with both operands of the product rounded to bf16 (round to
// nearest even) as they enter the matrix pipe, fp32 accumulation, fp32 tensors — one v_mfma_f32_16x16x32_bf16 takes the
// place of eight v_mfma_f32_16x16x4_f32.  The lane's K/4 channels stay where they are: MFMA m consumes the lane's
// values 8 m .. 8 m + 7 (zero past K/4), and the weight image holds the matching 8 weights per (lane, m) as one
// 16-byte item, so an output tile costs ceil(K/32) LDS reads and MFMAs instead of K/16 reads and K/4 MFMAs.
__device__ __forceinline__ v8bf_t pack8_bf16(float a0, float a1, float a2, float a3, float a4, float a5, float a6,
                                             float a7) {
  const v4f_t lo = {a0, a1, a2, a3}, hi = {a4, a5, a6, a7};
  const v4bf_t l = __builtin_convertvector(lo, v4bf_t), h = __builtin_convertvector(hi, v4bf_t);
  return __builtin_shufflevector(l, h, 0, 1, 2, 3, 4, 5, 6, 7);
}

// 1-KiB items (64 lanes x 16 bytes) of one 16-output tile in the LDS weight image
template <int K, bool BF>
__host__ __device__ constexpr int w_items() {
  return BF ? (K / 4 + 7) / 8 : K / 16;
}
template <int K, int N, bool BF>
__host__ __device__ constexpr int w_lds_floats() {
  return (N / 16) * w_items<K, BF>() * 256;
}

// sk / so: element strides of the input (k) and output (o) index in the source matrix.  BD = threads of the workgroup
// (compile-time: the trips are fully unrolled, so all of a thread's loads — 4 per 16-byte item, up to 12 items — are in
// flight together.  Rolled, a trip was one L2 round trip and the 147 KB image of in_proj took 21 us per workgroup: half
// of a small launch.)  LDS order, one conflict-free 16-byte write per item; an item's 4 values are 4 consecutive k of one
// output, and the 16 lanes of an output tile read 64 contiguous bytes of each source row (the matrix is L2-resident).
template <int K, int N, int BD, bool BF = false>
__device__ __forceinline__ void fill_w_lds_strided(float* lds, const float* __restrict__ w, int sk, int so, int kvalid,
                                                   int nvalid) {
  static_assert(K % 16 == 0 && N % 16 == 0, "whole k-step groups and output tiles");
  constexpr int KQ = K / 4, G = w_items<K, BF>(), TOTAL = (N / 16) * G * 64, TRIPS = (TOTAL + BD - 1) / BD;
  constexpr int PER = BF ? 8 : 4;                                    // k values of one item
  float v[TRIPS][PER];
#pragma unroll
  for (int u = 0; u < TRIPS; ++u) {
    const int idx = (int)threadIdx.x + u * BD;
    const int lane = idx & 63, g = (idx >> 6) % G, j = (idx >> 6) / G;
    const int kl = PER * g, k0 = (lane >> 4) * KQ + kl, o = 16 * j + (lane & 15);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      // unconditional load from a clamped address, then the choice: a conditional load is a branch and a wait per element
      const bool ok = idx < TOTAL && kl + i < KQ && k0 + i < kvalid && o < nvalid;
      const float x = w[ok ? (long long)(k0 + i) * sk + (long long)o * so : 0];
      v[u][i] = ok ? x : 0.f;
    }
  }
#pragma unroll
  for (int u = 0; u < TRIPS; ++u) {
    const int idx = (int)threadIdx.x + u * BD;
    if (idx < TOTAL) {
      if constexpr (BF)
        *reinterpret_cast<v8bf_t*>(lds + idx * 4) =
            pack8_bf16(v[u][0], v[u][1], v[u][2], v[u][3], v[u][PER - 4], v[u][PER - 3], v[u][PER - 2], v[u][PER - 1]);
      else
        *reinterpret_cast<float4*>(lds + idx * 4) = make_float4(v[u][0], v[u][1], v[u][2], v[u][3]);
    }
  }
}

template <int K, int N, int BD, bool BF = false>
__device__ __forceinline__ void fill_w_lds(float* lds, const float* __restrict__ wT, int ldw, int kvalid, int nvalid) {
  fill_w_lds_strided<K, N, BD, BF>(lds, wT, ldw, 1, kvalid, nvalid);
}

// lane n of a 16-lane row reads lane n - j (row_shr:j = 0x110 + j) or n + j (row_shl:j = 0x100 + j); 0 outside the row
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}

// bf16: the lane's K/4 values as ceil(K/32) packed operands (done once when several calls share them)
template <int K>
__device__ __forceinline__ void pack_operand(const float (&a)[K / 4], v8bf_t (&b)[w_items<K, true>()]) {
  constexpr int KQ = K / 4;
#pragma unroll
  for (int m = 0; m < w_items<K, true>(); ++m) {
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = 8 * m + e < KQ ? a[8 * m + e < KQ ? 8 * m + e : 0] : 0.f;
    b[m] = pack8_bf16(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
  }
}
template <int K, int NJ>
__device__ __forceinline__ void mfma_tiles_packed(const v8bf_t (&b)[w_items<K, true>()], const float* ldsw_lane, int j0,
                                                  v4f_t (&acc)[NJ]) {
  constexpr int G = w_items<K, true>();
#pragma unroll
  for (int m = 0; m < G; ++m)
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      const v8bf_t w = *reinterpret_cast<const v8bf_t*>(ldsw_lane + ((j0 + jj) * G + m) * 256);
      acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, b[m], acc[jj], 0, 0, 0);
    }
}

// acc[jj] += W-tile (j0 + jj) . x   for NJ output tiles at once (independent accumulators keep the pipe busy)
template <int K, int NJ, bool BF = false>
__device__ __forceinline__ void mfma_tiles(const float (&a)[K / 4], const float* ldsw_lane, int j0, v4f_t (&acc)[NJ]) {
  constexpr int G = w_items<K, BF>();
  if constexpr (BF) {
    constexpr int KQ = K / 4;
#pragma unroll
    for (int m = 0; m < G; ++m) {
      float t[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = 8 * m + e < KQ ? a[8 * m + e < KQ ? 8 * m + e : 0] : 0.f;
      const v8bf_t b = pack8_bf16(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) {
        const v8bf_t w = *reinterpret_cast<const v8bf_t*>(ldsw_lane + ((j0 + jj) * G + m) * 256);
        acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, b, acc[jj], 0, 0, 0);
      }
    }
  } else {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      v4f_t w[NJ];
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) w[jj] = *reinterpret_cast<const v4f_t*>(ldsw_lane + ((j0 + jj) * G + g) * 256);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj)
          acc[jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[jj][i], a[4 * g + i], acc[jj], 0, 0, 0);
      // keep the scheduler from hoisting every group's LDS reads to the top (it spills the operand registers)
      if ((g & 1) == 1) __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
inline bool view_ok(const fnssl_btf_view* v) {
  return v && v->p && (reinterpret_cast<size_t>(v->p) % 16 == 0) && v->sb % 4 == 0 && v->st % 4 == 0 && v->sf % 4 == 0;
}
inline bool out_ok(const float* p, long long sb, long long st, long long sf) {
  return p && (reinterpret_cast<size_t>(p) % 16 == 0) && sb % 4 == 0 && st % 4 == 0 && sf % 4 == 0;
}
inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

using fnssl::check_workspace;
using fnssl::enqueue;
using fnssl::Kernel;
using fnssl::with_bool;
using fnssl::with_value;
using fnssl::WsRegion;

// The regions of a workspace, front to back: the one description behind its size, its check and its carve-up.
struct MambaWsLayout {            // fnssl_sn_mamba, npts = nb * nt * nf points
  WsRegion xz, dbl, y;            // [npts, 2E], [npts, XP], [npts, E]
  size_t total;
  explicit MambaWsLayout(long long npts) {
    const size_t pt = (size_t)npts * sizeof(float);
    xz = {0, pt * 2 * E};
    dbl = {xz.end(), pt * XP};
    y = {dbl.end(), pt * E};
    total = y.end();
  }
};

// workgroups of the matrix-pipe kernels: 8 waves x one 16-point tile each per pass, per_cu workgroups per CU (what
// the kernel's LDS weight image allows)
inline unsigned mfma_grid(long long npts, int per_cu, int waves = 8) {
  const long long wgs = ((npts + 15) / 16 + waves - 1) / waves;
  const long long cap = (long long)fnssl::device_cus() * per_cu;
  return (unsigned)(wgs < cap ? wgs : cap);
}

// ---------------------------------------------------------------------------------------------------------
// ordered reduction of per-workgroup (or per-slab, per-sequence) partial sums: the last step of every backward
// ---------------------------------------------------------------------------------------------------------
// One row of partials may feed several gradients: column i of the row belongs to segment k with end[k-1] <= i < end[k].
struct RowSegs {
  int end[4];
  float* out[4];
};

// out[i] = part[0][i] + part[1][i] + ...   (rows `stride` floats apart), in row order
__global__ void __launch_bounds__(256)
sn_reduce_rows_kernel(const float* __restrict__ part, int rows, long long stride, RowSegs segs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= segs.end[3]) return;
  float v = 0.f;
#pragma unroll 16
  for (int r = 0; r < rows; ++r) v += part[r * stride + i];        // the loads of 16 rows in flight, the adds in row order
  const int k = (i >= segs.end[0]) + (i >= segs.end[1]) + (i >= segs.end[2]);
  segs.out[k][i - (k ? segs.end[k - 1] : 0)] = v;
}

// the row's columns go to o0 (n0 of them), then o1 (n1), ...; unused segments: n = 0
inline int reduce_rows(hipStream_t s, const float* part, long long rows, long long stride, int n0, float* o0, int n1 = 0,
                       float* o1 = nullptr, int n2 = 0, float* o2 = nullptr, int n3 = 0, float* o3 = nullptr) {
  const RowSegs segs = {{n0, n0 + n1, n0 + n1 + n2, n0 + n1 + n2 + n3}, {o0, o1, o2, o3}};
  return enqueue(s, Kernel{sn_reduce_rows_kernel, 256, 0, "sn_reduce_rows_kernel"}, blocks_of(segs.end[3]), part, (int)rows, stride,
                 segs);
}

}  // namespace
