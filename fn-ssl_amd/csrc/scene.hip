// Scene finish (fnssl/scene.py; what AcousticScene.simulate() and NoiseDataset.gen_diffuse_noise / mix_signals of the
// reference's Dataset.py do around the three gpuRIR calls).  The model is DESIGN.md §18.
//   fnssl_anf_coherence   spherical coherence matrices of a microphone set, in double
//   fnssl_anf_factor      upper Cholesky factor per bin, in double, stored as float with the bin fastest
//   fnssl_anf_mean        mean of a vector, fixed chunks added in order
//   fnssl_anf_mix         STFT -> triangular per-bin mix -> iSTFT -> overlap-add, one kernel, no spectrum in HBM
//   fnssl_scene_power     acoustic_power of every channel of a sum of signals
//   fnssl_scene_finish    SNR gain on the device, mic = sum of sources + g noise, per-source VAD
//   fnssl_scene_power_batch / fnssl_scene_finish_batch   the last two for a batch of scenes in one launch set
//
// Determinism.  No float atomics.  Mix: a workgroup is ONE wave; it owns a run of output hops and walks the frames that reach
// them in frame order, three frames early from a zero accumulator, so every output hop is ((0 + f0) + f1) + f2) + f3 whatever
// the tiling; a frame's arithmetic does not depend on the tile it is computed in.  Reductions are per-thread strided sums in
// ascending order, the xor butterfly of a wave, and the waves' partial sums added in wave order.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "frontend_core.h"
#include "host.h"

using fnssl::enqueue;
using fnssl::Kernel;
namespace fe = fnssl_frontend;

namespace {

constexpr int kK = FNSSL_ANF_NFFT;                       // 256: one radix-4 transform of frontend_core.h
constexpr int kHop = 64;
constexpr int kBins = FNSSL_ANF_BINS;                    // 129
constexpr int kMaxMics = FNSSL_ANF_MAX_MICS;
constexpr int kMaxTileHops = 16;                         // 19 frames for 16 hops: 19 % of the frames are computed twice
constexpr int kMinTileHops = 2;                          // 5 frames for 2 hops
constexpr int kMixWavesPerCu = 2;                        // the planner's target: a wave's frames are one serial chain, so one
                                                         // utterance (1198 hops) is spread over the device before tiles grow
static_assert(kK == fe::kNF && kBins == kK / 2 + 1, "fft256_radix4 is the transform");

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// coherence and factor (double stays in here: fp32 cannot hold pivots of 1e-7 next to ones)
// ---------------------------------------------------------------------------------------------------------------------------
// grid (m * m, nb), 192 threads: thread k < 129 writes dc[b][p][q][k].  The operations and their order are numpy's in the
// reference (ww = 2 pi fs k / nfft; sinc(ww d / (c pi)) = sin(y) / y with y = pi (ww d / (c pi))), unfused: a factorisation on
// the edge of positive definiteness is decided by the last bits of these entries.
__global__ void __launch_bounds__(192) anf_coherence_kernel(const double* __restrict__ pos, int m, double two_pi_fs, double nfft,
                                                            double c_pi, double* __restrict__ dc) {
#pragma clang fp contract(off)
  const int k = threadIdx.x;
  const int p = blockIdx.x / m, q = blockIdx.x - p * m, b = blockIdx.y;
  if (k >= kBins) return;
  const double* const a = pos + ((size_t)b * m + p) * 3;
  const double* const c = pos + ((size_t)b * m + q) * 3;
  const double dx = a[0] - c[0], dy = a[1] - c[1], dz = a[2] - c[2];
  const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
  const double ww = two_pi_fs * (double)k / nfft;
  const double y = 3.14159265358979323846 * (ww * dist / c_pi);
  dc[(((size_t)b * m + p) * m + q) * kBins + k] = (p == q || y == 0.0) ? 1.0 : sin(y) / y;
}

// grid (128, nb), one wave: bin k = blockIdx.x + 1.  Right-looking factorisation in LDS, a[r][i] for i >= r; step j divides row
// j by the root of its pivot and takes its outer product from the rows below, every entry by its own lane: fixed order,
// and plain IEEE double operations (no fused multiply-add), so that a host restatement in float64 meets the same pivots.
__global__ void __launch_bounds__(64) anf_factor_kernel(const double* __restrict__ dc, int m, float* __restrict__ cfac,
                                                        unsigned* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ double a[kMaxMics][kMaxMics + 1];
  const int lane = threadIdx.x, k = blockIdx.x + 1, b = blockIdx.y;
  const double* const src = dc + (size_t)b * m * m * kBins;
  float* const dst = cfac + (size_t)b * kMaxMics * kMaxMics * kBins;   // rows of kMaxMics entries whatever m
  for (int e = lane; e < m * m; e += 64) {
    const int r = e / m, i = e - r * m;
    a[r][i] = src[(size_t)e * kBins + k];
    if (k == 1) dst[(size_t)(r * kMaxMics + i) * kBins] = 0.f;         // the unused slot of bin 0
  }
  __syncthreads();
  bool ok = true;
  for (int j = 0; j < m; ++j) {
    const double piv = a[j][j];                          // (uniform)
    if (!(piv > 0.0) || !(piv <= 1.7976931348623157e308)) {
      ok = false;
      break;
    }
    const double d = sqrt(piv);
    __syncthreads();
    if (lane >= j && lane < m) a[j][lane] = a[j][lane] / d;
    __syncthreads();
    for (int e = lane; e < m * m; e += 64) {
      const int r = e / m, i = e - r * m;
      if (r > j && i >= r) a[r][i] -= a[j][r] * a[j][i];
    }
    __syncthreads();
  }
  if (!ok) {
    if (lane == 0) atomicMin(status + b, (unsigned)k);
    return;
  }
  for (int e = lane; e < m * m; e += 64) {
    const int r = e / m, i = e - r * m;
    dst[(size_t)(r * kMaxMics + i) * kBins + k] = i >= r ? (float)a[r][i] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// mean
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kMeanChunk = FNSSL_ANF_MEAN_CHUNK;

// grid (nchunks, nb), 256 threads: partial[b][chunk] = sum of the chunk
__global__ void __launch_bounds__(256) anf_mean_partial_kernel(const float* __restrict__ x, long long count, long long item_stride,
                                                               float* __restrict__ partial) {
  __shared__ float part[4];
  const int tid = threadIdx.x;
  const long long lo = (long long)blockIdx.x * kMeanChunk;
  const long long hi = lo + kMeanChunk < count ? lo + kMeanChunk : count;
  const float* const src = x + (long long)blockIdx.y * item_stride;
  float v = 0.f;
  for (long long i = lo + tid; i < hi; i += 256) v += src[i];
  v = wave_sum(v);
  if ((tid & 63) == 0) part[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// grid nb, one wave
__global__ void __launch_bounds__(64) anf_mean_final_kernel(const float* __restrict__ partial, int nchunks, long long count,
                                                            float* __restrict__ mean) {
  float v = 0.f;
  for (int i = threadIdx.x; i < nchunks; i += 64) v += partial[(size_t)blockIdx.x * nchunks + i];
  v = wave_sum(v);
  if (threadIdx.x == 0) mean[blockIdx.x] = v / (float)count;
}

// ---------------------------------------------------------------------------------------------------------------------------
// mix
// ---------------------------------------------------------------------------------------------------------------------------
struct MixParams {
  const float* x;
  const float* mean;                                     // [nb] or null
  const float* cfac;                                     // [items][16][16][129]
  float* y;                                              // [nb][lout][m]
  long long stride_b, stride_n, stride_m, cfac_stride;   // floats; cfac_stride 0: one factor for every item
  int len, lout, m, tile_hops;
};

// MP = channel pairs (m <= 2 MP): channels 2c and 2c + 1 ride transform c as its real and imaginary parts.
// LDS: tables 5 KB, z 2 KB per pair, accumulator ring 2 KB per pair (37 KB at 16 channels).
// Frame f covers padded samples [64 f, 64 f + 256) = noise samples [64 f - 256, 64 f); the ring slot of padded sample s is
// s mod 256, so frame f adds into slots (64 (f mod 4) + n) mod 256 and completes the hop in slots [64 (f mod 4), + 64), which is
// output hop f - 4.  The tile of output hops [h0, h1) walks f = h0 + 1 .. h1 + 3 and drops the hops completed before f = h0 + 4.
template <int MP>
__global__ void __launch_bounds__(64) anf_mix_kernel(const MixParams p) {
#pragma clang fp contract(off)
  __shared__ float2 tw[fe::kTwiddles];
  __shared__ float hann[fe::kWin];                       // Hann-512: the periodic Hann-256 is its even samples
  __shared__ float2 z[MP][kK];
  __shared__ float acc[2 * MP][kK];
  constexpr int CH = 2 * MP;
  const int lane = threadIdx.x, b = blockIdx.y;
  const int nh = p.lout / kHop;
  const int h0 = blockIdx.x * p.tile_hops;
  const int h1 = min(h0 + p.tile_hops, nh);
  const int M = p.m;
  const float mean = p.mean ? p.mean[b] : 0.f;
  const float* const xb = p.x + (long long)b * p.stride_b;
  const float* const cf = p.cfac + (long long)b * p.cfac_stride;
  float* const yb = p.y + (size_t)b * p.lout * M;

  fe::fill_tables(tw, hann, lane, 64);
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[c][lane + 64 * r] = 0.f;
  fe::wave_lds_sync();

  for (int f = h0 + 1; f <= h1 + 3; ++f) {
    // window and pack, digit-reversed for the transform; the padding stays zero (the mean leaves real samples only)
    const int n0 = kHop * f - kK;
    for (int i = 0; i < kK * CH / 64; ++i) {
      const int idx = lane + 64 * i;
      const int t = idx / CH, c = idx % CH;
      const int n = n0 + t;
      float v = 0.f;
      if (c < M && n >= 0 && n < p.len) v = xb[(long long)n * p.stride_n + (long long)c * p.stride_m] - mean;
      reinterpret_cast<float*>(&z[c >> 1][fe::digitrev4_8((unsigned)t)])[c & 1] = hann[2 * t] * v;
    }
    fe::wave_lds_sync();
#pragma unroll
    for (int c = 0; c < MP; ++c) fe::fft256_radix4(z[c], tw, lane);

    // lanes on bins, k = lane + 1 then lane + 65: split by conjugate symmetry, mix, and store X in place.  Channel 2 c keeps
    // slot k of its pair, channel 2 c + 1 slot 256 - k (for k = 128 the free slot of bin 0): a lane reads and writes only the
    // slots of its own bins.
#pragma unroll 1
    for (int r = 0; r < 2; ++r) {
      const int k = lane + 1 + 64 * r;
      const int kb = k == kK / 2 ? 0 : kK - k;
      // N_2c = (Z[k] + conj Z[-k]) / 2, N_2c+1 = (Z[k] - conj Z[-k]) / (2 i)
      float2 n[CH];
#pragma unroll
      for (int c = 0; c < MP; ++c) {
        const float2 zk = z[c][k], zn = z[c][kK - k];
        n[2 * c] = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
        n[2 * c + 1] = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
      }
      // X_p = sum_{q <= p} C[q][p] N_q in place, p descending, q ascending.  The channel count is compared afresh in every
      // round: hoisted out of the frame loop, the 16 conditions are 32 scalar registers and the allocator spills one.
      const float* const ck = cf + k;
      int mm = M;
      asm volatile("" : "+s"(mm));
#pragma unroll
      for (int pp = CH - 1; pp >= 0; --pp) {
        float2 s = make_float2(0.f, 0.f);
        if (pp < mm) {                                   // (uniform)
          const float* const col = ck + pp * kBins;      // rows of kMaxMics entries whatever m: constant offsets
          const float c0 = col[0];
          s = make_float2(c0 * n[0].x, c0 * n[0].y);
#pragma unroll
          for (int q = 1; q <= pp; ++q) {
            const float cq = col[q * kMaxMics * kBins];
            s.x = fmaf(cq, n[q].x, s.x);
            s.y = fmaf(cq, n[q].y, s.y);
          }
        }
        n[pp] = s;
      }
#pragma unroll
      for (int c = 0; c < MP; ++c) {
        z[c][k] = n[2 * c];
        z[c][kb] = n[2 * c + 1];
      }
    }
    fe::wave_lds_sync();
    // W[k] = X_a[k] + i X_b[k], W[-k] = conj X_a[k] + i conj X_b[k], digit-reversed for the transform: those are other lanes'
    // slots, so a pair is read whole before it is written (bin 128 writes one value twice; bin 0 stays zero)
#pragma unroll
    for (int c = 0; c < MP; ++c) {
      float2 xa[2], xc[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int k = lane + 1 + 64 * r;
        xa[r] = z[c][k];
        xc[r] = z[c][k == kK / 2 ? 0 : kK - k];
      }
      fe::wave_lds_sync();
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int k = lane + 1 + 64 * r;
        z[c][fe::digitrev4_8((unsigned)k)] = make_float2(xa[r].x - xc[r].y, xa[r].y + xc[r].x);
        z[c][fe::digitrev4_8((unsigned)(kK - k))] = make_float2(xa[r].x + xc[r].y, xc[r].x - xa[r].y);
      }
      if (lane == 0) z[c][0] = make_float2(0.f, 0.f);
    }
    fe::wave_lds_sync();
#pragma unroll
    for (int c = 0; c < MP; ++c) fe::fft256_radix4(z[c], tw, lane);

    // o[n] = F[-n] / 256 (the inverse through the forward transform), windowed and added
    const int ring = (f & 3) * kHop;
#pragma unroll
    for (int c = 0; c < MP; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n_ = lane + 64 * r;
        const float2 v = z[c][(kK - n_) & (kK - 1)];
        const float w = hann[2 * n_];
        const int slot = (ring + n_) & (kK - 1);
        acc[2 * c][slot] = acc[2 * c][slot] + w * (v.x * (1.f / kK));
        acc[2 * c + 1][slot] = acc[2 * c + 1][slot] + w * (v.y * (1.f / kK));
      }
    fe::wave_lds_sync();
    if (f >= h0 + 4) {                                   // (uniform) the hop has its four frames
      float* const dst = yb + (size_t)(f - 4) * kHop * M;
      for (int idx = lane; idx < kHop * M; idx += 64) {
        const int t = idx / M, c = idx - t * M;
        dst[idx] = acc[c][ring + t] / 1.5f;
      }
      fe::wave_lds_sync();
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c][ring + lane] = 0.f;
    fe::wave_lds_sync();
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// acoustic_power
// ---------------------------------------------------------------------------------------------------------------------------
struct SumPtrs {
  const float* a[FNSSL_SCENE_MAX_SOURCES];
};

// grid (n / 256), 256 threads: blocks[c][j] = sum over the 256 samples of block j of (sum_s a_s[t][c])^2
__device__ __forceinline__ void block_sums_body(const SumPtrs& P, int nsum, int m, int nblk, float* __restrict__ blocks, const int j) {
#pragma clang fp contract(off)
  __shared__ float part[4];
  const int tid = threadIdx.x;
  const size_t row = ((size_t)j * 256 + tid) * m;
  for (int c = 0; c < m; ++c) {
    float v = P.a[0][row + c];
    for (int s = 1; s < nsum; ++s) v += P.a[s][row + c];
    v = wave_sum(v * v);
    __syncthreads();
    if ((tid & 63) == 0) part[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) blocks[(size_t)c * nblk + j] = ((part[0] + part[1]) + part[2]) + part[3];
  }
}

__global__ void __launch_bounds__(256) scene_block_sums_kernel(const SumPtrs P, int nsum, int m, int nblk, float* __restrict__ blocks) {
  block_sums_body(P, nsum, m, nblk, blocks, blockIdx.x);
}

// A batch (fnssl_scene_power_batch): the records travel by value in the kernel arguments, blockIdx.y is the record.  A scene
// is two records, its direct-path signals over n rows and its noise over its own length.
constexpr int kBatchScenes = FNSSL_SCENE_BATCH_SCENES;

struct PowerJob {
  SumPtrs a;
  float* blocks;                                         // [m][nblk] of this record
  float* power;                                          // [m]
  int nsum, nblk;
};
struct PowerBatchParams {
  PowerJob job[2 * kBatchScenes];
};
static_assert(sizeof(PowerBatchParams) <= 4096, "the block's descriptors travel in the kernel arguments");

__global__ void __launch_bounds__(256) scene_block_sums_batch_kernel(const PowerBatchParams P, int m) {
  const PowerJob& j = P.job[blockIdx.y];
  if ((int)blockIdx.x >= j.nblk) return;                 // (uniform) the grid is sized for the longest record
  block_sums_body(j.a, j.nsum, m, j.nblk, j.blocks, blockIdx.x);
}

// grid m, 256 threads: window j = blocks j and j + 1
__device__ __forceinline__ void power_body(const float* __restrict__ blocks, int nblk, int nwin, float* __restrict__ power, const int c) {
#pragma clang fp contract(off)
  __shared__ float part[4], cnt[4];
  const int tid = threadIdx.x;
  const float* const bs = blocks + (size_t)c * nblk;
  float mx = 0.f;
  for (int j = tid; j < nwin; j += 256) mx = fmaxf(mx, (bs[j] + bs[j + 1]) * (1.f / 512.f));
  mx = wave_max(mx);
  if ((tid & 63) == 0) part[tid >> 6] = mx;
  __syncthreads();
  const float th = 0.01f * fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
  __syncthreads();
  float sum = 0.f, num = 0.f;
  for (int j = tid; j < nwin; j += 256) {
    const float w = (bs[j] + bs[j + 1]) * (1.f / 512.f);
    if (w > th) {
      sum += w;
      num += 1.f;
    }
  }
  sum = wave_sum(sum);
  num = wave_sum(num);
  if ((tid & 63) == 0) part[tid >> 6] = sum, cnt[tid >> 6] = num;
  __syncthreads();
  if (tid == 0) power[c] = (((part[0] + part[1]) + part[2]) + part[3]) / (((cnt[0] + cnt[1]) + cnt[2]) + cnt[3]);
}

__global__ void __launch_bounds__(256) scene_power_kernel(const float* __restrict__ blocks, int nblk, int nwin, float* __restrict__ power) {
  power_body(blocks, nblk, nwin, power, blockIdx.x);
}

__global__ void __launch_bounds__(256) scene_power_batch_kernel(const PowerBatchParams P) {
  const PowerJob& j = P.job[blockIdx.y];
  power_body(j.blocks, j.nblk, j.nblk - 1, j.power, blockIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------------------
// finish
// ---------------------------------------------------------------------------------------------------------------------------
// grid ns, 1024 threads: vmax[s] = max of vad_in[s][0 .. n)[0 .. m)
__device__ __forceinline__ void vmax_body(const SumPtrs& V, long long count, float* __restrict__ vmax, const int s) {
  __shared__ float part[16];
  const int tid = threadIdx.x;
  const float* const v = V.a[s];
  float mx = -INFINITY;
  for (long long i = tid; i < count; i += 1024) mx = fmaxf(mx, v[i]);
  mx = wave_max(mx);
  if ((tid & 63) == 0) part[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    float r = part[0];
    for (int w = 1; w < 16; ++w) r = fmaxf(r, part[w]);
    vmax[s] = r;
  }
}

__global__ void __launch_bounds__(1024) scene_vmax_kernel(const SumPtrs V, long long count, float* __restrict__ vmax) {
  vmax_body(V, count, vmax, blockIdx.x);
}

struct FinishParams {
  SumPtrs sig, vad_in;
  const float* noise;
  const float* p;
  const float* pn;
  const float* vmax;
  float* mic;
  float* g;
  unsigned char* vad_sources;
  unsigned char* vad;
  float snr_lin;
  int ns, n, m, with_vad;
};

// one thread per sample t: its m channels, then its VADs
__device__ __forceinline__ void finish_body(const FinishParams& P, const int t) {
#pragma clang fp contract(off)
  float sp = P.p[0], sn = P.pn[0];
  for (int c = 1; c < P.m; ++c) sp += P.p[c], sn += P.pn[c];
  const float g = sqrtf((sp / (float)P.m) / P.snr_lin) / sqrtf(sn / (float)P.m);
  if (t == 0) *P.g = g;
  if (t >= P.n) return;
  const size_t row = (size_t)t * P.m;
  for (int c = 0; c < P.m; ++c) {
    float v = P.sig.a[0][row + c];
    for (int s = 1; s < P.ns; ++s) v += P.sig.a[s][row + c];
    P.mic[row + c] = fmaf(g, P.noise[row + c], v);
  }
  if (P.with_vad) {
    unsigned char any = 0;
    for (int s = 0; s < P.ns; ++s) {
      float v = P.vad_in.a[s][row];
      for (int c = 1; c < P.m; ++c) v += P.vad_in.a[s][row + c];
      const unsigned char on = (v / (float)P.m) > 1e-3f * P.vmax[s] ? 1 : 0;
      P.vad_sources[(size_t)t * P.ns + s] = on;
      any |= on;
    }
    P.vad[t] = any;
  }
}

__global__ void __launch_bounds__(256) scene_finish_kernel(const FinishParams P) { finish_body(P, blockIdx.x * 256 + threadIdx.x); }

// A batch (fnssl_scene_finish_batch): one record per scene, blockIdx.y is the scene.
struct FinishBatchParams {
  FinishParams job[kBatchScenes];
};
static_assert(sizeof(FinishBatchParams) <= 4096, "the block's descriptors travel in the kernel arguments");

// grid (FNSSL_SCENE_MAX_SOURCES, scenes)
__global__ void __launch_bounds__(1024) scene_vmax_batch_kernel(const FinishBatchParams P) {
  const FinishParams& j = P.job[blockIdx.y];
  if (!j.with_vad || (int)blockIdx.x >= j.ns) return;    // (uniform)
  vmax_body(j.vad_in, (long long)j.n * j.m, const_cast<float*>(j.vmax), blockIdx.x);
}

__global__ void __launch_bounds__(256) scene_finish_batch_kernel(const FinishBatchParams P) {
  finish_body(P.job[blockIdx.y], blockIdx.x * 256 + threadIdx.x);
}

int check_anf(const char* who, int nb, int m, int nfft) {
  FNSSL_REQUIRE(nfft == FNSSL_ANF_NFFT, "%s: nfft = %d (only %d is built)", who, nfft, FNSSL_ANF_NFFT);
  FNSSL_REQUIRE(m >= 1 && m <= kMaxMics, "%s: %d microphones (1 .. %d)", who, m, kMaxMics);
  FNSSL_REQUIRE(nb >= 1 && nb <= 65535, "%s: %d items (1 .. 65535)", who, nb);
  return FNSSL_OK;
}

// The checks of fnssl_scene_power and its record; `who` names the call, and for a batch the scene.
int prepare_power(const char* who, const float* const* a, int nsum, int n, int m, float* blocks, size_t blocks_floats, float* power,
                  PowerJob* out) {
  FNSSL_REQUIRE(a && blocks && power, "%s: null pointer", who);
  FNSSL_REQUIRE(nsum >= 1 && nsum <= FNSSL_SCENE_MAX_SOURCES, "%s: %d summands (1 .. %d)", who, nsum, FNSSL_SCENE_MAX_SOURCES);
  FNSSL_REQUIRE(n >= 512, "%s: %d samples (acoustic_power needs one window of 512)", who, n);
  FNSSL_REQUIRE(n < (1 << 30) && m >= 1 && m <= 65535, "%s: %d samples, %d channels", who, n, m);
  const int nblk = n / 256;                              // windows: ceil((n - 511) / 256) = floor(n / 256) - 1 for n >= 512
  FNSSL_REQUIRE(blocks_floats >= (size_t)m * nblk, "%s: %zu floats of scratch, %zu needed", who, blocks_floats, (size_t)m * nblk);
  PowerJob j{};
  for (int s = 0; s < nsum; ++s) {
    FNSSL_REQUIRE(a[s], "%s: summand %d is null", who, s);
    j.a.a[s] = a[s];
  }
  j.blocks = blocks;
  j.power = power;
  j.nsum = nsum;
  j.nblk = nblk;
  *out = j;
  return FNSSL_OK;
}

// The checks of fnssl_scene_finish and its record.
int prepare_finish(const char* who, const float* const* sig, int ns, const float* noise, const float* const* vad_in, int n, int m,
                   const float* p, const float* pn, double snr_lin, float* mic, float* g, float* vmax, unsigned char* vad_sources,
                   unsigned char* vad, FinishParams* out) {
  FNSSL_REQUIRE(sig && noise && p && pn && mic && g, "%s: null pointer", who);
  FNSSL_REQUIRE(ns >= 1 && ns <= FNSSL_SCENE_MAX_SOURCES, "%s: %d sources (1 .. %d)", who, ns, FNSSL_SCENE_MAX_SOURCES);
  FNSSL_REQUIRE(n >= 1 && n < (1 << 30) && m >= 1 && m <= 65535, "%s: %d samples, %d channels", who, n, m);
  FNSSL_REQUIRE(snr_lin > 0.0 && std::isfinite(snr_lin), "%s: SNR ratio %g", who, snr_lin);
  FNSSL_REQUIRE(!vad_in || (vmax && vad_sources && vad), "%s: VAD inputs without VAD outputs", who);
  FinishParams P{};
  for (int s = 0; s < ns; ++s) {
    FNSSL_REQUIRE(sig[s] && (!vad_in || vad_in[s]), "%s: source %d is null", who, s);
    P.sig.a[s] = sig[s];
    if (vad_in) P.vad_in.a[s] = vad_in[s];
  }
  P.noise = noise;
  P.p = p;
  P.pn = pn;
  P.vmax = vmax;
  P.mic = mic;
  P.g = g;
  P.vad_sources = vad_sources;
  P.vad = vad;
  P.snr_lin = (float)snr_lin;
  P.ns = ns;
  P.n = n;
  P.m = m;
  P.with_vad = vad_in ? 1 : 0;
  *out = P;
  return FNSSL_OK;
}

}  // namespace

extern "C" {

int fnssl_anf_coherence(const double* mic_pos, int nb, int m, double fs, int nfft, double c, double* dc, void* stream) {
  FNSSL_TRY(check_anf("anf_coherence", nb, m, nfft));
  FNSSL_REQUIRE(mic_pos && dc, "anf_coherence: null pointer");
  FNSSL_REQUIRE(fs > 0.0 && c > 0.0, "anf_coherence: fs = %g, c = %g", fs, c);
  hipStream_t s = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl("anf_coherence", s);
  return enqueue(s, Kernel{anf_coherence_kernel, 192, 0, "anf_coherence_kernel"}, dim3((unsigned)(m * m), (unsigned)nb), mic_pos, m,
                 2.0 * 3.14159265358979323846 * fs, (double)nfft, c * 3.14159265358979323846, dc);
}

int fnssl_anf_factor(const double* dc, int nb, int m, int nfft, float* cfac, unsigned* status, void* stream) {
  FNSSL_TRY(check_anf("anf_factor", nb, m, nfft));
  FNSSL_REQUIRE(dc && cfac && status, "anf_factor: null pointer");
  hipStream_t s = fnssl::as_stream(stream);
  FNSSL_HIP(hipMemsetAsync(status, 0xff, (size_t)nb * sizeof(unsigned), s));
  fnssl::TimedLaunch tl("anf_factor", s);
  return enqueue(s, Kernel{anf_factor_kernel, 64, 0, "anf_factor_kernel"}, dim3((unsigned)(kBins - 1), (unsigned)nb), dc, m, cfac, status);
}

int fnssl_anf_status(const unsigned* status, int nb, void* stream, unsigned* host_words) {
  FNSSL_REQUIRE(status && host_words && nb >= 1, "anf_status: null pointer / no item");
  hipStream_t s = fnssl::as_stream(stream);
  FNSSL_HIP(hipMemcpyAsync(host_words, status, (size_t)nb * sizeof(unsigned), hipMemcpyDeviceToHost, s));
  FNSSL_HIP(hipStreamSynchronize(s));
  return FNSSL_OK;
}

int fnssl_anf_mean(const float* x, int nb, long long count, long long item_stride, float* partial, size_t partial_floats,
                   float* mean, void* stream) {
  FNSSL_REQUIRE(x && partial && mean, "anf_mean: null pointer");
  FNSSL_REQUIRE(nb >= 1 && nb <= 65535 && count >= 1 && count < (1ll << 40) && item_stride >= 0,
                "anf_mean: %d items of %lld floats", nb, count);
  const long long nchunks = (count + kMeanChunk - 1) / kMeanChunk;
  FNSSL_REQUIRE(partial_floats >= (size_t)nb * (size_t)nchunks, "anf_mean: %zu floats of scratch, %lld needed", partial_floats,
                (long long)nb * nchunks);
  hipStream_t s = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl("anf_mean", s);
  FNSSL_TRY(enqueue(s, Kernel{anf_mean_partial_kernel, 256, 0, "anf_mean_partial_kernel"}, dim3((unsigned)nchunks, (unsigned)nb), x,
                    count, item_stride, partial));
  return enqueue(s, Kernel{anf_mean_final_kernel, 64, 0, "anf_mean_final_kernel"}, dim3((unsigned)nb), static_cast<const float*>(partial),
                 (int)nchunks, count, mean);
}

int fnssl_anf_mix(const float* x, long long stride_b, long long stride_n, long long stride_m, const float* mean,
                  const float* cfac, int cfac_items, int nb, int len, int m, int nfft, int tile_hops, float* y, void* stream) {
  FNSSL_TRY(check_anf("anf_mix", nb, m, nfft));
  FNSSL_REQUIRE(x && cfac && y, "anf_mix: null pointer");
  FNSSL_REQUIRE(len >= 1 && len < (1 << 30), "anf_mix: %d samples (1 .. 2^30)", len);
  FNSSL_REQUIRE(cfac_items == 1 || cfac_items == nb, "anf_mix: %d factors for %d items (1 or one each)", cfac_items, nb);
  FNSSL_REQUIRE(tile_hops >= 0 && stride_b >= 0 && stride_n >= 0 && stride_m >= 0, "anf_mix: negative tile / stride");
  MixParams p{};
  p.x = x;
  p.mean = mean;
  p.cfac = cfac;
  p.y = y;
  p.stride_b = stride_b;
  p.stride_n = stride_n;
  p.stride_m = stride_m;
  p.cfac_stride = cfac_items == 1 ? 0 : (long long)kMaxMics * kMaxMics * kBins;
  p.len = len;
  p.lout = len + (kHop - len % kHop) % kHop;
  p.m = m;
  const int nh = p.lout / kHop;
  if (tile_hops > 0) {
    p.tile_hops = tile_hops;
  } else {                                               // (the bits do not depend on it)
    const long long waves = (long long)fnssl::device_cus() * kMixWavesPerCu;
    const long long t = ((long long)nh * nb + waves - 1) / waves;
    p.tile_hops = (int)std::min<long long>(kMaxTileHops, std::max<long long>(kMinTileHops, t));
  }
  const dim3 grid((unsigned)((nh + p.tile_hops - 1) / p.tile_hops), (unsigned)nb);
  const int mp = m <= 2 ? 1 : m <= 4 ? 2 : m <= 8 ? 4 : 8;
  hipStream_t s = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl("anf_mix", s);
  return fnssl::with_value<1, 2, 4, 8>(mp, [&](auto MP) {
    return enqueue(s, Kernel{anf_mix_kernel<MP>, 64, 0, "anf_mix_kernel"}, grid, p);
  });
}

int fnssl_scene_power(const float* const* a, int nsum, int n, int m, float* blocks, size_t blocks_floats, float* power,
                      void* stream) {
  PowerJob j{};
  FNSSL_TRY(prepare_power("scene_power", a, nsum, n, m, blocks, blocks_floats, power, &j));
  hipStream_t s = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl("scene_power", s);
  FNSSL_TRY(enqueue(s, Kernel{scene_block_sums_kernel, 256, 0, "scene_block_sums_kernel"}, dim3((unsigned)j.nblk), j.a, nsum, m, j.nblk, blocks));
  return enqueue(s, Kernel{scene_power_kernel, 256, 0, "scene_power_kernel"}, dim3((unsigned)m), static_cast<const float*>(blocks), j.nblk,
                 j.nblk - 1, power);
}

int fnssl_scene_finish(const float* const* sig, int ns, const float* noise, const float* const* vad_in, int n, int m,
                       const float* p, const float* pn, double snr_lin, float* mic, float* g, float* vmax,
                       unsigned char* vad_sources, unsigned char* vad, void* stream) {
  FinishParams P{};
  FNSSL_TRY(prepare_finish("scene_finish", sig, ns, noise, vad_in, n, m, p, pn, snr_lin, mic, g, vmax, vad_sources, vad, &P));
  hipStream_t s = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl("scene_finish", s);
  if (vad_in)
    FNSSL_TRY(enqueue(s, Kernel{scene_vmax_kernel, 1024, 0, "scene_vmax_kernel"}, dim3((unsigned)ns), P.vad_in, (long long)n * m, vmax));
  return enqueue(s, Kernel{scene_finish_kernel, 256, 0, "scene_finish_kernel"}, dim3((unsigned)((n + 255) / 256)), P);
}

// ---- a batch of scenes: every scene is checked first, then ceil(nscenes / FNSSL_SCENE_BATCH_SCENES) launch sets ------------
int fnssl_scene_power_batch(const fnssl_scene_desc* scenes, int nscenes, int n, int m, void* stream) {
  FNSSL_REQUIRE(scenes && nscenes >= 1, "scene_power_batch: null pointer / no scene");
  std::vector<PowerJob> jobs((size_t)2 * nscenes);
  for (int b = 0; b < nscenes; ++b) {
    const fnssl_scene_desc& d = scenes[b];
    char who[56];
    std::snprintf(who, sizeof who, "scene_power_batch: scene %d", b);
    FNSSL_TRY(prepare_power(who, d.dp, d.ns, n, m, d.blocks, d.blocks_floats, d.power, &jobs[2 * b]));
    std::snprintf(who, sizeof who, "scene_power_batch: scene %d (noise)", b);
    const float* const one[1] = {d.noise};
    FNSSL_REQUIRE(d.noise_len >= n, "%s: %d samples of noise for %d", who, d.noise_len, n);
    FNSSL_TRY(prepare_power(who, one, 1, d.noise_len, m, d.blocks_noise, d.blocks_noise_floats, d.power_noise, &jobs[2 * b + 1]));
  }
  hipStream_t s = fnssl::as_stream(stream);
  for (int k0 = 0; k0 < 2 * nscenes; k0 += 2 * kBatchScenes) {
    const int nb = std::min(2 * kBatchScenes, 2 * nscenes - k0);
    PowerBatchParams P{};
    int nblk = 0;
    for (int k = 0; k < nb; ++k) P.job[k] = jobs[k0 + k], nblk = std::max(nblk, P.job[k].nblk);
    fnssl::TimedLaunch tl("scene_power_batch", s);
    FNSSL_TRY(enqueue(s, Kernel{scene_block_sums_batch_kernel, 256, 0, "scene_block_sums_batch_kernel"}, dim3((unsigned)nblk, (unsigned)nb), P, m));
    FNSSL_TRY(enqueue(s, Kernel{scene_power_batch_kernel, 256, 0, "scene_power_batch_kernel"}, dim3((unsigned)m, (unsigned)nb), P));
  }
  return FNSSL_OK;
}

int fnssl_scene_finish_batch(const fnssl_scene_desc* scenes, int nscenes, int n, int m, void* stream) {
  FNSSL_REQUIRE(scenes && nscenes >= 1, "scene_finish_batch: null pointer / no scene");
  std::vector<FinishParams> jobs((size_t)nscenes);
  bool any_vad = false;
  for (int b = 0; b < nscenes; ++b) {
    const fnssl_scene_desc& d = scenes[b];
    char who[56];
    std::snprintf(who, sizeof who, "scene_finish_batch: scene %d", b);
    FNSSL_REQUIRE(d.noise_len >= n, "%s: %d samples of noise for %d", who, d.noise_len, n);
    FNSSL_TRY(prepare_finish(who, d.sig, d.ns, d.noise, d.with_vad ? d.vad_in : nullptr, n, m, d.power, d.power_noise, d.snr_lin, d.mic,
                             d.g, d.vmax, d.vad_sources, d.vad, &jobs[b]));
    any_vad = any_vad || d.with_vad;
  }
  hipStream_t s = fnssl::as_stream(stream);
  for (int b0 = 0; b0 < nscenes; b0 += kBatchScenes) {
    const int nb = std::min(kBatchScenes, nscenes - b0);
    FinishBatchParams P{};
    for (int b = 0; b < nb; ++b) P.job[b] = jobs[b0 + b];
    fnssl::TimedLaunch tl("scene_finish_batch", s);
    if (any_vad)
      FNSSL_TRY(enqueue(s, Kernel{scene_vmax_batch_kernel, 1024, 0, "scene_vmax_batch_kernel"}, dim3(FNSSL_SCENE_MAX_SOURCES, (unsigned)nb), P));
    FNSSL_TRY(enqueue(s, Kernel{scene_finish_batch_kernel, 256, 0, "scene_finish_batch_kernel"}, dim3((unsigned)((n + 255) / 256), (unsigned)nb), P));
  }
  return FNSSL_OK;
}

}  // extern "C"
