// Room simulation (fnssl/rir.py, the stage gpuRIR has in the reference's Simu.py / Dataset.py):
//   fnssl_rir_ism         image-source part of every (source, receiver) RIR, samples [0, nISM)
//   fnssl_rir_tail        diffuse tail, samples [nISM, nSamples): decay fitted to the ISM part, logistic noise from Philox4x32-10
//   fnssl_rir_trajectory  moving-source mixing: y[t, m] = sum_k RIRs[p(t - k), m, k] x[t - k], a batch of them per launch
//   fnssl_rir_ism_batch / fnssl_rir_tail_batch   the first two for a batch of jobs (one job = one call of each) in one launch
//                         set: the records travel in the kernel arguments, the kernels share the single forms' bodies
// Semantics are the published algorithm (Allen & Berkley 1979; Diaz-Guerra, Miguel, Beltran 2021) written from the formulas
// of DESIGN.md §17; nothing here is bit compatible with gpuRIR and nothing claims to be.
//
// Determinism.  No float atomics anywhere.  ISM: a workgroup is ONE wave that owns a private LDS tile of its RIR; it walks
// its images in index order and the lanes of one image own distinct taps, so every tile sample sees its additions in image
// order.  Several workgroups of one RIR write partial tiles to the workspace, which rir_sum_kernel adds in chunk order.
// Tail: every workgroup of a RIR repeats the same fit in the same order; the noise is a pure function of (seed, src, rcv, t).
// Trajectory: each output is one thread's running sum over ascending source samples.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host.h"

using fnssl::enqueue;
using fnssl::Kernel;

namespace {

constexpr float kPi = 3.14159265358979323846f;

// ---------------------------------------------------------------------------------------------------------------------------
// image-source part
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kIsmThreads = 64;                          // one wave: the tile is private to it, LDS operations of a wave stay in order
constexpr int kIsmMaxSamples = FNSSL_RIR_MAX_ISM_SAMPLES;
constexpr int kIsmMaxAxis = FNSSL_RIR_MAX_IMAGES_AXIS;
constexpr int kIsmWinRounds = 8;                         // a window of <= 8 x 64 taps: Tw + 1 <= 512, fs <= 63.8 kHz
constexpr int kIsmMinChunk = 256;                        // images: below this the tile's zeroing and store outweigh the windows
constexpr int kIsmWavesPerCu = 8;                        // the planner's target (19 KB of LDS per wave at the reference's sizes)

struct IsmParams {
  const float* pos_src;                                  // [m_src][3]
  const float* pos_rcv;                                  // [m_rcv][3]
  float* out;                                            // the RIRs (one chunk) or the workspace [chunk][rir][nism]
  long long rir_stride, chunk_stride;                    // floats
  float room[3];
  float beta[6];
  int n[3];
  int m_rcv, nism, chunk, total;
  float fs_over_c, tw;                                   // tw: the window in samples
};

__device__ __forceinline__ float lane_f(float v, int j) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}

// LDS: tile [nism] | squared coordinate difference per axis image [nx + ny + nz] | reflection amplitude per axis image
// [nx + ny + nz].  Every index below is bounded by the host's checks: t in [0, nism), axis indices < n[a].
// The body of both forms: `p` is the launch's one record (rir_ism_kernel) or the job's record of a descriptor block
// (rir_ism_batch_kernel); a workgroup is chunk `chunk` of RIR `rir` of that record.
__device__ __forceinline__ void ism_body(const IsmParams& p, const int chunk, const int rir) {
  extern __shared__ float lds[];
  const int nx = p.n[0], ny = p.n[1], nz = p.n[2];
  float* const tile = lds;
  float* const sq = tile + p.nism;
  float* const am = sq + (nx + ny + nz);
  const int lane = threadIdx.x;
  const int src = rir / p.m_rcv, rcv = rir - src * p.m_rcv;

  for (int i = lane; i < p.nism; i += kIsmThreads) tile[i] = 0.f;
  int off = 0;
  for (int a = 0; a < 3; ++a) {
    const float len = p.room[a], ps = p.pos_src[3 * src + a], pr = p.pos_rcv[3 * rcv + a];
    const float b0 = p.beta[2 * a], b1 = p.beta[2 * a + 1];
    for (int i = lane; i < p.n[a]; i += kIsmThreads) {
      const int n = i - p.n[a] / 2;
      const float x = (n & 1) ? (float)(n + 1) * len - ps : (float)n * len + ps;
      const float d = x - pr;
      sq[off + i] = d * d;
      // |n| reflections: for n > 0 ceil(n / 2) on the far wall and floor(n / 2) on the wall at 0, mirrored for n < 0
      const int an = n < 0 ? -n : n;
      const int more = (an + 1) / 2, less = an / 2;
      const int c0 = n > 0 ? less : more, c1 = n > 0 ? more : less;
      am[off + i] = powf(b0, (float)c0) * powf(b1, (float)c1);
    }
    off += p.n[a];
  }
  // cos / sin of the window phase of the taps this lane owns: cos(2 pi (x0 + k) / Tw) = ca ck - sa sk
  float ck[kIsmWinRounds], sk[kIsmWinRounds];
#pragma unroll
  for (int r = 0; r < kIsmWinRounds; ++r) sincospif(2.f * (float)(lane + 64 * r) / p.tw, &sk[r], &ck[r]);
  __syncthreads();

  const int i0 = chunk * p.chunk;
  const int i1 = min(i0 + p.chunk, p.total);
  const float half = 0.5f * p.tw;
  for (int base = i0; base < i1; base += kIsmThreads) {
    // one image per lane: amplitude, first tap, its offset from the arrival time, sin(pi x0), window phase
    const int idx = base + lane;
    float amp = 0.f, x0 = 0.f, s0 = 0.f, ca = 1.f, sa = 0.f;
    int tlo = 0, nt = 0;
    if (idx < i1) {
      const int iz = idx % nz, q = idx / nz;
      const int iy = q % ny, ix = q / ny;
      const float d = sqrtf(sq[ix] + sq[nx + iy] + sq[nx + ny + iz]);
      amp = am[ix] * am[nx + iy] * am[nx + ny + iz] / (4.f * kPi * d);
      const float tau = d * p.fs_over_c;
      const float lo = ceilf(tau - half), hi = floorf(tau + half);
      if (lo < (float)p.nism) {
        tlo = (int)lo;
        nt = (int)hi - tlo + 1;
        x0 = lo - tau;
        s0 = sinpif(x0);                                 // t is an integer: sin(pi (x0 + k)) = (-1)^k sin(pi x0)
        sincospif(2.f * x0 / p.tw, &sa, &ca);
      }
    }
    const int cnt = min(kIsmThreads, i1 - base);
    for (int j = 0; j < cnt; ++j) {
      const int ntj = __builtin_amdgcn_readlane(nt, j);
      if (ntj <= 0) continue;                            // (uniform) the image arrives past nISM
      const int tloj = __builtin_amdgcn_readlane(tlo, j);
      const float ampj = lane_f(amp, j), x0j = lane_f(x0, j), s0j = lane_f(s0, j), caj = lane_f(ca, j), saj = lane_f(sa, j);
#pragma unroll
      for (int r = 0; r < kIsmWinRounds; ++r) {
        const int k = lane + 64 * r;
        if (64 * r < ntj && k < ntj) {
          const int t = tloj + k;
          if (t >= 0 && t < p.nism) {
            const float x = x0j + (float)k;
            const float w = 0.5f * (1.f + (caj * ck[r] - saj * sk[r]));
            const float sn = (k & 1) ? -s0j : s0j;
            const float sinc = x == 0.f ? 1.f : sn / (kPi * x);
            tile[t] += ampj * w * sinc;
          }
        }
      }
    }
  }
  __syncthreads();
  float* const dst = p.out + (long long)chunk * p.chunk_stride + (long long)rir * p.rir_stride;
  for (int i = lane; i < p.nism; i += kIsmThreads) dst[i] = tile[i];
}

__global__ void __launch_bounds__(kIsmThreads) rir_ism_kernel(const IsmParams p) { ism_body(p, blockIdx.x, blockIdx.y); }

// One launch for a block of jobs (fnssl_rir_ism_batch).  The records travel by value in the kernel arguments, as
// TrajParams does; blockIdx.z is the job, the grid is sized for the block's largest job.
constexpr int kBatchJobs = FNSSL_RIR_BATCH_JOBS;

struct IsmJob {
  IsmParams p;
  int nchunks, nrir;
};
struct IsmBatchParams {
  IsmJob job[kBatchJobs];
};
static_assert(sizeof(IsmBatchParams) <= 4096, "the block's descriptors travel in the kernel arguments");

__global__ void __launch_bounds__(kIsmThreads) rir_ism_batch_kernel(const IsmBatchParams P) {
  const IsmJob& j = P.job[blockIdx.z];
  if ((int)blockIdx.x >= j.nchunks || (int)blockIdx.y >= j.nrir) return;     // (uniform) past the job's extent
  ism_body(j.p, blockIdx.x, blockIdx.y);
}

// rir[r][t] = sum over chunks c, in order, of part[c][r][t]
__device__ __forceinline__ void sum_body(const float* __restrict__ part, int nchunks, int nrir, int nism, float* __restrict__ rir,
                                         long long rir_stride, const int t, const int r) {
  if (t >= nism) return;
  float v = 0.f;
  for (int c = 0; c < nchunks; ++c) v += part[((size_t)c * nrir + r) * nism + t];
  rir[(long long)r * rir_stride + t] = v;
}

__global__ void __launch_bounds__(256) rir_sum_kernel(const float* __restrict__ part, int nchunks, int nrir, int nism,
                                                      float* __restrict__ rir, long long rir_stride) {
  sum_body(part, nchunks, nrir, nism, rir, rir_stride, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

struct SumJob {
  const float* part;                                     // the job's own slice of the workspace
  float* rir;
  long long rir_stride;
  int nchunks, nrir, nism;
};
struct SumBatchParams {
  SumJob job[kBatchJobs];
};
static_assert(sizeof(SumBatchParams) <= 4096, "the block's descriptors travel in the kernel arguments");

__global__ void __launch_bounds__(256) rir_sum_batch_kernel(const SumBatchParams P) {
  const SumJob& j = P.job[blockIdx.z];
  if ((int)blockIdx.y >= j.nrir) return;                 // (uniform); samples past nism leave in the body
  sum_body(j.part, j.nchunks, j.nrir, j.nism, j.rir, j.rir_stride, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

struct IsmPlan {
  int total, chunk, nchunks, last;
  size_t lds;
};

int plan_ism(const char* who, int m_src, int m_rcv, const int* nb_img, int nism, int cus, IsmPlan* pl) {
  FNSSL_REQUIRE(nb_img, "%s: null nb_img", who);
  FNSSL_REQUIRE(m_src >= 1 && m_rcv >= 1 && (long long)m_src * m_rcv <= 65535, "%s: %d sources x %d receivers (1 .. 65535 RIRs)",
                who, m_src, m_rcv);
  for (int a = 0; a < 3; ++a)
    FNSSL_REQUIRE(nb_img[a] >= 1 && nb_img[a] <= kIsmMaxAxis, "%s: nb_img[%d] = %d (1 .. %d images per axis)", who, a, nb_img[a],
                  kIsmMaxAxis);
  FNSSL_REQUIRE(nism >= 2 && nism % 2 == 0 && nism <= kIsmMaxSamples,
                "%s: nISM = %d samples (even, 2 .. %d: the image-source part of one RIR is one LDS tile; use a shorter Tdiff)", who,
                nism, kIsmMaxSamples);
  const long long total = (long long)nb_img[0] * nb_img[1] * nb_img[2];
  FNSSL_REQUIRE(total < (1ll << 30), "%s: %lld images per RIR (below 2^30)", who, total);
  if (cus <= 0) cus = fnssl::device_cus();
  const long long nrir = (long long)m_src * m_rcv;
  long long want = ((long long)cus * kIsmWavesPerCu + nrir - 1) / nrir;          // chunks per RIR that fill the device
  const long long most = (total + kIsmMinChunk - 1) / kIsmMinChunk;              // ... of at least kIsmMinChunk images
  if (want > most) want = most;
  if (want < 1) want = 1;
  long long chunk = (total + want - 1) / want;
  chunk = (chunk + kIsmThreads - 1) / kIsmThreads * kIsmThreads;
  pl->total = (int)total;
  pl->chunk = (int)chunk;
  pl->nchunks = (int)((total + chunk - 1) / chunk);
  pl->last = (int)(total - (long long)(pl->nchunks - 1) * chunk);
  pl->lds = ((size_t)nism + 2 * (size_t)(nb_img[0] + nb_img[1] + nb_img[2])) * sizeof(float);
  return FNSSL_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// diffuse tail
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kTailThreads = 256;
constexpr int kTailTile = 4096;                          // samples per workgroup
constexpr int kTailMaxSeg = 1024;
constexpr int kTailMinSeg = kIsmMaxSamples / kTailMaxSeg;

struct TailParams {
  float* rir;                                            // [nrir][nsamples]
  const float* pos_src;
  const float* pos_rcv;
  int m_rcv, nism, nsamples, ls;
  float fs_over_c, b_sabine;
  unsigned seed_lo, seed_hi;
};

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// The body of both forms: workgroup `tile` of RIR `rir` of the record `p`.
__device__ __forceinline__ void tail_body(const TailParams& p, const int tile, const int rir) {
  __shared__ float e[kTailMaxSeg];
  __shared__ float part[kTailThreads / 64];
  __shared__ float line[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int src = rir / p.m_rcv, rcv = rir - src * p.m_rcv;
  float* const h = p.rir + (size_t)rir * p.nsamples;

  float d2 = 0.f;
  for (int a = 0; a < 3; ++a) {
    const float d = p.pos_src[3 * src + a] - p.pos_rcv[3 * rcv + a];
    d2 += d * d;
  }
  const float tau = sqrtf(d2) * p.fs_over_c;
  const int t0 = tau < (float)p.nism ? (int)floorf(tau) : p.nism;
  const int nseg = (p.nism - t0) / p.ls;                 // whole segments inside [0, nISM); <= kTailMaxSeg by the host's checks
  for (int j = wave; j < nseg; j += kTailThreads / 64) {
    float v = 0.f;
    for (int i = lane; i < p.ls; i += 64) {
      const float s = h[t0 + j * p.ls + i];
      v += s * s;
    }
    v = wave_sum(v);
    if (lane == 0) e[j] = logf(v / (float)p.ls + 1e-30f);
  }
  if (nseg == 0) {                                       // (uniform) no whole segment: the mean square of the whole ISM part
    float v = 0.f;
    for (int i = tid; i < p.nism; i += kTailThreads) v += h[i] * h[i];
    v = wave_sum(v);
    if (lane == 0) part[wave] = v;
  }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    bool fitted = false;
    if (nseg >= 3) {
      double tm = 0.0, em = 0.0;
      for (int j = 0; j < nseg; ++j) {
        tm += (double)t0 + ((double)j + 0.5) * p.ls;
        em += (double)e[j];
      }
      tm /= nseg;
      em /= nseg;
      double stt = 0.0, ste = 0.0;
      for (int j = 0; j < nseg; ++j) {
        const double dt = (double)t0 + ((double)j + 0.5) * p.ls - tm;
        stt += dt * dt;
        ste += dt * ((double)e[j] - em);
      }
      b = ste / stt;
      a = em - b * tm;
      fitted = b < 0.0;
    }
    if (!fitted) {
      b = (double)p.b_sabine;
      if (nseg >= 1) {
        a = (double)e[nseg - 1] - b * ((double)t0 + ((double)nseg - 0.5) * p.ls);
      } else {
        float v = 0.f;
        for (int w = 0; w < kTailThreads / 64; ++w) v += part[w];
        a = (double)logf(v / (float)p.nism + 1e-30f) - b * (0.5 * p.nism);
      }
    }
    line[0] = (float)a;
    line[1] = (float)b;
  }
  __syncthreads();
  const float a = line[0], b = line[1];
  // four samples per Philox call: counter (t / 4, rcv, src, 0), word t % 4 — whatever the launch geometry
  const int q0 = (p.nism >> 2) + tile * (kTailTile / 4);
  for (int q = q0 + tid; q < q0 + kTailTile / 4; q += kTailThreads) {
    if (4 * q >= p.nsamples) break;
    unsigned w[4];
    philox4x32_10((unsigned)q, (unsigned)rcv, (unsigned)src, 0u, p.seed_lo, p.seed_hi, w);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = 4 * q + i;
      if (t >= p.nism && t < p.nsamples) {
        const float u = ((float)(w[i] >> 9) + 0.5f) * (1.f / 8388608.f);       // exact in fp32, in (0, 1); so is 1 - u
        const float xi = 0.55132889542179204f * (logf(u) - logf(1.f - u));     // sqrt(3) / pi: unit variance
        h[t] = expf(0.5f * (a + b * (float)t)) * xi;
      }
    }
  }
}

__global__ void __launch_bounds__(kTailThreads) rir_tail_kernel(const TailParams p) { tail_body(p, blockIdx.x, blockIdx.y); }

struct TailJob {
  TailParams p;
  int tiles, nrir;
};
struct TailBatchParams {
  TailJob job[kBatchJobs];
};
static_assert(sizeof(TailBatchParams) <= 4096, "the block's descriptors travel in the kernel arguments");

__global__ void __launch_bounds__(kTailThreads) rir_tail_batch_kernel(const TailBatchParams P) {
  const TailJob& j = P.job[blockIdx.z];
  if ((int)blockIdx.x >= j.tiles || (int)blockIdx.y >= j.nrir) return;       // (uniform) past the job's extent
  tail_body(j.p, blockIdx.x, blockIdx.y);
}

// ---------------------------------------------------------------------------------------------------------------------------
// moving-source mixing
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kTrajThreads = 256;
constexpr int kTrajOut = 4;                              // consecutive outputs per thread
constexpr int kTrajTile = kTrajThreads * kTrajOut;       // outputs per workgroup
constexpr int kTrajChunk = 256;                          // source samples staged at a time (a multiple of 4, see below)
static_assert(kTrajChunk == kTrajThreads && kTrajChunk % 4 == 0, "one staged source sample per thread; float4 steps");

struct TrajParams {
  fnssl_rir_traj_item item[FNSSL_RIR_TRAJ_MAX_BATCH];
};
static_assert(sizeof(TrajParams) <= 4096, "the batch's descriptors travel in the kernel arguments");

// A workgroup owns outputs [T0, T0 + 1024) of MR receivers of one batch item; thread tid owns t = T0 + 4 tid + u.  The
// source samples that reach the tile, s in (T0 - len, T0 + 1024), are walked point by point in chunks of 256: a chunk's
// samples go to xl (zeros past the segment's end) and the taps k = t - s it can meet to rl[m][i], i = k - kbase,
// kbase = T0 - s0 - 255 (zeros outside [0, len)).  With s = s0 + 4 jb + jj the tap of output u is i = 4 (tid - jb) + 252 + 3 +
// (u - jj): per step jb one 16-byte broadcast read of x and, per receiver, ONE 16-byte read of taps (the upper half of the
// 7-tap window is the previous step's lower half) for 16 multiply-adds.  Every receiver of the group shares the x read.
template <int MR>
__global__ void __launch_bounds__(kTrajThreads) rir_traj_kernel(const TrajParams P) {
  const fnssl_rir_traj_item it = P.item[blockIdx.z];
  const int tout = it.ns + it.len - 1;
  const int T0 = blockIdx.x * kTrajTile;
  const int m0 = blockIdx.y * MR;
  if (T0 >= tout || m0 >= it.m) return;                  // (uniform) the grid is sized for the batch's largest item
  __shared__ __attribute__((aligned(16))) float xl[kTrajChunk];
  __shared__ __attribute__((aligned(16))) float rl[MR][kTrajTile + kTrajChunk];
  const int tid = threadIdx.x;
  float acc[MR][kTrajOut];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int u = 0; u < kTrajOut; ++u) acc[m][u] = 0.f;

  const int slo = max(0, T0 - it.len + 1), shi = min(it.ns, T0 + kTrajTile);
  for (int p = 0; p < it.npts; ++p) {
    const int a = max(it.w_ini[p], slo), b = min(it.w_ini[p + 1], shi);          // empty for a repeated timestamp
    for (int s0 = a; s0 < b; s0 += kTrajChunk) {
      __syncthreads();
      xl[tid] = s0 + tid < b ? it.x[s0 + tid] : 0.f;
      const int kbase = T0 - s0 - (kTrajChunk - 1);
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const float* const r = it.rirs + ((size_t)p * it.m + (m0 + m < it.m ? m0 + m : 0)) * it.len;
        for (int i = tid; i < kTrajTile + kTrajChunk; i += kTrajThreads) {
          const int k = kbase + i;
          rl[m][i] = (m0 + m < it.m && k >= 0 && k < it.len) ? r[k] : 0.f;
        }
      }
      __syncthreads();
      float4 hi[MR];
#pragma unroll
      for (int m = 0; m < MR; ++m) hi[m] = *reinterpret_cast<const float4*>(&rl[m][4 * tid + kTrajChunk]);
      for (int jb = 0; jb < kTrajChunk / 4; ++jb) {
        const float4 xv = *reinterpret_cast<const float4*>(&xl[4 * jb]);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          const float4 lo = *reinterpret_cast<const float4*>(&rl[m][4 * (tid - jb) + kTrajChunk - 4]);
          const float w[8] = {lo.x, lo.y, lo.z, lo.w, hi[m].x, hi[m].y, hi[m].z, hi[m].w};
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)                 // ascending source sample: the order of the sum is fixed
#pragma unroll
            for (int u = 0; u < kTrajOut; ++u) acc[m][u] += xs[jj] * w[3 + u - jj];
          hi[m] = lo;
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kTrajOut; ++u) {
    const int t = T0 + kTrajOut * tid + u;
    if (t < tout) {
#pragma unroll
      for (int m = 0; m < MR; ++m)
        if (m0 + m < it.m) it.y[(size_t)t * it.m + m0 + m] = acc[m][u];
    }
  }
}

int check_geometry(const char* who, const float* room, const float* beta, const float* pos_src, const float* pos_rcv,
                   double fs, double c) {
  FNSSL_REQUIRE(room && beta && pos_src && pos_rcv, "%s: null pointer", who);
  for (int a = 0; a < 3; ++a) FNSSL_REQUIRE(room[a] > 0.f, "%s: room_sz[%d] = %g", who, a, (double)room[a]);
  for (int w = 0; w < 6; ++w) FNSSL_REQUIRE(beta[w] >= 0.f && beta[w] <= 1.f, "%s: beta[%d] = %g (0 .. 1)", who, w, (double)beta[w]);
  FNSSL_REQUIRE(fs > 0.0 && c > 0.0, "%s: fs = %g, c = %g", who, fs, c);
  return FNSSL_OK;
}

// The checks of fnssl_rir_ism and the record of its launch for a single-chunk plan (the RIR is the output); `who` names the
// call, and for a batch the job.  cus <= 0 asks the current device.
int prepare_ism(const char* who, const float* room_sz, const float* beta, const float* pos_src, int m_src, const float* pos_rcv,
                int m_rcv, const int* nb_img, int nism, int nsamples, double fs, double c, float* rir, int cus, IsmParams* out,
                IsmPlan* pl) {
  FNSSL_TRY(check_geometry(who, room_sz, beta, pos_src, pos_rcv, fs, c));
  FNSSL_REQUIRE(rir, "%s: null pointer", who);
  FNSSL_TRY(plan_ism(who, m_src, m_rcv, nb_img, nism, cus, pl));
  FNSSL_REQUIRE(nsamples >= nism, "%s: nSamples %d < nISM %d", who, nsamples, nism);
  const double tw = 8e-3 * fs;
  FNSSL_REQUIRE(tw >= 2.0 && tw + 1.0 <= 64.0 * kIsmWinRounds, "%s: a window of %g samples (2 .. %d: fs from 250 Hz to 63.8 kHz)", who,
                tw, 64 * kIsmWinRounds - 1);
  IsmParams p{};
  p.pos_src = pos_src;
  p.pos_rcv = pos_rcv;
  for (int a = 0; a < 3; ++a) p.room[a] = room_sz[a], p.n[a] = nb_img[a];
  for (int w = 0; w < 6; ++w) p.beta[w] = beta[w];
  p.m_rcv = m_rcv;
  p.nism = nism;
  p.chunk = pl->chunk;
  p.total = pl->total;
  p.fs_over_c = (float)(fs / c);
  p.tw = (float)tw;
  p.out = rir;
  p.rir_stride = nsamples;
  p.chunk_stride = 0;
  *out = p;
  return FNSSL_OK;
}

// several chunks: the partial tiles go to part [chunk][rir][nism]
void ism_to_workspace(IsmParams* p, float* part, int nrir) {
  p->out = part;
  p->rir_stride = p->nism;
  p->chunk_stride = (long long)nrir * p->nism;
}

// The checks of fnssl_rir_tail, its record and its grid's x (unused when nsamples == nism: there is no tail).
int prepare_tail(const char* who, const float* room_sz, const float* beta, const float* pos_src, int m_src, const float* pos_rcv,
                 int m_rcv, int nism, int nsamples, double fs, double c, unsigned long long seed, float* rir, TailParams* out,
                 unsigned* gx) {
  FNSSL_TRY(check_geometry(who, room_sz, beta, pos_src, pos_rcv, fs, c));
  FNSSL_REQUIRE(rir, "%s: null pointer", who);
  FNSSL_REQUIRE(m_src >= 1 && m_rcv >= 1 && (long long)m_src * m_rcv <= 65535, "%s: %d sources x %d receivers (1 .. 65535 RIRs)", who,
                m_src, m_rcv);
  FNSSL_REQUIRE(nism >= 2 && nism % 2 == 0 && nism <= kIsmMaxSamples, "%s: nISM = %d samples (even, 2 .. %d)", who, nism, kIsmMaxSamples);
  FNSSL_REQUIRE(nsamples >= nism && nsamples % 2 == 0 && nsamples < (1 << 30), "%s: nSamples = %d (even, nISM %d .. 2^30)", who,
                nsamples, nism);
  const int ls = (int)std::lround(8e-3 * fs);
  FNSSL_REQUIRE(ls >= kTailMinSeg, "%s: a segment of %d samples (at least %d: fs >= 1 kHz)", who, ls, kTailMinSeg);
  const double vol = (double)room_sz[0] * room_sz[1] * room_sz[2];
  const double area[3] = {(double)room_sz[1] * room_sz[2], (double)room_sz[0] * room_sz[2], (double)room_sz[0] * room_sz[1]};
  double absorb = 0.0;
  for (int w = 0; w < 6; ++w) absorb += area[w / 2] * (1.0 - (double)beta[w] * beta[w]);
  TailParams p{};
  p.rir = rir;
  p.pos_src = pos_src;
  p.pos_rcv = pos_rcv;
  p.m_rcv = m_rcv;
  p.nism = nism;
  p.nsamples = nsamples;
  p.ls = ls;
  p.fs_over_c = (float)(fs / c);
  p.b_sabine = absorb > 0.0 ? (float)(-std::log(1e6) / (0.161 * vol / absorb * fs)) : 0.f;
  p.seed_lo = (unsigned)(seed & 0xffffffffull);
  p.seed_hi = (unsigned)(seed >> 32);
  const int quads = ((nsamples + 3) >> 2) - (nism >> 2);
  *gx = (unsigned)((quads + kTailTile / 4 - 1) / (kTailTile / 4));
  *out = p;
  return FNSSL_OK;
}

}  // namespace

extern "C" {

int fnssl_rir_plan(int m_src, int m_rcv, const int* nb_img, int nism, int cus, fnssl_rir_plan_info* out) {
  FNSSL_REQUIRE(out, "rir_plan: null pointer");
  IsmPlan pl;
  FNSSL_TRY(plan_ism("rir_plan", m_src, m_rcv, nb_img, nism, cus, &pl));
  out->images = pl.total;
  out->chunk_images = pl.chunk;
  out->nchunks = pl.nchunks;
  out->last_chunk_images = pl.last;
  out->grid_x = pl.nchunks;
  out->grid_y = m_src * m_rcv;
  out->threads = kIsmThreads;
  out->lds_bytes = (int)pl.lds;
  out->workspace_bytes = pl.nchunks > 1 ? (size_t)pl.nchunks * m_src * m_rcv * nism * sizeof(float) : 0;
  return FNSSL_OK;
}

size_t fnssl_rir_workspace_bytes(int m_src, int m_rcv, const int* nb_img, int nism, int cus) {
  fnssl_rir_plan_info pi;
  return fnssl_rir_plan(m_src, m_rcv, nb_img, nism, cus, &pi) == FNSSL_OK ? pi.workspace_bytes : 0;
}

int fnssl_rir_ism(const float* room_sz, const float* beta, const float* pos_src, int m_src, const float* pos_rcv, int m_rcv,
                  const int* nb_img, int nism, int nsamples, double fs, double c, float* rir, void* workspace,
                  size_t workspace_bytes, void* stream) {
  IsmParams p{};
  IsmPlan pl;
  FNSSL_TRY(prepare_ism("rir_ism", room_sz, beta, pos_src, m_src, pos_rcv, m_rcv, nb_img, nism, nsamples, fs, c, rir, 0, &p, &pl));
  const int nrir = m_src * m_rcv;
  if (pl.nchunks > 1) {
    const size_t need = (size_t)pl.nchunks * nrir * nism * sizeof(float);
    FNSSL_TRY(fnssl::check_workspace("rir_ism", workspace, workspace_bytes, need));
    ism_to_workspace(&p, static_cast<float*>(workspace), nrir);
  }
  hipStream_t s = fnssl::as_stream(stream);
  {
    fnssl::TimedLaunch tl("rir_ism", s);
    FNSSL_TRY(enqueue(s, Kernel{rir_ism_kernel, kIsmThreads, pl.lds, "rir_ism_kernel"}, dim3((unsigned)pl.nchunks, (unsigned)nrir), p));
  }
  if (pl.nchunks > 1) {
    fnssl::TimedLaunch tl("rir_sum", s);
    FNSSL_TRY(enqueue(s, Kernel{rir_sum_kernel, 256, 0, "rir_sum_kernel"}, dim3((unsigned)((nism + 255) / 256), (unsigned)nrir),
                      static_cast<const float*>(workspace), pl.nchunks, nrir, nism, rir, (long long)nsamples));
  }
  return FNSSL_OK;
}

int fnssl_rir_tail(const float* room_sz, const float* beta, const float* pos_src, int m_src, const float* pos_rcv, int m_rcv,
                   int nism, int nsamples, double fs, double c, unsigned long long seed, float* rir, void* stream) {
  TailParams p{};
  unsigned gx = 0;
  FNSSL_TRY(prepare_tail("rir_tail", room_sz, beta, pos_src, m_src, pos_rcv, m_rcv, nism, nsamples, fs, c, seed, rir, &p, &gx));
  if (nsamples == nism) return FNSSL_OK;
  hipStream_t s = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl("rir_tail", s);
  return enqueue(s, Kernel{rir_tail_kernel, kTailThreads, 0, "rir_tail_kernel"}, dim3(gx, (unsigned)(m_src * m_rcv)), p);
}

// ---- a batch of jobs: every job is checked and planned first, then ceil(njobs / FNSSL_RIR_BATCH_JOBS) launch sets ----------
int fnssl_rir_batch_plan(const fnssl_rir_job* jobs, int njobs, int cus, fnssl_rir_job_plan* out) {
  FNSSL_REQUIRE(jobs && out && njobs >= 1, "rir_batch_plan: null pointer / no job");
  if (cus <= 0) cus = fnssl::device_cus();               // once: every job is planned for the same device
  size_t off = 0;
  for (int k = 0; k < njobs; ++k) {
    const fnssl_rir_job& j = jobs[k];
    char who[48];
    std::snprintf(who, sizeof who, "rir_batch_plan: job %d", k);
    IsmPlan pl;
    FNSSL_TRY(plan_ism(who, j.m_src, j.m_rcv, j.nb_img, j.nism, cus, &pl));
    fnssl_rir_plan_info& pi = out[k].plan;
    pi.images = pl.total;
    pi.chunk_images = pl.chunk;
    pi.nchunks = pl.nchunks;
    pi.last_chunk_images = pl.last;
    pi.grid_x = pl.nchunks;
    pi.grid_y = j.m_src * j.m_rcv;
    pi.threads = kIsmThreads;
    pi.lds_bytes = (int)pl.lds;
    pi.workspace_bytes = pl.nchunks > 1 ? (size_t)pl.nchunks * j.m_src * j.m_rcv * j.nism * sizeof(float) : 0;
    out[k].workspace_offset = off;
    off += pi.workspace_bytes;
  }
  return FNSSL_OK;
}

size_t fnssl_rir_batch_workspace_bytes(const fnssl_rir_job* jobs, int njobs, int cus) {
  if (!jobs || njobs < 1) return 0;
  if (cus <= 0) cus = fnssl::device_cus();
  size_t total = 0;
  for (int k = 0; k < njobs; ++k) {
    const fnssl_rir_job& j = jobs[k];
    total += fnssl_rir_workspace_bytes(j.m_src, j.m_rcv, j.nb_img, j.nism, cus);
  }
  return total;
}

int fnssl_rir_ism_batch(const fnssl_rir_job* jobs, int njobs, void* workspace, size_t workspace_bytes, void* stream) {
  FNSSL_REQUIRE(jobs && njobs >= 1, "rir_ism_batch: null pointer / no job");
  std::vector<IsmJob> ij((size_t)njobs);
  std::vector<IsmPlan> pls((size_t)njobs);
  std::vector<size_t> offs((size_t)njobs);
  const int cus = fnssl::device_cus();
  size_t need = 0;
  for (int k = 0; k < njobs; ++k) {                      // every check of every job before the first launch
    const fnssl_rir_job& j = jobs[k];
    char who[48];
    std::snprintf(who, sizeof who, "rir_ism_batch: job %d", k);
    FNSSL_TRY(prepare_ism(who, j.room_sz, j.beta, j.pos_src, j.m_src, j.pos_rcv, j.m_rcv, j.nb_img, j.nism, j.nsamples, j.fs,
                          j.c, j.rir, cus, &ij[k].p, &pls[k]));
    ij[k].nchunks = pls[k].nchunks;
    ij[k].nrir = j.m_src * j.m_rcv;
    offs[k] = need;
    if (pls[k].nchunks > 1) need += (size_t)pls[k].nchunks * ij[k].nrir * j.nism * sizeof(float);
  }
  if (need) FNSSL_TRY(fnssl::check_workspace("rir_ism_batch", workspace, workspace_bytes, need));
  for (int k = 0; k < njobs; ++k)
    if (pls[k].nchunks > 1) ism_to_workspace(&ij[k].p, reinterpret_cast<float*>(static_cast<char*>(workspace) + offs[k]), ij[k].nrir);

  hipStream_t s = fnssl::as_stream(stream);
  for (int k0 = 0; k0 < njobs; k0 += kBatchJobs) {
    const int nb = std::min(kBatchJobs, njobs - k0);
    IsmBatchParams P{};
    SumBatchParams S{};
    dim3 grid(1, 1, (unsigned)nb), sgrid(1, 1, 0);
    size_t lds = 0;                                      // dynamic LDS is per launch: the block's largest tile
    for (int k = 0; k < nb; ++k) {
      const IsmJob& j = ij[k0 + k];
      P.job[k] = j;
      grid.x = std::max(grid.x, (unsigned)j.nchunks);
      grid.y = std::max(grid.y, (unsigned)j.nrir);
      lds = std::max(lds, pls[k0 + k].lds);
      if (j.nchunks > 1) {
        const fnssl_rir_job& job = jobs[k0 + k];
        S.job[sgrid.z++] = SumJob{j.p.out, job.rir, (long long)job.nsamples, j.nchunks, j.nrir, job.nism};
        sgrid.x = std::max(sgrid.x, (unsigned)((job.nism + 255) / 256));
        sgrid.y = std::max(sgrid.y, (unsigned)j.nrir);
      }
    }
    {
      fnssl::TimedLaunch tl("rir_ism_batch", s);
      FNSSL_TRY(enqueue(s, Kernel{rir_ism_batch_kernel, kIsmThreads, lds, "rir_ism_batch_kernel"}, grid, P));
    }
    if (sgrid.z) {
      fnssl::TimedLaunch tl("rir_sum_batch", s);
      FNSSL_TRY(enqueue(s, Kernel{rir_sum_batch_kernel, 256, 0, "rir_sum_batch_kernel"}, sgrid, S));
    }
  }
  return FNSSL_OK;
}

int fnssl_rir_tail_batch(const fnssl_rir_job* jobs, int njobs, void* stream) {
  FNSSL_REQUIRE(jobs && njobs >= 1, "rir_tail_batch: null pointer / no job");
  std::vector<TailJob> tj;
  tj.reserve((size_t)njobs);
  for (int k = 0; k < njobs; ++k) {                      // every check of every job before the first launch
    const fnssl_rir_job& j = jobs[k];
    char who[48];
    std::snprintf(who, sizeof who, "rir_tail_batch: job %d", k);
    TailJob t{};
    unsigned gx = 0;
    FNSSL_TRY(prepare_tail(who, j.room_sz, j.beta, j.pos_src, j.m_src, j.pos_rcv, j.m_rcv, j.nism, j.nsamples, j.fs, j.c, j.seed,
                           j.rir, &t.p, &gx));
    if (j.nsamples == j.nism) continue;                  // no tail: the job takes no slot
    t.tiles = (int)gx;
    t.nrir = j.m_src * j.m_rcv;
    tj.push_back(t);
  }
  hipStream_t s = fnssl::as_stream(stream);
  const int n = (int)tj.size();
  for (int k0 = 0; k0 < n; k0 += kBatchJobs) {
    const int nb = std::min(kBatchJobs, n - k0);
    TailBatchParams P{};
    dim3 grid(1, 1, (unsigned)nb);
    for (int k = 0; k < nb; ++k) {
      P.job[k] = tj[k0 + k];
      grid.x = std::max(grid.x, (unsigned)P.job[k].tiles);
      grid.y = std::max(grid.y, (unsigned)P.job[k].nrir);
    }
    fnssl::TimedLaunch tl("rir_tail_batch", s);
    FNSSL_TRY(enqueue(s, Kernel{rir_tail_batch_kernel, kTailThreads, 0, "rir_tail_batch_kernel"}, grid, P));
  }
  return FNSSL_OK;
}

int fnssl_rir_trajectory(const fnssl_rir_traj_item* items, int nitems, void* stream) {
  FNSSL_REQUIRE(items, "rir_trajectory: null pointer");
  FNSSL_REQUIRE(nitems >= 1 && nitems <= FNSSL_RIR_TRAJ_MAX_BATCH, "rir_trajectory: %d items (1 .. %d)", nitems, FNSSL_RIR_TRAJ_MAX_BATCH);
  TrajParams P{};
  long long tout = 0;
  int mmax = 0;
  for (int k = 0; k < nitems; ++k) {
    const fnssl_rir_traj_item& it = items[k];
    FNSSL_REQUIRE(it.x && it.rirs && it.w_ini && it.y, "rir_trajectory: item %d: null pointer", k);
    FNSSL_REQUIRE(it.ns >= 1 && it.len >= 1 && it.npts >= 1 && it.m >= 1, "rir_trajectory: item %d: %d samples, %d taps, %d points, %d receivers",
                  k, it.ns, it.len, it.npts, it.m);
    FNSSL_REQUIRE((long long)it.ns + it.len < (1ll << 30), "rir_trajectory: item %d: %d + %d samples (below 2^30)", k, it.ns, it.len);
    P.item[k] = it;
    tout = std::max(tout, (long long)it.ns + it.len - 1);
    mmax = std::max(mmax, it.m);
  }
  const int mr = mmax == 1 ? 1 : mmax == 2 ? 2 : 4;      // receivers per workgroup
  const dim3 grid((unsigned)((tout + kTrajTile - 1) / kTrajTile), (unsigned)((mmax + mr - 1) / mr), (unsigned)nitems);
  FNSSL_REQUIRE(grid.y <= 65535, "rir_trajectory: %d receivers", mmax);
  hipStream_t s = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl("rir_trajectory", s);
  return fnssl::with_value<1, 2, 4>(mr, [&](auto MR) {
    return enqueue(s, Kernel{rir_traj_kernel<MR>, kTrajThreads, 0, "rir_traj_kernel"}, grid, P);
  });
}

}  // extern "C"
