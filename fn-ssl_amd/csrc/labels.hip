// Training labels of a batch of simulated scenes (fnssl/scene.py; what RandomTrajectoryDataset.getRandomScene, the
// Segmenting_SRPDNN transform and the gts dict of FixTrajectoryDataset.__getitem__ of the reference's Dataset.py do between
// AcousticScene.simulate() and a training step).  The model is DESIGN.md §20.
//   fnssl_scene_doa_batch      np.interp of the trajectory points at t = k / fs, then cart2sph: trajectory and DOA, in double
//   fnssl_scene_segment_batch  per window: the -pi / pi unwrap, the mean DOA, the fold; the VAD windows and their counts
//   fnssl_scene_pack_batch     the per-source direct-path signals of every scene into one padded [B, n, M, Smax]
//
// Batch conventions are scene.hip's: the per-scene records travel by value in the kernel arguments, FNSSL_SCENE_BATCH_SCENES per
// launch, the scene is a grid dimension, and every scene is checked before the first launch.
// Determinism.  No float atomics.  A window's sums are per-thread strided sums in ascending order, the xor butterfly of a
// wave, and the waves' partial sums added in wave order; the workgroup is always 256 threads, so a scene's bits depend on
// nothing but its own numbers.  All angle arithmetic is double and unfused: the interpolation is numpy's expression.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host.h"

using fnssl::enqueue;
using fnssl::Kernel;

namespace {

constexpr int kBatchScenes = FNSSL_SCENE_BATCH_SCENES;
constexpr int kThreads = 256;
constexpr double kPi = 3.14159265358979323846;
constexpr double kTwoPi = 2.0 * kPi;                     // numpy's 2 * np.pi, exact in binary

// ---------------------------------------------------------------------------------------------------------------------------
// trajectory and DOA
// ---------------------------------------------------------------------------------------------------------------------------
struct DoaJob {
  const double* pts;                                     // [npts][3][ns]
  const double* ts;                                      // [npts]
  double* traj;                                          // [n][3][ns]
  double* doa;                                           // [n][2][ns]
  double pos[3];
  double fs;
  int npts, ns, n;
};
struct DoaBatchParams {
  DoaJob job[kBatchScenes];
};
static_assert(sizeof(DoaBatchParams) <= 4096, "the block's descriptors travel in the kernel arguments");

// grid (ceil(n ns / 256), scenes): one thread per (sample k, source s), s fastest, so the ns doubles of a row are one run.
// np.interp: left of the first point its value, right of the last point its value, on a point its value, else
// slope (x - xp[j]) + fp[j] with slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]), j the last point at or before x.
__global__ void __launch_bounds__(kThreads) labels_doa_kernel(const DoaBatchParams P) {
#pragma clang fp contract(off)
  const DoaJob& j = P.job[blockIdx.y];
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (long long)j.n * j.ns) return;
  const int k = (int)(idx / j.ns), s = (int)(idx - (long long)k * j.ns);
  const double x = (double)k / j.fs;
  const int last = j.npts - 1;
  int lo = -1;                                           // the last point with ts <= x (-1: none, x lies left of all)
  if (x > j.ts[last]) {
    lo = j.npts;
  } else if (!(x < j.ts[0])) {
    int imin = 0, imax = j.npts;
    while (imin < imax) {
      const int imid = imin + ((imax - imin) >> 1);
      if (x >= j.ts[imid]) imin = imid + 1; else imax = imid;
    }
    lo = imin - 1;
  }
  double c[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double* const fp = j.pts + (size_t)i * j.ns + s;
    const size_t st = (size_t)3 * j.ns;
    double v;
    if (lo < 0) {
      v = fp[0];
    } else if (lo >= last) {
      v = fp[(size_t)last * st];
    } else if (j.ts[lo] == x) {
      v = fp[(size_t)lo * st];
    } else {
      const double slope = (fp[(size_t)(lo + 1) * st] - fp[(size_t)lo * st]) / (j.ts[lo + 1] - j.ts[lo]);
      v = slope * (x - j.ts[lo]) + fp[(size_t)lo * st];
    }
    j.traj[((size_t)k * 3 + i) * j.ns + s] = v;
    c[i] = v - j.pos[i];
  }
  const double xy2 = c[0] * c[0] + c[1] * c[1];
  j.doa[((size_t)k * 2 + 0) * j.ns + s] = atan2(sqrt(xy2), c[2]);      // elevation, from the z axis down
  j.doa[((size_t)k * 2 + 1) * j.ns + s] = atan2(c[1], c[0]);           // azimuth
}

// ---------------------------------------------------------------------------------------------------------------------------
// windows
// ---------------------------------------------------------------------------------------------------------------------------
struct SegJob {
  const double* doa;                                     // [>= (nw - 1) step + K][2][ns], or null (no DOA half)
  const unsigned char* vs;                               // [vad_len][ns], or null (zeros)
  const unsigned char* v;                                // [vad_len], or null (zeros)
  int ns, vad_len;
};
struct SegBatchParams {
  SegJob job[kBatchScenes];
  double* doaw;                                          // [scenes][nw][2][smax] of this block, or null
  unsigned char* vsw;                                    // [scenes][nw][K][smax], or null
  unsigned char* vw;                                     // [scenes][nw][K], or null
  int* count;                                            // [scenes][nw][smax], or null
  int K, step, nw, smax;
};
static_assert(sizeof(SegBatchParams) <= 4096, "the block's descriptors travel in the kernel arguments");

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// grid (nw, smax, scenes), 256 threads: one workgroup per (window w, source s, scene).
__global__ void __launch_bounds__(kThreads) labels_segment_kernel(const SegBatchParams P) {
#pragma clang fp contract(off)
  __shared__ double part[2][kThreads / 64];
  __shared__ int cnt[kThreads / 64];
  const SegJob& j = P.job[blockIdx.z];
  const int w = blockIdx.x, s = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int K = P.K;
  const size_t win = (size_t)b * P.nw + w;
  const long long t0 = (long long)w * P.step;
  const bool present = s < j.ns;                         // (uniform) an absent source is all zeros

  if (P.doaw && j.doa) {
    double el = 0.0, az = 0.0;
    if (present) {
      const double* const d = j.doa + (size_t)t0 * 2 * j.ns + s;
      const size_t st = (size_t)2 * j.ns;
      int jump = 0;
      for (int i = tid; i + 1 < K; i += kThreads) jump |= fabs(d[(size_t)(i + 1) * st + j.ns] - d[(size_t)i * st + j.ns]) > kPi;
      jump = __syncthreads_or(jump);
      for (int i = tid; i < K; i += kThreads) {
        const double a = d[(size_t)i * st + j.ns];
        el += d[(size_t)i * st];
        az += (jump && a < 0.0) ? a + kTwoPi : a;
      }
      el = wave_sum(el);
      az = wave_sum(az);
      if ((tid & 63) == 0) part[0][tid >> 6] = el, part[1][tid >> 6] = az;
      __syncthreads();
      el = (((part[0][0] + part[0][1]) + part[0][2]) + part[0][3]) / (double)K;
      az = (((part[1][0] + part[1][1]) + part[1][2]) + part[1][3]) / (double)K;
      if (az > kPi) az -= kTwoPi;
    }
    if (tid == 0) {
      P.doaw[(win * 2 + 0) * P.smax + s] = el;
      P.doaw[(win * 2 + 1) * P.smax + s] = az;
    }
  }

  if (P.vsw) {
    int c = 0;
    for (int i = tid; i < K; i += kThreads) {
      const long long t = t0 + i;
      const unsigned char on = (present && j.vs && t < j.vad_len && j.vs[(size_t)t * j.ns + s]) ? 1 : 0;
      P.vsw[(win * K + i) * P.smax + s] = on;
      c += on;
    }
    c = wave_sum(c);
    if ((tid & 63) == 0) cnt[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) P.count[win * P.smax + s] = ((cnt[0] + cnt[1]) + cnt[2]) + cnt[3];
  }
  if (P.vw && s == 0) {
    for (int i = tid; i < K; i += kThreads) {
      const long long t = t0 + i;
      P.vw[win * K + i] = (j.v && t < j.vad_len && j.v[t]) ? 1 : 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// padded direct-path signals
// ---------------------------------------------------------------------------------------------------------------------------
struct PackJob {
  const float* a[FNSSL_SCENE_MAX_SOURCES];               // element (t, c) of source s is a[s][t st_t + c st_c]
  long long st_t, st_c;
  int ns;
};
struct PackBatchParams {
  PackJob job[kBatchScenes];
  float* out;                                            // [scenes][n m][smax] of this block
  long long count;                                       // n m
  int m, smax, vec;
};
static_assert(sizeof(PackBatchParams) <= 4096, "the block's descriptors travel in the kernel arguments");

// element e = t m + c of source s, 0 for an absent source
__device__ __forceinline__ float pack_at(const PackJob& j, int m, int s, long long e) {
  if (s >= j.ns) return 0.f;
  if (j.st_c == 1 && j.st_t == m) return j.a[s][e];      // (uniform) rows of m floats, contiguous
  const long long t = e / m;
  return j.a[s][t * j.st_t + (e - t * m) * j.st_c];
}

// grid (ceil(items / 256), scenes).  vec (smax 1, 2 or 4, count smax a multiple of 4, out 16-byte aligned): an item is
// one float4 of the output, 4 / smax elements (t, c) of every source; else an item is one element and its smax floats.
__global__ void __launch_bounds__(kThreads) labels_pack_kernel(const PackBatchParams P) {
  const PackJob& j = P.job[blockIdx.y];
  const long long item = (long long)blockIdx.x * kThreads + threadIdx.x;
  float* const out = P.out + (size_t)blockIdx.y * (size_t)P.count * P.smax;
  if (P.vec) {
    const int per = 4 / P.smax;
    const long long e = item * per;
    if (e >= P.count) return;
    float4 v;
    if (P.smax == 4) {
      v = make_float4(pack_at(j, P.m, 0, e), pack_at(j, P.m, 1, e), pack_at(j, P.m, 2, e), pack_at(j, P.m, 3, e));
    } else if (P.smax == 2) {
      v = make_float4(pack_at(j, P.m, 0, e), pack_at(j, P.m, 1, e), pack_at(j, P.m, 0, e + 1), pack_at(j, P.m, 1, e + 1));
    } else {
      v = make_float4(pack_at(j, P.m, 0, e), pack_at(j, P.m, 0, e + 1), pack_at(j, P.m, 0, e + 2), pack_at(j, P.m, 0, e + 3));
    }
    reinterpret_cast<float4*>(out)[item] = v;
  } else {
    if (item >= P.count) return;
    for (int s = 0; s < P.smax; ++s) out[(size_t)item * P.smax + s] = pack_at(j, P.m, s, item);
  }
}

}  // namespace

extern "C" {

int fnssl_scene_doa_batch(const fnssl_scene_doa_desc* scenes, int nscenes, void* stream) {
  FNSSL_REQUIRE(scenes && nscenes >= 1, "scene_doa_batch: null pointer / no scene");
  std::vector<DoaJob> jobs((size_t)nscenes);
  for (int b = 0; b < nscenes; ++b) {
    const fnssl_scene_doa_desc& d = scenes[b];
    FNSSL_REQUIRE(d.traj_pts && d.timestamps && d.trajectory && d.doa, "scene_doa_batch: scene %d: null pointer", b);
    FNSSL_REQUIRE(d.npts >= 1 && d.npts < (1 << 24), "scene_doa_batch: scene %d: %d trajectory points", b, d.npts);
    FNSSL_REQUIRE(d.ns >= 1 && d.ns <= FNSSL_SCENE_MAX_SOURCES, "scene_doa_batch: scene %d: %d sources (1 .. %d)", b, d.ns,
                  FNSSL_SCENE_MAX_SOURCES);
    FNSSL_REQUIRE(d.n >= 1 && d.n < (1 << 28), "scene_doa_batch: scene %d: %d samples", b, d.n);
    FNSSL_REQUIRE(d.fs > 0.0 && std::isfinite(d.fs), "scene_doa_batch: scene %d: fs = %g", b, d.fs);
    FNSSL_REQUIRE(std::isfinite(d.array_pos[0]) && std::isfinite(d.array_pos[1]) && std::isfinite(d.array_pos[2]),
                  "scene_doa_batch: scene %d: array_pos is not finite", b);
    DoaJob j{};
    j.pts = d.traj_pts, j.ts = d.timestamps, j.traj = d.trajectory, j.doa = d.doa;
    for (int i = 0; i < 3; ++i) j.pos[i] = d.array_pos[i];
    j.fs = d.fs, j.npts = d.npts, j.ns = d.ns, j.n = d.n;
    jobs[b] = j;
  }
  hipStream_t s = fnssl::as_stream(stream);
  for (int b0 = 0; b0 < nscenes; b0 += kBatchScenes) {
    const int nb = std::min(kBatchScenes, nscenes - b0);
    DoaBatchParams P{};
    long long items = 0;
    for (int b = 0; b < nb; ++b) P.job[b] = jobs[b0 + b], items = std::max(items, (long long)P.job[b].n * P.job[b].ns);
    fnssl::TimedLaunch tl("scene_doa_batch", s);
    FNSSL_TRY(enqueue(s, Kernel{labels_doa_kernel, kThreads, 0, "labels_doa_kernel"},
                      dim3((unsigned)((items + kThreads - 1) / kThreads), (unsigned)nb), P));
  }
  return FNSSL_OK;
}

int fnssl_scene_segment_batch(const fnssl_scene_segment_desc* scenes, int nscenes, int len, int K, int step, int nw, int smax,
                              double* doaw, unsigned char* vad_sources, unsigned char* vad, int* vad_count, void* stream) {
  FNSSL_REQUIRE(scenes && nscenes >= 1, "scene_segment_batch: null pointer / no scene");
  FNSSL_REQUIRE(len >= 1 && len < (1 << 28), "scene_segment_batch: %d samples", len);
  FNSSL_REQUIRE(K >= 1 && K <= len, "scene_segment_batch: window %d for %d samples (1 .. the signal length)", K, len);
  FNSSL_REQUIRE(step >= 1 && step <= len, "scene_segment_batch: step %d for %d samples (1 .. the signal length)", step, len);
  FNSSL_REQUIRE(nw >= 1 && nw <= 65535 && (long long)(nw - 1) * step + K <= len,
                "scene_segment_batch: %d windows of %d every %d do not fit %d samples", nw, K, step, len);
  FNSSL_REQUIRE(smax >= 1 && smax <= FNSSL_SCENE_MAX_SOURCES, "scene_segment_batch: max_source = %d (1 .. %d)", smax,
                FNSSL_SCENE_MAX_SOURCES);
  FNSSL_REQUIRE(doaw || vad_sources || vad, "scene_segment_batch: no output");
  FNSSL_REQUIRE(!vad_sources == !vad_count, "scene_segment_batch: the VAD windows and their counts come together");
  for (int b = 0; b < nscenes; ++b) {
    const fnssl_scene_segment_desc& d = scenes[b];
    FNSSL_REQUIRE(d.ns >= 1 && d.ns <= smax, "scene_segment_batch: scene %d: %d sources (1 .. max_source = %d)", b, d.ns, smax);
    FNSSL_REQUIRE(!doaw || !d.doa || (long long)d.doa_len >= (long long)(nw - 1) * step + K,
                  "scene_segment_batch: scene %d: %d rows of DOA, the windows read %lld", b, d.doa_len, (long long)(nw - 1) * step + K);
    FNSSL_REQUIRE(d.vad_len >= 0 && d.vad_len <= len, "scene_segment_batch: scene %d: a VAD of %d samples for a signal of %d", b,
                  d.vad_len, len);
  }
  hipStream_t s = fnssl::as_stream(stream);
  for (int b0 = 0; b0 < nscenes; b0 += kBatchScenes) {
    const int nb = std::min(kBatchScenes, nscenes - b0);
    SegBatchParams P{};
    for (int b = 0; b < nb; ++b) {
      const fnssl_scene_segment_desc& d = scenes[b0 + b];
      P.job[b].doa = d.doa, P.job[b].vs = d.vad_sources, P.job[b].v = d.vad, P.job[b].ns = d.ns, P.job[b].vad_len = d.vad_len;
    }
    const size_t wins = (size_t)b0 * nw;
    P.doaw = doaw ? doaw + wins * 2 * smax : nullptr;
    P.vsw = vad_sources ? vad_sources + wins * K * smax : nullptr;
    P.vw = vad ? vad + wins * K : nullptr;
    P.count = vad_count ? vad_count + wins * smax : nullptr;
    P.K = K, P.step = step, P.nw = nw, P.smax = smax;
    fnssl::TimedLaunch tl("scene_segment_batch", s);
    FNSSL_TRY(enqueue(s, Kernel{labels_segment_kernel, kThreads, 0, "labels_segment_kernel"},
                      dim3((unsigned)nw, (unsigned)smax, (unsigned)nb), P));
  }
  return FNSSL_OK;
}

int fnssl_scene_pack_batch(const fnssl_scene_pack_desc* scenes, int nscenes, int n, int m, int smax, float* out, void* stream) {
  FNSSL_REQUIRE(scenes && out && nscenes >= 1, "scene_pack_batch: null pointer / no scene");
  FNSSL_REQUIRE(n >= 1 && n < (1 << 28) && m >= 1 && m <= 65535, "scene_pack_batch: %d samples, %d channels", n, m);
  FNSSL_REQUIRE(smax >= 1 && smax <= FNSSL_SCENE_MAX_SOURCES, "scene_pack_batch: max_source = %d (1 .. %d)", smax,
                FNSSL_SCENE_MAX_SOURCES);
  for (int b = 0; b < nscenes; ++b) {
    FNSSL_REQUIRE(scenes[b].ns >= 1 && scenes[b].ns <= smax, "scene_pack_batch: scene %d: %d sources (1 .. max_source = %d)", b,
                  scenes[b].ns, smax);
    for (int k = 0; k < scenes[b].ns; ++k) FNSSL_REQUIRE(scenes[b].dp[k], "scene_pack_batch: scene %d: source %d is null", b, k);
    FNSSL_REQUIRE(scenes[b].stride_t >= 1 && scenes[b].stride_c >= 1, "scene_pack_batch: scene %d: strides %lld, %lld", b,
                  scenes[b].stride_t, scenes[b].stride_c);
  }
  const long long count = (long long)n * m;
  FNSSL_REQUIRE(count < (1ll << 38), "scene_pack_batch: %d samples x %d channels (fewer than 2^38 elements per scene)", n, m);
  const int vec = smax != 3 && (count * smax) % 4 == 0 && fnssl::aligned16(out);
  const long long items = vec ? count * smax / 4 : count;
  hipStream_t s = fnssl::as_stream(stream);
  for (int b0 = 0; b0 < nscenes; b0 += kBatchScenes) {
    const int nb = std::min(kBatchScenes, nscenes - b0);
    PackBatchParams P{};
    for (int b = 0; b < nb; ++b) {
      P.job[b].ns = scenes[b0 + b].ns, P.job[b].st_t = scenes[b0 + b].stride_t, P.job[b].st_c = scenes[b0 + b].stride_c;
      for (int k = 0; k < scenes[b0 + b].ns; ++k) P.job[b].a[k] = scenes[b0 + b].dp[k];
    }
    P.out = out + (size_t)b0 * (size_t)count * smax;
    P.count = count, P.m = m, P.smax = smax, P.vec = vec;
    fnssl::TimedLaunch tl("scene_pack_batch", s);
    FNSSL_TRY(enqueue(s, Kernel{labels_pack_kernel, kThreads, 0, "labels_pack_kernel"},
                      dim3((unsigned)((items + kThreads - 1) / kThreads), (unsigned)nb), P));
  }
  return FNSSL_OK;
}

}  // extern "C"
