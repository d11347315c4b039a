// The data and loss half of IPDnet's training step (reference IPDnet/runIPDnetOn.py:144-154 training_step):
//
//   pit_row_kernel      cal_loss (:196-206): frame-level permutation-invariant MSE with its gradient.  One workgroup per
//                       (utterance, segment) row: pass 1 the nsrc x nsrc error matrix E[i][j] = sum_d (pred[d, i] - gt[d, j])^2,
//                       thread 0 the best permutation, pass 2 dpred (the row, <= 2 x 28 KB at 8 microphones, comes back
//                       from L2).  pred is read through its five strides: the train-mode forward returns a permuted view.
//   pit_loss_kernel     the rows' minima summed in a fixed order (two stages, no float atomics: two runs give the same bits)
//   dp_vad_kernel       cal_vad (:224-235): mean over a segment's 12 frames x 257 bins of |direct path| / |mixture|, channel 0
//   targets_kernel      the ground-truth half of data_preprocess (:256-283): per-source DP-IPD of the reference-microphone
//                       pairs (IPDnet/Module.py:368-403), gated by the DP-VAD, silent slots = the Bessel non-source target
//
// All three are HBM- or latency-bound and small beside the network's step; they exist so that a batch of
// (waveforms, {doa, dp_signal}) becomes a loss without a host round trip.
#include "host.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

using fnssl::aligned16;
using fnssl::enqueue;
using fnssl::Kernel;

namespace {

constexpr int kSeg = FNSSL_SEG_FRAMES;   // 12
constexpr int kMaxSrc = 4;
constexpr int kMaxPairs = 63;

struct PitView {
  long long sb, st, sf, sm, ss;   // element strides of [nb, nt2, 2nf, nmic - 1, nsrc]
};

// How a chunk of 4 consecutive d (d = f * nm1 + m) is fetched.
enum { kScalar = 0, kSrcInner = 1, kDInner = 2 };
//   kSrcInner  [.., D, nsrc] contiguous per row: the chunk is 4 * nsrc consecutive floats
//   kDInner    d contiguous per source (the network's view: source stride outermost): one float4 per source

template <int N>
struct Chunk {
  float v[N][4];   // [source][k]
};

template <int N>
__device__ __forceinline__ void load_chunk(const float* __restrict__ p, const PitView& s, int kind, int nm1, int d0, int nk,
                                           Chunk<N>& c) {
  if (nk == 4 && kind == kSrcInner) {
#pragma unroll
    for (int q = 0; q < N; ++q) {          // element e = k * N + i of the chunk
      const float4 t = reinterpret_cast<const float4*>(p + (long long)d0 * N)[q];
      c.v[(4 * q) % N][(4 * q) / N] = t.x;
      c.v[(4 * q + 1) % N][(4 * q + 1) / N] = t.y;
      c.v[(4 * q + 2) % N][(4 * q + 2) / N] = t.z;
      c.v[(4 * q + 3) % N][(4 * q + 3) / N] = t.w;
    }
  } else if (nk == 4 && kind == kDInner) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const float4 t = *reinterpret_cast<const float4*>(p + i * s.ss + d0);
      c.v[i][0] = t.x, c.v[i][1] = t.y, c.v[i][2] = t.z, c.v[i][3] = t.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int d = d0 + k, f = d / nm1, m = d - f * nm1;
#pragma unroll
      for (int i = 0; i < N; ++i) c.v[i][k] = k < nk ? p[f * s.sf + m * s.sm + i * s.ss] : 0.f;
    }
  }
}

template <int N>
__device__ __forceinline__ void store_chunk(float* __restrict__ p, const PitView& s, int kind, int nm1, int d0, int nk,
                                            const Chunk<N>& c) {
  if (nk == 4 && kind == kSrcInner) {
#pragma unroll
    for (int q = 0; q < N; ++q)
      reinterpret_cast<float4*>(p + (long long)d0 * N)[q] =
          make_float4(c.v[(4 * q) % N][(4 * q) / N], c.v[(4 * q + 1) % N][(4 * q + 1) / N], c.v[(4 * q + 2) % N][(4 * q + 2) / N],
                      c.v[(4 * q + 3) % N][(4 * q + 3) / N]);
  } else if (nk == 4 && kind == kDInner) {
#pragma unroll
    for (int i = 0; i < N; ++i)
      *reinterpret_cast<float4*>(p + i * s.ss + d0) = make_float4(c.v[i][0], c.v[i][1], c.v[i][2], c.v[i][3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int d = d0 + k, f = d / nm1, m = d - f * nm1;
      if (k < nk) {
#pragma unroll
        for (int i = 0; i < N; ++i) p[f * s.sf + m * s.sm + i * s.ss] = c.v[i][k];
      }
    }
  }
}

// Chunk c of a row goes to thread c % 256 whatever the access kind, and every kind feeds the same arithmetic: a strided view
// and its contiguous copy give the same bits.
template <int N>
__global__ void __launch_bounds__(256)
pit_row_kernel(const float* __restrict__ pred, const PitView ps, int pkind, const float* __restrict__ gt, int gkind, int nt2,
               int nm1, int D, float gscale, float* __restrict__ dpred, float* __restrict__ row_min,
               int* __restrict__ perm_out) {
  __shared__ float wave_e[4][N * N];
  __shared__ float e_s[N * N];
  __shared__ int inv_s[kMaxSrc];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int b = row / nt2, t = row - b * nt2;
  const long long pbase = b * ps.sb + t * ps.st;
  const float* prow = pred + pbase;
  float* drow = dpred + pbase;
  const float* grow = gt + (long long)row * D * N;
  const PitView gs = {0, 0, (long long)nm1 * N, N, 1};
  const int nchunks = (D + 3) >> 2;

  float e[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) e[i][j] = 0.f;
  for (int c = tid; c < nchunks; c += 256) {
    const int d0 = 4 * c, nk = min(4, D - d0);
    Chunk<N> p, g;
    load_chunk<N>(prow, ps, pkind, nm1, d0, nk, p);
    load_chunk<N>(grow, gs, gkind, nm1, d0, nk, g);
#pragma unroll
    for (int k = 0; k < 4; ++k)          // lanes past the row's end hold 0 - 0
#pragma unroll
      for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const float df = p.v[i][k] - g.v[j][k];
          e[i][j] = fmaf(df, df, e[i][j]);
        }
  }
  // wave tree, then the four waves in order
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      float v = e[i][j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
      if ((tid & 63) == 0) wave_e[tid >> 6][i * N + j] = v;
    }
  __syncthreads();
  if (tid < N * N) e_s[tid] = ((wave_e[0][tid] + wave_e[1][tid]) + wave_e[2][tid]) + wave_e[3][tid];
  __syncthreads();
  if (tid == 0) {
    // itertools.permutations(range(N)) order = lexicographic in (pm[0], pm[1], ...); pm[j] = the predicted track paired
    // with target j.  The identity comes first and a later permutation must be strictly better (ties, and rows whose
    // costs are NaN, keep the earlier one).
    int idx = 0, best = 0;
    float bc = 0.f;
    for (int a = 0; a < N; ++a)
      for (int bb = 0; bb < (N > 1 ? N : 1); ++bb) {
        if (N > 1 && bb == a) continue;
        for (int cc = 0; cc < (N > 2 ? N : 1); ++cc) {
          if (N > 2 && (cc == a || cc == bb)) continue;
          for (int dd = 0; dd < (N > 3 ? N : 1); ++dd) {
            if (N > 3 && (dd == a || dd == bb || dd == cc)) continue;
            float cost = e_s[a * N];
            if (N > 1) cost += e_s[bb * N + 1];
            if (N > 2) cost += e_s[cc * N + 2];
            if (N > 3) cost += e_s[dd * N + 3];
            if (idx == 0 || cost < bc) {
              bc = cost;
              best = idx;
              inv_s[a] = 0;
              if (N > 1) inv_s[bb] = 1;
              if (N > 2) inv_s[cc] = 2;
              if (N > 3) inv_s[dd] = 3;
            }
            ++idx;
          }
        }
      }
    row_min[row] = bc;
    if (perm_out) perm_out[row] = best;
  }
  __syncthreads();
  int inv[N];                              // inv[i] = the target paired with predicted track i
#pragma unroll
  for (int i = 0; i < N; ++i) inv[i] = __builtin_amdgcn_readfirstlane(inv_s[i]);   // uniform: the selects below stay selects
  for (int c = tid; c < nchunks; c += 256) {
    const int d0 = 4 * c, nk = min(4, D - d0);
    Chunk<N> p, g, o;
    load_chunk<N>(prow, ps, pkind, nm1, d0, nk, p);
    load_chunk<N>(grow, gs, gkind, nm1, d0, nk, g);
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        unsigned gv = 0;                   // bit masks, not an indexed read: the chunk stays in registers
#pragma unroll
        for (int j = 0; j < N; ++j) gv |= __float_as_uint(g.v[j][k]) & (inv[i] == j ? 0xffffffffu : 0u);
        o.v[i][k] = gscale * (p.v[i][k] - __uint_as_float(gv));
      }
    store_chunk<N>(drow, ps, pkind, nm1, d0, nk, o);
  }
}

// *loss (+)= (sum_rows row_min) / n_total: a strided partial per thread, then a tree
__global__ void __launch_bounds__(256)
pit_loss_kernel(const float* __restrict__ row_min, int rows, float n_total, float* __restrict__ loss, int accumulate) {
  __shared__ float red[256];
  float s = 0.f;
  for (int r = threadIdx.x; r < rows; r += 256) s += row_min[r];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float v = red[0] / n_total;
    *loss = accumulate ? *loss + v : v;
  }
}

// One workgroup per (utterance, segment, source): the 12 frames x 257 bins of a segment are 3084 consecutive complex
// numbers in both spectra.  |z| as torch.abs (hypot), IEEE division: x / 0 = inf and 0 / 0 = NaN reach the mean.
__global__ void __launch_bounds__(256)
dp_vad_kernel(const float2* __restrict__ mix, const float2* __restrict__ dp, int nch, int nsrc, int nt, int nseg,
              float* __restrict__ out) {
  __shared__ float red[256];
  const int s = blockIdx.x % nsrc, bs = blockIdx.x / nsrc, seg = bs % nseg, b = bs / nseg;
  const float2* m = mix + ((long long)b * nch * nt + (long long)seg * kSeg) * FNSSL_NBIN;              // channel 0
  const float2* d = dp + (((long long)b * nsrc + s) * nt + (long long)seg * kSeg) * FNSSL_NBIN;
  float acc = 0.f;
  for (int i = threadIdx.x; i < kSeg * FNSSL_NBIN; i += 256) {
    const float2 a = d[i], c = m[i];
    acc += hypotf(a.x, a.y) / hypotf(c.x, c.y);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0] / (float)(kSeg * FNSSL_NBIN);
}

// One workgroup per (utterance, segment).  The delay tau_m = r(doa) . (mic_0 - mic_m) / speed is formed in float32 — the
// reference hands DPIPD.forward float32 DOAs and a float32 array (Module.py:380-388) — and the phase 2 pi f_k tau_m in
// double like numpy's (:389-393); cos | sin are rounded to float32 once.
__global__ void __launch_bounds__(256)
targets_kernel(const float* __restrict__ doa, const float* __restrict__ vad, const float* __restrict__ mic,
               const float* __restrict__ non_source, int nsrc, int nm1, int bin0, int nf_used, int nbins, float fre_max,
               float speed, float th, float* __restrict__ ipd) {
  __shared__ double tau_s[kMaxSrc * kMaxPairs];
  __shared__ int gate_s[kMaxSrc];          // 0: DP-IPD, 1: non-source target, 2: NaN
  const int bs = blockIdx.x, tid = threadIdx.x;
  if (tid < nsrc) {
    int g = 0;
    if (vad) {
      const float v = vad[(long long)bs * nsrc + tid];
      g = v > th ? 0 : (v <= th ? 1 : 2);
    }
    gate_s[tid] = g;
  }
  for (int i = tid; i < nsrc * nm1; i += 256) {
    const int s = i / nm1, m = i - s * nm1 + 1;
    const float ele = doa[((long long)bs * 2 + 0) * nsrc + s], azi = doa[((long long)bs * 2 + 1) * nsrc + s];
    const float se = (float)sin((double)ele), ce = (float)cos((double)ele), sa = (float)sin((double)azi),
                ca = (float)cos((double)azi);
    const float rx = __fmul_rn(se, ca), ry = __fmul_rn(se, sa), rz = ce;
    const float dx = __fsub_rn(mic[0], mic[m * 3]), dy = __fsub_rn(mic[1], mic[m * 3 + 1]), dz = __fsub_rn(mic[2], mic[m * 3 + 2]);
    const float dot = __fadd_rn(__fadd_rn(__fmul_rn(rx, dx), __fmul_rn(ry, dy)), __fmul_rn(rz, dz));
    tau_s[s * nm1 + (m - 1)] = (double)__fdiv_rn(dot, speed);
  }
  __syncthreads();
  const double two_pi = 6.283185307179586476925286766559;
  const double step = (double)fre_max / (double)(nbins - 1);                    // np.linspace(0, fre_max, nbins)
  const int per_bin = nm1 * nsrc;
  float* o = ipd + (long long)bs * 2 * nf_used * per_bin;
  for (int i = tid; i < nf_used * per_bin; i += 256) {
    const int k = i / per_bin, r = i - k * per_bin, m = r / nsrc, s = r - m * nsrc;
    const int g = gate_s[s];
    float re, im;
    if (g == 0) {
      double sn, cs;
      sincos((two_pi * ((double)(bin0 + k) * step)) * tau_s[s * nm1 + m], &sn, &cs);
      re = (float)cs, im = (float)sn;
    } else if (g == 1) {
      re = non_source[(long long)k * nm1 + m], im = non_source[(long long)(nf_used + k) * nm1 + m];
    } else {
      re = im = __builtin_nanf("");
    }
    o[i] = re;
    o[(long long)nf_used * per_bin + i] = im;
  }
}

// IPDnet2's near-field targets (DPIPD2.forward(source_doa, source_distance), IPDnet2/Module.py:443-483, as
// run_IPDnet2.py:290-328 drives it).  One workgroup per (utterance, frame).  Where the chain rounds, for fp32 DOAs and
// distances and a float64 microphone table, is where numpy rounds it:
//   fp32    sin / cos of the DOA (np.sin of a float32 array is float32; here the correctly rounded value), then the source
//           position x = (d * sin ele) * cos azi, y = (d * sin ele) * sin azi, z = d * cos ele, one fp32 product at a time
//   double  position - microphone, the norm sqrt((dx^2 + dy^2) + dz^2) with no fused multiply-add, tau_m = (|src - mic_m|
//           - |src - mic_0|) / speed, the phase (2 pi f_k) tau_m
//   fp32    cos | sin of the phase, rounded once (.astype(np.float32), run_IPDnet2.py:303)
__global__ void __launch_bounds__(256)
targets2_kernel(const float* __restrict__ doa, const float* __restrict__ distance, const float* __restrict__ vad,
                const double* __restrict__ mic, const float* __restrict__ non_source, int nsrc, int nm1, int bin0, int nf_used,
                int nbins, float fre_max, float speed, float th, float* __restrict__ ipd) {
  __shared__ double dist_s[kMaxSrc * (kMaxPairs + 1)];   // [source][microphone]
  __shared__ double tau_s[kMaxSrc * kMaxPairs];
  __shared__ int gate_s[kMaxSrc];          // 0: DP-IPD, 1: non-source target, 2: NaN
  const int bs = blockIdx.x, tid = threadIdx.x, nmic = nm1 + 1;
  if (tid < nsrc) {
    int g = 0;
    if (vad) {
      const float v = vad[(long long)bs * nsrc + tid];
      g = v > th ? 0 : (v <= th ? 1 : 2);
    }
    gate_s[tid] = g;
  }
  for (int i = tid; i < nsrc * nmic; i += 256) {
    const int s = i / nmic, m = i - s * nmic;
    const float ele = doa[((long long)bs * 2 + 0) * nsrc + s], azi = doa[((long long)bs * 2 + 1) * nsrc + s];
    const float d = distance[(long long)bs * nsrc + s];
    const float se = (float)sin((double)ele), ce = (float)cos((double)ele), sa = (float)sin((double)azi),
                ca = (float)cos((double)azi);
    const float dse = __fmul_rn(d, se);
    const float x = __fmul_rn(dse, ca), y = __fmul_rn(dse, sa), z = __fmul_rn(d, ce);
    const double dx = __dsub_rn((double)x, mic[m * 3]), dy = __dsub_rn((double)y, mic[m * 3 + 1]),
                 dz = __dsub_rn((double)z, mic[m * 3 + 2]);
    dist_s[s * nmic + m] = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
  }
  __syncthreads();
  for (int i = tid; i < nsrc * nm1; i += 256) {
    const int s = i / nm1, m = i - s * nm1;
    tau_s[i] = __ddiv_rn(__dsub_rn(dist_s[s * nmic + m + 1], dist_s[s * nmic]), (double)speed);
  }
  __syncthreads();
  const double two_pi = 6.283185307179586476925286766559;
  const double step = (double)fre_max / (double)(nbins - 1);                    // np.linspace(0, fre_max, nbins)
  const int per_bin = nm1 * nsrc;
  float* o = ipd + (long long)bs * 2 * nf_used * per_bin;
  for (int i = tid; i < nf_used * per_bin; i += 256) {
    const int k = i / per_bin, r = i - k * per_bin, m = r / nsrc, s = r - m * nsrc;
    const int g = gate_s[s];
    float re, im;
    if (g == 0) {
      double sn, cs;
      sincos(__dmul_rn(__dmul_rn(two_pi, __dmul_rn((double)(bin0 + k), step)), tau_s[s * nm1 + m]), &sn, &cs);
      re = (float)cs, im = (float)sn;
    } else if (g == 1) {
      re = non_source[(long long)k * nm1 + m], im = non_source[(long long)(nf_used + k) * nm1 + m];
    } else {
      re = im = __builtin_nanf("");
    }
    o[i] = re;
    o[(long long)nf_used * per_bin + i] = im;
  }
}


}  // namespace

extern "C" {

size_t fnssl_pit_mse_workspace_bytes(int rows) { return rows > 0 ? ((size_t)rows * sizeof(float) + 255) / 256 * 256 : 0; }

int fnssl_pit_mse_loss(const float* pred, const long long* pred_strides, const float* gt, int nb, int nt2, int nf2, int nm1,
                       int nsrc, long long n_total, float* dpred, float* loss, int accumulate, int* perm_out,
                       void* workspace, size_t workspace_bytes, void* stream) {
  FNSSL_REQUIRE(pred && pred_strides && gt && dpred && loss, "pit_mse_loss: null pointer");
  FNSSL_REQUIRE(nsrc >= 1 && nsrc <= kMaxSrc, "pit_mse_loss: %d sources (1..%d)", nsrc, kMaxSrc);
  FNSSL_REQUIRE(nb > 0 && nt2 > 0 && nf2 > 0 && nm1 > 0, "pit_mse_loss: empty problem (nb %d, segments %d, D = %d x %d)", nb, nt2,
                nf2, nm1);
  const long long rows = (long long)nb * nt2, D = (long long)nf2 * nm1;
  FNSSL_REQUIRE(rows <= 0x7fffffffLL && D * nsrc <= 0x7fffffffLL, "pit_mse_loss: %lld rows x %lld elements is out of range", rows,
                D * nsrc);
  FNSSL_REQUIRE(n_total >= rows * D * nsrc, "pit_mse_loss: n_total %lld is less than the %lld elements passed", n_total,
                rows * D * nsrc);
  // dpred is written through the same strides: they must describe distinct elements
  const int ext[5] = {nb, nt2, nf2, nm1, nsrc};
  int order[5] = {0, 1, 2, 3, 4};
  std::sort(order, order + 5, [&](int a, int b) { return pred_strides[a] < pred_strides[b]; });
  long long span = 1;
  for (int q = 0; q < 5; ++q) {
    const int d = order[q];
    if (ext[d] == 1) continue;
    FNSSL_REQUIRE(pred_strides[d] >= span, "pit_mse_loss: pred strides (%lld, %lld, %lld, %lld, %lld) overlap or are not positive",
                  pred_strides[0], pred_strides[1], pred_strides[2], pred_strides[3], pred_strides[4]);
    span = pred_strides[d] * ext[d];
  }
  FNSSL_REQUIRE(workspace && workspace_bytes >= fnssl_pit_mse_workspace_bytes((int)rows),
                "pit_mse_loss: workspace too small (%zu bytes, need %zu)", workspace_bytes, fnssl_pit_mse_workspace_bytes((int)rows));
  PitView ps = {nb > 1 ? pred_strides[0] : 0, nt2 > 1 ? pred_strides[1] : 0, nf2 > 1 ? pred_strides[2] : 0,
                nm1 > 1 ? pred_strides[3] : 0, nsrc > 1 ? pred_strides[4] : 0};
  // 16-byte accesses where every chunk of 4 d starts on a 16-byte boundary
  const bool rows16 = aligned16(pred) && aligned16(dpred) && ps.sb % 4 == 0 && ps.st % 4 == 0 && D >= 4;
  const bool d_contig = (nm1 == 1 || ps.sm == 1) && (nf2 == 1 || ps.sf == nm1);
  const bool src_inner = (nsrc == 1 || ps.ss == 1) && (nm1 == 1 || ps.sm == nsrc) && (nf2 == 1 || ps.sf == (long long)nm1 * nsrc);
  int pkind = kScalar;
  if (rows16 && src_inner) pkind = kSrcInner;
  else if (rows16 && d_contig && ps.ss % 4 == 0) pkind = kDInner;
  const int gkind = aligned16(gt) && (D * nsrc) % 4 == 0 && D >= 4 ? kSrcInner : kScalar;
  hipStream_t st = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl("pit_mse", st);
  float* row_min = static_cast<float*>(workspace);
  const float gscale = 2.0f / (float)n_total;
  FNSSL_TRY(fnssl::with_value<1, 2, 3, 4>(nsrc, [&](auto N) {
    return enqueue(st, Kernel{pit_row_kernel<N>, 256, 0, "pit_row_kernel"}, (unsigned)rows, pred, ps, pkind, gt, gkind, nt2, nm1, (int)D,
                   gscale, dpred, row_min, perm_out);
  }));
  return enqueue(st, Kernel{pit_loss_kernel, 256, 0, "pit_loss_kernel"}, 1, row_min, (int)rows, (float)n_total, loss, accumulate);
}

int fnssl_dp_vad(const float* mix_spec, const float* dp_spec, int nb, int nch, int nsrc, int nt, float* dp_vad, void* stream) {
  FNSSL_REQUIRE(mix_spec && dp_spec && dp_vad, "dp_vad: null pointer");
  FNSSL_REQUIRE(nb > 0 && nch > 0 && nsrc > 0 && nt >= kSeg, "dp_vad: nb %d channels %d sources %d frames %d (at least %d)", nb, nch,
                nsrc, nt, kSeg);
  const int nseg = nt / kSeg;
  FNSSL_REQUIRE((long long)nb * nseg * nsrc <= 0x7fffffffLL, "dp_vad: %d x %d x %d outputs is out of range", nb, nseg, nsrc);
  hipStream_t st = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl("dp_vad", st);
  return enqueue(st, Kernel{dp_vad_kernel, 256, 0, "dp_vad_kernel"}, nb * nseg * nsrc, reinterpret_cast<const float2*>(mix_spec),
                 reinterpret_cast<const float2*>(dp_spec), nch, nsrc, nt, nseg, dp_vad);
}

int fnssl_ipdnet_targets(const float* doa, const float* dp_vad, int nb, int nseg, int nsrc, const float* mic_loc, int nmic,
                         const float* non_source, int bin0, int nf_used, int nbins, float fre_max, float speed, float vad_th,
                         float* ipd, void* stream) {
  FNSSL_REQUIRE(doa && mic_loc && ipd && (non_source || !dp_vad), "ipdnet_targets: null pointer");
  FNSSL_REQUIRE(nb > 0 && nseg > 0 && (long long)nb * nseg <= 0x7fffffffLL, "ipdnet_targets: nb %d segments %d", nb, nseg);
  FNSSL_REQUIRE(nsrc >= 1 && nsrc <= kMaxSrc, "ipdnet_targets: %d sources (1..%d)", nsrc, kMaxSrc);
  FNSSL_REQUIRE(nmic >= 2 && nmic - 1 <= kMaxPairs, "ipdnet_targets: %d microphones (2..%d)", nmic, kMaxPairs + 1);
  FNSSL_REQUIRE(nbins >= 2 && bin0 >= 0 && nf_used >= 1 && bin0 + nf_used <= nbins && fre_max > 0.f && speed > 0.f,
                "ipdnet_targets: bins [%d, %d) of %d, fre_max %g, speed %g", bin0, bin0 + nf_used, nbins, (double)fre_max,
                (double)speed);
  FNSSL_REQUIRE(vad_th == vad_th, "ipdnet_targets: the VAD threshold is NaN");
  hipStream_t st = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl("ipdnet_targets", st);
  return enqueue(st, Kernel{targets_kernel, 256, 0, "targets_kernel"}, nb * nseg, doa, dp_vad, mic_loc, non_source, nsrc,
                 nmic - 1, bin0, nf_used, nbins, fre_max, speed, vad_th, ipd);
}

int fnssl_ipdnet2_targets(const float* doa, const float* distance, const float* vad, int nb, int nseg, int nsrc,
                          const double* mic_loc, int nmic, const float* non_source, int bin0, int nf_used, int nbins,
                          float fre_max, float speed, float vad_th, float* ipd, void* stream) {
  FNSSL_REQUIRE(doa && distance && mic_loc && ipd && (non_source || !vad), "ipdnet2_targets: null pointer");
  FNSSL_REQUIRE(nb > 0 && nseg > 0 && (long long)nb * nseg <= 0x7fffffffLL, "ipdnet2_targets: nb %d frames %d", nb, nseg);
  FNSSL_REQUIRE(nsrc >= 1 && nsrc <= kMaxSrc, "ipdnet2_targets: %d sources (1..%d)", nsrc, kMaxSrc);
  FNSSL_REQUIRE(nmic >= 2 && nmic - 1 <= kMaxPairs, "ipdnet2_targets: %d microphones (2..%d)", nmic, kMaxPairs + 1);
  FNSSL_REQUIRE(nbins >= 2 && bin0 >= 0 && nf_used >= 1 && bin0 + nf_used <= nbins && fre_max > 0.f && speed > 0.f,
                "ipdnet2_targets: bins [%d, %d) of %d, fre_max %g, speed %g", bin0, bin0 + nf_used, nbins, (double)fre_max,
                (double)speed);
  FNSSL_REQUIRE(vad_th == vad_th, "ipdnet2_targets: the VAD threshold is NaN");
  hipStream_t st = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl("ipdnet2_targets", st);
  return enqueue(st, Kernel{targets2_kernel, 256, 0, "targets2_kernel"}, nb * nseg, doa, distance, vad, mic_loc, non_source, nsrc,
                 nmic - 1, bin0, nf_used, nbins, fre_max, speed, vad_th, ipd);
}

}  // extern "C"
