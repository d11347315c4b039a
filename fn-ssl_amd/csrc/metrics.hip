// DOA evaluation on device: getMetric.forward of both reference versions
// (FN-SSL/Lightning/Module.py:126-276, source_mode 'single' as FN-SSL uses it; IPDnet/Module.py:92-237, 'multiple').
//
// The reference evaluates in Python loops over every (utterance, segment) with .item() calls and a scipy assignment
// inside.  Here one workgroup (one wavefront) owns one utterance: its lanes walk the segments, each lane decides its
// segments completely (thresholds, the <= 4 x 4 azimuth cost matrix, the minimum-cost assignment, judge_assignment) and
// keeps integer counts and fp32 error sums; a butterfly reduction in a fixed order closes the utterance, and a second
// one-wavefront launch reduces over the utterances in a fixed order.  No float atomics: two runs give the same bits.
// The work is a few thousand flops per utterance — latency-bound and tiny by design; nothing here is tuned.
//
// Arithmetic is the reference's fp32 arithmetic in its order, so every `< ae_TH`, `> ae_TH`, `> vad_TH` is decided on
// the same fp32 value: degrees are x * 180 / pi (fp32 multiply, fp32 divide), the azimuth error is
// abs((est - gt + 180) % 360 - 180) with torch's floored remainder, the elevation error abs(est - gt), and 'aziele' the
// clamped acos form (Module.py:296-303; its cos / sin / acos are this device's, so it can differ from the host's in the
// last bits — no decision depends on it).  The true divide is the form torch gives the reference on the CPU (the G20
// fixture); run on a GPU, the reference divides through a reciprocal, so its degrees, and a decision that sits within
// one fp32 step of a threshold, can differ in the last bit from the kernel's.  Not reproduced: in 'single' the reference multiplies the error by vad_gt, so a
// NaN DOA in a SILENT slot turns its sums into NaN; here a silent slot contributes nothing.
//
// The assignment restates, in one thread and in double, the shortest-augmenting-path algorithm that
// scipy.optimize.linear_sum_assignment runs (Crouse's rectangular LSAP: rows in order, unassigned columns scanned from the
// highest index down so that of equal reduced costs the lowest column wins, a free column preferred on a tie; a matrix
// with more rows than columns is solved transposed and the pairs sorted by row).  It is not enough to find SOME optimal
// assignment: an invalid pair costs 10000 whichever row takes it, so with more ground truths than estimates optimal
// assignments tie exactly, and judge_assignment — restated AS WRITTEN (:239-246): its else branch clears
// final_assignment[i], the position in the pair list, not the pair's row — erases an earlier valid assignment for one of
// the tied choices and not for the other.  The steps below are scipy's, additions and subtractions of the same doubles
// in the same order, so exact ties fall the same way (tests/test_doa_metrics_host.py compares the restatement with
// scipy on tie-heavy matrices where scipy is installed).  Among valid pairs, totals that differ only by rounding are
// not protected: the fixtures keep them apart.
#include "host.h"

using fnssl::enqueue;
using fnssl::Kernel;

namespace {

constexpr int kMaxSrc = 4;                  // = kMaxSrc of ipdnet_step.hip
constexpr int kSlots = FNSSL_DOA_METRIC_FLOATS;
constexpr float kPi = 3.14159265358979323846f;     // float(np.pi)

struct View4 {
  const float* p;
  long long s0, s1, s2, s3;
};
struct View3 {
  const float* p;
  long long s0, s1, s2;
};

__device__ __forceinline__ float to_deg(float x, int radians) {
  return radians ? __fdiv_rn(__fmul_rn(x, 180.f), kPi) : x;                   // x * 180 / np.pi
}

__device__ __forceinline__ float azi_err(float est, float gt) {
  const float a = __fadd_rn(__fsub_rn(est, gt), 180.f);
  float m = fmodf(a, 360.f);                                                  // exact
  if (m != 0.f && m < 0.f) m = __fadd_rn(m, 360.f);                           // torch.remainder: the divisor's sign
  return fabsf(__fsub_rn(m, 180.f));
}

__device__ __forceinline__ float ele_err(float est, float gt) { return fabsf(__fsub_rn(est, gt)); }

__device__ __forceinline__ float aziele_err(float ele_e, float azi_e, float ele_g, float azi_g) {
  const float eg = __fmul_rn(__fdiv_rn(ele_g, 180.f), kPi), ag = __fmul_rn(__fdiv_rn(azi_g, 180.f), kPi);
  const float ee = __fmul_rn(__fdiv_rn(ele_e, 180.f), kPi), ae = __fmul_rn(__fdiv_rn(azi_e, 180.f), kPi);
  float aux = __fadd_rn(__fmul_rn(cosf(eg), cosf(ee)), __fmul_rn(__fmul_rn(sinf(eg), sinf(ee)), cosf(__fsub_rn(ag, ae))));
  if (aux > 0.99999f) aux = 0.99999f;
  if (aux < -0.99999f) aux = -0.99999f;
  return __fdiv_rn(__fmul_rn(fabsf(acosf(aux)), 180.f), kPi);
}

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ int wsum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// scipy.optimize.linear_sum_assignment for an ng x ne (<= 4 x 4) fp32 cost matrix; writes min(ng, ne) pairs, rows ascending
// (returned); 0 pairs if a path search runs dry, which finite costs cannot cause
__device__ int lsap(const float (*cost)[kMaxSrc], int ng, int ne, int* prow, int* pcol) {
  const bool tr = ne < ng;                               // more rows than columns: solve the transpose
  const int nr = tr ? ne : ng, nc = tr ? ng : ne;
  double u[kMaxSrc] = {0, 0, 0, 0}, v[kMaxSrc] = {0, 0, 0, 0}, spc[kMaxSrc];
  int path[kMaxSrc] = {-1, -1, -1, -1}, col4row[kMaxSrc] = {-1, -1, -1, -1}, row4col[kMaxSrc] = {-1, -1, -1, -1}, remaining[kMaxSrc];
  bool SR[kMaxSrc], SC[kMaxSrc];
  for (int cur = 0; cur < nr; ++cur) {
    // augmenting path from row cur
    double min_val = 0.0;
    int num_remaining = nc, sink = -1, i = cur;
    for (int it = 0; it < nc; ++it) remaining[it] = nc - it - 1;
    for (int k = 0; k < kMaxSrc; ++k) {
      SR[k] = SC[k] = false;
      spc[k] = INFINITY;
    }
    while (sink == -1) {
      int index = -1;
      double lowest = INFINITY;
      SR[i] = true;
      for (int it = 0; it < num_remaining; ++it) {
        const int j = remaining[it];
        const double r = min_val + (double)(tr ? cost[j][i] : cost[i][j]) - u[i] - v[j];
        if (r < spc[j]) {
          path[j] = i;
          spc[j] = r;
        }
        if (spc[j] < lowest || (spc[j] == lowest && row4col[j] == -1)) {
          lowest = spc[j];
          index = it;
        }
      }
      if (index < 0) return 0;
      min_val = lowest;
      const int j = remaining[index];
      if (row4col[j] == -1)
        sink = j;
      else
        i = row4col[j];
      SC[j] = true;
      remaining[index] = remaining[--num_remaining];
    }
    // dual update
    u[cur] += min_val;
    for (int k = 0; k < nr; ++k)
      if (SR[k] && k != cur) u[k] += min_val - spc[col4row[k]];
    for (int j = 0; j < nc; ++j)
      if (SC[j]) v[j] -= min_val - spc[j];
    // augment
    int j = sink;
    while (true) {
      const int k = path[j];
      row4col[j] = k;
      const int tmp = col4row[k];
      col4row[k] = j;
      j = tmp;
      if (k == cur) break;
    }
  }
  if (!tr) {
    for (int k = 0; k < nr; ++k) {
      prow[k] = k;
      pcol[k] = col4row[k];
    }
    return nr;
  }
  int n = 0;                                             // pairs (row = col4row[c], col = c) sorted by row
  for (int r = 0; r < nc; ++r)
    if (row4col[r] >= 0) {
      prow[n] = r;
      pcol[n] = row4col[r];
      ++n;
    }
  return n;
}

// One wavefront per utterance.  part [nb, kSlots]:
//   'multiple': the utterance's ratios  ACC, MDR, FAR, MAE(azi, ele, aziele), RMSE(azi, ele, aziele)
//   'single'  : slots 3..5 = sum of vad_gt * error (azi, ele, aziele); the counts travel in k_gt / k_corr
__global__ void __launch_bounds__(64)
doa_metrics_utt_kernel(View4 dg, View3 vg, View4 de, View3 ve, int nt, int ns_gt, int ns_est, int mode, int ae_modes,
                       float ae_th, float th_gt, float th_est, int use_vad, int gt_radians, int est_radians, int est_below,
                       float ratio_eps, float inf_cost, float eps,
                       float* __restrict__ part, int* __restrict__ k_gt, int* __restrict__ k_est, int* __restrict__ k_corr) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int n_gt = 0, n_est = 0, n_corr = 0;
  float s1[3] = {0.f, 0.f, 0.f}, s2[3] = {0.f, 0.f, 0.f};                     // sums of error, error^2: azi, ele, aziele
  for (int t = lane; t < nt; t += 64) {
    float g_ele[kMaxSrc], g_azi[kMaxSrc], e_ele[kMaxSrc], e_azi[kMaxSrc];
    bool g_on[kMaxSrc], e_on[kMaxSrc];
#pragma unroll
    for (int s = 0; s < kMaxSrc; ++s) {
      g_on[s] = e_on[s] = false;
      g_ele[s] = g_azi[s] = e_ele[s] = e_azi[s] = 0.f;
      if (s < ns_gt) {
        g_ele[s] = to_deg(dg.p[b * dg.s0 + t * dg.s1 + 0 * dg.s2 + s * dg.s3], gt_radians);
        g_azi[s] = to_deg(dg.p[b * dg.s0 + t * dg.s1 + 1 * dg.s2 + s * dg.s3], gt_radians);
        g_on[s] = use_vad ? vg.p[b * vg.s0 + t * vg.s1 + s * vg.s2] > th_gt : true;
      }
      if (s < ns_est) {
        e_ele[s] = to_deg(de.p[b * de.s0 + t * de.s1 + 0 * de.s2 + s * de.s3], est_radians);
        e_azi[s] = to_deg(de.p[b * de.s0 + t * de.s1 + 1 * de.s2 + s * de.s3], est_radians);
        if (use_vad) {                                                         // IPDnet2's activity is an MSE: active BELOW
          const float v = ve.p[b * ve.s0 + t * ve.s1 + s * ve.s2];
          e_on[s] = est_below ? v < th_est : v > th_est;
        } else {
          e_on[s] = true;
        }
      }
    }
    if (mode == FNSSL_METRIC_SINGLE) {
      // :140-173 — element-wise, source s against source s
#pragma unroll
      for (int s = 0; s < kMaxSrc; ++s) {
        if (s >= ns_gt) continue;
        const bool est_on = e_on[s] && g_on[s];
        const float ea = azi_err(e_azi[s], g_azi[s]);
        n_gt += g_on[s] ? 1 : 0;
        n_est += est_on ? 1 : 0;
        n_corr += (ea < ae_th && est_on) ? 1 : 0;
        if (g_on[s]) {                                                         // vad_gt * error (a NaN error of a silent slot
          if (ae_modes & FNSSL_AE_AZI) s1[0] += ea;                            //  would poison torch's sum: not reproduced)
          if (ae_modes & FNSSL_AE_ELE) s1[1] += ele_err(e_ele[s], g_ele[s]);
          if (ae_modes & FNSSL_AE_AZIELE) s1[2] += aziele_err(e_ele[s], e_azi[s], g_ele[s], g_azi[s]);
        }
      }
      continue;
    }
    // 'multiple' (:172-204): compact the active entries
    int gi[kMaxSrc], ei[kMaxSrc], ng = 0, ne = 0;
#pragma unroll
    for (int s = 0; s < kMaxSrc; ++s)
      if (g_on[s]) gi[ng++] = s;
#pragma unroll
    for (int s = 0; s < kMaxSrc; ++s)
      if (e_on[s] && ng > 0) ei[ne++] = s;                                     // estimates gated by "any source active"
    n_gt += ng;
    n_est += ne;
    if (ng == 0 || ne == 0) continue;
    float cost[kMaxSrc][kMaxSrc];
    for (int r = 0; r < ng; ++r)
      for (int c = 0; c < ne; ++c) {
        const float d = azi_err(e_azi[ei[c]], g_azi[gi[r]]);
        cost[r][c] = (d > ae_th || d != d) ? inf_cost : d;                     // (a NaN error makes scipy raise: invalid here)
      }
    // minimum-total-cost assignment -> the pair list as linear_sum_assignment returns it (rows ascending)
    int prow[kMaxSrc], pcol[kMaxSrc];
    const int nsml = lsap(cost, ng, ne, prow, pcol);
    // judge_assignment, as written (:239-246)
    int fin[kMaxSrc] = {-1, -1, -1, -1};
    for (int i = 0; i < nsml; ++i) {
      if (cost[prow[i]][pcol[i]] != inf_cost)
        fin[prow[i]] = pcol[i];
      else
        fin[i] = -1;
    }
    for (int r = 0; r < ng; ++r) {
      if (fin[r] < 0) continue;
      const int g = gi[r], e = ei[fin[r]];
      ++n_corr;
      if (ae_modes & FNSSL_AE_AZI) {
        const float d = azi_err(e_azi[e], g_azi[g]);
        s1[0] += d;
        s2[0] += __fmul_rn(d, d);
      }
      if (ae_modes & FNSSL_AE_ELE) {
        const float d = ele_err(e_ele[e], g_ele[g]);
        s1[1] += d;
        s2[1] += __fmul_rn(d, d);
      }
      if (ae_modes & FNSSL_AE_AZIELE) {
        const float d = aziele_err(e_ele[e], e_azi[e], g_ele[g], g_azi[g]);
        s1[2] += d;
        s2[2] += __fmul_rn(d, d);
      }
    }
  }
  n_gt = wsum(n_gt);
  n_est = wsum(n_est);
  n_corr = wsum(n_corr);
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    s1[m] = wsum(s1[m]);
    s2[m] = wsum(s2[m]);
  }
  if (lane != 0) return;
  k_gt[b] = n_gt;
  k_est[b] = n_est;
  k_corr[b] = n_corr;
  float* o = part + (size_t)b * kSlots;
  for (int i = 0; i < kSlots; ++i) o[i] = 0.f;
  if (mode == FNSSL_METRIC_SINGLE) {
    for (int m = 0; m < 3; ++m) o[3 + m] = s1[m];
    return;
  }
  const float kg = (float)n_gt, kc = (float)n_corr, ke = (float)n_est;
  const float dg_ = ratio_eps != 0.f ? __fadd_rn(kg, ratio_eps) : kg;          // IPDnet2: K_gt + 1e-6 (IPDnet2/Module.py:208-210)
  o[0] = __fdiv_rn(kc, dg_);                                                   // 0 / 0 = NaN, as in torch (:207-209)
  o[1] = __fdiv_rn(__fsub_rn(kg, kc), dg_);
  o[2] = __fdiv_rn(__fsub_rn(ke, kc), dg_);
  const float den = __fadd_rn(kc, eps);                                        // + 1e-5 here and nowhere else (:214-221)
  for (int m = 0; m < 3; ++m)
    if (ae_modes & (1 << m)) {
      o[3 + m] = __fdiv_rn(s1[m], den);
      o[6 + m] = sqrtf(__fdiv_rn(s2[m], den));
    }
}

// The batch result, one wavefront, utterances in a fixed order: 'multiple' = mean over the utterances of their ratios
// (a NaN stays a NaN); 'single' = sums over the whole batch, then the two ratios (:158-168).
__global__ void __launch_bounds__(64)
doa_metrics_batch_kernel(const float* __restrict__ part, const int* __restrict__ k_gt, const int* __restrict__ k_corr, int nb,
                         int mode, int ae_modes, float* __restrict__ metrics) {
  const int lane = threadIdx.x;
  float acc[kSlots];
  for (int i = 0; i < kSlots; ++i) acc[i] = 0.f;
  int ng = 0, nc = 0;
  for (int b = lane; b < nb; b += 64) {
    for (int i = 0; i < kSlots; ++i) acc[i] += part[(size_t)b * kSlots + i];
    ng += k_gt[b];
    nc += k_corr[b];
  }
  for (int i = 0; i < kSlots; ++i) acc[i] = wsum(acc[i]);
  ng = wsum(ng);
  nc = wsum(nc);
  if (lane != 0) return;
  for (int i = 0; i < kSlots; ++i) metrics[i] = 0.f;
  if (mode == FNSSL_METRIC_SINGLE) {
    metrics[0] = __fdiv_rn((float)nc, (float)ng);
    for (int m = 0; m < 3; ++m)
      if (ae_modes & (1 << m)) metrics[3 + m] = __fdiv_rn(acc[3 + m], (float)ng);
    return;
  }
  for (int i = 0; i < kSlots; ++i) metrics[i] = __fdiv_rn(acc[i], (float)nb);
}

}  // namespace

extern "C" int fnssl_doa_metrics_ex(const float* doa_gt, const long long* doa_gt_strides, const float* vad_gt,
                                    const long long* vad_gt_strides, const float* doa_est, const long long* doa_est_strides,
                                    const float* vad_est, const long long* vad_est_strides, int nb, int nt, int ns_gt,
                                    int ns_est, int mode, int ae_modes, float ae_th, float vad_th_gt, float vad_th_est,
                                    int use_vad, int gt_radians, int est_radians, int est_below, float ratio_eps,
                                    float large_number, float eps, float* metrics, float* per_utt, int* k_gt, int* k_est,
                                    int* k_corr, void* stream) {
  FNSSL_REQUIRE(mode == FNSSL_METRIC_SINGLE || mode == FNSSL_METRIC_MULTIPLE, "doa_metrics: unknown source mode %d", mode);
  FNSSL_REQUIRE(nb > 0 && nt > 0, "doa_metrics: %d utterances x %d segments", nb, nt);
  FNSSL_REQUIRE(ns_gt >= 1 && ns_gt <= kMaxSrc && ns_est >= 1 && ns_est <= kMaxSrc,
                "doa_metrics: %d ground-truth and %d estimated sources (1..%d each)", ns_gt, ns_est, kMaxSrc);
  FNSSL_REQUIRE(mode != FNSSL_METRIC_SINGLE || ns_gt == ns_est, "doa_metrics: 'single' compares source s with source s (%d != %d)",
                ns_gt, ns_est);
  FNSSL_REQUIRE(ae_modes > 0 && ae_modes <= (FNSSL_AE_AZI | FNSSL_AE_ELE | FNSSL_AE_AZIELE), "doa_metrics: angle-error modes %d",
                ae_modes);
  FNSSL_REQUIRE(doa_gt && doa_est && doa_gt_strides && doa_est_strides, "doa_metrics: null pointer (doa)");
  FNSSL_REQUIRE(!use_vad || (vad_gt && vad_est && vad_gt_strides && vad_est_strides), "doa_metrics: null pointer (vad)");
  FNSSL_REQUIRE(metrics && per_utt && k_gt && k_est && k_corr, "doa_metrics: null pointer (outputs)");
  FNSSL_REQUIRE(large_number > 360.f, "doa_metrics: large_number %g must exceed every angular error", (double)large_number);
  FNSSL_REQUIRE(ratio_eps >= 0.f, "doa_metrics: ratio_eps %g must not be negative", (double)ratio_eps);
  const View4 dg{doa_gt, doa_gt_strides[0], doa_gt_strides[1], doa_gt_strides[2], doa_gt_strides[3]};
  const View4 de{doa_est, doa_est_strides[0], doa_est_strides[1], doa_est_strides[2], doa_est_strides[3]};
  View3 vg{nullptr, 0, 0, 0}, ve{nullptr, 0, 0, 0};
  if (use_vad) {
    vg = View3{vad_gt, vad_gt_strides[0], vad_gt_strides[1], vad_gt_strides[2]};
    ve = View3{vad_est, vad_est_strides[0], vad_est_strides[1], vad_est_strides[2]};
  }
  hipStream_t s = fnssl::as_stream(stream);
  {
    fnssl::TimedLaunch tl("doa_metrics_utt", s);
    FNSSL_TRY(enqueue(s, Kernel{doa_metrics_utt_kernel, 64, 0, "doa_metrics_utt_kernel"}, nb, dg, vg, de, ve, nt, ns_gt, ns_est,
                      mode, ae_modes, ae_th, vad_th_gt, vad_th_est, use_vad, gt_radians, est_radians, est_below, ratio_eps,
                      large_number, eps, per_utt, k_gt, k_est, k_corr));
  }
  fnssl::TimedLaunch tl("doa_metrics_batch", s);
  return enqueue(s, Kernel{doa_metrics_batch_kernel, 64, 0, "doa_metrics_batch_kernel"}, 1, per_utt, k_gt, k_corr, nb, mode,
                 ae_modes, metrics);
}

// The entry point of before the _ex form: estimates active ABOVE their threshold, bare K_gt denominators, one unit for
// both sides.  Same kernels, same arguments, same bits.
extern "C" int fnssl_doa_metrics(const float* doa_gt, const long long* doa_gt_strides, const float* vad_gt,
                                 const long long* vad_gt_strides, const float* doa_est, const long long* doa_est_strides,
                                 const float* vad_est, const long long* vad_est_strides, int nb, int nt, int ns_gt, int ns_est,
                                 int mode, int ae_modes, float ae_th, float vad_th_gt, float vad_th_est, int use_vad,
                                 int radians, float large_number, float eps, float* metrics, float* per_utt, int* k_gt,
                                 int* k_est, int* k_corr, void* stream) {
  return fnssl_doa_metrics_ex(doa_gt, doa_gt_strides, vad_gt, vad_gt_strides, doa_est, doa_est_strides, vad_est, vad_est_strides,
                              nb, nt, ns_gt, ns_est, mode, ae_modes, ae_th, vad_th_gt, vad_th_est, use_vad, radians, radians, 0,
                              0.f, large_number, eps, metrics, per_utt, k_gt, k_est, k_corr, stream);
}
