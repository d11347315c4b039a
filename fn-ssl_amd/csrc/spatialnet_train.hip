// Backward of one IPDnet2 Mamba block (fnssl_sn_mamba_backward; forward: fnssl_sn_mamba in spatialnet.hip), fp32, whole
// sequences from zero state.  The forward's workspace (xz | dbl | y) is the saved state; everything else is recomputed.
//
//   out     dO = broadcast of dout over its pooling window / pool (0 past the last whole window);  dy = dO . W_out
//           — matrix pipe, W_out resident in LDS, points on the lanes as in the forward kernels
//   scan    one workgroup per sequence, two lanes per inner channel (8 states each).  h_{t-1} is needed going backwards and the
//           recurrence cannot be inverted (the decay underflows on purpose), so a first pass walks the sequence forwards
//           and stores h every TC steps; the second pass walks the chunks last to first, rebuilds the chunk's h_t from its
//           checkpoint into registers (TC x 8 per lane) and runs the reverse recurrence over them.  The 38 sums over
//           the 192 channels that a step owes (d delta, dB, dC) are staged transposed in LDS, SB steps at a time, and added
//           up by one thread per (step, value) in channel order: one barrier pair per SB steps, no atomics.
//           dD, dA, dW_dt, db_dt stay in registers over the sequence and leave as per-sequence partials.
//   xproj   du += ddbl . W_x on the matrix pipe; then the depthwise conv's backward, one workgroup per sequence: dpre = du .
//           SiLU'(pre), the anti-causal dxi, dw_c / db_c partials per sequence, and u for dW_x
//   in      dln = [dxi | dz] . W_in on the matrix pipe, LayerNorm backward (mean / rstd recomputed from x) and the
//           residual's dO fused behind it; d gamma / d beta leave as per-workgroup partials
//   wgrad   dW_out^T = y^T dO, dW_x^T = u^T ddbl, dW_in^T = ln^T [dxi | dz]: split-K v_mfma_f32_16x16x4_f32 over the
//           points, partial tiles to a slab per split, slabs and every partial above added in a fixed order
// Gradients are written (not accumulated) and bitwise reproducible: no float atomics anywhere.
#include <algorithm>

#include "spatialnet_common.h"

namespace {

constexpr int TC = 8;              // steps between two checkpoints of h = steps whose h_t a lane rebuilds at once
constexpr int SB = 4;               // steps per batch of cross-channel sums (SB * NV * (E + 1) floats of LDS)
constexpr int NH = NST / 2;         // states per lane of the reverse scan (two lanes per channel)
constexpr int NV = RK + 2 * NST;    // sums per step: d delta (6) | dB (16) | dC (16), the column order of dbl
constexpr int LDV = E + 1;          // row of the sum image: one pad float, so that the summing threads hit 32 banks
constexpr int KX = 48;              // the 40 dbl columns as whole 16-wide k groups
constexpr int kLnParts = 256;       // most workgroups of the `in` kernel = rows of its d gamma / d beta partials
constexpr int kMaxSplits = 256;     // most point slabs of a weight-gradient product
constexpr int kSeqPart = E * (NST + 1 + RK + 1);   // per-sequence partials of the scan: dA | dD | dW_dt | db_dt
constexpr int kConvPart = E * (KC + 1);            // of the conv backward: dw_c | db_c
constexpr float kLog2e = 1.44269504088896340736f;

static_assert(TC % SB == 0 && SB * XP <= E, "one summing thread per (step, value) of a batch");

// softplus as the forward scan computes it, and its derivative branch by branch
__device__ __forceinline__ float softplus_fwd(float dtv) {
  float dt = dtv;
  if (dtv <= 20.f) {
    const float ex = __expf(dtv), u1 = 1.f + ex;
    dt = u1 == 1.f ? ex : __logf(u1) * __fdividef(ex, u1 - 1.f);
  }
  return dt;
}
__device__ __forceinline__ float softplus_bwd(float dtv) {
  float d = 1.f;
  if (dtv <= 20.f) {
    const float ex = __expf(dtv), u1 = 1.f + ex;
    d = u1 == 1.f ? ex : __fdividef(ex, u1);
  }
  return d;
}
__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }

// ---------------------------------------------------------------------------------------------------------
// out: dO[p, 0:96] and dy[p, 0:192] = dO . W_out,  p = (b*nf + f)*nt + t
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(512)
sn_mamba_bwd_out_kernel(const float* __restrict__ dout, long long d_sb, long long d_st, long long d_sf, int nt, int nt2,
                        int nf, int tp, long long npts, const float* __restrict__ woT, float* __restrict__ dO,
                        float* __restrict__ dy) {
  extern __shared__ __attribute__((aligned(16))) float ldsw[];     // 12 tiles x 6 groups x 1 KiB
  fill_w_lds_strided<H, E, 512>(ldsw, woT, 1, H, H, E);             // W[k = h][o = e] = woT[e][h]
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = lane & 15, kq = lane >> 4;
  const float* ldsw_lane = ldsw + lane * 4;
  const long long ntiles = (npts + 15) / 16;
  const float inv = 1.f / (float)tp;
  for (long long tile = (long long)blockIdx.x * 8 + w; tile < ntiles; tile += (long long)gridDim.x * 8) {
    const long long p = tile * 16 + n;
    const long long pc = p < npts ? p : npts - 1;
    int t, f;
    const long long b = divmod(divmod(pc, nt, t), nf, f);
    const int t2 = t / tp;
    const bool live = t2 < nt2;                                     // frames past the last whole window get no gradient
    const float4* row = reinterpret_cast<const float4*>(dout + b * d_sb + (long long)t2 * d_st + f * d_sf + kq * (H / 4));
    float a[H / 4];
#pragma unroll
    for (int i = 0; i < H / 16; ++i) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live) v = row[i];
      a[4 * i] = v.x * inv;
      a[4 * i + 1] = v.y * inv;
      a[4 * i + 2] = v.z * inv;
      a[4 * i + 3] = v.w * inv;
    }
    if (p < npts) {
      float4* dst = reinterpret_cast<float4*>(dO + p * H + kq * (H / 4));
#pragma unroll
      for (int i = 0; i < H / 16; ++i) dst[i] = make_float4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]);
    }
    float* dst = dy + p * E + 4 * kq;
#pragma unroll 1
    for (int j0 = 0; j0 < E / 16; j0 += 4) {
      v4f_t acc[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) acc[jj] = v4f_t{0.f, 0.f, 0.f, 0.f};
      mfma_tiles<H, 4>(a, ldsw_lane, j0, acc);
      if (p < npts) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
          *reinterpret_cast<float4*>(dst + 16 * (j0 + jj)) = make_float4(acc[jj][0], acc[jj][1], acc[jj][2], acc[jj][3]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// scan: the reverse recurrence.  dyu holds dy on entry and du (the scan's share: dys D + dt sum_n g B) on exit.
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(2 * E)
sn_mamba_bwd_scan_kernel(const float* __restrict__ xz, const float* __restrict__ dbl, float* dyu, int nt,
                         const float* __restrict__ conv_w, const float* __restrict__ conv_b,
                         const float* __restrict__ wdt, const float* __restrict__ bdt, const float* __restrict__ a,
                         const float* __restrict__ dpar, float* __restrict__ dxz, float* __restrict__ ddbl,
                         float* ckpt, float* __restrict__ pseq) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* sdbl = lds;                      // [TC][XP]: the chunk's dbl rows, read as broadcasts
  float* ssum = lds + TC * XP;            // [SB * NV][LDV]: the lanes' terms of a batch of sums, transposed
  const long long s = blockIdx.x;
  // two neighbouring lanes per channel, NH states each: half the history per lane.  What a step sums over the 16 states
  // (ys, the B and ddt sums) is completed by one swap inside the pair; everything per channel is computed by both lanes
  // (bit-equal: a + b = b + a) and stored by the even one.
  const int tid = threadIdx.x, e = tid >> 1, half = tid & 1, n0 = half * NH;
  const int nch = (nt + TC - 1) / TC;
  float A[NH], wd[RK], wdh[RK / 2], cw[KC];
#pragma unroll
  for (int n = 0; n < NH; ++n) A[n] = a[e * NST + n0 + n];
#pragma unroll
  for (int r = 0; r < RK; ++r) wd[r] = wdt[e * RK + r];
#pragma unroll
  for (int r = 0; r < RK / 2; ++r) wdh[r] = wdt[e * RK + half * (RK / 2) + r];   // the lane's three d delta terms
#pragma unroll
  for (int k = 0; k < KC; ++k) cw[k] = conv_w[e * KC + k];
  const float cb = conv_b[e], bd = bdt[e], dp = dpar[e];
  const float* xrow = xz + s * nt * (2 * E) + e;
  const float* drow = dbl + s * nt * XP;
  float* dyrow = dyu + s * nt * E + e;
  float* ck = ckpt + s * nch * (NST * E) + n0 * E + e;   // [chunk][n][e]: h before the chunk's first step

  // the chunk's dbl rows -> LDS (rows past the sequence as zeros)
  auto stage = [&](int t0) {
    for (int i = tid; i < TC * XP / 4; i += 2 * E) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t0 + (4 * i) / XP < nt) v = *reinterpret_cast<const float4*>(drow + (long long)t0 * XP + 4 * i);
      *reinterpret_cast<float4*>(sdbl + 4 * i) = v;
    }
  };
  // xi of the chunk's frames and of the three before it (zeros outside the sequence)
  auto load_xi = [&](int t0, float (&xi)[TC + KC - 1]) {
#pragma unroll
    for (int j = 0; j < TC + KC - 1; ++j) {
      const int t = t0 - (KC - 1) + j;
      xi[j] = (t >= 0 && t < nt) ? xrow[(long long)t * (2 * E)] : 0.f;
    }
  };
  // one step's u, dtv (as the forward scan forms them)
  auto step_in = [&](const float (&xi)[TC + KC - 1], int j, float& u, float& dtv) {
    float v = cb;
    v = fmaf(cw[0], xi[j], v);
    v = fmaf(cw[1], xi[j + 1], v);
    v = fmaf(cw[2], xi[j + 2], v);
    v = fmaf(cw[3], xi[j + 3], v);
    u = silu_f(v);
    dtv = bd;
#pragma unroll
    for (int r = 0; r < RK; ++r) dtv = fmaf(wd[r], sdbl[j * XP + r], dtv);
  };
  auto pair_sum = [](float v) { return v + dpp_f<0xB1>(v); };       // quad_perm [1, 0, 3, 2]: the other lane of the pair

  // ---- pass 1: forwards, h checkpointed at every chunk boundary (the last chunk is rebuilt in pass 2 anyway)
  {
    float h[NH];
#pragma unroll
    for (int n = 0; n < NH; ++n) h[n] = 0.f;
    for (int c = 0; c + 1 < nch; ++c) {
      const int t0 = c * TC;
      stage(t0);
      float xi[TC + KC - 1];
      load_xi(t0, xi);
      __syncthreads();
#pragma unroll
      for (int j = 0; j < TC; ++j) {
        float u, dtv;
        step_in(xi, j, u, dtv);
        const float dt = softplus_fwd(dtv), dtu = dt * u;
#pragma unroll
        for (int n = 0; n < NH; ++n)
          h[n] = fmaf(__builtin_amdgcn_exp2f(dt * (A[n] * kLog2e)), h[n], dtu * sdbl[j * XP + RK + n0 + n]);
      }
#pragma unroll
      for (int n = 0; n < NH; ++n) ck[((long long)(c + 1) * NST + n) * E] = h[n];
      __syncthreads();                                   // every lane is done with sdbl before the next chunk's rows land
    }
  }

  // ---- pass 2: chunks last to first
  float g[NH], dA[NH], dwd[RK];                          // g: exp(dt_{t+1} A) g_{t+1}, the carry into step t
#pragma unroll
  for (int n = 0; n < NH; ++n) g[n] = dA[n] = 0.f;
#pragma unroll
  for (int r = 0; r < RK; ++r) dwd[r] = 0.f;
  float dD = 0.f, dbd = 0.f;
  for (int c = nch - 1; c >= 0; --c) {
    const int t0 = c * TC;
    stage(t0);
    float h0[NH], xi[TC + KC - 1], z[TC], dyv[TC];
#pragma unroll
    for (int n = 0; n < NH; ++n) h0[n] = c > 0 ? ck[((long long)c * NST + n) * E] : 0.f;
    load_xi(t0, xi);
#pragma unroll
    for (int j = 0; j < TC; ++j) {
      const bool in = t0 + j < nt;
      z[j] = in ? xrow[(long long)(t0 + j) * (2 * E) + E] : 0.f;
      dyv[j] = in ? dyrow[(long long)(t0 + j) * E] : 0.f;
    }
    __syncthreads();
    float hist[TC][NH], u[TC], dtv[TC], dt[TC];
#pragma unroll
    for (int j = 0; j < TC; ++j) {
      step_in(xi, j, u[j], dtv[j]);
      dt[j] = softplus_fwd(dtv[j]);
      const float dtu = dt[j] * u[j];
      const bool in = t0 + j < nt;
#pragma unroll
      for (int n = 0; n < NH; ++n) {
        const float hp = j ? hist[j ? j - 1 : 0][n] : h0[n];
        const float hn = fmaf(__builtin_amdgcn_exp2f(dt[j] * (A[n] * kLog2e)), hp, dtu * sdbl[j * XP + RK + n0 + n]);
        hist[j][n] = in ? hn : hp;
      }
    }
#pragma unroll
    for (int j = TC - 1; j >= 0; --j) {
      const int t = t0 + j;
      if (t < nt) {
        const float* row = sdbl + j * XP;
        const float *rb = row + RK + n0, *rc = row + RK + NST + n0;    // the lane's B_t and C_t
        float* sj = ssum + (j % SB) * NV * LDV + e;
        float ys = 0.f;
#pragma unroll
        for (int n = 0; n < NH; ++n) ys = fmaf(hist[j][n], rc[n], ys);
        ys = fmaf(dp, u[j], pair_sum(ys));
        const float sg = sigmoid_f(z[j]);
        const float dys = dyv[j] * (z[j] * sg);
        if (!half) dxz[(s * nt + t) * (2 * E) + E + e] = dyv[j] * ys * (sg * fmaf(z[j], 1.f - sg, 1.f));
        dD = fmaf(dys, u[j], dD);
        const float dtu = dt[j] * u[j];
        // the decays are formed again, from a copy of dt the compiler cannot match with the rebuild's: kept from there, the
        // chunk's 64 decays cost 64 registers and the kernel spills 60
        float dtr = dt[j];
        asm volatile("" : "+v"(dtr));
        float sgb = 0.f, sddt = 0.f;
#pragma unroll
        for (int n = 0; n < NH; ++n) {
          const float bn = rb[n];
          const float gn = fmaf(dys, rc[n], g[n]);
          const float dec = __builtin_amdgcn_exp2f(dtr * (A[n] * kLog2e));
          const float hpd = (j ? hist[j ? j - 1 : 0][n] : h0[n]) * dec;
          sgb = fmaf(gn, bn, sgb);
          sddt = fmaf(gn, fmaf(hpd, A[n], u[j] * bn), sddt);
          dA[n] = fmaf(gn * hpd, dt[j], dA[n]);
          sj[(RK + n0 + n) * LDV] = gn * dtu;                         // dB_t[n]
          sj[(RK + NST + n0 + n) * LDV] = dys * hist[j][n];           // dC_t[n]
          g[n] = dec * gn;
        }
        sgb = pair_sum(sgb);
        sddt = pair_sum(sddt);
        if (!half) dyrow[(long long)t * E] = fmaf(dt[j], sgb, dys * dp);
        const float ddtv = sddt * softplus_bwd(dtv[j]);
        dbd += ddtv;
#pragma unroll
        for (int r = 0; r < RK; ++r) dwd[r] = fmaf(ddtv, row[r], dwd[r]);
#pragma unroll
        for (int r = 0; r < RK / 2; ++r) sj[(half * (RK / 2) + r) * LDV] = ddtv * wdh[r];   // d delta_t[r]
      }
      if (j % SB == 0 && t < nt) {                                    // (uniform) the batch j .. j + SB - 1 is staged
        __syncthreads();
        if (tid < SB * XP) {
          const int jj = tid / XP, v = tid - jj * XP;
          if (t + jj < nt) {
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            if (v < NV) {
              const float* col = ssum + (jj * NV + v) * LDV;
#pragma unroll 4
              for (int k = 0; k < E; k += 4) {
                s0 += col[k];
                s1 += col[k + 1];
                s2 += col[k + 2];
                s3 += col[k + 3];
              }
            }
            ddbl[(s * nt + t + jj) * XP + v] = (s0 + s1) + (s2 + s3);   // the two pad columns as zeros
          }
        }
        __syncthreads();
      }
    }
  }
  float* ps = pseq + s * kSeqPart;
#pragma unroll
  for (int n = 0; n < NH; ++n) ps[e * NST + n0 + n] = dA[n];
  if (!half) {
    ps[E * NST + e] = dD;
#pragma unroll
    for (int r = 0; r < RK; ++r) ps[E * (NST + 1) + e * RK + r] = dwd[r];
    ps[E * (NST + 1 + RK) + e] = dbd;
  }
}

// ---------------------------------------------------------------------------------------------------------
// xproj: du[p, 0:192] += ddbl[p, 0:40] . W_x
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(512)
sn_mamba_bwd_xproj_kernel(const float* __restrict__ ddbl, long long npts, const float* __restrict__ wxT, float* du) {
  extern __shared__ __attribute__((aligned(16))) float ldsw[];     // 12 tiles x 3 groups x 1 KiB
  fill_w_lds_strided<KX, E, 512>(ldsw, wxT, 1, XP, NV, E);          // W[k = v][o = e] = wxT[e][v]
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = lane & 15, kq = lane >> 4;
  const float* ldsw_lane = ldsw + lane * 4;
  const long long ntiles = (npts + 15) / 16;
  for (long long tile = (long long)blockIdx.x * 8 + w; tile < ntiles; tile += (long long)gridDim.x * 8) {
    const long long p = tile * 16 + n;
    const long long pc = p < npts ? p : npts - 1;
    const float* row = ddbl + pc * XP + kq * (KX / 4);
    float a[KX / 4];
#pragma unroll
    for (int i = 0; i < KX / 16; ++i) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kq * (KX / 4) + 4 * i < XP) v = *reinterpret_cast<const float4*>(row + 4 * i);
      a[4 * i] = v.x;
      a[4 * i + 1] = v.y;
      a[4 * i + 2] = v.z;
      a[4 * i + 3] = v.w;
    }
    float* dst = du + p * E + 4 * kq;
#pragma unroll 1
    for (int j0 = 0; j0 < E / 16; j0 += 4) {
      v4f_t acc[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) acc[jj] = v4f_t{0.f, 0.f, 0.f, 0.f};
      mfma_tiles<KX, 4>(a, ldsw_lane, j0, acc);
      if (p < npts) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          float4* d4 = reinterpret_cast<float4*>(dst + 16 * (j0 + jj));
          const float4 v = *d4;
          *d4 = make_float4(v.x + acc[jj][0], v.y + acc[jj][1], v.z + acc[jj][2], v.w + acc[jj][3]);
        }
      }
    }
  }
}

// The depthwise conv's backward, one workgroup per sequence, one thread per channel, forwards in time: frame t adds
// w_c[k] dpre_t to dxi_{t-3+k}, so dxi_{t-3} is complete after frame t and three running sums are all that is carried.
__global__ void __launch_bounds__(E)
sn_mamba_bwd_conv_kernel(const float* __restrict__ xz, const float* __restrict__ du, int nt,
                         const float* __restrict__ conv_w, const float* __restrict__ conv_b, float* __restrict__ dxz,
                         float* __restrict__ u_out, float* __restrict__ pconv) {
  const long long s = blockIdx.x;
  const int e = threadIdx.x;
  float cw[KC];
#pragma unroll
  for (int k = 0; k < KC; ++k) cw[k] = conv_w[e * KC + k];
  const float cb = conv_b[e];
  const float* xrow = xz + s * nt * (2 * E) + e;
  const float* drow = du + s * nt * E + e;
  float* orow = dxz + s * nt * (2 * E) + e;
  float* urow = u_out + s * nt * E + e;
  float x0 = 0.f, x1 = 0.f, x2 = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f;
  float dw0 = 0.f, dw1 = 0.f, dw2 = 0.f, dw3 = 0.f, db = 0.f;
#pragma unroll 4
  for (int t = 0; t < nt; ++t) {
    const float xi = xrow[(long long)t * (2 * E)], d = drow[(long long)t * E];
    float pre = cb;
    pre = fmaf(cw[0], x0, pre);
    pre = fmaf(cw[1], x1, pre);
    pre = fmaf(cw[2], x2, pre);
    pre = fmaf(cw[3], xi, pre);
    const float sg = sigmoid_f(pre);
    urow[(long long)t * E] = pre * sg;
    const float dpre = d * (sg * fmaf(pre, 1.f - sg, 1.f));
    db += dpre;
    dw0 = fmaf(dpre, x0, dw0);
    dw1 = fmaf(dpre, x1, dw1);
    dw2 = fmaf(dpre, x2, dw2);
    dw3 = fmaf(dpre, xi, dw3);
    if (t >= KC - 1) orow[(long long)(t - (KC - 1)) * (2 * E)] = fmaf(cw[0], dpre, a0);
    a0 = fmaf(cw[1], dpre, a1);
    a1 = fmaf(cw[2], dpre, a2);
    a2 = cw[3] * dpre;
    x0 = x1;
    x1 = x2;
    x2 = xi;
  }
  if (nt >= 3) orow[(long long)(nt - 3) * (2 * E)] = a0;
  if (nt >= 2) orow[(long long)(nt - 2) * (2 * E)] = a1;
  orow[(long long)(nt - 1) * (2 * E)] = a2;
  float* pc = pconv + s * kConvPart;
  pc[e * KC + 0] = dw0;
  pc[e * KC + 1] = dw1;
  pc[e * KC + 2] = dw2;
  pc[e * KC + 3] = dw3;
  pc[E * KC + e] = db;
}

// ---------------------------------------------------------------------------------------------------------
// in: dln = [dxi | dz] . W_in, then LayerNorm backward + residual:  dx = rstd (g - mean(g) - xhat mean(g xhat)) + res dO
// with g = dln * gamma.  A lane holds the channels 16 j + 4 kq + r of its point (the product's outputs as they fall).
// Also writes ln = LN(x) (the operand of dW_in) and the workgroup's partial d gamma | d beta.
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(512)
sn_mamba_bwd_in_kernel(const float* __restrict__ dxz, fnssl_btf_view xv, int nt, int nf, long long npts,
                       const float* __restrict__ ln_w, const float* __restrict__ ln_b, const float* __restrict__ winT,
                       const float* __restrict__ dO, int residual, float* __restrict__ dx, long long x_sb,
                       long long x_st, long long x_sf, float* __restrict__ lnbuf, float* __restrict__ pln) {
  extern __shared__ __attribute__((aligned(16))) float ldsw[];     // 6 tiles x 24 groups x 1 KiB, then the small images
  constexpr int WF = w_lds_floats<2 * E, H, false>();
  float* lgb = ldsw + WF;                 // gamma [96] | beta [96]
  float* red = lgb + 2 * H;               // [8 waves][gamma 96 | beta 96]
  fill_w_lds_strided<2 * E, H, 512>(ldsw, winT, 1, 2 * E, 2 * E, H);   // W[k][o = h] = winT[h][k]
  if (threadIdx.x < H) {
    lgb[threadIdx.x] = ln_w[threadIdx.x];
    lgb[H + threadIdx.x] = ln_b[threadIdx.x];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = lane & 15, kq = lane >> 4;
  const float* ldsw_lane = ldsw + lane * 4;
  const long long ntiles = (npts + 15) / 16;
  float gacc[H / 4], bacc[H / 4];
#pragma unroll
  for (int i = 0; i < H / 4; ++i) gacc[i] = bacc[i] = 0.f;
  for (long long tile = (long long)blockIdx.x * 8 + w; tile < ntiles; tile += (long long)gridDim.x * 8) {
    const long long p = tile * 16 + n;
    const bool ok = p < npts;
    const long long pc = ok ? p : npts - 1;
    int t, f;
    const long long b = divmod(divmod(pc, nt, t), nf, f);
    v4f_t acc[H / 16];
    {
      const float4* row = reinterpret_cast<const float4*>(dxz + pc * (2 * E) + kq * (2 * E / 4));
      float a[2 * E / 4];
#pragma unroll
      for (int i = 0; i < 2 * E / 16; ++i) {
        const float4 v = row[i];
        a[4 * i] = v.x;
        a[4 * i + 1] = v.y;
        a[4 * i + 2] = v.z;
        a[4 * i + 3] = v.w;
      }
#pragma unroll
      for (int j = 0; j < H / 16; ++j) acc[j] = v4f_t{0.f, 0.f, 0.f, 0.f};
      mfma_tiles<2 * E, H / 16>(a, ldsw_lane, 0, acc);
    }
    const float* xb = xv.p + b * xv.sb + t * xv.st + f * xv.sf + 4 * kq;
    float xh[H / 4];
#pragma unroll
    for (int j = 0; j < H / 16; ++j) {
      const float4 v = *reinterpret_cast<const float4*>(xb + 16 * j);
      xh[4 * j] = v.x;
      xh[4 * j + 1] = v.y;
      xh[4 * j + 2] = v.z;
      xh[4 * j + 3] = v.w;
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < H / 4; ++i) sum += xh[i];
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum * (1.f / H);
    float var = 0.f;
#pragma unroll
    for (int i = 0; i < H / 4; ++i) {
      const float d = xh[i] - mean;
      var = fmaf(d, d, var);
    }
    var += __shfl_xor(var, 16, 64);
    var += __shfl_xor(var, 32, 64);
    const float rstd = 1.f / sqrtf(var * (1.f / H) + kEps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < H / 16; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * j + r, ch = 16 * j + 4 * kq + r;
        xh[i] = (xh[i] - mean) * rstd;
        const float gch = acc[j][r] * lgb[ch];
        s1 += gch;
        s2 = fmaf(gch, xh[i], s2);
      }
    s1 += __shfl_xor(s1, 16, 64);
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 16, 64);
    s2 += __shfl_xor(s2, 32, 64);
    s1 *= 1.f / H;
    s2 *= 1.f / H;
    if (ok) {
      float* dxp = dx + b * x_sb + t * x_st + f * x_sf + 4 * kq;
      float* lnp = lnbuf + p * H + 4 * kq;
      const float* dop = dO + p * H + 4 * kq;
#pragma unroll
      for (int j = 0; j < H / 16; ++j) {
        float o[4], l[4];
        float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (residual) rv = *reinterpret_cast<const float4*>(dop + 16 * j);
        const float rs[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 4 * j + r, ch = 16 * j + 4 * kq + r;
          const float gch = acc[j][r] * lgb[ch];
          o[r] = fmaf(rstd, gch - s1 - xh[i] * s2, rs[r]);
          l[r] = fmaf(xh[i], lgb[ch], lgb[H + ch]);
          gacc[i] = fmaf(acc[j][r], xh[i], gacc[i]);
          bacc[i] += acc[j][r];
        }
        *reinterpret_cast<float4*>(dxp + 16 * j) = make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<float4*>(lnp + 16 * j) = make_float4(l[0], l[1], l[2], l[3]);
      }
    }
  }
  // d gamma | d beta of the workgroup: the 16 points of a row by butterfly, the 8 waves through LDS in wave order
#pragma unroll
  for (int i = 0; i < H / 4; ++i) {
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
      gacc[i] += __shfl_xor(gacc[i], d, 64);
      bacc[i] += __shfl_xor(bacc[i], d, 64);
    }
  }
  if (n == 0) {
#pragma unroll
    for (int i = 0; i < H / 4; ++i) {
      const int ch = 16 * (i >> 2) + 4 * kq + (i & 3);
      red[w * 2 * H + ch] = gacc[i];
      red[w * 2 * H + H + ch] = bacc[i];
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * H) {
    float v = 0.f;
#pragma unroll
    for (int ww = 0; ww < 8; ++ww) v += red[ww * 2 * H + threadIdx.x];
    pln[(long long)blockIdx.x * 2 * H + threadIdx.x] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------
// wgrad: part[split][m][n] = sum over the split's points of A[p][m] B[p][n]   (A [npts, lda], B [npts, ldb]).
// Both operands are row-major in p, which is the MFMA's "k across lane groups" operand shape: lane (i, kq) feeds
// A[p0 + kq][16 mt + i] and B[p0 + kq][16 nt + i].  A wave owns one 16-row tile of the output and NT of its 16-column
// tiles; the four waves of a workgroup take every fourth group of 4 points and are added through LDS in wave order.
// ---------------------------------------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(256)
sn_wgrad_pts_kernel(const float* __restrict__ A, int lda, int M, const float* __restrict__ B, int ldb, int N,
                    long long npts, long long per_split, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float red[3][NT][256];
  const int mtiles = M / 16;
  const int mt = blockIdx.x % mtiles, ng = blockIdx.x / mtiles;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  const long long p_begin = (long long)blockIdx.y * per_split;
  const long long p_end = p_begin + per_split < npts ? p_begin + per_split : npts;
  int ncol[NT];
  bool nok[NT];
#pragma unroll
  for (int jj = 0; jj < NT; ++jj) {
    const int c = (ng * NT + jj) * 16 + i;
    nok[jj] = c < N;
    ncol[jj] = nok[jj] ? c : 0;
  }
  v4f_t acc[NT];
#pragma unroll
  for (int jj = 0; jj < NT; ++jj) acc[jj] = v4f_t{0.f, 0.f, 0.f, 0.f};
  // four groups of 4 points per trip: their loads (clamped addresses, the choice afterwards) are in flight together
  for (long long p0 = p_begin + 4 * w; p0 < p_end; p0 += 64) {
    float av[4], bv[4][NT];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long p = p0 + 16 * u + kq;
      ok[u] = p < p_end;
      const long long pc = ok[u] ? p : p_begin;
      av[u] = A[pc * lda + mt * 16 + i];
#pragma unroll
      for (int jj = 0; jj < NT; ++jj) bv[u][jj] = B[pc * ldb + ncol[jj]];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int jj = 0; jj < NT; ++jj)
        acc[jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(ok[u] ? av[u] : 0.f, ok[u] && nok[jj] ? bv[u][jj] : 0.f, acc[jj], 0, 0, 0);
  }
  if (w > 0) {
#pragma unroll
    for (int jj = 0; jj < NT; ++jj) *reinterpret_cast<v4f_t*>(&red[w - 1][jj][lane * 4]) = acc[jj];
  }
  __syncthreads();
  if (w == 0) {
    float* dst = part + (long long)blockIdx.y * M * N;
#pragma unroll
    for (int jj = 0; jj < NT; ++jj) {
      v4f_t v = acc[jj];
#pragma unroll
      for (int ww = 0; ww < 3; ++ww) v += *reinterpret_cast<const v4f_t*>(&red[ww][jj][lane * 4]);
      if (nok[jj]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(long long)(mt * 16 + 4 * kq + r) * N + ncol[jj]] = v[r];
      }
    }
  }
}

// The regions of the backward workspace, front to back: the one description behind its size, its check and its carve-up.
struct MambaBwdWsLayout {         // fnssl_sn_mamba_backward, npts = nb * nt * nf points, nseq = nb * nf sequences
  WsRegion dyu, dxz, ddbl, u, ln, dO;   // [npts, E] (dy, then du), [npts, 2E], [npts, XP], [npts, E], [npts, H], [npts, H]
  WsRegion ckpt;                  // [nseq, ceil(nt / TC), NST, E]
  WsRegion pseq, pconv, pln, pw;  // [nseq, kSeqPart], [nseq, kConvPart], [kLnParts, 2H], [kMaxSplits, 2E * H]
  size_t total;
  MambaBwdWsLayout(long long npts, long long nseq, int nt) {
    const size_t pt = (size_t)npts * sizeof(float), sq = (size_t)nseq * sizeof(float);
    dyu = {0, pt * E};
    dxz = {dyu.end(), pt * 2 * E};
    ddbl = {dxz.end(), pt * XP};
    u = {ddbl.end(), pt * E};
    ln = {u.end(), pt * H};
    dO = {ln.end(), pt * H};
    ckpt = {dO.end(), sq * ((nt + TC - 1) / TC) * NST * E};
    pseq = {ckpt.end(), sq * kSeqPart};
    pconv = {pseq.end(), sq * kConvPart};
    pln = {pconv.end(), sizeof(float) * kLnParts * 2 * H};
    pw = {pln.end(), sizeof(float) * kMaxSplits * 2 * E * H};
    total = pw.end();
  }
};

// out[M][N] = A^T B over the points: split-K partial tiles, then the slabs in order
template <int NT>
int wgrad_pts(hipStream_t s, const float* A, int lda, int M, const float* B, int ldb, int N, long long npts, float* part,
              float* out) {
  long long splits = (npts + 1023) / 1024;
  if (splits > kMaxSplits) splits = kMaxSplits;
  const long long per_split = ((npts + splits - 1) / splits + 15) / 16 * 16;
  const int ngroups = (N + 16 * NT - 1) / (16 * NT);
  FNSSL_TRY(enqueue(s, Kernel{sn_wgrad_pts_kernel<NT>, 256, 0, "sn_wgrad_pts_kernel"}, dim3((M / 16) * ngroups, (unsigned)splits), A,
                    lda, M, B, ldb, N, npts, per_split, part));
  return reduce_rows(s, part, splits, (long long)M * N, M * N, out);
}

}  // namespace

extern "C" {

int fnssl_sn_mamba_backward_chunk(void) { return TC; }

size_t fnssl_sn_mamba_backward_workspace_bytes(int nb, int nt, int nf) {
  if (nb <= 0 || nt <= 0 || nf <= 0) return 0;
  return MambaBwdWsLayout((long long)nb * nt * nf, (long long)nb * nf, nt).total;
}

int fnssl_sn_mamba_backward(const fnssl_btf_view* x, int nb, int nt, int nf, const fnssl_sn_mamba_w* w, int residual,
                            int time_pool, const void* fwd_workspace, size_t fwd_workspace_bytes, const float* dout,
                            long long d_sb, long long d_st, long long d_sf, float* dx, long long x_sb, long long x_st,
                            long long x_sf, const fnssl_sn_mamba_grads* g, void* workspace, size_t workspace_bytes,
                            void* stream) {
  FNSSL_REQUIRE(view_ok(x), "sn_mamba_backward: x must be 16-byte aligned with strides %% 4 == 0");
  FNSSL_REQUIRE(w && w->ln_w && w->ln_b && w->winT && w->conv_w && w->conv_b && w->wxT && w->wdt && w->bdt && w->a &&
                    w->d && w->woT, "sn_mamba_backward: null weights");
  FNSSL_REQUIRE(g && g->ln_w && g->ln_b && g->winT && g->conv_w && g->conv_b && g->wxT && g->wdt && g->bdt && g->a &&
                    g->d && g->woT, "sn_mamba_backward: null gradient pointer");
  FNSSL_REQUIRE(nb > 0 && nt > 0 && nf > 0, "sn_mamba_backward: empty problem");
  FNSSL_REQUIRE(time_pool >= 1 && time_pool <= 16, "sn_mamba_backward: time_pool must be in [1, 16]");
  FNSSL_REQUIRE(nt / time_pool == 0 || out_ok(dout, d_sb, d_st, d_sf),
                "sn_mamba_backward: dout must be 16-byte aligned with strides %% 4 == 0");
  FNSSL_REQUIRE(out_ok(dx, x_sb, x_st, x_sf), "sn_mamba_backward: dx must be 16-byte aligned with strides %% 4 == 0");
  const long long npts = (long long)nb * nt * nf, nseq = (long long)nb * nf;
  FNSSL_REQUIRE(npts < (1ll << 31) && nseq * kSeqPart < (1ll << 31), "sn_mamba_backward: too many points");
  const MambaWsLayout fws(npts);
  FNSSL_REQUIRE(fwd_workspace && fwd_workspace_bytes == fws.total,
                "sn_mamba_backward: forward workspace of %zu bytes, fnssl_sn_mamba leaves %zu for this shape",
                fwd_workspace_bytes, fws.total);
  const MambaBwdWsLayout ws(npts, nseq, nt);
  FNSSL_TRY(check_workspace("sn_mamba_backward", workspace, workspace_bytes, ws.total));
  void* const fw = const_cast<void*>(fwd_workspace);
  const float *const xz = fws.xz.floats(fw), *const dbl = fws.dbl.floats(fw), *const y = fws.y.floats(fw);
  float *const dyu = ws.dyu.floats(workspace), *const dxz = ws.dxz.floats(workspace), *const ddbl = ws.ddbl.floats(workspace);
  float *const u = ws.u.floats(workspace), *const ln = ws.ln.floats(workspace), *const dO = ws.dO.floats(workspace);
  float *const ckpt = ws.ckpt.floats(workspace), *const pseq = ws.pseq.floats(workspace);
  float *const pconv = ws.pconv.floats(workspace), *const pln = ws.pln.floats(workspace), *const pw = ws.pw.floats(workspace);
  hipStream_t s = fnssl::as_stream(stream);
  {
    fnssl::TimedLaunch tl("sn_mamba_bwd_out", s, 2.0 * npts * H * E);
    const size_t lds = (size_t)w_lds_floats<H, E, false>() * sizeof(float);
    FNSSL_TRY(enqueue(s, Kernel{sn_mamba_bwd_out_kernel, 512, lds, "sn_mamba_bwd_out_kernel"}, mfma_grid(npts, 2), dout, d_sb, d_st,
                      d_sf, nt, nt / time_pool, nf, time_pool, npts, w->woT, dO, dyu));
  }
  {
    fnssl::TimedLaunch tl("sn_mamba_bwd_scan", s, (double)npts * E * (30.0 * NST + 4 * RK + 2 * KC));
    const size_t lds = (size_t)(TC * XP + SB * NV * LDV) * sizeof(float);
    FNSSL_TRY(enqueue(s, Kernel{sn_mamba_bwd_scan_kernel, 2 * E, lds, "sn_mamba_bwd_scan_kernel"}, (unsigned)nseq, xz, dbl, dyu, nt,
                      w->conv_w, w->conv_b, w->wdt, w->bdt, w->a, w->d, dxz, ddbl, ckpt, pseq));
  }
  {
    fnssl::TimedLaunch tl("sn_mamba_bwd_xproj", s, 2.0 * npts * E * (NV + 2 * KC));
    const size_t lds = (size_t)w_lds_floats<KX, E, false>() * sizeof(float);
    FNSSL_TRY(enqueue(s, Kernel{sn_mamba_bwd_xproj_kernel, 512, lds, "sn_mamba_bwd_xproj_kernel"}, mfma_grid(npts, 4), ddbl, npts,
                      w->wxT, dyu));
    FNSSL_TRY(enqueue(s, Kernel{sn_mamba_bwd_conv_kernel, E, 0, "sn_mamba_bwd_conv_kernel"}, (unsigned)nseq, xz, dyu, nt, w->conv_w,
                      w->conv_b, dxz, u, pconv));
  }
  const unsigned grid_in = std::min(mfma_grid(npts, 1), (unsigned)kLnParts);
  {
    fnssl::TimedLaunch tl("sn_mamba_bwd_in", s, 2.0 * npts * 2 * E * H);
    const size_t lds = (size_t)(w_lds_floats<2 * E, H, false>() + 2 * H + 8 * 2 * H) * sizeof(float);
    FNSSL_TRY(enqueue(s, Kernel{sn_mamba_bwd_in_kernel, 512, lds, "sn_mamba_bwd_in_kernel"}, grid_in, dxz, *x, nt, nf, npts, w->ln_w,
                      w->ln_b, w->winT, dO, residual, dx, x_sb, x_st, x_sf, ln, pln));
  }
  fnssl::TimedLaunch tl("sn_mamba_bwd_wgrad", s, 2.0 * npts * (E * H + E * NV + 2 * E * H));
  FNSSL_TRY(wgrad_pts<6>(s, y, E, E, dO, H, H, npts, pw, g->woT));
  FNSSL_TRY(wgrad_pts<3>(s, u, E, E, ddbl, XP, XP, npts, pw, g->wxT));
  FNSSL_TRY(wgrad_pts<6>(s, ln, H, H, dxz, 2 * E, 2 * E, npts, pw, g->winT));
  FNSSL_TRY(reduce_rows(s, pln, grid_in, 2 * H, H, g->ln_w, H, g->ln_b));
  FNSSL_TRY(reduce_rows(s, pseq, nseq, kSeqPart, E * NST, g->a, E, g->d, E * RK, g->wdt, E, g->bdt));
  return reduce_rows(s, pconv, nseq, kConvPart, E * KC, g->conv_w, E, g->conv_b);
}

}  // extern "C"
