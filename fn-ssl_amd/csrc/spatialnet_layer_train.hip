// IPDnet2 on gfx950, training: the backward of the f-conv branch (fnssl_sn_fconv) and of the full-band branch
// (fnssl_sn_full), include/fnssl.h "f-conv and full-band branch, backward"; DESIGN.md section 15.
//
// Both branches are local to one (b, t) frame, so x is the only saved state: LayerNorm statistics, the conv
// pre-activation and the squeeze / Linear / unsqueeze intermediates are recomputed per frame.  The formulation is the
// scalar forward's (spatialnet.hip): one workgroup = 256 points = 256 / nf whole frames, one THREAD = one point, weights
// wave-uniform through the scalar cache, neighbours along F through LDS tiles.  Unlike the forward, a thread does not hold
// its point's 96 inputs: it keeps the 96 dln (f-conv) or 8 + 8 squeeze values (full) and re-reads x a slice at a time.
//
// Data gradients (dx) are computed point-parallel, like the forward.  Parameter gradients are sums over points, and a
// point is a thread, so they change hands through LDS: the point-parallel phase leaves its per-point factors in a tile
// (one 12-channel group of the f-conv, one 32-channel chunk of the full-band branch at a time), and after a barrier
// the same 256 threads each OWN a fixed set of parameter elements and add the tile's 256 points to their register
// accumulators in point order.  Workgroups are persistent (grid <= CU count, blocks taken round robin), so a
// workgroup's accumulators hold its blocks in ascending order; at the end each workgroup writes ONE row of partial sums
// and sn_reduce_rows_kernel adds the rows in workgroup order.  No atomics anywhere: the result depends on the CU count
// of the device and on nothing else.
#include "spatialnet_common.h"

namespace {

constexpr int kFconvTile = 4992;       // floats: max over nf in [8, 256] of (256 / nf) * (nf + 4) * 13
constexpr int kPt = 256 * 13;          // a per-point tile of one 12-channel group (stride 13: conflict-free columns)
constexpr int kFconvParams = NG * KF * CG * CG + 4 * H;   // wT | bias | prelu | ln_w | ln_b = 6144 floats
constexpr int kFconvWElems = KF * CG * CG;                // 720 conv weights per group
constexpr int kFconvOwn = 3;           // ceil(720 / 256) weights of a group per thread
constexpr int kRole0 = 208;            // threads 208 .. 255 own 2 weights per group and one of the 4 x 12 channel sums

constexpr int CH = 32;                 // channels per chunk of the full-band branch's per-point tiles
constexpr int CT = CH + 1;             // tile stride
constexpr int kFullFixed = 2 * H * HS + H + HS;           // wuT | bu | G | bs = 1640 floats beside wfT | bf

__host__ __device__ constexpr int full_params(int nf) { return nf * nf + nf + kFullFixed; }
__host__ __device__ constexpr int full_wf_mode(int nf) { return nf <= 32 ? 0 : (nf <= 128 ? 1 : 2); }

__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }

// The same address as p, opaque to the compiler: x is read again where it is needed (a 12- or 32-channel slice, a float4
// at a time) instead of being kept, and a reload the compiler could prove equal to the first would be kept after all —
// 96 live registers per point through every phase, which is what spilled.
__device__ __forceinline__ const float* reload_ptr(const float* p) {
  asm volatile("" : "+v"(p));
  return p;
}

// ---------------------------------------------------------------------------------------------------------
// f-conv backward.  Per 12-channel group g (the conv never mixes groups):
//   A  thread = point   ln_g -> lnT (rows padded by the conv's 2 zero rows either side of every frame)
//   B  thread = point   a = bias + conv(ln_g);  dpre = dO (a >= 0 ? 1 : slope) -> dpT (same padding);  dO a [a < 0] -> sT
//   C  thread = point   dln_g = transposed conv of dpT (registers);  dln_g x^, dln_g -> uT, vT
//   D  thread = owner   dW_g[tap][ci][o] += sum_rows dpT[r][o] lnT[r + tap - 2][ci];  the 48 channel sums of the group
// then, per point, the LayerNorm backward over the 96 dln in registers.
// ---------------------------------------------------------------------------------------------------------
template <int POOL>
__global__ void __launch_bounds__(256)
sn_fconv_bwd_kernel(fnssl_btf_view xv, int nt, int nf, int lg_nf, long long nframes, long long nblk, fnssl_sn_fconv_w w,
                    int residual, const float* __restrict__ dout, long long d_sb, long long d_st, long long d_sf,
                    float* __restrict__ dx, long long x_sb, long long x_st, long long x_sf, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float lds_fc[];
  float* const lnT = lds_fc;
  float* const dpT = lnT + kFconvTile;
  float* const sT = dpT + kFconvTile;
  float* const uT = sT + kPt;
  float* const vT = uT + kPt;
  const int tid = threadIdx.x;
  const int fr = tid >> lg_nf, f = tid & (nf - 1);
  const int rows = nf + 4, nrows = (256 >> lg_nf) * rows;
  const int myrow = fr * rows + f + 2;
  if (f < 2) {                                   // the 'same' padding of both tiles: never written again
#pragma unroll
    for (int ci = 0; ci < CG; ++ci) {
      lnT[(fr * rows + f) * 13 + ci] = 0.f;
      lnT[(fr * rows + nf + 2 + f) * 13 + ci] = 0.f;
      dpT[(fr * rows + f) * 13 + ci] = 0.f;
      dpT[(fr * rows + nf + 2 + f) * 13 + ci] = 0.f;
    }
  }
  // what this thread owns: weights tid, tid + 256, tid + 512 (< 720) of every group as (tap, ci, o), and from kRole0 on
  // one channel sum: role 0 dbias, 1 dslope, 2 dgamma, 3 dbeta, channel ro of the group
  int wo[kFconvOwn], wl[kFconvOwn];              // dpT column; lnT offset (tap * 13 + ci)
#pragma unroll
  for (int k = 0; k < kFconvOwn; ++k) {
    const int idx = tid + 256 * k, tap = idx / (CG * CG), rem = idx - tap * (CG * CG), ci = rem / CG;
    wo[k] = rem - ci * CG;
    wl[k] = tap * 13 + ci;
  }
  const int role = tid >= kRole0 ? (tid - kRole0) / CG : -1, ro = tid >= kRole0 ? (tid - kRole0) % CG : 0;
  float accW[NG][kFconvOwn], accS[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    accS[g] = 0.f;
#pragma unroll
    for (int k = 0; k < kFconvOwn; ++k) accW[g][k] = 0.f;
  }

  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const long long frame = blk * (256 >> lg_nf) + fr;
    const bool valid = frame < nframes;
    const long long b = frame / nt;
    const int t = (int)(frame - b * nt);
    // a frame past the end reads frame 0 (any readable row does) and takes part with dO = 0: every sum it feeds gets
    // exact zeros
    const float* xp = xv.p + (valid ? b * xv.sb + t * xv.st + f * xv.sf : (long long)f * xv.sf);
    float dln[H], mean, rstd;
    {
      float x[H];
      load_row(x, xp);
      ln_stats(x, mean, rstd);
    }
    const float* dop = dout + (valid ? b * d_sb + t * d_st + (f / POOL) * d_sf : 0);
    const float dscale = valid ? 1.f / POOL : 0.f;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      float xh[CG];
      {
        const float4* x4 = reinterpret_cast<const float4*>(reload_ptr(xp) + g * CG);
        const float4 q0 = x4[0], q1 = x4[1], q2 = x4[2];
        const float xg[CG] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
        for (int ci = 0; ci < CG; ++ci) {
          xh[ci] = (xg[ci] - mean) * rstd;
          lnT[myrow * 13 + ci] = xh[ci] * w.ln_w[g * CG + ci] + w.ln_b[g * CG + ci];
        }
      }
      __syncthreads();
      float acc[CG];
#pragma unroll
      for (int o = 0; o < CG; ++o) acc[o] = w.bias[g * CG + o];
      const float* wg = w.wT + g * (KF * CG * CG);
      {
        const float* base = lnT + (myrow - 2) * 13;
        // rolled, as in sn_fconv_kernel: unrolled, the scalar weight loads of the whole group are hoisted and spill
#pragma unroll 1
        for (int j = 0; j < KF * CG; j += 4) {
          const int tap = j / CG, ci = j - tap * CG;
          const float* bj = base + tap * 13 + ci;
          const float v0 = bj[0], v1 = bj[1], v2 = bj[2], v3 = bj[3];
          const float* wj = wg + j * CG;
#pragma unroll
          for (int o = 0; o < CG; ++o) acc[o] = fmaf(wj[o], v0, acc[o]);
#pragma unroll
          for (int o = 0; o < CG; ++o) acc[o] = fmaf(wj[CG + o], v1, acc[o]);
#pragma unroll
          for (int o = 0; o < CG; ++o) acc[o] = fmaf(wj[2 * CG + o], v2, acc[o]);
#pragma unroll
          for (int o = 0; o < CG; ++o) acc[o] = fmaf(wj[3 * CG + o], v3, acc[o]);
        }
      }
      {
        const float4* d4 = reinterpret_cast<const float4*>(dop + g * CG);
        const float4 q0 = d4[0], q1 = d4[1], q2 = d4[2];
        const float dO[CG] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
        for (int o = 0; o < CG; ++o) {
          const float a = acc[o], d = dO[o] * dscale;
          dpT[myrow * 13 + o] = a >= 0.f ? d : w.prelu[g * CG + o] * d;
          sT[tid * 13 + o] = a >= 0.f ? 0.f : d * a;
        }
      }
      __syncthreads();
      {
        float dl[CG];
#pragma unroll
        for (int ci = 0; ci < CG; ++ci) dl[ci] = 0.f;
        // dln[f][ci] = sum_{tap, o} W[o][ci][tap] dpre[f - tap + 2][o]: the padded row of f - tap + 2 is myrow + 2 - tap
#pragma unroll 1
        for (int tap = 0; tap < KF; ++tap) {
          const float* dr = dpT + (myrow + 2 - tap) * 13;
          float d[CG];
#pragma unroll
          for (int o = 0; o < CG; ++o) d[o] = dr[o];
          const float* wt = wg + tap * (CG * CG);
#pragma unroll
          for (int ci = 0; ci < CG; ++ci)
#pragma unroll
            for (int o = 0; o < CG; ++o) dl[ci] = fmaf(wt[ci * CG + o], d[o], dl[ci]);
        }
#pragma unroll
        for (int ci = 0; ci < CG; ++ci) {
          dln[g * CG + ci] = dl[ci];
          uT[tid * 13 + ci] = dl[ci] * xh[ci];
          vT[tid * 13 + ci] = dl[ci];
        }
      }
      __syncthreads();
      // owner phase: the pad rows of dpT are zero, so running over every padded row adds exact zeros for them and an
      // lnT row of the neighbouring frame is only ever met by a zero
#pragma unroll
      for (int k = 0; k < kFconvOwn; ++k) {
        if (tid + 256 * k < kFconvWElems) {
          float a = accW[g][k];
          const float* dp = dpT + wo[k];
          const float* lp = lnT + wl[k];
#pragma unroll 8
          for (int r = 2; r < nrows - 2; ++r) a = fmaf(dp[r * 13], lp[(r - 2) * 13], a);
          accW[g][k] = a;
        }
      }
      if (role >= 0) {
        float a = accS[g];
        if (role == 0) {
#pragma unroll 8
          for (int r = 2; r < nrows - 2; ++r) a += dpT[r * 13 + ro];
        } else {
          const float* src = (role == 1 ? sT : (role == 2 ? uT : vT)) + ro;
#pragma unroll 8
          for (int p = 0; p < 256; ++p) a += src[p * 13];
        }
        accS[g] = a;
      }
      __syncthreads();
    }
    // LayerNorm backward: dl = dln gamma;  dx = rstd (dl - mean(dl) - x^ mean(dl x^)) + residual dO
    float m1 = 0.f, m2 = 0.f;
    {
      const float4* x4 = reinterpret_cast<const float4*>(reload_ptr(xp));
#pragma unroll
      for (int i = 0; i < H / 4; ++i) {
        const float4 q = x4[i];
        const float xq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 4 * i + e;
          dln[c] *= w.ln_w[c];
          m1 += dln[c];
          m2 = fmaf(dln[c], (xq[e] - mean) * rstd, m2);
        }
      }
    }
    m1 *= 1.f / H;
    m2 *= 1.f / H;
    if (valid) {
      const float rs = residual ? dscale : 0.f;
      const float4* d4 = reinterpret_cast<const float4*>(dop);
      const float4* x4 = reinterpret_cast<const float4*>(reload_ptr(xp));
      float4* o4 = reinterpret_cast<float4*>(dx + b * x_sb + t * x_st + f * x_sf);
#pragma unroll
      for (int i = 0; i < H / 4; ++i) {
        const float4 q = d4[i], xq4 = x4[i];
        const float dq[4] = {q.x, q.y, q.z, q.w}, xq[4] = {xq4.x, xq4.y, xq4.z, xq4.w};
        float r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 4 * i + e;
          r[e] = fmaf(rstd, dln[c] - m1 - (xq[e] - mean) * rstd * m2, rs * dq[e]);
        }
        o4[i] = make_float4(r[0], r[1], r[2], r[3]);
      }
    }
  }
  float* row = part + (long long)blockIdx.x * kFconvParams;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
#pragma unroll
    for (int k = 0; k < kFconvOwn; ++k)
      if (tid + 256 * k < kFconvWElems) row[g * kFconvWElems + tid + 256 * k] = accW[g][k];
    if (role >= 0) row[NG * kFconvWElems + role * H + g * CG + ro] = accS[g];
  }
}

// ---------------------------------------------------------------------------------------------------------
// full-band backward.  Per block of 256 / NF frames:
//   thread = point   LN, ps = Ws ln + bs, s = SiLU(ps) -> S;   v = Wf s + bf -> V
//   per 32-channel chunk:  dpu = dO SiLU'(Wu v + bu) -> CTl,  dv += Wu^T dpu;   owners: dWu += CTl^T V, dbu
//   dv -> DV;  ds = Wf^T dv;  owners: dWf[f][f2] += sum_{frame, q} dv[f][q] s[f2][q], dbf;   dps = ds SiLU'(ps) -> V
//   per 32-channel chunk:  x^ -> CTl;   owners: G[h][q] += sum_p x^[p][h] dps[p][q], dbs
//   thread = point   dln = Ws^T dps, LayerNorm backward
// ln = gamma x^ + beta is linear in x^, so the three sums over points that involve ln or dln all follow from G and dbs
// (sn_full_bwd_finish_kernel): dWs[q][h] = gamma[h] G[h][q] + beta[h] dbs[q], dgamma[h] = sum_q Ws[q][h] G[h][q],
// dbeta[h] = sum_q Ws[q][h] dbs[q].  That leaves one per-point tile instead of three.
// dWf has NF^2 elements, NF^2 / 256 per owner: register accumulators up to NF = 32 (4 per thread); an LDS image of the
// matrix at NF = 64 and 128 (16 and 64 KB; 64 register accumulators and the reads that feed them did not fit the register
// file); at NF = 256 (256 KB, and no hot shape runs there) the workgroup's own partial row in memory.  One owner per
// element in every case, so no atomics.
// ---------------------------------------------------------------------------------------------------------
template <int NF>
__global__ void __launch_bounds__(256)
sn_full_bwd_kernel(fnssl_btf_view xv, int nt, long long nframes, long long nblk, fnssl_sn_full_w w, int residual,
                   const float* __restrict__ dout, long long d_sb, long long d_st, long long d_sf, float* __restrict__ dx,
                   long long x_sb, long long x_st, long long x_sf, float* __restrict__ part) {
  constexpr int FPB = 256 / NF;                             // frames per block
  constexpr int LG = NF == 8 ? 3 : NF == 16 ? 4 : NF == 32 ? 5 : NF == 64 ? 6 : NF == 128 ? 7 : 8;
  constexpr int EW = NF * NF;
  constexpr int MODE = full_wf_mode(NF);                    // where dWf accumulates: 0 registers, 1 LDS, 2 the partial row
  constexpr bool REG = MODE == 0;
  constexpr int EPT = REG ? (EW >= 256 ? EW / 256 : 1) : 1;
  extern __shared__ __attribute__((aligned(16))) float lds_fu[];
  float* const S = lds_fu;                                  // [256][8]
  float* const V = S + 256 * HS;                            // [256][8]: v, later dps
  float* const DV = V + 256 * HS;                           // [256][8]
  float* const CTl = DV + 256 * HS;                         // [256][33]
  float* const WA = CTl + 256 * CT;                         // [NF][NF], MODE 1 only
  const int tid = threadIdx.x;
  const int fr = tid >> LG, f = tid & (NF - 1);
  float* const row = part + (long long)blockIdx.x * full_params(NF);
  float accWf[EPT], accBf = 0.f, accWu[H / CH], accBu[H / CH], accG[H / CH], accBs = 0.f;
#pragma unroll
  for (int k = 0; k < EPT; ++k) accWf[k] = 0.f;
#pragma unroll
  for (int c = 0; c < H / CH; ++c) accWu[c] = accBu[c] = accG[c] = 0.f;
  const int oh = tid >> 3, oq = tid & 7;                    // the (channel of the chunk, squeeze channel) this thread owns
  bool first = true;
  if constexpr (MODE == 1) {
    for (int k = 0; k < EW / 256; ++k) WA[tid + 256 * k] = 0.f;   // touched by its owner only: no barrier
  }

  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const long long frame = blk * FPB + fr;
    const bool valid = frame < nframes;
    const long long b = frame / nt;
    const int t = (int)(frame - b * nt);
    // a frame past the end reads frame 0 (any readable row does) and takes part with dO = 0: every sum it feeds gets
    // exact zeros
    const float* xp = xv.p + (valid ? b * xv.sb + t * xv.st + f * xv.sf : (long long)f * xv.sf);
    float mean, rstd, ps[HS];
    {
      float x[H];
      load_row(x, xp);
      ln_stats(x, mean, rstd);
#pragma unroll
      for (int q = 0; q < HS; ++q) ps[q] = w.bs[q];
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float ln = (x[h] - mean) * rstd * w.ln_w[h] + w.ln_b[h];
#pragma unroll
        for (int q = 0; q < HS; ++q) ps[q] = fmaf(w.wsT[h * HS + q], ln, ps[q]);
      }
    }
    {
      float4* mine = reinterpret_cast<float4*>(S + tid * HS);
      mine[0] = make_float4(silu_f(ps[0]), silu_f(ps[1]), silu_f(ps[2]), silu_f(ps[3]));
      mine[1] = make_float4(silu_f(ps[4]), silu_f(ps[5]), silu_f(ps[6]), silu_f(ps[7]));
    }
    __syncthreads();
    float v[HS], dv[HS];
    {
      const float bfv = w.bf[f];
#pragma unroll
      for (int q = 0; q < HS; ++q) {
        v[q] = bfv;
        dv[q] = 0.f;
      }
      const float4* sf = reinterpret_cast<const float4*>(S + fr * NF * HS);
#pragma unroll 4
      for (int f2 = 0; f2 < NF; ++f2) {
        const float wv = w.wfT[f2 * NF + f];
        const float4 a = sf[f2 * 2], c = sf[f2 * 2 + 1];
        v[0] = fmaf(wv, a.x, v[0]);
        v[1] = fmaf(wv, a.y, v[1]);
        v[2] = fmaf(wv, a.z, v[2]);
        v[3] = fmaf(wv, a.w, v[3]);
        v[4] = fmaf(wv, c.x, v[4]);
        v[5] = fmaf(wv, c.y, v[5]);
        v[6] = fmaf(wv, c.z, v[6]);
        v[7] = fmaf(wv, c.w, v[7]);
      }
      float4* mine = reinterpret_cast<float4*>(V + tid * HS);
      mine[0] = make_float4(v[0], v[1], v[2], v[3]);
      mine[1] = make_float4(v[4], v[5], v[6], v[7]);
    }
    const float* dop = dout + (valid ? b * d_sb + t * d_st + f * d_sf : 0);
    const float dscale = valid ? 1.f : 0.f;
#pragma unroll
    for (int c = 0; c < H / CH; ++c) {
#pragma unroll
      for (int i = 0; i < CH / 4; ++i) {
        const float4 q4 = reinterpret_cast<const float4*>(dop + c * CH)[i];
        const float dq[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int hh = 4 * i + e, h = c * CH + hh;
          float pu = w.bu[h];
#pragma unroll
          for (int q = 0; q < HS; ++q) pu = fmaf(w.wuT[q * H + h], v[q], pu);
          const float sg = sigmoid_f(pu);
          const float d = dq[e] * dscale * (sg * fmaf(pu, 1.f - sg, 1.f));
#pragma unroll
          for (int q = 0; q < HS; ++q) dv[q] = fmaf(w.wuT[q * H + h], d, dv[q]);
          CTl[tid * CT + hh] = d;
        }
      }
      __syncthreads();
      {
        float a = accWu[c];
#pragma unroll 8
        for (int p = 0; p < 256; ++p) a = fmaf(CTl[p * CT + oh], V[p * HS + oq], a);
        accWu[c] = a;
        if (tid < CH) {
          float s = accBu[c];
#pragma unroll 8
          for (int p = 0; p < 256; ++p) s += CTl[p * CT + tid];
          accBu[c] = s;
        }
      }
      __syncthreads();
    }
    {
      float4* mine = reinterpret_cast<float4*>(DV + tid * HS);
      mine[0] = make_float4(dv[0], dv[1], dv[2], dv[3]);
      mine[1] = make_float4(dv[4], dv[5], dv[6], dv[7]);
    }
    __syncthreads();
    float dps[HS];
    {
#pragma unroll
      for (int q = 0; q < HS; ++q) dps[q] = 0.f;
      const float4* df = reinterpret_cast<const float4*>(DV + fr * NF * HS);
#pragma unroll 4
      for (int f1 = 0; f1 < NF; ++f1) {                     // ds[f][q] = sum_f1 Wf[f1][f] dv[f1][q]
        const float wv = w.wfT[f * NF + f1];
        const float4 a = df[f1 * 2], c = df[f1 * 2 + 1];
        dps[0] = fmaf(wv, a.x, dps[0]);
        dps[1] = fmaf(wv, a.y, dps[1]);
        dps[2] = fmaf(wv, a.z, dps[2]);
        dps[3] = fmaf(wv, a.w, dps[3]);
        dps[4] = fmaf(wv, c.x, dps[4]);
        dps[5] = fmaf(wv, c.y, dps[5]);
        dps[6] = fmaf(wv, c.z, dps[6]);
        dps[7] = fmaf(wv, c.w, dps[7]);
      }
#pragma unroll
      for (int q = 0; q < HS; ++q) {
        const float sg = sigmoid_f(ps[q]);
        dps[q] *= sg * fmaf(ps[q], 1.f - sg, 1.f);
      }
    }
    // owners of dWf in wfT's layout: element idx = f2 * NF + fo holds d Wf[fo][f2] = sum_{frame, q} dv[fo][q] s[f2][q]
    auto wf_elem = [&](int idx) {
      const int f2 = idx >> LG, fo = idx & (NF - 1);
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < FPB; ++j) {
        const float4* dp = reinterpret_cast<const float4*>(DV + (j * NF + fo) * HS);
        const float4* sp = reinterpret_cast<const float4*>(S + (j * NF + f2) * HS);
        const float4 d0 = dp[0], d1 = dp[1], s0 = sp[0], s1 = sp[1];
        a = fmaf(d0.x, s0.x, a);
        a = fmaf(d0.y, s0.y, a);
        a = fmaf(d0.z, s0.z, a);
        a = fmaf(d0.w, s0.w, a);
        a = fmaf(d1.x, s1.x, a);
        a = fmaf(d1.y, s1.y, a);
        a = fmaf(d1.z, s1.z, a);
        a = fmaf(d1.w, s1.w, a);
      }
      return a;
    };
    if constexpr (REG) {
#pragma unroll
      for (int k = 0; k < EPT; ++k) {
        if (tid + 256 * k < EW) accWf[k] += wf_elem(tid + 256 * k);
        // keep the LDS reads of the elements to come where they are: hoisted, all EPT x 4 of them are live at once
        if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
    } else if constexpr (MODE == 1) {
#pragma unroll 2
      for (int k = 0; k < EW / 256; ++k) WA[tid + 256 * k] += wf_elem(tid + 256 * k);
    } else {
#pragma unroll 2
      for (int k = 0; k < EW / 256; ++k) {
        const int idx = tid + 256 * k;
        row[idx] = (first ? 0.f : row[idx]) + wf_elem(idx);
      }
    }
    if (tid < NF) {
      float a = accBf;
#pragma unroll
      for (int j = 0; j < FPB; ++j)
#pragma unroll
        for (int q = 0; q < HS; ++q) a += DV[(j * NF + tid) * HS + q];
      accBf = a;
    }
    {
      float4* mine = reinterpret_cast<float4*>(V + tid * HS);   // V's readers finished before the last barrier
      mine[0] = make_float4(dps[0], dps[1], dps[2], dps[3]);
      mine[1] = make_float4(dps[4], dps[5], dps[6], dps[7]);
    }
#pragma unroll
    for (int c = 0; c < H / CH; ++c) {
      {
        const float4* x4 = reinterpret_cast<const float4*>(reload_ptr(xp) + c * CH);
#pragma unroll
        for (int i = 0; i < CH / 4; ++i) {
          const float4 q4 = x4[i];
          CTl[tid * CT + 4 * i] = (q4.x - mean) * rstd;
          CTl[tid * CT + 4 * i + 1] = (q4.y - mean) * rstd;
          CTl[tid * CT + 4 * i + 2] = (q4.z - mean) * rstd;
          CTl[tid * CT + 4 * i + 3] = (q4.w - mean) * rstd;
        }
      }
      __syncthreads();
      {
        float a = accG[c];
#pragma unroll 8
        for (int p = 0; p < 256; ++p) a = fmaf(CTl[p * CT + oh], V[p * HS + oq], a);
        accG[c] = a;
        if (c == 0 && tid < HS) {
          float s = accBs;
#pragma unroll 8
          for (int p = 0; p < 256; ++p) s += V[p * HS + tid];
          accBs = s;
        }
      }
      __syncthreads();
    }
    // LayerNorm backward: dln[h] = sum_q Ws[q][h] dps[q] is 8 FMAs, so it is formed twice instead of kept
    float m1 = 0.f, m2 = 0.f;
    {
      const float4* x4 = reinterpret_cast<const float4*>(reload_ptr(xp));
#pragma unroll
      for (int i = 0; i < H / 4; ++i) {
        const float4 q4 = x4[i];
        const float xq[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int h = 4 * i + e;
          float d = 0.f;
#pragma unroll
          for (int q = 0; q < HS; ++q) d = fmaf(w.wsT[h * HS + q], dps[q], d);
          d *= w.ln_w[h];
          m1 += d;
          m2 = fmaf(d, (xq[e] - mean) * rstd, m2);
        }
      }
    }
    m1 *= 1.f / H;
    m2 *= 1.f / H;
    if (valid) {
      const float rs = residual ? 1.f : 0.f;
      float4* o4 = reinterpret_cast<float4*>(dx + b * x_sb + t * x_st + f * x_sf);
      const float4* x4 = reinterpret_cast<const float4*>(reload_ptr(xp));
#pragma unroll
      for (int i = 0; i < H / 4; ++i) {
        const float4 q4 = reinterpret_cast<const float4*>(dop)[i], xq4 = x4[i];
        const float dq[4] = {q4.x, q4.y, q4.z, q4.w}, xq[4] = {xq4.x, xq4.y, xq4.z, xq4.w};
        float r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int h = 4 * i + e;
          float d = 0.f;
#pragma unroll
          for (int q = 0; q < HS; ++q) d = fmaf(w.wsT[h * HS + q], dps[q], d);
          d *= w.ln_w[h];
          r[e] = fmaf(rstd, d - m1 - (xq[e] - mean) * rstd * m2, rs * dq[e]);
        }
        o4[i] = make_float4(r[0], r[1], r[2], r[3]);
      }
    }
    first = false;
  }
  // the workgroup's row: wfT [NF][NF] | bf [NF] | wuT [8][96] | bu [96] | G [96][8] | bs [8]
  if constexpr (REG) {
#pragma unroll
    for (int k = 0; k < EPT; ++k)
      if (tid + 256 * k < EW) row[tid + 256 * k] = accWf[k];
  } else if constexpr (MODE == 1) {
    for (int k = 0; k < EW / 256; ++k) row[tid + 256 * k] = WA[tid + 256 * k];
  }
  if (tid < NF) row[EW + tid] = accBf;
  float* fixed = row + EW + NF;
#pragma unroll
  for (int c = 0; c < H / CH; ++c) {
    fixed[oq * H + c * CH + oh] = accWu[c];
    if (tid < CH) fixed[HS * H + c * CH + tid] = accBu[c];
    fixed[HS * H + H + (c * CH + oh) * HS + oq] = accG[c];
  }
  if (tid < HS) fixed[HS * H + H + H * HS + tid] = accBs;
}

// red = G [96][8] | dbs [8] summed over the workgroups.  One thread per channel.
__global__ void __launch_bounds__(H)
sn_full_bwd_finish_kernel(const float* __restrict__ red, fnssl_sn_full_w w, fnssl_sn_full_grads g) {
  const int h = threadIdx.x;
  const float gamma = w.ln_w[h], beta = w.ln_b[h];
  float dgam = 0.f, dbet = 0.f;
#pragma unroll
  for (int q = 0; q < HS; ++q) {
    const float G = red[h * HS + q], dbs = red[H * HS + q], ws = w.wsT[h * HS + q];
    g.wsT[h * HS + q] = fmaf(gamma, G, beta * dbs);
    dgam = fmaf(ws, G, dgam);
    dbet = fmaf(ws, dbs, dbet);
  }
  g.ln_w[h] = dgam;
  g.ln_b[h] = dbet;
  if (h < HS) g.bs[h] = red[H * HS + h];
}

inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
inline int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// blocks of 256 points (whole frames) and the persistent grid that takes them round robin
struct BwdGrid {
  long long nframes, nblk;
  unsigned grid;
  BwdGrid(int nb, int nt, int nf) {
    nframes = (long long)nb * nt;
    const int fpb = 256 / nf;
    nblk = (nframes + fpb - 1) / fpb;
    const long long cus = fnssl::device_cus();
    grid = (unsigned)(nblk < cus ? nblk : cus);
  }
};

// The regions of the two workspaces, front to back: one row of partial parameter sums per workgroup, nothing per point.
struct FconvBwdWsLayout {
  WsRegion part;                  // [grid, kFconvParams]
  size_t total;
  explicit FconvBwdWsLayout(unsigned grid) {
    part = {0, sizeof(float) * grid * kFconvParams};
    total = part.end();
  }
};
struct FullBwdWsLayout {
  WsRegion part, red;             // [grid, full_params(nf)], then G | dbs summed: [H * HS + HS]
  size_t total;
  FullBwdWsLayout(unsigned grid, int nf) {
    part = {0, (sizeof(float) * grid * full_params(nf) + 15) / 16 * 16};
    red = {part.end(), sizeof(float) * (H * HS + HS)};
    total = red.end();
  }
};

}  // namespace

extern "C" {

size_t fnssl_sn_fconv_backward_workspace_bytes(int nb, int nt, int nf) {
  if (nb <= 0 || nt <= 0 || !pow2(nf) || nf < 8 || nf > 256) return 0;
  return FconvBwdWsLayout(BwdGrid(nb, nt, nf).grid).total;
}

int fnssl_sn_fconv_backward(const fnssl_btf_view* x, int nb, int nt, int nf, const fnssl_sn_fconv_w* w, int residual,
                            int pool, const float* dout, long long d_sb, long long d_st, long long d_sf, float* dx,
                            long long x_sb, long long x_st, long long x_sf, const fnssl_sn_fconv_grads* g, void* workspace,
                            size_t workspace_bytes, void* stream) {
  FNSSL_REQUIRE(view_ok(x), "sn_fconv_backward: x must be 16-byte aligned with strides %% 4 == 0");
  FNSSL_REQUIRE(w && w->ln_w && w->ln_b && w->wT && w->bias && w->prelu, "sn_fconv_backward: null weights (w)");
  FNSSL_REQUIRE(g && g->ln_w && g->ln_b && g->wT && g->bias && g->prelu, "sn_fconv_backward: null gradient pointer (g)");
  FNSSL_REQUIRE(nb > 0 && nt > 0, "sn_fconv_backward: empty problem (nb, nt)");
  FNSSL_REQUIRE(pow2(nf) && nf >= 8 && nf <= 256, "sn_fconv_backward: nf must be a power of two in [8, 256], got %d", nf);
  FNSSL_REQUIRE(pool == 1 || pool == 2 || pool == 8, "sn_fconv_backward: pool must be 1, 2 or 8, got %d", pool);
  FNSSL_REQUIRE(out_ok(dout, d_sb, d_st, d_sf), "sn_fconv_backward: dout must be 16-byte aligned with strides %% 4 == 0");
  FNSSL_REQUIRE(out_ok(dx, x_sb, x_st, x_sf), "sn_fconv_backward: dx must be 16-byte aligned with strides %% 4 == 0");
  const BwdGrid bg(nb, nt, nf);
  FNSSL_REQUIRE(bg.nblk < (1ll << 31), "sn_fconv_backward: too many frames (nb * nt)");
  const FconvBwdWsLayout ws(bg.grid);
  FNSSL_TRY(check_workspace("sn_fconv_backward", workspace, workspace_bytes, ws.total));
  float* const part = ws.part.floats(workspace);
  hipStream_t s = fnssl::as_stream(stream);
  {
    fnssl::TimedLaunch tl("sn_fconv_bwd", s, 3.0 * 2.0 * bg.nframes * nf * H * CG * KF);
    const size_t lds = (size_t)(2 * kFconvTile + 3 * kPt) * sizeof(float);
    FNSSL_TRY(with_value<1, 2, 8>(pool, [&](auto P_) {
      constexpr int P = P_;
      return enqueue(s, Kernel{sn_fconv_bwd_kernel<P>, 256, lds, "sn_fconv_bwd_kernel"}, bg.grid, *x, nt, nf, ilog2(nf), bg.nframes,
                     bg.nblk, *w, residual, dout, d_sb, d_st, d_sf, dx, x_sb, x_st, x_sf, part);
    }));
  }
  fnssl::TimedLaunch tl("sn_fconv_bwd_reduce", s);
  FNSSL_TRY(reduce_rows(s, part, bg.grid, kFconvParams, NG * kFconvWElems, g->wT, H, g->bias, H, g->prelu, H, g->ln_w));
  return reduce_rows(s, part + NG * kFconvWElems + 3 * H, bg.grid, kFconvParams, H, g->ln_b);
}

size_t fnssl_sn_full_backward_workspace_bytes(int nb, int nt, int nf) {
  if (nb <= 0 || nt <= 0 || !pow2(nf) || nf < 8 || nf > 256) return 0;
  return FullBwdWsLayout(BwdGrid(nb, nt, nf).grid, nf).total;
}

int fnssl_sn_full_backward(const fnssl_btf_view* x, int nb, int nt, int nf, const fnssl_sn_full_w* w, int residual,
                           const float* dout, long long d_sb, long long d_st, long long d_sf, float* dx, long long x_sb,
                           long long x_st, long long x_sf, const fnssl_sn_full_grads* g, void* workspace,
                           size_t workspace_bytes, void* stream) {
  FNSSL_REQUIRE(view_ok(x), "sn_full_backward: x must be 16-byte aligned with strides %% 4 == 0");
  FNSSL_REQUIRE(w && w->ln_w && w->ln_b && w->wsT && w->bs && w->wfT && w->bf && w->wuT && w->bu,
                "sn_full_backward: null weights (w)");
  FNSSL_REQUIRE(g && g->ln_w && g->ln_b && g->wsT && g->bs && g->wfT && g->bf && g->wuT && g->bu,
                "sn_full_backward: null gradient pointer (g)");
  FNSSL_REQUIRE(nb > 0 && nt > 0, "sn_full_backward: empty problem (nb, nt)");
  FNSSL_REQUIRE(pow2(nf) && nf >= 8 && nf <= 256, "sn_full_backward: nf must be a power of two in [8, 256], got %d", nf);
  FNSSL_REQUIRE(out_ok(dout, d_sb, d_st, d_sf), "sn_full_backward: dout must be 16-byte aligned with strides %% 4 == 0");
  FNSSL_REQUIRE(out_ok(dx, x_sb, x_st, x_sf), "sn_full_backward: dx must be 16-byte aligned with strides %% 4 == 0");
  const BwdGrid bg(nb, nt, nf);
  FNSSL_REQUIRE(bg.nblk < (1ll << 31), "sn_full_backward: too many frames (nb * nt)");
  const FullBwdWsLayout ws(bg.grid, nf);
  FNSSL_TRY(check_workspace("sn_full_backward", workspace, workspace_bytes, ws.total));
  float* const part = ws.part.floats(workspace);
  float* const red = ws.red.floats(workspace);
  hipStream_t s = fnssl::as_stream(stream);
  {
    fnssl::TimedLaunch tl("sn_full_bwd", s, 3.0 * 2.0 * bg.nframes * nf * (2.0 * H * HS + (double)HS * nf));
    const size_t lds = (size_t)(3 * 256 * HS + 256 * CT + (full_wf_mode(nf) == 1 ? nf * nf : 0)) * sizeof(float);
    FNSSL_TRY(with_value<8, 16, 32, 64, 128, 256>(nf, [&](auto NF_) {
      constexpr int NFV = NF_;
      return enqueue(s, Kernel{sn_full_bwd_kernel<NFV>, 256, lds, "sn_full_bwd_kernel"}, bg.grid, *x, nt, bg.nframes, bg.nblk, *w,
                     residual, dout, d_sb, d_st, d_sf, dx, x_sb, x_st, x_sf, part);
    }));
  }
  fnssl::TimedLaunch tl("sn_full_bwd_reduce", s);
  const int np = full_params(nf);
  FNSSL_TRY(reduce_rows(s, part, bg.grid, np, nf * nf, g->wfT, nf, g->bf, HS * H, g->wuT, H, g->bu));
  FNSSL_TRY(reduce_rows(s, part + nf * nf + nf + HS * H + H, bg.grid, np, H * HS, red, HS, red + H * HS));
  return enqueue(s, Kernel{sn_full_bwd_finish_kernel, H, 0, "sn_full_bwd_finish_kernel"}, 1u, red, *w, *g);
}

}  // extern "C"
