// Shape-specialised twin of lstm_rec_kernel (lstm_kernel.h) for the layer shapes of the
// FN-SSL network itself.  Same formulation, same packed stream, same k-ordered fp32 MFMA
// chain per sequence (results are bit-identical to the generic kernel), but the whole
// structure of a hidden slice is known at compile time:
//   * the x-part / h-part loops are fully unrolled, so every ring read is
//     `chunk base VGPR + immediate` and the per-quad scalar bookkeeping and branches of the
//     generic ring reader disappear (micro-benchmark tools/ubench/mfma_peak.hip: a lone
//     wave issues MFMAs at 99 % of the pipe rate without them, 89 % with them);
//   * ring commits sit at fixed positions (chunk ends coincide with slice ends);
//   * the x operand ring is 4 blocks deep with a fixed 3-quad prefetch distance.
// Inputs are restricted to what the fused forward needs: one summed input tensor of C0
// channels (C0 = 16*NV0 or the 4-channel remainder NS0 = 1), an optional 4-channel
// concatenated tensor (NS2 = 1) and the optional fused residual output.
#pragma once

#include "lstm_wave.h"

#pragma clang fp contract(off)

namespace fnssl_lstm {

// ABL = true: timing-ablation twin driven by FNSSL_ABLATE (bits as in lstm_rec_kernel); wrong results.
template <int H, int NW, int M, int NV0, int NS0, int NS2, int CHQ, int PAD, int MODE, bool ABL = false, int XD = 4,
          int NV2 = 0>
__global__ void __launch_bounds__(NW * 64) lstm_static_kernel(const LstmParams p) {
  FNSSL_GUARDED_KERNEL(p);
  constexpr int NS = H / 16;
  constexpr bool HAS2 = (MODE & kHas2) != 0, SUM = (MODE & kSum) != 0;
  static_assert(!(MODE & kHas1), "static kernel: single summed input only");
  static_assert(HAS2 == (NS2 + NV2 > 0), "NS2 / NV2 must match the mode");
  constexpr int QPS = 1 + NV0 + NS0 + NV2 + NS2 + NS;  // real quads per slice
  constexpr int VQ = QPS + PAD;                         // virtual quads per slice
  static_assert(VQ % CHQ == 0, "chunks must tile the (padded) slice");
  constexpr int CH = 4 * CHQ;                           // records per chunk
  static_assert(CH <= NW * M, "chunk does not fit the staging registers");
  static_assert(NV0 == 0 || NV0 % XD == 0, "the x ring depth must divide the block count");
  static_assert(!(NS0 && NV0), "remainder-only or block-only summed input");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const WaveSeq<H, NW, 1, HAS2, SUM> pl(p);
  const int lane = pl.lane, w = pl.w;
  const unsigned vo0 = pl.vo0 - (NS0 ? 12 * pl.g : 0);   // remainder-only input: lane (n, g) reads channel g, not 4g..4g+3
  const unsigned vo2v = pl.vo2 + 12 * pl.g;   // 16-channel blocks of the concatenated input: lane (n, g) reads 4g..4g+3
  const unsigned cy = (unsigned)p.carry;      // streaming (see lstm_rec_kernel)
  const int abl = ABL ? p.ablate : 0;

  // ---- weight ring (this kernel's own, not lstm_wave.h's RegRing / quad_step: through those its registers move and
  // the compiler peels the slice loop of other instantiations — tools/isa_compare.py, profiles/r12/) ---------------
  char* const lds_rd = smem + lane * 16;
  char* const lds_wr = smem + w * 1024 + lane * 16;
  constexpr int NSLOT = 2;
  int wslot = 0;          // slot the staged chunk is committed to
  int rslot = 0;          // slot being read
  int src_rec = 0;        // real record index of the next chunk to stage
  int src_vq = 0;         // its virtual quad offset inside the slice
  v4f stg[M];
  auto issue_loads = [&]() {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int r = w + m * NW;
      if (r < CH && src_vq * 4 + r < QPS * 4) stg[m] = bld4(pl.rw, pl.vlane, (unsigned)(src_rec + r) * 1024u);
    }
    src_vq += CHQ;
    src_rec += CH;
    if (src_vq == VQ) {
      src_vq = 0;
      src_rec -= PAD * 4;                       // the padding quads do not exist in the stream
      if (src_rec == NS * QPS * 4) src_rec = 0;
    }
  };
  // The staged chunk goes to the slot that was read during the PREVIOUS chunk period, which is
  // free for the whole current period, so the wait-for-data + ds_write sits in the middle of the
  // chunk (where waves are not lined up at a barrier and the in-order vmcnt wait costs least)
  // and the chunk end is only `lgkmcnt(0); s_barrier`.
  auto stage_write = [&]() {
#pragma unroll
    for (int m = 0; m < M; ++m)
      if (w + m * NW < CH) *reinterpret_cast<v4f*>(lds_wr + wslot * (CH * 1024) + m * (NW * 1024)) = stg[m];
    wslot = (wslot + 1 == NSLOT) ? 0 : wslot + 1;
  };
  auto sync = [&]() {
    if (ABL && (abl & 8))
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    else
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  };
  issue_loads();
  stage_write();
  sync();
  issue_loads();
  const char* cb = lds_rd;                      // base of the chunk being read
  auto rec = [&](auto ql, int j) {              // record j of quad ql (compile time) of the current chunk
    return *reinterpret_cast<const v4f*>(cb + decltype(ql)::value * 4096 + j * 1024);
  };
  v4f a0 = rec(ic<0>{}, 0), a1 = rec(ic<0>{}, 1);

  v4f hold[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) hold[s] = v4f{0.f, 0.f, 0.f, 0.f};
  const v4f zero4 = v4f{0.f, 0.f, 0.f, 0.f};
  v4f acc[4];

  // end-of-quad ring step for the quad with virtual index QI inside the slice: peek the next
  // quad's first two records (same chunk) or, at a chunk end, commit and re-read
  auto ring_step = [&](auto qi_c) {
    constexpr int QL = decltype(qi_c)::value % CHQ;
    if constexpr (QL + 1 < CHQ) {
      a0 = rec(ic<QL + 1>{}, 0);
      a1 = rec(ic<QL + 1>{}, 1);
    }
  };
  auto ring_end = [&](auto qi_c) {
    constexpr int QL = decltype(qi_c)::value % CHQ;
    if constexpr (QL + 1 == (CHQ + 1) / 2 && CHQ > 1) stage_write();
    if constexpr (QL + 1 == CHQ) {
      if constexpr (CHQ == 1) stage_write();
      sync();
      issue_loads();
      rslot = (rslot + 1 == NSLOT) ? 0 : rslot + 1;
      cb = lds_rd + rslot * (CH * 1024);
      a0 = rec(ic<0>{}, 0);
      a1 = rec(ic<0>{}, 1);
    }
  };
#define SQUAD(QI, B0, B1, B2, B3)                                               \
  do {                                                                          \
    const v4f a2_ = rec(ic<(QI) % CHQ>{}, 2), a3_ = rec(ic<(QI) % CHQ>{}, 3);   \
    __builtin_amdgcn_sched_barrier(0);                                          \
    MFMA4(acc, a0, B0);                                                         \
    MFMA4(acc, a1, B1);                                                         \
    ring_step(ic<(QI)>{});                                                      \
    __builtin_amdgcn_sched_barrier(0);                                          \
    MFMA4(acc, a2_, B2);                                                        \
    MFMA4(acc, a3_, B3);                                                        \
    ring_end(ic<(QI)>{});                                                       \
  } while (0)
#define SQUAD1(QI, B0)         \
  do {                         \
    MFMA4(acc, a0, B0);        \
    ring_step(ic<(QI)>{});     \
    ring_end(ic<(QI)>{});      \
  } while (0)

  // ---- x operand ring: block v lives in xr[v % XD], requested XD-1 quads before its use --
  v4f xr[XD];
#pragma unroll
  for (int i = 0; i < XD; ++i) xr[i] = zero4;
  {
    const unsigned tt0 = pl.rev ? p.nsteps - 1 : 0;
    static_for<(NV0 < XD ? NV0 : XD)>([&](auto v) { xr[v.value] = bld4(pl.rx0, vo0, tt0 * pl.st0 + 64 * v.value); });
  }

  for (int step = 0; step < p.nsteps; ++step) {
    const unsigned tt = pl.rev ? p.nsteps - 1 - step : step;
    const unsigned ttn = step + 1 < p.nsteps ? (pl.rev ? tt - 1 : tt + 1) : tt;
    const unsigned o0 = tt * pl.st0, o2 = tt * pl.st2, oo = (tt + cy) * pl.sto, ok = tt * pl.stk;
    float xs0[NS0 > 0 ? NS0 : 1], xs2[NS2 > 0 ? NS2 : 1];   // 4-channel remainder blocks: lane (n, g) holds channel 4u + g
    static_for<NS0>([&](auto u) { xs0[u.value] = bld1(pl.rx0, vo0, o0 + 64 * NV0 + 16 * u.value); });
    static_for<NS2>([&](auto u) { xs2[u.value] = bld1(pl.rx2, pl.vo2, o2 + 64 * NV2 + 16 * u.value); });
    v4f xv2[NV2 > 0 ? NV2 : 1];   // the concatenated input is the same for every slice: held for the whole step
    static_for<NV2>([&](auto v) { xv2[v.value] = bld4(pl.rx2, vo2v, o2 + 64 * v.value); });
    if ((step > 0 || cy) && !(abl & 32)) {
      const unsigned op = (pl.rev ? tt + 1 : tt - 1 + cy) * pl.sto;
#pragma unroll
      for (int s = 0; s < NS; ++s) hold[s] = bld4(pl.ro, pl.voo, op + 64 * s);
    }

    for (int s = 0; s < NS; ++s) {
      v4f cprev = zero4, skipv = zero4;
      const unsigned nx = (s + 1 < NS ? tt : ttn) * pl.st0;   // x of the next slice / next step

      // quad 0: bias -> accumulators
      acc[0] = a0;
      acc[1] = a1;
      acc[2] = rec(ic<0>{}, 2);
      acc[3] = rec(ic<0>{}, 3);
      ring_step(ic<0>{});
      ring_end(ic<0>{});
      // summed input, 16 channels per quad
      static_for<NV0>([&](auto v) {
        constexpr int V = decltype(v)::value;
        const v4f xb = xr[V % XD];
        SQUAD(1 + V, xb.x, xb.y, xb.z, xb.w);
        if (!(abl & 1)) {
          if constexpr (V + XD < NV0)
            xr[V % XD] = bld4(pl.rx0, vo0, o0 + 64 * (V + XD));
          else
            xr[V % XD] = bld4(pl.rx0, vo0, nx + 64 * (V + XD - NV0));   // wraps into the next slice
        }
      });
      // cell state and residual operand of this slice: requested after the x part (whose ring
      // registers they reuse), still a whole recurrent part ahead of their use
      if ((step > 0 || cy) && !(abl & 16)) cprev = bld4(pl.rc, pl.vlane, s * 1024);
      if (SUM && !(abl & 16)) skipv = bld4(pl.rsk, pl.vok, ok + 64 * s);
      static_for<NS0>([&](auto u) { SQUAD1(1 + NV0 + decltype(u)::value, xs0[decltype(u)::value]); });
      static_for<NV2>([&](auto v) {
        constexpr int V = decltype(v)::value;
        SQUAD(1 + NV0 + NS0 + V, xv2[V].x, xv2[V].y, xv2[V].z, xv2[V].w);
      });
      static_for<NS2>([&](auto u) { SQUAD1(1 + NV0 + NS0 + NV2 + decltype(u)::value, xs2[decltype(u)::value]); });
      // recurrent part
      static_for<NS>([&](auto sp) {
        constexpr int SP = decltype(sp)::value;
        SQUAD(1 + NV0 + NS0 + NV2 + NS2 + SP, hold[SP].x, hold[SP].y, hold[SP].z, hold[SP].w);
      });
      // ring padding
      static_for<PAD>([&](auto u) {
        ring_step(ic<QPS + decltype(u)::value>{});
        ring_end(ic<QPS + decltype(u)::value>{});
      });
      // cell update
      if (ABL && (abl & 6)) {   // timing-ablation twin (wrong results): bit 2 = no gate math, bit 4 = no stores
        Cell c;
        if (abl & 2) {
          c.cn = acc[1] + cprev + acc[0];
          c.hn = acc[3] + acc[2];
        } else {
          c = cell_math(acc, cprev);
        }
        if (!(abl & 4)) {
          bst4(c.cn, pl.rc, pl.vlane, s * 1024);
          if (pl.valid) {
            bst4(c.hn, pl.ro, pl.voo, oo + 64 * s);
            if (SUM) bst4(add_rn4(c.hn, skipv), pl.ro2, pl.voo2, oo + 64 * s);
          }
        } else {
          asm volatile("" ::"v"(c.cn), "v"(c.hn));
        }
      } else {
        cell_step(pl, acc, cprev, skipv, s * 1024, oo + 64 * s);
      }
    }
  }
#undef SQUAD
#undef SQUAD1
}

template <int H, int NW, int M, int NV0, int NS0, int NS2, int CHQ, int PAD, int MODE, bool ABL = false, int XD = 4,
          int NV2 = 0>
int launch_static_k(const LstmParams& p, int nwg, const LaunchCtx& lc) {
  const size_t lds = (size_t)2 * CHQ * 4096;
  static_assert(2 * CHQ * 4096 <= 160 * 1024, "ring does not fit the LDS");
  return enqueue(lc, Kernel{lstm_static_kernel<H, NW, M, NV0, NS0, NS2, CHQ, PAD, MODE, ABL, XD, NV2>, NW * 64, lds, "lstm_static_kernel"}, nwg, p);
}

// Each returns kNoStatic when no specialisation exists for (c0, c2, mode, NW).
int launch_static_h128(const LstmParams& p, int mode, int NW, int nwg, const LaunchCtx& lc);
int launch_static_h256(const LstmParams& p, int mode, int NW, int nwg, const LaunchCtx& lc);
int launch_static3_h256(const LstmParams& p, int mode, int nwg, const LaunchCtx& lc);   // lstm_static3.h, pair-interleaved stream
int launch_static4_h256(const LstmParams& p, int mode, int nwg, const LaunchCtx& lc);   // lstm_static4.h, quad-interleaved stream
int launch_static_ipdnet(const LstmParams& p, int mode, int H, int NW, int nwg, const LaunchCtx& lc);

}  // namespace fnssl_lstm
