// Shape-specialised kernel for launches with FEW 16-sequence groups (the training step's per-GPU shard):
// the compile-time slice structure of lstm_static.h (immediate LDS offsets, fixed ring commit points,
// 4-deep operand ring) combined with the hidden-slice split of lstm_rec_kernel — SPLIT waves of a
// workgroup share one group, wave part p computes slices [p*NS/SPLIT, (p+1)*NS/SPLIT) of every step,
// the ring carries super-quads (the same quad position of the SPLIT slices in flight), and all waves
// re-read the complete h_{t-1} from the output tensor after a workgroup barrier at the step end.
// Inputs: one tensor of 16*NV0 (+ NS0 = 1: a 4-channel one instead) channels, optionally a concatenated
// 4-channel tensor (NS2 = 1); MODE may carry kSave (training: gates + cell state to the reserve).
// Same k-ordered fp32 MFMA chain per sequence as every other fp32 kernel: bit-identical results.
#pragma once

#include "lstm_static.h"

namespace fnssl_lstm {

// A super-quad is the quads at one position of the SPLIT parts' slices, part by part (each wave reads its part's four
// records); the stream holds whole slices.  Record r of a chunk is record r & 3 of part (r / 4) % SPLIT at quad position
// r / (4 SPLIT) after the chunk's first.
template <int SPLIT, int NSL, int QPS>
struct SuperQuadStream {
  __device__ __forceinline__ int operator()(int /*rec*/, int unit, int vq, int r) const {
    const int sq = vq + r / (4 * SPLIT), pr = (r / 4) % SPLIT;
    return ((pr * NSL + unit) * QPS + sq) * 4 + (r & 3);
  }
};

// DIRECT = true: no LDS ring — each wave streams its own quads of the weight stream straight from L2 through a
// 4-quad-deep register pipeline (launches with few waves leave the L2 bandwidth to spare, and the ring's
// workgroup barriers — one per CHQ quads — are what limits the split geometries); CHQ / PAD / M are unused.
// NV2 = 16-channel blocks of the concatenated input (IPDnet), held in registers for the whole step.
template <int H, int NW, int M, int SPLIT, int NV0, int NS0, int NS2, int CHQ, int PAD, int MODE, bool DIRECT = false,
          int NV2 = 0>
__global__ void __launch_bounds__(NW * 64, (NW == 4 && !DIRECT ? 3 : 1)) lstm_split_static_kernel(const LstmParams p) {
  FNSSL_GUARDED_KERNEL(p);
  constexpr int NS = H / 16, NSL = NS / SPLIT;
  constexpr bool HAS2 = (MODE & kHas2) != 0, SAVE = (MODE & kSave) != 0, SUM = (MODE & kSum) != 0;
  static_assert(!(MODE & kHas1), "single summed input");
  static_assert(HAS2 == (NS2 + NV2 > 0) && NS2 <= 1 && NS0 <= 1 && !(NS0 && NV0), "input segments");
  static_assert(NS % SPLIT == 0 && NW % SPLIT == 0, "split geometry");
  constexpr int QPS = 1 + NV0 + NS0 + NV2 + NS2 + NS;  // real quads per slice
  constexpr int VQ = QPS + (DIRECT ? 0 : PAD);          // virtual quads per slice
  static_assert(DIRECT || VQ % CHQ == 0, "chunks must tile the (padded) slice");
  static_assert(!DIRECT || (NSL * QPS) % 4 == 0, "DIRECT: the 4-deep register pipeline must close once per step");
  static_assert(4 * CHQ * SPLIT <= NW * M, "chunk (CHQ super-quads) does not fit the staging registers");
  constexpr int XD = 4;
  static_assert(NV0 == 0 || NV0 % XD == 0, "the x ring depth must divide the block count");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const WaveSeq<H, NW, SPLIT, HAS2, SUM> pl(p);
  const unsigned vo0 = pl.vo0 - (NS0 ? 12 * pl.g : 0);   // remainder-only input: lane (n, g) reads channel g, not 4g..4g+3
  const unsigned vo2v = pl.vo2 + 12 * pl.g;   // 16-channel blocks of the concatenated input: lane (n, g) reads 4g..4g+3
  const rsrc_t rres = SAVE ? make_rsrc(reinterpret_cast<const char*>(p.reserve) +
                                       ((size_t)pl.dir * p.ntasks + (pl.tvalid ? pl.task : 0)) * p.nsteps *
                                           (size_t)(NS * kReserveRecs * 1024))
                           : pl.rc;
  const int part = pl.part;

  // ---- weight ring of super-quads -----------------------------------------------------
  RegRing<NW, M, CHQ, PAD, QPS, 4 * SPLIT, NSL, SuperQuadStream<SPLIT, NSL, QPS>> ring(smem, pl.rw, pl.lane, pl.w, part * 4096, {});
  if constexpr (!DIRECT) ring.prime();
  // DIRECT: ar[k] holds quad (cursor + k) of this wave's cyclic share of the stream: local slices
  // [part*NSL, (part+1)*NSL), QPS quads each, contiguous in the standard stream
  v4f ar[4][4];
  unsigned dq_off = 0;                                       // byte offset of the next quad to request
  const unsigned dq_base = (unsigned)(part * NSL * QPS) * 4096u, dq_len = (unsigned)(NSL * QPS) * 4096u;
  auto dq_load = [&](auto k) {
#pragma unroll
    for (int j = 0; j < 4; ++j) ar[decltype(k)::value][j] = bld4(pl.rw, pl.vlane, dq_base + dq_off + j * 1024u);
    dq_off = dq_off + 4096u == dq_len ? 0u : dq_off + 4096u;
  };
  if constexpr (DIRECT) {
    dq_load(ic<0>{});
    dq_load(ic<1>{});
    dq_load(ic<2>{});
    dq_load(ic<3>{});
  }

  v4f hold[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) hold[s] = v4f{0.f, 0.f, 0.f, 0.f};
  const v4f zero4 = v4f{0.f, 0.f, 0.f, 0.f};
  v4f acc[4];

  // (SL = the local slice being unrolled; in DIRECT mode quad SL*QPS + QI of the step lives in ar[.. % 4])
#define SQUAD(QI, B0, B1, B2, B3)                                 \
  do {                                                            \
    if constexpr (DIRECT) {                                       \
      constexpr int K_ = (SL * QPS + (QI)) % 4;                   \
      MFMA4(acc, ar[K_][0], B0);                                  \
      MFMA4(acc, ar[K_][1], B1);                                  \
      MFMA4(acc, ar[K_][2], B2);                                  \
      MFMA4(acc, ar[K_][3], B3);                                  \
      dq_load(ic<K_>{});                                          \
    } else {                                                      \
      quad_step<1>(ring, ic<(QI)>{}, acc, B0, B1, B2, B3);        \
    }                                                             \
  } while (0)
#define SQUAD1(QI, B0)                              \
  do {                                              \
    if constexpr (DIRECT) {                         \
      constexpr int K_ = (SL * QPS + (QI)) % 4;     \
      MFMA4(acc, ar[K_][0], B0);                    \
      dq_load(ic<K_>{});                            \
    } else {                                        \
      quad_step1<1>(ring, ic<(QI)>{}, acc, B0);     \
    }                                               \
  } while (0)

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
    const unsigned o0 = tt * pl.st0, o2 = tt * pl.st2, oo = tt * pl.sto, ok = tt * pl.stk;
    float xs0 = 0.f, xs2 = 0.f;
    if (NS0) xs0 = bld1(pl.rx0, vo0, o0);
    if (NS2) xs2 = bld1(pl.rx2, pl.vo2, o2 + 64 * NV2);
    v4f xv2[NV2 > 0 ? NV2 : 1];   // the concatenated input is the same for every slice: held for the whole step
    static_for<NV2>([&](auto v) { xv2[v.value] = bld4(pl.rx2, vo2v, o2 + 64 * v.value); });
    if (step > 0) {
      const unsigned op = (pl.rev ? tt + 1 : tt - 1) * pl.sto;
#pragma unroll
      for (int s = 0; s < NS; ++s) hold[s] = bld4(pl.ro, pl.voo, op + 64 * s);
    }

    static_for<NSL>([&](auto slc) {
      constexpr int SL = decltype(slc)::value;
      const unsigned sg = (unsigned)(part * NSL + SL);          // global hidden slice of this wave
      v4f cprev = zero4;
      const unsigned nx = (SL + 1 < NSL ? tt : ttn) * pl.st0;   // x of the next slice / next step
      if constexpr (DIRECT) {   // bias quad
        constexpr int K0 = (SL * QPS) % 4;
        acc[0] = ar[K0][0];
        acc[1] = ar[K0][1];
        acc[2] = ar[K0][2];
        acc[3] = ar[K0][3];
        dq_load(ic<K0>{});
      } else {
        bias_step<1>(ring, ic<0>{}, acc);
      }
      static_for<NV0>([&](auto v) {
        constexpr int V = decltype(v)::value;
        const v4f xb = xr[V % XD];
        SQUAD(1 + V, xb.x, xb.y, xb.z, xb.w);
        if constexpr (V + XD < NV0)
          xr[V % XD] = bld4(pl.rx0, vo0, o0 + 64 * (V + XD));
        else
          xr[V % XD] = bld4(pl.rx0, vo0, nx + 64 * (V + XD - NV0));   // wraps into the next slice
      });
      if (step > 0) cprev = bld4(pl.rc, pl.vlane, sg * 1024);
      v4f skipv = zero4;
      if (SUM) skipv = bld4(pl.rsk, pl.vok, ok + 64 * sg);
      if constexpr (NS0 > 0) SQUAD1(1 + NV0, xs0);
      static_for<NV2>([&](auto v) {
        constexpr int V2 = decltype(v)::value;
        SQUAD(1 + NV0 + NS0 + V2, xv2[V2].x, xv2[V2].y, xv2[V2].z, xv2[V2].w);
      });
      if constexpr (NS2 > 0) SQUAD1(1 + NV0 + NS0 + NV2, xs2);
      static_for<NS>([&](auto sp) {
        constexpr int SP = decltype(sp)::value;
        SQUAD(1 + NV0 + NS0 + NV2 + NS2 + SP, hold[SP].x, hold[SP].y, hold[SP].z, hold[SP].w);
      });
      if constexpr (!DIRECT) static_for<PAD>([&](auto u) { pad_step(ring, ic<QPS + decltype(u)::value>{}); });
      const Cell c = cell_step(pl, acc, cprev, skipv, sg * 1024, oo + 64 * sg);
      if (SAVE && pl.tvalid) {
        const unsigned rb = (tt * NS + sg) * (kReserveRecs * 1024);
        bst4(c.ig, rres, pl.vlane, rb);
        bst4(c.fg, rres, pl.vlane, rb + 1024);
        bst4(c.gg, rres, pl.vlane, rb + 2048);
        bst4(c.og, rres, pl.vlane, rb + 3072);
        bst4(c.cn, rres, pl.vlane, rb + 4096);
      }
    });
    // the partner waves read my h slices at the start of the next step: stores performed, then meet
    if constexpr (SPLIT > 1) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
  }
#undef SQUAD
#undef SQUAD1
}

template <int H, int NW, int M, int SPLIT, int NV0, int NS0, int NS2, int CHQ, int PAD, int MODE, bool DIRECT = false,
          int NV2 = 0>
int launch_split_static_k(const LstmParams& p, int nwg, const LaunchCtx& lc) {
  const size_t lds = DIRECT ? 0 : (size_t)2 * CHQ * SPLIT * 4096;
  static_assert(2 * CHQ * SPLIT * 4096 <= 160 * 1024, "ring does not fit the LDS");
  auto k = lstm_split_static_kernel<H, NW, M, SPLIT, NV0, NS0, NS2, CHQ, PAD, MODE, DIRECT, NV2>;
  return enqueue(lc, Kernel{k, NW * 64, lds, "lstm_split_static_kernel"}, nwg, p);
}

// kNoStatic when (H, nw, split, c0, c2, mode, chunk cap) has no instantiation; max_chq = LDS budget in super-quads
int launch_split_static(const LstmParams& p, int H, int nw, int split, int mode, int max_chq, int nwg, const LaunchCtx& lc);

}  // namespace fnssl_lstm
