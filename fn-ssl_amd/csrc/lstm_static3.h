// Operand-ring kernel for the H = 256 narrow-band layers (round 4): two hidden slices per pass over a pair-interleaved
// weight stream, with the recurrent operand h_{t-1} STREAMED like the input operand x_t instead of held in 64 registers
// for the whole step, as its predecessor did (lstm_static2_kernel, round 3's two-slice kernel; removed in round 5).
//
// Why.  The predecessor needed 168 of the 168 registers three waves per SIMD allow — 64 of them for h_{t-1} — and its
// register demand peaked at the cell update; the allocator spilled the per-lane offsets of the residual operands to scratch
// memory, and each reload (scratch_load + s_waitcnt vmcnt(0)) drained the wave's whole prefetch window three times per
// slice pair: the residual-summing variant ran 3.3 % behind the plain one (112.2 against 108.5 ms per launch at config 2,
// profiles/r04/) for two extra memory operations per slice.  h_t is written to the output tensor anyway and every step
// already re-read it from there once; here each slice PAIR re-reads it through the same 4-deep operand ring as x_t:
// [x_t | h_{t-1}] is one stream of 32 sixteen-channel blocks per pass.  That is 16 more loads per pass (measured cost of a
// load beside the matrix instructions: ~13 cycles, tools/ubench/issue_model.hip: +0.6 %), and frees 48 registers: no
// spills (146 registers), and room for the concatenated 4-channel input of block 1, which had to stay on the one-slice
// kernel.  Measured at config 2 (profiles/r04/): 110.3 against 112.0 ms per launch with the fused residual, 107.5 against
// 109.2 without, 110.7 against 111.1 for block 1's layer.
//
// Same k order per sequence and slice as every other fp32 family, same gate code: bit-identical results.
// Step 0 reads h_{-1} = 0 through a descriptor with zero records (out-of-range buffer loads return 0): no branch around
// the loads.  The h row of step t - 1 is complete before step t starts (this wave wrote it; a wave's own accesses to one
// address stay ordered), exactly as the once-per-step reload of the one-slice kernel (lstm_static.h) assumes.
#pragma once

#include "lstm_static.h"

#pragma clang fp contract(off)

namespace fnssl_lstm {

template <int H, int NW, int M, int NV0, int NS2, int CHQ, int PAD, int MODE, int XD = 4>
__global__ void __launch_bounds__(NW * 64) lstm_static3_kernel(const LstmParams p) {
  FNSSL_GUARDED_KERNEL(p);
  constexpr int NS = H / 16, NP = NS / 2;
  constexpr bool HAS2 = (MODE & kHas2) != 0, SUM = (MODE & kSum) != 0;
  static_assert(!(MODE & kHas1) && HAS2 == (NS2 > 0) && NS % 2 == 0 && NS2 <= 1, "modes");
  constexpr int QPS = 1 + NV0 + NS2 + NS;               // real (pair-)quads per slice pair
  static_assert((QPS + PAD) % CHQ == 0, "chunks must tile the (padded) slice pair");
  static_assert(8 * CHQ <= NW * M, "chunk does not fit the staging registers");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const WaveSeq<H, NW, 1, HAS2, SUM> pl(p);
  // h_{-1} = 0: the same base with ZERO records — every lane is out of range and the load returns 0
  const rsrc_t rzero = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.out), 0, 0, 0x00020000);

  // ---- weight ring: 2 slots of CHQ pair-quads = 8 CHQ records, pair-interleaved stream ---------------------------------
  RegRing<NW, M, CHQ, PAD, QPS, 8, NP, ContiguousStream> ring(smem, pl.rw, pl.lane, pl.w, 0, {});
  ring.prime();

  const v4f zero4 = v4f{0.f, 0.f, 0.f, 0.f};
  v4f acc[8];                                      // [slice of the pair][gate]

  OperandRing<XD, NV0, NS> ops;
  constexpr int NB = OperandRing<XD, NV0, NS>::NB;
  ops.prime(pl.rx0, pl.vo0, (pl.rev ? p.nsteps - 1 : 0) * pl.st0);

  for (int step = 0; step < p.nsteps; ++step) {
    const unsigned tt = pl.rev ? p.nsteps - 1 - step : step;
    const unsigned ttn = step + 1 < p.nsteps ? (pl.rev ? tt - 1 : tt + 1) : tt;
    const unsigned o0 = tt * pl.st0, o2 = tt * pl.st2, oo = tt * pl.sto, ok = tt * pl.stk;
    const unsigned op = (pl.rev ? tt + 1 : tt - 1) * pl.sto;     // row of h_{step - 1} (not addressed at step 0: zero records)
    const rsrc_t rh = step > 0 ? pl.ro : rzero;
    float xs2 = 0.f;
    if (NS2) xs2 = bld1(pl.rx2, pl.vo2, o2);

    for (int pr = 0; pr < NP; ++pr) {
      const int s0 = 2 * pr;
#ifdef FNSSL_BUILD_ABLATE   // timing ablation (wrong results): FNSSL_STATIC3_ABL bit 1 = no operand loads in every second pass (what
      // four slices per pass would request), bit 2 = no operand loads at all
      const bool skip_ring = (p.ablate & 2) || ((p.ablate & 1) && (pr & 1));
#else
      constexpr bool skip_ring = false;
#endif
      v4f cprev0 = zero4, cprev1 = zero4, skip0 = zero4, skip1 = zero4;
      // the input blocks requested across the end of the pass: the same row, or (last pair) the next step's
      const unsigned nx = (pr + 1 == NP ? ttn : tt) * pl.st0;
      bias_step<2>(ring, ic<0>{}, acc);
      static_for<NB>([&](auto bc) {
        constexpr int B = decltype(bc)::value;
        constexpr int QI = B < NV0 ? 1 + B : 1 + NS2 + B;          // the 4-channel quad of block 1 sits between x and h
        if constexpr (NS2 > 0 && B == NV0) quad_step1<2>(ring, ic<1 + NV0>{}, acc, xs2);
        const v4f ob = ops.get(bc);
        quad_step<2>(ring, ic<QI>{}, acc, ob.x, ob.y, ob.z, ob.w);
        if (!skip_ring) ops.request(bc, pl.rx0, pl.vo0, o0, nx, rh, pl.voo, op);
        if constexpr (B == NB - 4) {       // cell state / residual operand of the first slice: four quads ahead of their use
          if (step > 0) cprev0 = bld4(pl.rc, pl.vlane, s0 * 1024);
          if (SUM) skip0 = bld4(pl.rsk, pl.vok, ok + 64 * s0);
        }
      });
      static_for<PAD>([&](auto u) { pad_step(ring, ic<QPS + decltype(u)::value>{}); });
      // cell updates of the two slices; the second one's cell state / residual operand in flight under the first's gate math
      if (step > 0) cprev1 = bld4(pl.rc, pl.vlane, s0 * 1024 + 1024);
      if (SUM) skip1 = bld4(pl.rsk, pl.vok, ok + 64 * s0 + 64);
      cell_step(pl, acc, cprev0, skip0, s0 * 1024, oo + 64 * s0);
      cell_step(pl, acc + 4, cprev1, skip1, s0 * 1024 + 1024, oo + 64 * s0 + 64);
    }
  }
}

template <int H, int NW, int M, int NV0, int NS2, int CHQ, int PAD, int MODE, int XD = 4>
int launch_static3_k(const LstmParams& p, int nwg, const LaunchCtx& lc) {
  const size_t lds = (size_t)2 * CHQ * 8192;
  static_assert(2 * CHQ * 8192 <= 160 * 1024, "ring does not fit the LDS");
  return enqueue(lc, Kernel{lstm_static3_kernel<H, NW, M, NV0, NS2, CHQ, PAD, MODE, XD>, NW * 64, lds, "lstm_static3_kernel"}, nwg, p);
}

}  // namespace fnssl_lstm
