// "Wide" bf16-MFMA LSTM recurrence: 32 sequences per wave on v_mfma_f32_32x32x16_bf16 (BASELINE config 3).
//
// Why a second bf16 kernel (profiles/r02/c_pmc_ipdnet_bf16.json): lstm_bf16.h reads every weight from
// LDS once per step for only 16 sequences (1 KiB of ds_read per 16-cycle MFMA = the whole 256 B/clk LDS port at
// 4 waves per CU), stages the stream through VGPRs (ds_write_b128 costs 13 LDS cycles per KiB) one chunk ahead,
// and sits at 20 % MFMA-busy with its waves parked 41 % of the time.  Here
//   * a wave owns 32 sequences: one 1 KiB A record (32 gate rows x 16 channels) feeds a 32-cycle MFMA, so LDS reads
//     per flop halve and one wave per SIMD can keep its matrix pipe busy;
//   * the weight stream goes global -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds: no staging registers, no
//     ds_write) into a 3-slot ring of whole gate-row TILES (consuming T, T + 1 complete, T + 2 in flight: a whole
//     tile-time, > 1000 cycles, of cover for an L2 round trip), one workgroup barrier per tile, completion by a
//     hand-placed s_waitcnt vmcnt(0); the A operands are read from LDS AD = 4 records ahead of their MFMA, across
//     tile boundaries (without that depth every MFMA waits out an LDS round trip: measured 95 k cycles per step
//     against 35 k of MFMA issue);
//   * activations travel between layers as bf16 (they are rounded to bf16 on entry to the next MFMA anyway, so
//     the numbers are those of the fp32-in-HBM path) — x_t arrives as ready-made B operands, no conversion, half
//     the HBM bytes;
//   * the bias rides in the product: a constant-one "block" whose three live columns carry bias = hi + mid + lo
//     (three bf16 terms reproduce the fp32 bias exactly), consumed first, so every accumulator starts at +0;
//   * h_{t-1} (packed bf16 B operands) and the cell state (fp32) live in registers: the D fragment of tile T holds
//     the four gates of units 8T + 4*hb + j for the lane's own sequence, and the K order of the recurrent blocks
//     is permuted in the packer so that a lane's own outputs ARE its B operand of the next step; h_t is parked in
//     a lane-private LDS area during the step (8 bytes per tile) and reloaded as 16 operand registers at its end,
//     which frees the 64 registers a second operand set would take for the A-operand pipeline.
//
// Stream layout (fnssl_lstm_pack_bf16w): tile T (32 rows = [gate 0..3][unit 8T .. 8T+7]) = KT records of 1 KiB,
//   record 0          ones block   (k-slot (hb 0, i 0..2) = bias hi, mid, lo; everything else 0)
//   records 1..NKX    input blocks (16 channels each: src0 blocks, then src2 blocks), k = 16 b + 8 hb + i
//   then NKH records  recurrent blocks s: k-slot (hb, i) <-> unit 16 s + 8 (i >> 2) + 4 hb + (i & 3)
// A-operand element i of lane (row = lane & 31, hb = lane >> 5).
#pragma once

#include "lstm_static.h"

namespace fnssl_lstm {

typedef float v16f __attribute__((ext_vector_type(16)));
typedef __bf16 v8bfw __attribute__((ext_vector_type(8)));
typedef __bf16 v4bfw __attribute__((ext_vector_type(4)));
typedef unsigned int v2u __attribute__((ext_vector_type(2)));

// element types of the activation tensors of one launch (fnssl_lstm_desc.f32_mask)
constexpr int kW_F0 = 1, kW_F2 = 2, kW_OUTF = 4;   // bit set = that tensor is fp32

__host__ __device__ inline int bf16w_records_per_tile(int c0, int c2, int H) { return 1 + (c0 >> 4) + (c2 >> 4) + (H >> 4); }

// split_addr for a tensor of ES-byte elements: wave-uniform base (the wave's minimum) + per-lane byte offset
template <int ES>
__device__ __forceinline__ rsrc_t split_addr_e(const void* base, long long off_elems, unsigned& voff) {
  long long mn = off_elems;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const long long o = __shfl_xor(mn, d, 64);
    mn = o < mn ? o : mn;
  }
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(mn & 0xffffffffll));
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)mn >> 32));
  const long long mnu = (long long)(((unsigned long long)hi << 32) | lo);
  voff = (unsigned)((off_elems - mnu) * ES);
  return make_rsrc(reinterpret_cast<const char*>(base) + mnu * ES);
}

// LDS-DMA, one wave-instruction = 1 KiB: lane l's 16 bytes of the stream at soff + IMM land at lds + IMM + 16 l.  M0 is
// written in the same statement that reads it (the compiler does not preserve it); hipcc does not count this load: hence
// the hand-placed vmcnt(N) of the rings.  (readfirstlane: the operands are wave-uniform by construction; this makes the
// compiler keep them in SGPRs.)  The compile-time byte offset IMM is added to both the stream offset and the LDS
// destination inside the statement (two SALU adds with a literal instead of four instructions of address arithmetic).
template <int IMM>
__device__ __forceinline__ void dma16_imm(rsrc_t r, unsigned voff, unsigned soff, unsigned lds) {
  unsigned tmp;
  asm volatile("s_add_u32 m0, %3, %5\n\ts_add_u32 %0, %4, %5\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %0 offen lds"
               : "=&s"(tmp)
               : "v"(voff), "s"(r), "s"(__builtin_amdgcn_readfirstlane(lds)), "s"(__builtin_amdgcn_readfirstlane(soff)),
                 "n"(IMM)
               : "memory", "scc");   // s_add_u32 writes SCC: without the clobber the compiler keeps a loop condition in it
}

__device__ __forceinline__ v8bfw join8(v4bfw lo, v4bfw hi) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); }

// ---- pieces shared by the wide kernels (this file, lstm_bf16p.h, lstm_bf16c.h): what a wave does for its 32 sequences
//   wide_ones, wide_cell, wide_arec     bias operand; D fragment -> c_t, h_t; one A record from LDS          all three
//   wide_xblock, wide_store_h           one input block as a B operand; a lane's four units of h_t           bf16w, bf16p
//   wide_mfma, stage_h, reload_h        the MFMA of K-step K; h_t through the lane-private LDS area           bf16w, bf16p
//   WideSeq                             lane / sequence prologue with the tail rule                          bf16w
// lstm_bf16p_kernel keeps its own prologue: through WideSeq its H = 256 instantiations move one s_waitcnt lgkmcnt between
// neighbouring counts, and no smaller private piece puts it back (profiles/r16/README.md).  lstm_bf16c.h
// keeps its own: three parts per wave, each with a presence rule, outputs addressed after its lane-pair swap.  The deferred
// h store stays four variables in each kernel (as a struct, lstm_bf16w_kernel's NL = 0 instantiations move three such
// waits).  The rings, their barriers and the vmcnt accounting are different protocols and stay where they are.
// Everything is __forceinline__ and indexed at compile time; the three families are bit-identical to each other
// (tests/test_gpu_parity.py) because every one of them goes through wide_cell and the same MFMA order.

// input block b (16 channels: a lane's 8 are 16 b + 8 hb + i) of the row at byte offset `row` -> B operand
template <bool FP32>
__device__ __forceinline__ v8bfw wide_xblock(rsrc_t rx, unsigned vo, unsigned row, int b) {
  if constexpr (FP32) {
    const v4f a = bld4(rx, vo, row + 64 * b), c = bld4(rx, vo, row + 64 * b + 16);
    return join8(__builtin_convertvector(a, v4bfw), __builtin_convertvector(c, v4bfw));
  } else {
    return __builtin_bit_cast(v8bfw, bld4(rx, vo, row + 32 * b));
  }
}
// the lane's four units of one tile, fp32 or bf16, to byte offset `off` of its output row
template <bool FP32>
__device__ __forceinline__ void wide_store_h(rsrc_t ro, unsigned voo, const v4f& hn, v4bfw hb4, unsigned off) {
  if constexpr (FP32)
    bst4(hn, ro, voo, off);
  else
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, hb4), ro, voo, off, 0);
}

// Lane (n, hb) of a wave works on sequence n of 32-sequence group `task`: channels 8 hb + i of an input block, units
// 4 hb + j of a gate-row tile.  Tail rule, in ONE place: a lane past the last sequence computes the last sequence again
// (q clamped), a wave past the last group likewise; only `valid` lanes store h.
template <int H, int NB0, int NB2, int FLAGS>
struct WideSeq {
  static constexpr bool F0 = FLAGS & kW_F0, F2 = FLAGS & kW_F2, OUTF = FLAGS & kW_OUTF;
  static constexpr int E0 = F0 ? 4 : 2, E2 = F2 ? 4 : 2, EO = OUTF ? 4 : 2;   // element sizes by template flag
  static constexpr int kTileBytes = 8 * EO;                                  // one tile's 8 units in an output row
  int n, hb;
  bool valid, rev;
  unsigned vo0 = 0, vo2 = 0, voo = 0, vlane;   // per-lane byte offsets into the descriptors below
  rsrc_t rx0, rx2, ro, rw;                     // input, concatenated input, h, weight stream
  unsigned st0, st2, sto;                      // their step strides in bytes

  // unit0: the first hidden unit of the wave's tiles
  __device__ __forceinline__ WideSeq(const LstmParams& p, int lane, int dir, int task, int unit0) {
    n = lane & 31, hb = lane >> 5;
    int q = task * 32 + n;
    valid = q < p.nseq && task < p.task1;
    if (q >= p.nseq) q = p.nseq - 1;
    const long long qo = q / p.q_inner, qi = q - qo * p.q_inner;
    rx0 = make_rsrc(p.out), rx2 = make_rsrc(p.out);
    if constexpr (NB0 > 0) rx0 = split_addr_e<E0>(p.src0.p, qo * p.src0.so + qi * p.src0.si + 8 * hb, vo0);
    if constexpr (NB2 > 0) rx2 = split_addr_e<E2>(p.src2.p, qo * p.src2.so + qi * p.src2.si + 8 * hb, vo2);
    ro = split_addr_e<EO>(p.out, qo * p.out_so + qi * p.out_si + dir * H + unit0 + 4 * hb, voo);
    st0 = (unsigned)(p.src0.st * E0), st2 = (unsigned)(p.src2.st * E2), sto = (unsigned)(p.out_st * EO);
    rw = make_rsrc(p.wpack[dir]);
    vlane = lane * 16;
    rev = dir == 1;
  }
  // input block B (src0's blocks, then src2's) of time tt
  template <int B>
  __device__ __forceinline__ v8bfw load_x(ic<B>, unsigned tt) const {
    if constexpr (B < NB0)
      return wide_xblock<F0>(rx0, vo0, tt * st0, B);
    else
      return wide_xblock<F2>(rx2, vo2, tt * st2, B - NB0);
  }
  // h_t of one tile to byte offset `off` of the output row, if there is one (`live`) and the lane has a sequence
  __device__ __forceinline__ void store_h(const v4f& hn, v4bfw hb4, unsigned off, bool live = true) const {
    if (live && valid) wide_store_h<OUTF>(ro, voo, hn, hb4, off);
  }
};

// B operand of the ones block: k-slots (hb 0, i 0..2) = 1
__device__ __forceinline__ v8bfw wide_ones(int hb) {
  const __bf16 o1 = (__bf16)(hb == 0 ? 1.0f : 0.0f);
  return v8bfw{o1, o1, o1, 0, 0, 0, 0, 0};
}

// Gates of units 8 T + 4 hb + j (j = 0..3) of the lane's sequence: D register 4 * gate + j of tile T's accumulator.
// c: the cell state of those units, updated; returns h_t (fp32).  The ABLATE arms stay at the call sites.
__device__ __forceinline__ v4f wide_cell(const v16f& acc, v4f& c) {
  const v4f ig = sigmoid4(v4f{acc[0], acc[1], acc[2], acc[3]});
  const v4f fg = sigmoid4(v4f{acc[4], acc[5], acc[6], acc[7]});
  const v4f gg = tanh4(v4f{acc[8], acc[9], acc[10], acc[11]});
  const v4f og = sigmoid4(v4f{acc[12], acc[13], acc[14], acc[15]});
  const v4f cn = cell4(fg, c, ig, gg);
  const v4f hn = mul_rn4(og, tanh4(cn));
  c = cn;
  return hn;
}

// record r (1 KiB: 16 bytes per lane) behind `base`, this lane's 16 bytes of a record in LDS
__device__ __forceinline__ v8bfw wide_arec(const char* base, int r) {
  return __builtin_bit_cast(v8bfw, *reinterpret_cast<const v4f*>(base + r * 1024));
}

// the MFMA of K-step K of a tile: K = 0 the ones block (+ bias, exact), K <= NKX input block K - 1, then the recurrent blocks
template <int K, int NKX>
__device__ __forceinline__ v16f wide_mfma(v8bfw a, v8bfw ones, const v8bfw* xb, const v8bfw* hop, v16f acc) {
  if constexpr (K == 0)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ones, acc, 0, 0, 0);
  else if constexpr (K <= NKX)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xb[K - 1], acc, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, hop[K - 1 - NKX], acc, 0, 0, 0);
}

// h_t travels to the next step through a lane-private LDS area, hbuf = [block s][lane][16 B]: the lane's four units of
// tile G are elements 4 (G & 1) .. + 3 of operand block G / 2; reload_h makes the area the recurrent operands
__device__ __forceinline__ void stage_h(char* hbuf, int G, v4bfw hb4) {
  *reinterpret_cast<v4bfw*>(hbuf + (G >> 1) * 1024 + 8 * (G & 1)) = hb4;
}
template <int NKH>
__device__ __forceinline__ void reload_h(const char* hbuf, v8bfw* hop) {
#pragma unroll
  for (int i = 0; i < NKH; ++i) hop[i] = wide_arec(hbuf, i);
}

// NW consumer waves (32 sequences each) + NL loader waves.  NL = 0: the consumers fetch the stream themselves.  NL > 0
// (launches that leave SIMDs idle anyway — IPDnet's narrow-band layers at batch 64 are 2 groups per CU): the DMA issue
// (4 instructions per KiB) moves to waves on the idle SIMDs and the consumers' issue slots go to MFMAs and gate math.
// ABL (make ABLATE=1 builds only): timing ablations with wrong results — 1 no gate math, 2 no barriers, 4 no MFMAs,
// 8 no A-operand LDS reads, 16 no output stores / h staging, 32 no x loads
template <int H, int NW, int NB0, int NB2, int FLAGS, int NSLOT, int NL, int ABL = 0>
__global__ void __launch_bounds__((NW + NL) * 64) lstm_bf16w_kernel(const LstmParams p) {
  constexpr int NT = H / 8, NKH = H / 16, NKX = NB0 + NB2, KT = 1 + NKX + NKH;
  constexpr int NF = NL > 0 ? NL : NW;                    // waves that fetch
  constexpr int KP = KT / 2;                              // ring granule: half a tile ("piece")
  constexpr int KPW = (KP + NF - 1) / NF;                 // records each fetching wave requests per piece
  constexpr int NPS = 2 * NT;                             // pieces per step
  static_assert(KT % 2 == 0, "tiles are fetched in two pieces");
  constexpr int AD = 4;                                  // A-operand reads in flight ahead of the MFMA that uses them
  constexpr int RING = NSLOT * KT * 1024, HBUF = NKH * 1024;   // bytes: weight ring; one wave's h_t staging area
  static_assert(NSLOT == 3, "protocol below: consuming T, T + 1 landed, T + 2 in flight");
  static_assert(RING + NW * HBUF <= 160 * 1024, "ring + h staging do not fit the LDS");
  static_assert(AD < KT, "prefetch depth");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int dir = blockIdx.x / p.wgs_per_dir;
  const int wg = blockIdx.x - dir * p.wgs_per_dir;
  const WideSeq<H, NB0, NB2, FLAGS> q(p, lane, dir, p.task0 + wg * NW + w, 0);
  const unsigned lds0 = (unsigned)(size_t)smem;            // LDS byte address of the ring

  // ---- weight ring: NSLOT tiles = 6 half-tile pieces of KP KiB, one barrier per piece.  At the barrier that opens
  // piece j: piece j + 1 has landed everywhere (so the A-operand prefetch may run across the boundary), pieces
  // j + 2 .. j + 4 are in flight (1.5 tile-times, > 1500 cycles, of cover for an L2 round trip under load — with
  // whole tiles and one request in flight per loader the ring, not the MFMAs, set the pace: 2400 cycles per tile),
  // and everybody is done with piece j - 1, whose slot the request for piece j + 5 takes.  A fetching wave certifies
  // its share with s_waitcnt vmcnt(3 * KPW): loads complete in order, so all but its youngest 3 * KPW are done.
  const int fw = NL > 0 ? w - NW : w;                      // my index among the fetching waves (< 0: I do not fetch)
  const int rlast = fw + (KPW - 1) * NF < KP ? fw + (KPW - 1) * NF : KP - 1;   // past the end: repeat the last record
  auto fetch_piece = [&](int piece_in_step, int slot) {   // my share: records fw, fw + NF, ... of the piece
    const unsigned sb = (unsigned)(piece_in_step * KP) * 1024u, lb = lds0 + (unsigned)(slot * KP) * 1024u;
    static_for<KPW - 1>([&](auto mc) {
      dma16_imm<decltype(mc)::value * NF * 1024>(q.rw, q.vlane, sb + (unsigned)fw * 1024u, lb + (unsigned)fw * 1024u);
    });
    dma16_imm<0>(q.rw, q.vlane, sb + (unsigned)rlast * 1024u, lb + (unsigned)rlast * 1024u);
  };
  int ft = 0, fslot = 0;                                   // next piece to request (position inside the step), its slot
  auto fetch_next = [&]() {
    fetch_piece(ft, fslot);
    ft = ft + 1 == NPS ? 0 : ft + 1;
    fslot = fslot + 1 == 2 * NSLOT ? 0 : fslot + 1;
  };
  auto fetch_barrier = [&]() { asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(3 * KPW) : "memory"); };
  if (fw >= 0) {
#pragma unroll
    for (int i = 0; i < 5; ++i) fetch_next();
  }
  if constexpr (NL > 0) {
    if (w >= NW) {   // ---- loader wave: the same barrier sequence as the consumers, nothing but DMA in between
      const long long npieces = (long long)NPS * p.nsteps;
      for (long long g = 0; g < npieces; ++g) {
        if constexpr (ABL & 2)
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * KPW) : "memory");
        else
          fetch_barrier();
        fetch_next();
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      return;
    }
  }
  int cslot = 0;                                           // slot (in tiles) of the tile being consumed

  // ---- state ---------------------------------------------------------------------------------------------------
  const v4bfw zb4 = v4bfw{0, 0, 0, 0};
  const v8bfw ones = wide_ones(q.hb);
  v8bfw xb[NKX > 0 ? NKX : 1], xn[NKX > 0 ? NKX : 1];     // this step's / the next step's input operands
  v8bfw hop[NKH];                                          // h_{t-1} as B operands; h_t is staged in LDS (hbuf)
  v4f creg[NT];
#pragma unroll
  for (int i = 0; i < NKH; ++i) hop[i] = join8(zb4, zb4);
#pragma unroll
  for (int i = 0; i < NT; ++i) creg[i] = v4f{0.f, 0.f, 0.f, 0.f};
  char* const hbuf = smem + RING + w * HBUF + lane * 16;   // [block s][lane][16 B]: tile 2s -> bytes 0-7, 2s+1 -> 8-15

  static_for<NKX>([&](auto b) { xb[decltype(b)::value] = q.load_x(b, q.rev ? p.nsteps - 1 : 0); });

  const char* const lds_rd = smem + lane * 16;
  // With loader waves the consumers never wait on vector memory at a tile boundary (their x loads and h stores are
  // waited for where the compiler needs them); without, a wave also certifies its own DMA share.
  auto piece_barrier = [&]() {
    if constexpr (ABL & 2) return;
    if constexpr (NL > 0) {
      asm volatile("s_barrier" ::: "memory");
    } else {
      fetch_barrier();
      fetch_next();
    }
  };
  // the first piece of all: wait for it, publish, and prime the A pipeline
  piece_barrier();
  v8bfw apipe[AD];
#pragma unroll
  for (int i = 0; i < AD; ++i) apipe[i] = wide_arec(lds_rd, i);

  // Software pipeline over tiles: the gate math of tile T - 1 (VALU: 20 exp, 20 rcp, ~70 others per lane) is issued
  // in the shadow of tile T's MFMAs — its result is only needed by the NEXT step — so the matrix pipe does not idle
  // while a tile's D fragment is post-processed.  accp = the finished accumulator of the previous tile.
  v16f accp = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // NL == 0 only: the h store of a tile is issued one tile later still (right after a barrier), so that the
  // s_waitcnt vmcnt(0) of the following barrier finds it a whole tile-time old
  v4f pend_f = {0.f, 0.f, 0.f, 0.f};
  v4bfw pend_b = zb4;
  unsigned pend_off = 0;
  bool pend_live = false;
  auto gate = [&](auto tp, unsigned oo_t) {     // post-process tile TP (of the step whose output offset is oo_t)
    constexpr int TP = decltype(tp)::value;
    if constexpr (ABL & 1) {
      creg[TP] += v4f{accp[0], accp[5], accp[10], accp[15]};
      return;
    }
    const v4f hn = wide_cell(accp, creg[TP]);
    const v4bfw hb4 = __builtin_convertvector(hn, v4bfw);
    if constexpr (ABL & 16) {
      creg[TP].x += (float)hb4[0];
      return;
    }
    if constexpr (NL > 0)
      q.store_h(hn, hb4, oo_t + q.kTileBytes * TP);
    else
      pend_f = hn, pend_b = hb4, pend_off = oo_t + q.kTileBytes * TP, pend_live = true;
    stage_h(hbuf, TP, hb4);                                 // for the next step
  };
  auto flush_pending = [&]() {
    if constexpr (NL == 0) {
      q.store_h(pend_f, pend_b, pend_off, pend_live);
      pend_live = false;
    }
  };

  unsigned oo_prev = 0;
  for (int step = 0; step < p.nsteps; ++step) {
    const unsigned tt = q.rev ? p.nsteps - 1 - step : step;
    const unsigned ttn = step + 1 < p.nsteps ? (q.rev ? tt - 1 : tt + 1) : tt;
    const unsigned oo = tt * q.sto;

    static_for<NT>([&](auto tc) {
      constexpr int T = decltype(tc)::value;
      if (T > 0 || step > 0) piece_barrier();               // see the protocol above
      flush_pending();
      // the next step's input blocks trickle in, one block per tile
      if constexpr (T < NKX && !(ABL & 32)) xn[T] = q.load_x(ic<T>{}, ttn);

      const char* cb = lds_rd + cslot * (KT * 1024);
      cslot = cslot + 1 == NSLOT ? 0 : cslot + 1;
      const char* nb_ = lds_rd + cslot * (KT * 1024);       // the next tile (already complete in LDS)
      // previous tile's gates, to be scheduled under this tile's MFMAs
      if constexpr (T > 0) {
        gate(ic<T - 1>{}, oo);
      } else {
        if (step > 0) gate(ic<NT - 1>{}, oo_prev);
      }
      // (two alternating accumulators were tried — a same-accumulator MFMA chain with instructions in between pays a
      //  re-issue penalty — and lost 8 %: the chain is not what paces this loop)
      v16f acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      // record K of tile T sits in register (T * KT + K) % AD of the A pipeline, which runs on across tiles;
      // NT * KT % AD == 0, so the phase only depends on the tile's position inside the step
      static_assert((NT * KT) % AD == 0, "A pipeline phase must repeat every step");
      static_for<KT>([&](auto kc) {
        constexpr int K = decltype(kc)::value;
        constexpr int R = (T * KT + K) % AD;
        if constexpr (K == KP) piece_barrier();             // second half of the tile
        if constexpr (T == 0 && K == 1 + NKX) {
          if (step > 0) reload_h<NKH>(hbuf, hop);           // the last tile's h has just been staged (by this wave alone)
        }
        if constexpr (!(ABL & 4)) {
          const v8bfw a = apipe[R];
          if constexpr (!(ABL & 8)) apipe[R] = (K + AD < KT) ? wide_arec(cb, K + AD) : wide_arec(nb_, K + AD - KT);
          acc = wide_mfma<K, NKX>(a, ones, xb, hop, acc);
        } else {
          acc[K % 16] += (float)apipe[R][0];
          apipe[R] = (K + AD < KT) ? wide_arec(cb, K + AD) : wide_arec(nb_, K + AD - KT);
        }
      });
      accp = acc;
    });
    static_for<(NKX > NT ? NKX - NT : 0)>([&](auto e) { xn[NT + decltype(e)::value] = q.load_x(ic<NT + decltype(e)::value>{}, ttn); });
#pragma unroll
    for (int i = 0; i < NKX; ++i) xb[i] = xn[i];
    oo_prev = oo;
  }
  // epilogue: the last tile of the last step
  flush_pending();
  gate(ic<NT - 1>{}, oo_prev);
  flush_pending();
  // drain: the look-ahead requested tiles past the end (harmless re-reads of the stream's first tiles)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int H, int NW, int NB0, int NB2, int FLAGS, int NSLOT, int NL, int ABL = 0>
int launch_bf16w_k(const LstmParams& p, int nwg, const LaunchCtx& lc) {
  constexpr int KT = 1 + NB0 + NB2 + H / 16;
  const size_t lds = (size_t)NSLOT * KT * 1024 + (size_t)NW * (H / 16) * 1024;
  return enqueue(lc, Kernel{lstm_bf16w_kernel<H, NW, NB0, NB2, FLAGS, NSLOT, NL, ABL>, (NW + NL) * 64, lds, "lstm_bf16w_kernel"}, nwg, p);
}

// kNoStatic when the shape / element types have no instantiation
int launch_bf16w(const LstmParams& p, int H, int NW, int flags, int nwg, const LaunchCtx& lc);
// cluster_bytes = the size of p.cluster_ws (the hand-off area of the cluster-resident kernel, lstm_bf16c.h)
int forward_bf16w(LstmParams p, int H, int flags, size_t cluster_bytes, const LaunchCtx& lc, int* family = nullptr);

}  // namespace fnssl_lstm
