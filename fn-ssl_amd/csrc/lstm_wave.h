// Building blocks shared by the shape-specialised fp32 LSTM kernels (lstm_static.h, lstm_static3.h, lstm_static4.h,
// lstm_split_static.h): what one wave does for its 16 sequences, whatever the kernel around it looks like.
//   WaveSeq      lane / sequence prologue: which sequences, which descriptors, the tail handling        (all four)
//   cell_step    gates -> c_t, h_t, h_t + skip, stored                                                   (all four)
//   OperandRing  [x_t | h_{t-1}] as one stream of sixteen-channel blocks, requested XD blocks ahead     (static3, static4)
//   RegRing      two-slot LDS weight ring filled through staging registers, on RingReader, its read side
//   quad_step    one operand block against 1 or 2 hidden slices: records read two ahead of their MFMAs
//                                                                     (ring and quad step: static3, split_static)
// lstm_static.h and lstm_static4.h keep their hand-written ring and quad macros: through these pieces the compiler
// allocates and peels their loops differently (profiles/r12/README.md).  Everything is __forceinline__
// and indexed at compile time; tools/isa_compare.py holds each kernel to its hand-written form.
#pragma once

#include "lstm_kernel.h"

#pragma clang fp contract(off)

namespace fnssl_lstm {

template <int I>
using ic = std::integral_constant<int, I>;

template <int N, int I = 0, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(ic<I>{});
    static_for<N, I + 1>(f);
  }
}

// ---- prologue ------------------------------------------------------------------------------------------------------
// Lane (n, g) of wave w works on sequence n of 16-sequence group `task`; SPLIT waves share a group (wave part `part`).
// Tail handling, in ONE place: a lane past the last sequence computes the last sequence again (q clamped) and a wave
// past the last group keeps its cell state in a private spare slot (p.ntasks + w), so that every wave runs the same
// instruction stream up to the barriers; only `valid` lanes store h.
template <int H, int NW, int SPLIT, bool HAS2, bool SUM>
struct WaveSeq {
  static constexpr bool kSum = SUM;
  int lane, n, g, w, dir, wg, part, task;
  bool tvalid, valid, rev;
  unsigned vo0 = 0, vo2 = 0, voo = 0, vok = 0, voo2 = 0, vlane;   // per-lane byte offsets into the descriptors below
  rsrc_t rx0, rx2, rsk, ro, ro2, rc, rw;                          // input, concatenated input, skip, h, h + skip, cell, weights
  unsigned st0, st2, sto, stk;                                    // their step strides in bytes

  __device__ __forceinline__ explicit WaveSeq(const LstmParams& p) {
    lane = threadIdx.x & 63;
    n = lane & 15, g = lane >> 4;
    w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    dir = blockIdx.x / p.wgs_per_dir;
    wg = blockIdx.x - dir * p.wgs_per_dir;
    part = w % SPLIT;
    task = p.task0 + wg * (NW / SPLIT) + w / SPLIT;
    tvalid = task < p.task1;
    int q = task * 16 + n;
    valid = q < p.nseq && tvalid;
    if (q >= p.nseq) q = p.nseq - 1;
    const long long qo = q / p.q_inner, qi = q - qo * p.q_inner;

    rx0 = split_addr(p.src0.p, qo * p.src0.so + qi * p.src0.si, 4 * g, vo0);
    rx2 = HAS2 ? split_addr(p.src2.p, qo * p.src2.so + qi * p.src2.si, g, vo2) : rx0;
    rsk = SUM ? split_addr(p.skip.p, qo * p.skip.so + qi * p.skip.si, dir * H + 4 * g, vok) : rx0;
    ro = split_addr(p.out, qo * p.out_so + qi * p.out_si, dir * H + 4 * g, voo);
    ro2 = SUM ? split_addr(p.out_sum, qo * p.out_so + qi * p.out_si, dir * H + 4 * g, voo2) : ro;
    rc = make_rsrc(cell_record<H / 16>(p.cscratch, p.ntasks, dir, tvalid ? task : p.ntasks + w));
    rw = make_rsrc(p.wpack[dir]);
    st0 = (unsigned)(p.src0.st * 4), st2 = HAS2 ? (unsigned)(p.src2.st * 4) : 0u;
    sto = (unsigned)(p.out_st * 4), stk = SUM ? (unsigned)(p.skip.st * 4) : 0u;
    vlane = lane * 16;
    rev = dir == 1;
  }
};

// ---- weight ring ---------------------------------------------------------------------------------------------------
// Read side: two slots of CHQ virtual quads, RPQ records (1 KiB: 16 bytes per lane) per quad.  Every read is `chunk base
// + immediate`; a0 / a1 are the first two records of the NEXT quad, read one half-quad ahead of their MFMAs.
template <int CHQ, int RPQ>
struct RingReader {
  static constexpr int kCHQ = CHQ, CH = RPQ * CHQ;   // quads, records per chunk
  const char* lds_rd;                             // this lane's 16 bytes of record 0, slot 0
  const char* cb;                                 // ... of the chunk being read
  int rslot = 0;
  v4f a0, a1;

  __device__ __forceinline__ explicit RingReader(const char* rd) : lds_rd(rd), cb(rd) {}
  template <int QL>
  __device__ __forceinline__ v4f rec(ic<QL>, int j) const {   // record j of quad QL of the current chunk
    return *reinterpret_cast<const v4f*>(cb + QL * (RPQ * 1024) + j * 1024);
  }
  __device__ __forceinline__ void peek() {
    a0 = rec(ic<0>{}, 0);
    a1 = rec(ic<0>{}, 1);
  }
  // end-of-quad step for the quad with virtual index QI inside the slice: peek the next quad of the same chunk (at a
  // chunk end, the ring's end() commits and re-reads)
  template <int QI>
  __device__ __forceinline__ void step(ic<QI>) {
    constexpr int QL = QI % CHQ;
    if constexpr (QL + 1 < CHQ) {
      a0 = rec(ic<QL + 1>{}, 0);
      a1 = rec(ic<QL + 1>{}, 1);
    }
  }
  __device__ __forceinline__ void flip() {
    rslot ^= 1;
    cb = lds_rd + rslot * (CH * 1024);
    peek();
  }
};

// Filled through M staging registers per lane: wave w carries records w, w + NW, ... of a chunk L2 -> registers -> LDS.
// A slice (pair, quad of slices: the ring's unit, NU of them per step) is QPS real quads in the stream and PAD more
// virtual ones in the ring, so that chunks tile it.  `src(rec, unit, vq, r)` is the one thing that differs between the
// callers: the stream index of record r of the next chunk, from whichever of the ring's running positions suits the
// stream's layout (the ones a caller does not use cost nothing).
template <int NW, int M, int CHQ, int PAD, int QPS, int RPQ, int NU, class Src>
struct RegRing : RingReader<CHQ, RPQ> {
  using RingReader<CHQ, RPQ>::CH;
  static constexpr int VQ = QPS + PAD;
  const rsrc_t rw;
  const unsigned vlane;
  const int w;
  char* const lds_wr;
  const Src src;
  int wslot = 0;          // slot the staged chunk is committed to
  int src_rec = 0;        // records staged so far this step, padding not counted
  int src_unit = 0;       // unit of the next chunk to stage
  int src_vq = 0;         // its first virtual quad inside the unit
  v4f stg[M];

  // rd_off: where inside a quad this wave starts reading (a SPLIT part reads its own 4 records)
  __device__ __forceinline__ RegRing(char* smem, rsrc_t rw_, int lane, int w_, int rd_off, Src src_)
      : RingReader<CHQ, RPQ>(smem + lane * 16 + rd_off), rw(rw_), vlane(lane * 16), w(w_),
        lds_wr(smem + w_ * 1024 + lane * 16), src(src_) {}

  __device__ __forceinline__ void issue_loads() {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int r = w + m * NW;
      // (formed ahead of the test: inside it, the compiler computes split_static's index in vector registers and wraps
      // the load in a loop over its distinct values)
      const int sr = src(src_rec, src_unit, src_vq, r);
      if (r < CH && src_vq + r / RPQ < QPS) stg[m] = bld4(rw, vlane, (unsigned)sr * 1024u);
    }
    src_vq += CHQ;
    src_rec += CH;
    if (src_vq == VQ) {
      src_vq = 0;
      src_rec -= PAD * RPQ;                       // the padding quads do not exist in the stream
      src_unit = src_unit + 1 == NU ? 0 : src_unit + 1;
      if (src_rec == NU * QPS * RPQ) src_rec = 0;
    }
  }
  // The staged chunk goes to the slot that was read during the PREVIOUS chunk period, which is free for the whole
  // current period, so the wait-for-data + ds_write sits in the middle of the chunk (where waves are not lined up at a
  // barrier and the in-order vmcnt wait costs least) and the chunk end is only `lgkmcnt(0); s_barrier`.
  __device__ __forceinline__ void stage_write() {
#pragma unroll
    for (int m = 0; m < M; ++m)
      if (w + m * NW < CH) *reinterpret_cast<v4f*>(lds_wr + wslot * (CH * 1024) + m * (NW * 1024)) = stg[m];
    wslot ^= 1;
  }
  __device__ __forceinline__ void sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
  __device__ __forceinline__ void prime() {
    issue_loads();
    stage_write();
    sync();
    issue_loads();
    this->peek();
  }
  template <int QI>
  __device__ __forceinline__ void end(ic<QI>) {
    constexpr int QL = QI % CHQ;
    if constexpr (QL + 1 == (CHQ + 1) / 2 && CHQ > 1) stage_write();
    if constexpr (QL + 1 == CHQ) {
      if constexpr (CHQ == 1) stage_write();
      sync();
      issue_loads();
      this->flip();
    }
  }
};

// the stream holds the ring's units one after the other (static, static3)
struct ContiguousStream {
  __device__ __forceinline__ int operator()(int rec, int, int, int r) const { return rec + r; }
};

// ---- quad step -----------------------------------------------------------------------------------------------------
// One operand block (B0..B3: its four k values of this lane's sequence) against NSLICE hidden slices: 4 NSLICE records of
// quad QI, two MFMA4s per pair of records, each pair read while the previous pair's MFMAs issue; the last pair overlaps
// the peek of the next quad.  The sched_barriers pin that order: without them the compiler hoists all reads to the top
// and the accumulators' neighbours pay for the registers.  acc: [slice][gate].
template <int NSLICE, int QI, class Ring>
__device__ __forceinline__ void quad_step(Ring& ring, ic<QI>, v4f* acc, float B0, float B1, float B2, float B3) {
  constexpr int QL = QI % Ring::kCHQ;
  v4f r0[2 * NSLICE], r1[2 * NSLICE];   // pair k = records 2k, 2k + 1: slice k / 2, k values (B0, B1) or (B2, B3)
  r0[0] = ring.a0, r1[0] = ring.a1;
  static_for<2 * NSLICE>([&](auto kc) {
    constexpr int K = decltype(kc)::value;
    if constexpr (K + 1 < 2 * NSLICE) {
      r0[K + 1] = ring.rec(ic<QL>{}, 2 * K + 2);
      r1[K + 1] = ring.rec(ic<QL>{}, 2 * K + 3);
    } else {
      ring.step(ic<QI>{});
    }
    __builtin_amdgcn_sched_barrier(0);
    v4f* const as = acc + 4 * (K / 2);
    MFMA4(as, r0[K], (K % 2 ? B2 : B0));
    MFMA4(as, r1[K], (K % 2 ? B3 : B1));
  });
  ring.end(ic<QI>{});
}
// ... a 4-channel remainder block: one k value per lane, the first record of each slice
template <int NSLICE, int QI, class Ring>
__device__ __forceinline__ void quad_step1(Ring& ring, ic<QI>, v4f* acc, float B0) {
  constexpr int QL = QI % Ring::kCHQ;
  v4f r[NSLICE];
  r[0] = ring.a0;
  static_for<NSLICE - 1>([&](auto sc) { r[sc.value + 1] = ring.rec(ic<QL>{}, 4 * (sc.value + 1)); });
  static_for<NSLICE>([&](auto sc) {
    v4f* const as = acc + 4 * sc.value;
    MFMA4(as, r[sc.value], B0);
  });
  ring.step(ic<QI>{});
  ring.end(ic<QI>{});
}
// ... no operand at all: the bias quad (records -> accumulators) and the ring's padding quads
template <int NSLICE, int QI, class Ring>
__device__ __forceinline__ void bias_step(Ring& ring, ic<QI>, v4f* acc) {
  acc[0] = ring.a0;
  acc[1] = ring.a1;
  static_for<4 * NSLICE - 2>([&](auto j) { acc[j.value + 2] = ring.rec(ic<QI % Ring::kCHQ>{}, j.value + 2); });
  ring.step(ic<QI>{});
  ring.end(ic<QI>{});
}
template <int QI, class Ring>
__device__ __forceinline__ void pad_step(Ring& ring, ic<QI>) {
  ring.step(ic<QI>{});
  ring.end(ic<QI>{});
}

// ---- operand ring --------------------------------------------------------------------------------------------------
// Block b of a pass (b < NV0: channels 16 b.. of x_t; else hidden units 16 (b - NV0).. of h_{t-1}) lives in br[b % XD]
// and is requested right after block b - XD has been consumed.
template <int XD, int NV0, int NS>
struct OperandRing {
  static constexpr int NB = NV0 + NS;   // sixteen-channel operand blocks per pass
  static_assert(NB % XD == 0 && XD <= NV0, "the operand ring depth must divide the block count");
  v4f br[XD];

  __device__ __forceinline__ void prime(rsrc_t rx0, unsigned vo0, unsigned o0) {
    static_for<XD>([&](auto v) { br[v.value] = bld4(rx0, vo0, o0 + 64 * v.value); });
  }
  template <int B>
  __device__ __forceinline__ v4f get(ic<B>) const {
    return br[B % XD];
  }
  // request block B + XD into block B's register: of this pass (x_t at o0, h_{t-1} through rh at op) or, wrapping, of
  // the next pass or step (x at nx)
  template <int B>
  __device__ __forceinline__ void request(ic<B>, rsrc_t rx0, unsigned vo0, unsigned o0, unsigned nx, rsrc_t rh,
                                          unsigned voo, unsigned op) {
    constexpr int BN = (B + XD) % NB;
    if constexpr (B + XD < NB) {
      if constexpr (BN < NV0)
        br[B % XD] = bld4(rx0, vo0, o0 + 64 * BN);
      else
        br[B % XD] = bld4(rh, voo, op + 64 * (BN - NV0));
    } else {
      static_assert(BN < NV0, "the wrapped requests are input blocks");
      br[B % XD] = bld4(rx0, vo0, nx + 64 * BN);
    }
  }
};

// ---- cell update ---------------------------------------------------------------------------------------------------
struct Cell {
  v4f ig, fg, gg, og, cn, hn;
};
// `between` runs after the gates and before the cell update: where static3 and static4 request the NEXT slice's cell
// state / residual operand (in flight under this slice's gate math; requested any earlier, the kernels at their register
// limit are allocated differently and wait in front of the gate math — profiles/r12/).
template <class F>
__device__ __forceinline__ Cell cell_math(const v4f* acc, const v4f& cprev, F&& between) {
  Cell c;
  c.ig = sigmoid4(acc[0]);
  c.fg = sigmoid4(acc[1]);
  c.gg = tanh4(acc[2]);
  c.og = sigmoid4(acc[3]);
  const v4f cp = cprev;
  between();
  c.cn = cell4(c.fg, cp, c.ig, c.gg);
  c.hn = mul_rn4(c.og, tanh4(c.cn));
  // h + skip adds the ROUNDED h, as the generic kernel and the reference do: behind this fence h is a value in
  // registers, not an expression the compiler may fold into the add as one fma (the fp32 families are bit-identical to
  // each other, with and without the fused residual, because every one of them goes through here)
  asm("" : "+v"(c.hn.x), "+v"(c.hn.y), "+v"(c.hn.z), "+v"(c.hn.w));
  return c;
}
__device__ __forceinline__ Cell cell_math(const v4f* acc, const v4f& cprev) {
  return cell_math(acc, cprev, [] {});
}
// Gates of one slice -> c_t to the cell record (byte offset coff), h_t and h_t + skip to their rows (byte offset hoff).
// The offsets come as the callers' loops form them (s0 * 1024 + 1024, oo + 64 * s0 + 64, ...): a slice index multiplied
// in here costs scalar arithmetic per slice.  Returns the gates: split_static's kSave stores (profiles/r12/README.md).
template <class Seq, class F>
__device__ __forceinline__ Cell cell_step(const Seq& q, const v4f* acc, const v4f& cprev, const v4f& skip, unsigned coff,
                                          unsigned hoff, F&& between) {
  const v4f sk = skip;
  const Cell c = cell_math(acc, cprev, between);
  bst4(c.cn, q.rc, q.vlane, coff);
  if (q.valid) {
    bst4(c.hn, q.ro, q.voo, hoff);
    if (Seq::kSum) bst4(add_rn4(c.hn, sk), q.ro2, q.voo2, hoff);
  }
  return c;
}
template <class Seq>
__device__ __forceinline__ Cell cell_step(const Seq& q, const v4f* acc, const v4f& cprev, const v4f& skip, unsigned coff,
                                          unsigned hoff) {
  return cell_step(q, acc, cprev, skip, coff, hoff, [] {});
}

}  // namespace fnssl_lstm
