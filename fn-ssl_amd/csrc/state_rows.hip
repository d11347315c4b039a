// Rows of a carried state that is a LIST of batch-leading tensors (the forward_stream dicts of FN-SSL and IPDnet: per
// narrow-band layer the cell block of its LSTM workspace and the h / tail tensors beside it): fnssl_state_rows moves the
// rows of some slots of a pool's state to a compact state and back, across every tensor of the list, in one launch per 64
// rows.  The general form of fnssl_sn_state_rows (spatialnet.hip), whose state is one buffer with a layout of its own.
#include <cstdint>
#include <vector>

#include "host.h"

using fnssl::enqueue;
using fnssl::Kernel;

namespace {

constexpr int kRowsPerLaunch = 64;
constexpr int kThreads = 256;
constexpr int kQuadsPerThread = 8;

// The segment table, the slot list and the flags travel by value in the kernel arguments: no host-to-device copy, no
// staging buffer the next call could overwrite.
struct StateRowsParams {
  fnssl_state_seg seg[FNSSL_STATE_ROWS_MAX_SEGS];
  unsigned row0;                                          // this launch serves compact rows row0 .. row0 + gridDim.y - 1
  int scatter;
  int slot[kRowsPerLaunch];
  unsigned char fresh[kRowsPerLaunch];
};
static_assert(sizeof(StateRowsParams) <= 4096, "the table and the slot list of one launch must fit the kernel-argument segment");

// blockIdx.z is the segment, blockIdx.y the compact row, the x dimension strides over the row's float4s: consecutive
// threads copy consecutive float4s on both sides, so the copy streams; no LDS, no atomics.  The x extent is sized for the
// longest segment; workgroups past the end of a shorter one have nothing to do.
__global__ void __launch_bounds__(kThreads) state_rows_kernel(const StateRowsParams p) {
  const fnssl_state_seg s = p.seg[blockIdx.z];
  const unsigned a = blockIdx.y;
  const unsigned nq = (unsigned)(s.row_floats / 4);       // (the host has checked row_floats < 2^32)
  const size_t row4 = (size_t)nq;
  float4* const pool = reinterpret_cast<float4*>(s.pool) + (size_t)p.slot[a] * row4;
  float4* const comp = reinterpret_cast<float4*>(s.compact) + (size_t)(p.row0 + a) * row4;
  const bool zero = !p.scatter && p.fresh[a];
  for (size_t q = (size_t)blockIdx.x * kThreads + threadIdx.x; q < nq; q += (size_t)gridDim.x * kThreads) {
    if (p.scatter) pool[q] = comp[q];
    else comp[q] = zero ? make_float4(0.f, 0.f, 0.f, 0.f) : pool[q];
  }
}

}  // namespace

extern "C" {

int fnssl_state_rows(const fnssl_state_seg* segs, int nsegs, int nslots, int nrows, const int* slots,
                     const unsigned char* fresh, int direction, void* stream) {
  FNSSL_REQUIRE(segs && slots, "state_rows: null pointer");
  FNSSL_REQUIRE(nsegs >= 1 && nsegs <= FNSSL_STATE_ROWS_MAX_SEGS, "state_rows: %d segments (1..%d)", nsegs,
                FNSSL_STATE_ROWS_MAX_SEGS);
  FNSSL_REQUIRE(direction == FNSSL_SN_ROWS_GATHER || direction == FNSSL_SN_ROWS_SCATTER, "state_rows: direction %d", direction);
  FNSSL_REQUIRE(nslots > 0 && nrows > 0 && nrows <= nslots, "state_rows: %d rows of %d slots", nrows, nslots);
  long long longest = 0;
  for (int k = 0; k < nsegs; ++k) {
    const fnssl_state_seg& s = segs[k];
    FNSSL_REQUIRE(s.pool && s.compact, "state_rows: segment %d: null pointer", k);
    FNSSL_REQUIRE((uintptr_t)s.pool % 16 == 0 && (uintptr_t)s.compact % 16 == 0,
                  "state_rows: segment %d: the tensors must be 16-byte aligned", k);
    FNSSL_REQUIRE(s.row_floats > 0 && s.row_floats % 4 == 0 && s.row_floats < (1ll << 32),
                  "state_rows: segment %d: a row of %lld floats (a positive multiple of 4 below 2^32)", k, s.row_floats);
    FNSSL_REQUIRE(s.pool != s.compact, "state_rows: segment %d: pool and compact tensor are the same", k);
    for (int j = 0; j < k; ++j)
      FNSSL_REQUIRE(s.pool != segs[j].pool && s.pool != segs[j].compact && s.compact != segs[j].pool &&
                        s.compact != segs[j].compact,
                    "state_rows: segment %d shares a tensor with segment %d (the tensors must be distinct)", k, j);
    longest = s.row_floats > longest ? s.row_floats : longest;
  }
  std::vector<char> seen(nslots, 0);
  for (int a = 0; a < nrows; ++a) {
    FNSSL_REQUIRE(slots[a] >= 0 && slots[a] < nslots, "state_rows: row %d: slot %d of %d", a, slots[a], nslots);
    FNSSL_REQUIRE(!seen[slots[a]], "state_rows: row %d: slot %d appears twice", a, slots[a]);
    seen[slots[a]] = 1;
  }
  StateRowsParams p{};
  for (int k = 0; k < nsegs; ++k) p.seg[k] = segs[k];
  p.scatter = direction == FNSSL_SN_ROWS_SCATTER;
  hipStream_t s = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl(p.scatter ? "state_scatter" : "state_gather", s);
  // enough workgroups per row to fill the device at one row, at most 8 float4 per thread
  const size_t per_wg = (size_t)kThreads * kQuadsPerThread;
  const unsigned gx = (unsigned)(((size_t)longest / 4 + per_wg - 1) / per_wg);
  for (int r0 = 0; r0 < nrows; r0 += kRowsPerLaunch) {
    const int n = nrows - r0 < kRowsPerLaunch ? nrows - r0 : kRowsPerLaunch;
    p.row0 = (unsigned)r0;
    for (int a = 0; a < n; ++a) {
      p.slot[a] = slots[r0 + a];
      p.fresh[a] = fresh ? fresh[r0 + a] : 0;
    }
    FNSSL_TRY(enqueue(s, Kernel{state_rows_kernel, kThreads, 0, "state_rows_kernel"}, dim3(gx, (unsigned)n, (unsigned)nsegs), p));
  }
  return FNSSL_OK;
}

}  // extern "C"
