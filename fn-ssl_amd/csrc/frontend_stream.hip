// The front end for a stream of microphone samples: ONE launch per pushed chunk takes the new samples to normalised
// network features, continuing the recursive magnitude normalisation from a carried mu, and produces the bits
// fnssl_stft_ex + fnssl_pair_features / fnssl_array_features (layout 0) give on the whole signal.
//
// The hop-256 transform is not centred, so frame t is a function of samples [256 t, 256 t + 512) alone; the recursion is a
// sequential chain per microphone pair (pair mode) or per utterance (array mode).  Frame t's features need mu_t, which
// needs every channel's magnitude sum up to t, so ONE workgroup serves an utterance and the dependency stays inside its
// barriers: per tile of kStreamTile frames
//   A  the waves transform the tile's (frame, channel) windows side by side (frontend_core.h: the whole-signal kernels'
//      own window, radix-4 transform and bin split), keep bins 1..256 and the wave-reduced sum_k |X[k]|;
//   B  one wave per chain forms the tile's means and runs the recursion from the carried mu (ema_scan_tile);
//   C  all threads divide by (mu_t + eps) and write the feature rows.
// The tile's spectra live in LDS while they fit (12 frames x 4 channels = 96 KiB beside the transform staging) and in a
// caller-owned scratch inside the state otherwise (8 channels: 192 KiB): written in A, re-read in C by other waves of the
// SAME workgroup behind the workgroup barrier, whose workgroup-scope release / acquire is all that needs (one CU, one L1).
//
// IPDnet2's transform (fnssl_stream_frontend_centred) is the same kernel with two compile-time parameters: hop 320, and
// CENTRED = torch.stft(center=True), where frame t covers samples 320 t - 256 .. 320 t + 255 of the signal extended by
// reflection.  The index is folded per sample in phase A exactly as the whole-signal kernels fold it (the start always,
// the end only once the caller knows the total length); everything after the fetch is the code of the hop-256
// instantiations, whose bits therefore stay what they were.  Its tile is 10 frames (two of the 5-frame groups IPDnet2's
// time pooling consumes): 10 frames x 5 channels = 100 KiB of spectra beside the 37 KiB of staging, so the shipped
// five-microphone array (and six channels) stays in LDS; from 7 channels on a full tile goes through the scratch.
//
// A pool of independent streams (fnssl_stream_frontend_centred_pool) is the third compile-time parameter, POOL: workgroup
// i serves the stream of descriptor i (its own first frame, frame count, window, total length, state row and output row;
// a fresh stream starts from mu = 0 without a memset), so ONE launch serves any subset of the pool's slots, each at its
// own position.  Its tile is always the full 10 frames, so the scratch rows keep the spacing the state was sized with.
// fnssl_stream_frontend_pool is the same for the hop-256 models (<0, 0, 1> FN-SSL pairs, <1, 0, 1> IPDnet arrays), with
// the full 12-frame tile: a descriptor's np pair rows follow each other in x (row out_row * np + pair).
#include <cstdint>
#include <type_traits>
#include <vector>

#include "host.h"
#include "frontend_core.h"

using fnssl::enqueue;
using fnssl::Kernel;

namespace {

using namespace fnssl_frontend;

constexpr int kStreamWaves = 16;
constexpr int kStreamThreads = kStreamWaves * 64;
constexpr int kStreamTile = 12;            // frames per pass: the chunk the online models consume
constexpr int kCentredTile = 10;           // the centred hop-320 entry: two groups of IPDnet2's time pooling
constexpr int kCentredHop = 320;
constexpr int kStreamMaxCh = 16;
constexpr size_t kLdsBudget = 160 * 1024;
constexpr size_t kStateAlign = 256;

struct StreamParams {
  const float* sig;        // first sample of frame `frame0`; CENTRED: sample `sample0` of the signal
  long long sb, sn, sc;
  long long sample0;       // CENTRED: absolute index of sig's first sample
  long long total;         // CENTRED: length of the whole signal, negative while it is not known (no end reflection)
  int nch, nchain, ch_mode;
  int frame0, nframes, tile, sample_length;
  const float* ca;         // [sample_length + 1], indexed by min(t, sample_length)
  const float* cb;
  float eps;
  float* mu;               // [nb, nchain], carried
  float2* scratch;         // nullptr: spectra in LDS; else [nb][tile * nch * 256]
  float* x;                // pair: [nb * np, nframes, 256, 4]; array: [nb, nframes, 256, 2 nch]
};

// The pool entry (fnssl_stream_frontend_centred_pool): every workgroup is an independent stream and takes what the other
// instantiations share (first frame, frame count, window position, total length, signal base, state row, output row)
// from its own descriptor.  The descriptors travel by value in the kernel arguments, so a push makes no host-to-device
// copy and owns no staging buffer the next push could overwrite; kPoolMaxDesc of them and the shared parameters stay
// under the 4 KiB the kernel-argument segment holds.
constexpr int kPoolMaxDesc = FNSSL_STREAM_POOL_MAX_DESC;

struct PoolParams {
  StreamParams p;          // the shared part: strides, channels, tables, eps, state, x; frame0 / nframes / sample0 / total unused
  int out_frames;          // frames of one row of x
  fnssl_stream_pool_desc d[kPoolMaxDesc];
};
static_assert(sizeof(fnssl_stream_pool_desc) == 48, "the descriptor is part of the ABI (fnssl/_lib.py mirrors it)");
static_assert(sizeof(PoolParams) <= 4096, "the descriptors of one launch must fit the kernel-argument segment");

// floats of the fixed LDS carve; the spectra ([tile * nch * 256] float2) follow when they fit
__host__ __device__ inline int fixed_lds_floats(int nch, int nchain, int tile) {
  const int n = 2 * kTwiddles + kWin + kStreamWaves * 512 + tile * nch + nchain * tile + tile + nchain;
  return (n + 3) & ~3;
}

size_t spectra_bytes(int nch, int tile) { return (size_t)tile * nch * kNF * sizeof(float2); }

bool spectra_in_lds(int nch, int nchain, int tile) {
  return fixed_lds_floats(nch, nchain, tile) * sizeof(float) + spectra_bytes(nch, tile) <= kLdsBudget;
}

template <int ARRAY, int CENTRED, int POOL = 0>
__global__ void __launch_bounds__(kStreamThreads)
stream_frontend_kernel(const std::conditional_t<POOL != 0, PoolParams, StreamParams> args) {
  constexpr int HOP = CENTRED ? kCentredHop : kHop;
  const StreamParams& p = [&]() -> const StreamParams& {
    if constexpr (POOL) return args.p; else return args;
  }();
  // what a workgroup works on: shared by the launch, or (POOL) its own descriptor, read once into wave-uniform values
  int frame0, nframes;
  long long sample0, sig_total, sig_base, srow, xrow, xframes;
  bool fresh = false;
  if constexpr (POOL) {
    const fnssl_stream_pool_desc& d = args.d[blockIdx.x];
    frame0 = d.frame0; nframes = d.nframes;
    sample0 = d.sample0; sig_total = d.total; sig_base = d.sig_offset;
    srow = d.slot; xrow = d.out_row; xframes = args.out_frames;
    fresh = d.fresh != 0;
  } else {
    frame0 = p.frame0; nframes = p.nframes;
    sample0 = p.sample0; sig_total = p.total; sig_base = (long long)blockIdx.x * p.sb;
    srow = blockIdx.x; xrow = blockIdx.x; xframes = p.nframes;
  }
  extern __shared__ __attribute__((aligned(16))) float smem_stream[];
  float2* tw = reinterpret_cast<float2*>(smem_stream);                  // [kTwiddles]
  float* hann = smem_stream + 2 * kTwiddles;                            // [512]
  float2* zbuf = reinterpret_cast<float2*>(hann + kWin);                // [kStreamWaves][256]
  float* msum_s = hann + kWin + kStreamWaves * 512;                     // [tile][nch]
  float* bm_s = msum_s + p.tile * p.nch;                                // [nchain][tile]: b_t * mean_t, then mu_t
  float* ca_s = bm_s + p.nchain * p.tile;                               // [tile]
  float* mu_s = ca_s + p.tile;                                          // [nchain]: the carried mu
  float2* spec = reinterpret_cast<float2*>(smem_stream + fixed_lds_floats(p.nch, p.nchain, p.tile));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (p.scratch) spec = p.scratch + srow * p.tile * p.nch * kNF;
  fill_tables(tw, hann, tid, kStreamThreads);
  for (int i = tid; i < p.nchain; i += kStreamThreads) mu_s[i] = fresh ? 0.f : p.mu[srow * p.nchain + i];   // a fresh slot starts from mu_{-1} = 0
  float2* z = zbuf + wave * 256;
  const float* ub = p.sig + sig_base;
  const int rowlen = kNF * 2 * p.nch;                                   // array mode: floats of a frame's feature row
  for (int f0 = 0; f0 < nframes; f0 += p.tile) {
    const int n = min(p.tile, nframes - f0);
    __syncthreads();               // tables and mu_s ready; the previous tile's pack is done with spec / bm_s
    for (int i = tid; i < n; i += kStreamThreads) ca_s[i] = p.ca[min(frame0 + f0 + i, p.sample_length)];
    // A: transforms, one wave per (frame, channel)
    for (int w = wave; w < n * p.nch; w += kStreamWaves) {
      const int f = w / p.nch, c = w - f * p.nch;
      if (CENTRED) {
        // torch.stft(center=True): the frame starts half a window before 320 t; reflection at both ends as an index fold,
        // in the order of stft_rows_kernel; the host has checked that every folded index lies in the window
        const float* xc = ub + (long long)c * p.sc;
        const long long n0 = (long long)(frame0 + f0 + f) * HOP - kWin / 2;
        auto at = [&](long long src) {
          src = src < 0 ? -src : src;
          src = (sig_total >= 0 && src >= sig_total) ? 2 * (sig_total - 1) - src : src;
          return xc[(src - sample0) * p.sn];
        };
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = lane + 64 * r;
          window_store(z, hann, m, at(n0 + 2 * m), at(n0 + 2 * m + 1));
        }
      } else {
        const float* xc = ub + (long long)c * p.sc + (long long)(f0 + f) * HOP * p.sn;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = lane + 64 * r;
          window_store(z, hann, m, xc[(long long)(2 * m) * p.sn], xc[(long long)(2 * m + 1) * p.sn]);
        }
      }
      wave_lds_sync();
      fft256_radix4(z, tw, lane);
      float2* so = spec + (long long)w * kNF;                           // bins 1..256 of (f, c)
      const float msum = split_bins<true>(z, tw, lane, [&](int k, float xr, float xi) {
        if (k >= 1) so[k - 1] = make_float2(xr, xi);
      });
      if (lane == 0) msum_s[w] = msum;
      wave_lds_sync();                                                  // z is reused by this wave's next window
    }
    if (p.scratch) __threadfence_block();   // spectra staged in memory: release them to the workgroup's other waves
    __syncthreads();
    // B: the recursion, one wave per chain
    for (int ch = wave; ch < p.nchain; ch += kStreamWaves) {
      float* bm = bm_s + ch * p.tile;
      int mi = 0, mj = 0;
      if (!ARRAY) pair_of(ch, p.nch, p.ch_mode, mi, mj);
      for (int t = lane; t < n; t += 64) {
        const float* s = msum_s + t * p.nch;
        const float mean = ARRAY ? array_mean(s, 1, p.nch) : pair_mean(s[mi], s[mj]);
        bm[t] = ema_term(p.cb[min(frame0 + f0 + t, p.sample_length)], mean);
      }
      float m = mu_s[ch];
      ema_scan_tile(bm, ca_s, n, m, lane);
      if (lane == 0) mu_s[ch] = m;
    }
    __syncthreads();
    // C: features
    if (ARRAY) {
      // the tile's rows [n][256][Re ch 0.. | Im ch 0..] are one contiguous piece of x: float4 stores
      float* o = p.x + (xrow * xframes + f0) * (long long)rowlen;
      const int total = n * rowlen;                                     // multiple of 4
      for (int e0 = 4 * tid; e0 < total; e0 += 4 * kStreamThreads) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e = e0 + q;
          const int f = e / rowlen, rem = e - f * rowlen;
          const int k = rem / (2 * p.nch), cc = rem - k * 2 * p.nch;
          const int c = cc < p.nch ? cc : cc - p.nch;
          const float2 s = spec[((long long)f * p.nch + c) * kNF + k];
          v[q] = feature(cc < p.nch ? s.x : s.y, feature_den(bm_s[f], p.eps));
        }
        *reinterpret_cast<float4*>(o + e0) = make_float4(v[0], v[1], v[2], v[3]);
      }
    } else {
      const int k = tid & (kNF - 1);
      for (int row = tid >> 8; row < p.nchain * n; row += kStreamThreads / kNF) {
        const int ch = row / n, f = row - ch * n;
        int mi, mj;
        pair_of(ch, p.nch, p.ch_mode, mi, mj);
        const float2 xi = spec[((long long)f * p.nch + mi) * kNF + k];
        const float2 xj = spec[((long long)f * p.nch + mj) * kNF + k];
        const float4 o = pair_feature(xi, xj, feature_den(bm_s[ch * p.tile + f], p.eps));
        reinterpret_cast<float4*>(p.x)[((xrow * p.nchain + ch) * xframes + f0 + f) * kNF + k] = o;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < p.nchain; i += kStreamThreads) p.mu[srow * p.nchain + i] = mu_s[i];
}

int chains(int nch, int mode, int ch_mode) { return mode == FNSSL_STREAM_ARRAY ? 1 : fnssl_num_pairs(nch, ch_mode); }

size_t mu_bytes(int nb, int nchain) {
  return ((size_t)nb * nchain * sizeof(float) + kStateAlign - 1) / kStateAlign * kStateAlign;
}

bool bad_shape(int nb, int nch, int mode, int ch_mode) {
  if (mode != FNSSL_STREAM_PAIR && mode != FNSSL_STREAM_ARRAY) return true;
  if (mode == FNSSL_STREAM_PAIR && ch_mode != FNSSL_CH_MODE_M && ch_mode != FNSSL_CH_MODE_MM) return true;
  return nb <= 0 || nch < (mode == FNSSL_STREAM_PAIR ? 2 : 1) || nch > kStreamMaxCh;
}

// Carve the state, size the LDS and launch: p holds the problem; nb workgroups.
int launch_stream(StreamParams p, int nb, bool array, bool centred, void* state, const char* name, void* stream) {
  p.mu = static_cast<float*>(state);
  const bool in_lds = spectra_in_lds(p.nch, p.nchain, p.tile);
  p.scratch = in_lds ? nullptr : reinterpret_cast<float2*>(static_cast<char*>(state) + mu_bytes(nb, p.nchain));
  const size_t lds = fixed_lds_floats(p.nch, p.nchain, p.tile) * sizeof(float) + (in_lds ? spectra_bytes(p.nch, p.tile) : 0);
  hipStream_t st = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl(name, st);
  if (centred)
    return enqueue(st, Kernel{stream_frontend_kernel<1, 1>, kStreamThreads, lds, "stream_frontend_kernel"}, (unsigned)nb, p);
  return fnssl::with_bool(array, [&](auto ARRAY) {
    return enqueue(st, Kernel{stream_frontend_kernel<ARRAY, 0>, kStreamThreads, lds, "stream_frontend_kernel"}, (unsigned)nb, p);
  });
}

// The signal indices frame t of the centred hop-320 transform reads after folding, [lo, hi]: the start fold always, the
// end fold when the total length is known (total >= 0; the caller has checked t <= total / 320 and total > 256).
void centred_reach(long long t, long long total, long long& lo, long long& hi) {
  const long long a = t * kCentredHop - kWin / 2, b = a + kWin - 1;
  lo = a < 0 ? 0 : a;
  hi = a < 0 && -a > b ? -a : b;
  if (total >= 0 && hi >= total) {
    const long long folded = 2 * (total - 1) - hi;
    lo = folded < lo ? folded : lo;
    hi = total - 1;
  }
}

}  // namespace

extern "C" {

size_t fnssl_stream_frontend_state_bytes(int nb, int nch, int mode, int ch_mode, int max_new_frames) {
  if (bad_shape(nb, nch, mode, ch_mode) || max_new_frames <= 0) return 0;
  const int nchain = chains(nch, mode, ch_mode);
  const int tile = max_new_frames < kStreamTile ? max_new_frames : kStreamTile;
  return mu_bytes(nb, nchain) + (spectra_in_lds(nch, nchain, tile) ? 0 : (size_t)nb * spectra_bytes(nch, tile));
}

int fnssl_stream_frontend(const float* sig, int nb, int ns, int nch, long long sb, long long sn, long long sc, int mode,
                          int ch_mode, int frame0, int nframes, const float* coef_a, const float* coef_b,
                          int sample_length, float eps, void* state, size_t state_bytes, float* x, void* stream) {
  FNSSL_REQUIRE(sig && coef_a && coef_b && state && x, "stream_frontend: null pointer");
  FNSSL_REQUIRE(mode == FNSSL_STREAM_PAIR || mode == FNSSL_STREAM_ARRAY, "stream_frontend: mode %d", mode);
  FNSSL_REQUIRE(mode == FNSSL_STREAM_ARRAY || ch_mode == FNSSL_CH_MODE_M || ch_mode == FNSSL_CH_MODE_MM,
                "stream_frontend: ch_mode %d", ch_mode);
  FNSSL_REQUIRE(nb > 0, "stream_frontend: empty batch (nb %d)", nb);
  FNSSL_REQUIRE(nch >= (mode == FNSSL_STREAM_PAIR ? 2 : 1), "stream_frontend: %d channels (pair mode needs >= 2)", nch);
  FNSSL_REQUIRE(nch <= kStreamMaxCh, "stream_frontend: at most %d channels (%d given)", kStreamMaxCh, nch);
  FNSSL_REQUIRE(nframes > 0, "stream_frontend: frame count %d", nframes);
  FNSSL_REQUIRE(frame0 >= 0 && (long long)frame0 + nframes < (1ll << 31), "stream_frontend: first frame %d", frame0);
  FNSSL_REQUIRE(sample_length > 0, "stream_frontend: sample_length %d", sample_length);
  FNSSL_REQUIRE((long long)ns >= (long long)(nframes - 1) * kHop + kWin,
                "stream_frontend: %d frames need %lld samples, the window has %d", nframes,
                (long long)(nframes - 1) * kHop + kWin, ns);
  const size_t need = fnssl_stream_frontend_state_bytes(nb, nch, mode, ch_mode, nframes);
  FNSSL_REQUIRE(state_bytes >= need, "stream_frontend: state of %zu bytes, fnssl_stream_frontend_state_bytes asks for %zu",
                state_bytes, need);
  FNSSL_REQUIRE(((uintptr_t)sig | (uintptr_t)coef_a | (uintptr_t)coef_b) % 4 == 0 && (uintptr_t)state % 16 == 0 &&
                    (uintptr_t)x % 16 == 0,
                "stream_frontend: misaligned pointer (samples and coefficients 4 bytes, state and output 16)");
  StreamParams p{};
  p.sig = sig;
  p.sb = sb; p.sn = sn; p.sc = sc;
  p.nch = nch;
  p.nchain = chains(nch, mode, ch_mode);
  p.ch_mode = ch_mode;
  p.frame0 = frame0;
  p.nframes = nframes;
  p.tile = nframes < kStreamTile ? nframes : kStreamTile;
  p.sample_length = sample_length;
  p.ca = coef_a;
  p.cb = coef_b;
  p.eps = eps;
  p.x = x;
  return launch_stream(p, nb, mode == FNSSL_STREAM_ARRAY, false, state, "stream_frontend", stream);
}

size_t fnssl_stream_frontend_centred_state_bytes(int nb, int nch, int max_new_frames) {
  if (nb <= 0 || nch < 1 || nch > kStreamMaxCh || max_new_frames <= 0) return 0;
  const int tile = max_new_frames < kCentredTile ? max_new_frames : kCentredTile;
  return mu_bytes(nb, 1) + (spectra_in_lds(nch, 1, tile) ? 0 : (size_t)nb * spectra_bytes(nch, tile));
}

int fnssl_stream_frontend_centred(const float* sig, int nb, int ns, int nch, long long sb, long long sn, long long sc,
                                  long long sample0, int frame0, int nframes, long long total, const float* coef_a,
                                  const float* coef_b, int sample_length, float eps, void* state, size_t state_bytes,
                                  float* x, void* stream) {
  FNSSL_REQUIRE(sig && coef_a && coef_b && state && x, "stream_frontend_centred: null pointer");
  FNSSL_REQUIRE(nb > 0, "stream_frontend_centred: empty batch (nb %d)", nb);
  FNSSL_REQUIRE(nch >= 1 && nch <= kStreamMaxCh, "stream_frontend_centred: 1 to %d channels (%d given)", kStreamMaxCh, nch);
  FNSSL_REQUIRE(nframes > 0, "stream_frontend_centred: frame count %d", nframes);
  FNSSL_REQUIRE(frame0 >= 0 && (long long)frame0 + nframes < (1ll << 31) / kCentredHop,
                "stream_frontend_centred: first frame %d", frame0);
  FNSSL_REQUIRE(sample_length > 0, "stream_frontend_centred: sample_length %d", sample_length);
  FNSSL_REQUIRE(total < 0 || total > kWin / 2,
                "stream_frontend_centred: total length %lld is too short for reflect padding of %d", total, kWin / 2);
  const long long last = (long long)frame0 + nframes - 1;
  FNSSL_REQUIRE(total < 0 || last <= total / kCentredHop,
                "stream_frontend_centred: frame %lld does not exist in a signal of total length %lld", last, total);
  FNSSL_REQUIRE(ns > 0 && sample0 >= 0, "stream_frontend_centred: window of %d samples at %lld", ns, sample0);
  for (long long t = frame0; t <= last; ++t) {
    long long lo, hi;
    centred_reach(t, total, lo, hi);
    FNSSL_REQUIRE(lo >= sample0 && hi < sample0 + ns,
                  "stream_frontend_centred: frame %lld reads samples %lld..%lld, the window holds %lld..%lld", t, lo, hi,
                  sample0, sample0 + ns - 1);
  }
  const size_t need = fnssl_stream_frontend_centred_state_bytes(nb, nch, nframes);
  FNSSL_REQUIRE(state_bytes >= need,
                "stream_frontend_centred: state of %zu bytes, fnssl_stream_frontend_centred_state_bytes asks for %zu",
                state_bytes, need);
  FNSSL_REQUIRE(((uintptr_t)sig | (uintptr_t)coef_a | (uintptr_t)coef_b) % 4 == 0 && (uintptr_t)state % 16 == 0 &&
                    (uintptr_t)x % 16 == 0,
                "stream_frontend_centred: misaligned pointer (samples and coefficients 4 bytes, state and output 16)");
  StreamParams p{};
  p.sig = sig;
  p.sb = sb; p.sn = sn; p.sc = sc;
  p.sample0 = sample0;
  p.total = total;
  p.nch = nch;
  p.nchain = 1;
  p.ch_mode = FNSSL_CH_MODE_M;
  p.frame0 = frame0;
  p.nframes = nframes;
  p.tile = nframes < kCentredTile ? nframes : kCentredTile;
  p.sample_length = sample_length;
  p.ca = coef_a;
  p.cb = coef_b;
  p.eps = eps;
  p.x = x;
  return launch_stream(p, nb, true, true, state, "stream_frontend_centred", stream);
}

int fnssl_stream_frontend_centred_pool(const float* sig, int nslots, int nch, long long sn, long long sc,
                                       const fnssl_stream_pool_desc* desc, int ndesc, const float* coef_a,
                                       const float* coef_b, int sample_length, float eps, void* state, size_t state_bytes,
                                       float* x, int out_rows, int out_frames, void* stream) {
  FNSSL_REQUIRE(sig && desc && coef_a && coef_b && state && x, "stream_frontend_centred_pool: null pointer");
  FNSSL_REQUIRE(nslots > 0, "stream_frontend_centred_pool: empty pool (%d slots)", nslots);
  FNSSL_REQUIRE(nch >= 1 && nch <= kStreamMaxCh, "stream_frontend_centred_pool: 1 to %d channels (%d given)", kStreamMaxCh, nch);
  FNSSL_REQUIRE(ndesc > 0, "stream_frontend_centred_pool: %d descriptors", ndesc);
  FNSSL_REQUIRE(out_rows > 0 && out_frames > 0, "stream_frontend_centred_pool: output of %d rows x %d frames", out_rows, out_frames);
  FNSSL_REQUIRE(sample_length > 0, "stream_frontend_centred_pool: sample_length %d", sample_length);
  // the state is sized, and its scratch rows are spaced, for full tiles whatever the frame counts of this call
  const size_t need = fnssl_stream_frontend_centred_state_bytes(nslots, nch, kCentredTile);
  FNSSL_REQUIRE(state_bytes >= need,
                "stream_frontend_centred_pool: state of %zu bytes, fnssl_stream_frontend_centred_state_bytes asks for %zu",
                state_bytes, need);
  FNSSL_REQUIRE(((uintptr_t)sig | (uintptr_t)coef_a | (uintptr_t)coef_b) % 4 == 0 && (uintptr_t)state % 16 == 0 &&
                    (uintptr_t)x % 16 == 0,
                "stream_frontend_centred_pool: misaligned pointer (samples and coefficients 4 bytes, state and output 16)");
  // every descriptor is checked before the first launch
  std::vector<char> slot_seen(nslots, 0), row_seen(out_rows, 0);
  for (int i = 0; i < ndesc; ++i) {
    const fnssl_stream_pool_desc& d = desc[i];
    FNSSL_REQUIRE(d.slot >= 0 && d.slot < nslots, "stream_frontend_centred_pool: descriptor %d: slot %d of %d", i, d.slot, nslots);
    FNSSL_REQUIRE(!slot_seen[d.slot], "stream_frontend_centred_pool: descriptor %d: slot %d appears twice", i, d.slot);
    slot_seen[d.slot] = 1;
    FNSSL_REQUIRE(d.out_row >= 0 && d.out_row < out_rows, "stream_frontend_centred_pool: descriptor %d: output row %d of %d", i,
                  d.out_row, out_rows);
    FNSSL_REQUIRE(!row_seen[d.out_row], "stream_frontend_centred_pool: descriptor %d: output row %d appears twice", i, d.out_row);
    row_seen[d.out_row] = 1;
    FNSSL_REQUIRE(d.nframes > 0 && d.nframes <= out_frames, "stream_frontend_centred_pool: descriptor %d: %d frames in rows of %d",
                  i, d.nframes, out_frames);
    FNSSL_REQUIRE(d.frame0 >= 0 && (long long)d.frame0 + d.nframes < (1ll << 31) / kCentredHop,
                  "stream_frontend_centred_pool: descriptor %d: first frame %d", i, d.frame0);
    FNSSL_REQUIRE(d.total < 0 || d.total > kWin / 2,
                  "stream_frontend_centred_pool: descriptor %d: total length %lld is too short for reflect padding of %d", i,
                  d.total, kWin / 2);
    const long long last = (long long)d.frame0 + d.nframes - 1;
    FNSSL_REQUIRE(d.total < 0 || last <= d.total / kCentredHop,
                  "stream_frontend_centred_pool: descriptor %d: frame %lld does not exist in a signal of total length %lld", i,
                  last, d.total);
    FNSSL_REQUIRE(d.ns > 0 && d.sample0 >= 0, "stream_frontend_centred_pool: descriptor %d: window of %d samples at %lld", i, d.ns,
                  d.sample0);
    for (long long t = d.frame0; t <= last; ++t) {
      long long lo, hi;
      centred_reach(t, d.total, lo, hi);
      FNSSL_REQUIRE(lo >= d.sample0 && hi < d.sample0 + d.ns,
                    "stream_frontend_centred_pool: descriptor %d: frame %lld reads samples %lld..%lld, the window holds %lld..%lld",
                    i, t, lo, hi, d.sample0, d.sample0 + d.ns - 1);
    }
  }
  PoolParams pp{};
  StreamParams& p = pp.p;
  p.sig = sig;
  p.sn = sn; p.sc = sc;
  p.nch = nch;
  p.nchain = 1;
  p.ch_mode = FNSSL_CH_MODE_M;
  p.tile = kCentredTile;
  p.sample_length = sample_length;
  p.ca = coef_a;
  p.cb = coef_b;
  p.eps = eps;
  p.x = x;
  p.mu = static_cast<float*>(state);
  const bool in_lds = spectra_in_lds(nch, 1, kCentredTile);
  p.scratch = in_lds ? nullptr : reinterpret_cast<float2*>(static_cast<char*>(state) + mu_bytes(nslots, 1));
  pp.out_frames = out_frames;
  const size_t lds = fixed_lds_floats(nch, 1, kCentredTile) * sizeof(float) + (in_lds ? spectra_bytes(nch, kCentredTile) : 0);
  hipStream_t st = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl("stream_frontend_centred_pool", st);
  for (int i0 = 0; i0 < ndesc; i0 += kPoolMaxDesc) {      // more active slots than one launch carries: more launches
    const int n = ndesc - i0 < kPoolMaxDesc ? ndesc - i0 : kPoolMaxDesc;
    for (int i = 0; i < n; ++i) pp.d[i] = desc[i0 + i];
    FNSSL_TRY(enqueue(st, Kernel{stream_frontend_kernel<1, 1, 1>, kStreamThreads, lds, "stream_frontend_kernel"}, (unsigned)n, pp));
  }
  return FNSSL_OK;
}

int fnssl_stream_frontend_pool(const float* sig, int nslots, int nch, long long sn, long long sc, int mode, int ch_mode,
                               const fnssl_stream_pool_desc* desc, int ndesc, const float* coef_a, const float* coef_b,
                               int sample_length, float eps, void* state, size_t state_bytes, float* x, int out_rows,
                               int out_frames, void* stream) {
  FNSSL_REQUIRE(sig && desc && coef_a && coef_b && state && x, "stream_frontend_pool: null pointer");
  FNSSL_REQUIRE(mode == FNSSL_STREAM_PAIR || mode == FNSSL_STREAM_ARRAY, "stream_frontend_pool: mode %d", mode);
  FNSSL_REQUIRE(mode == FNSSL_STREAM_ARRAY || ch_mode == FNSSL_CH_MODE_M || ch_mode == FNSSL_CH_MODE_MM,
                "stream_frontend_pool: ch_mode %d", ch_mode);
  FNSSL_REQUIRE(nslots > 0, "stream_frontend_pool: empty pool (%d slots)", nslots);
  FNSSL_REQUIRE(nch >= (mode == FNSSL_STREAM_PAIR ? 2 : 1), "stream_frontend_pool: %d channels (pair mode needs >= 2)", nch);
  FNSSL_REQUIRE(nch <= kStreamMaxCh, "stream_frontend_pool: at most %d channels (%d given)", kStreamMaxCh, nch);
  FNSSL_REQUIRE(ndesc > 0, "stream_frontend_pool: %d descriptors", ndesc);
  FNSSL_REQUIRE(out_rows > 0 && out_frames > 0, "stream_frontend_pool: output of %d rows x %d frames", out_rows, out_frames);
  FNSSL_REQUIRE(sample_length > 0, "stream_frontend_pool: sample_length %d", sample_length);
  const bool array = mode == FNSSL_STREAM_ARRAY;
  const int nchain = chains(nch, mode, ch_mode);
  // the state is sized, and its scratch rows are spaced, for full tiles whatever the frame counts of this call
  const size_t need = fnssl_stream_frontend_state_bytes(nslots, nch, mode, ch_mode, kStreamTile);
  FNSSL_REQUIRE(state_bytes >= need, "stream_frontend_pool: state of %zu bytes, fnssl_stream_frontend_state_bytes asks for %zu",
                state_bytes, need);
  FNSSL_REQUIRE(((uintptr_t)sig | (uintptr_t)coef_a | (uintptr_t)coef_b) % 4 == 0 && (uintptr_t)state % 16 == 0 &&
                    (uintptr_t)x % 16 == 0,
                "stream_frontend_pool: misaligned pointer (samples and coefficients 4 bytes, state and output 16)");
  // every descriptor is checked before the first launch
  std::vector<char> slot_seen(nslots, 0), row_seen(out_rows, 0);
  for (int i = 0; i < ndesc; ++i) {
    const fnssl_stream_pool_desc& d = desc[i];
    FNSSL_REQUIRE(d.slot >= 0 && d.slot < nslots, "stream_frontend_pool: descriptor %d: slot %d of %d", i, d.slot, nslots);
    FNSSL_REQUIRE(!slot_seen[d.slot], "stream_frontend_pool: descriptor %d: slot %d appears twice", i, d.slot);
    slot_seen[d.slot] = 1;
    FNSSL_REQUIRE(d.out_row >= 0 && d.out_row < out_rows, "stream_frontend_pool: descriptor %d: output row %d of %d", i,
                  d.out_row, out_rows);
    FNSSL_REQUIRE(!row_seen[d.out_row], "stream_frontend_pool: descriptor %d: output row %d appears twice", i, d.out_row);
    row_seen[d.out_row] = 1;
    FNSSL_REQUIRE(d.nframes > 0 && d.nframes <= out_frames, "stream_frontend_pool: descriptor %d: %d frames in rows of %d", i,
                  d.nframes, out_frames);
    FNSSL_REQUIRE(d.frame0 >= 0 && (long long)d.frame0 + d.nframes < (1ll << 31),
                  "stream_frontend_pool: descriptor %d: first frame %d", i, d.frame0);
    FNSSL_REQUIRE(d.sample0 == (long long)kHop * d.frame0,
                  "stream_frontend_pool: descriptor %d: the window starts at sample %lld, frame %d starts at %lld", i, d.sample0,
                  d.frame0, (long long)kHop * d.frame0);
    FNSSL_REQUIRE(d.total < 0, "stream_frontend_pool: descriptor %d: total length %lld (the hop-256 transform has no end "
                  "reflection: pass a negative total)", i, d.total);
    FNSSL_REQUIRE((long long)d.ns >= (long long)(d.nframes - 1) * kHop + kWin,
                  "stream_frontend_pool: descriptor %d: %d frames need %lld samples, the window has %d", i, d.nframes,
                  (long long)(d.nframes - 1) * kHop + kWin, d.ns);
  }
  PoolParams pp{};
  StreamParams& p = pp.p;
  p.sig = sig;
  p.sn = sn; p.sc = sc;
  p.nch = nch;
  p.nchain = nchain;
  p.ch_mode = ch_mode;
  p.tile = kStreamTile;
  p.sample_length = sample_length;
  p.ca = coef_a;
  p.cb = coef_b;
  p.eps = eps;
  p.x = x;
  p.mu = static_cast<float*>(state);
  const bool in_lds = spectra_in_lds(nch, nchain, kStreamTile);
  p.scratch = in_lds ? nullptr : reinterpret_cast<float2*>(static_cast<char*>(state) + mu_bytes(nslots, nchain));
  pp.out_frames = out_frames;
  const size_t lds = fixed_lds_floats(nch, nchain, kStreamTile) * sizeof(float) + (in_lds ? spectra_bytes(nch, kStreamTile) : 0);
  hipStream_t st = fnssl::as_stream(stream);
  fnssl::TimedLaunch tl("stream_frontend_pool", st);
  for (int i0 = 0; i0 < ndesc; i0 += kPoolMaxDesc) {      // more active slots than one launch carries: more launches
    const int n = ndesc - i0 < kPoolMaxDesc ? ndesc - i0 : kPoolMaxDesc;
    for (int i = 0; i < n; ++i) pp.d[i] = desc[i0 + i];
    FNSSL_TRY(fnssl::with_bool(array, [&](auto ARRAY) {
      return enqueue(st, Kernel{stream_frontend_kernel<ARRAY, 0, 1>, kStreamThreads, lds, "stream_frontend_kernel"}, (unsigned)n, pp);
    }));
  }
  return FNSSL_OK;
}

}  // extern "C"
