// Backward of the causal conv head of IPDnet (CausCnnBlock, reference IPDnet/FixedAarryIPDnet.py:42-73), the training
// twin of conv.hip.  Forward per stage:  Z = conv3x3(X) (pad (1, 2), crop the last 2 frames: out[t] sees t-2..t),
// Y = act(Z) (ReLU / ReLU / tanh), P = AvgPool((1, K))(Y) (K = 3 / 4 / none).  Backward per stage, channels-last
// [nb, nf, nt, C] like the forward:
//
//   * act_pool_backward (elementwise): dZ[t] = act'(Y[t]) * (t < K * (nt / K) ? dP[t / K] / K : 0)
//     (frames past the last whole pooling window get no gradient — AvgPool floors); act' = (Y > 0) or 1 - Y^2.
//   * input gradient (dgrad), fp32 MFMA: dX[f, t] = sum_{df, dt} W[:, :, df, dt]^T dZ[f + 1 - df, t + 2 - dt].  That
//     is the forward conv3x3_kernel with anti-causal taps (t .. t + 2, zero past the last frame), the bin taps
//     flipped and the weights transposed: dX^T [Cin_g x 16] = W^T [Cin_g x 9 Cout] * dZ-patches^T, the same LDS weight
//     ring and MFMA schedule as the forward (conv.hip, ANTI = true).  The stream is packed per 128 input channels
//     (the kernel's output tile limit): conv 1's 256 FN-block channels are two launches; the 16 channels of the
//     network input (the concat skip) get no gradient.
//   * weight gradient (wgrad), split-K fp32 MFMA: dW[co][(tap, ci)] = sum_r dZ[r][co] * X[r + shift(tap)][ci] over
//     r = (b, f, t).  The nine taps are index shifts of one channels-last tensor with per-row predicates at the f / t
//     edges (the trick wgrad.hip uses for h_prev), conv 1's X = [Y | x] is read in place from two tensors.  A workgroup
//     (4 waves) owns a 128 (co) x 128 (tap, ci) tile of dW over one slab of rows; a wave 64 x 64 = 16 accumulator quads
//     of v_mfma_f32_16x16x4_f32; a stage = 16 rows of both panels, register-staged one stage ahead into two LDS buffers
//     (rows padded by 16 floats: conflict-free column reads).  Partial tiles go to a workspace [slab][cout][9 cin]; a
//     second kernel adds them up in slab order (deterministic, no float atomics) and += into the [cout][cin][3][3]
//     gradient.
// Algorithmic work: dgrad 2 * 9 * Cout * Cin_g per position, wgrad 2 * 9 * Cout * Cin per position.
#include <cstring>
#include <vector>

#include "host.h"

using fnssl::enqueue;
using fnssl::Kernel;

namespace fnssl {
int conv3x3_anticausal_f32(const float* xa, long long a_sb, long long a_sf, long long a_st, int ca, const float* xb,
                           long long b_sb, long long b_sf, long long b_st, int cb, const float* wpack, int cout, int nb,
                           int nf, int nt, float* out, int cout_stride, void* stream);
}

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kChunk = 128;                       // input channels per dgrad launch (conv3x3_kernel: cout <= 128)

// ---------------------------------------------------------------------------------------------------------------
// activation + pooling backward
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
act_pool_bwd_kernel(const v4f* __restrict__ dp, const v4f* __restrict__ y, long long rows, int nt, int c4, int K,
                    int act, v4f* __restrict__ dz) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;   // over rows * nt * c4
  if (idx >= rows * nt * c4) return;
  const int c = (int)(idx % c4);
  const long long rt = idx / c4;
  const int t = (int)(rt % nt);
  const long long row = rt / nt;
  const int ntp = nt / K;
  v4f g = v4f{0.f, 0.f, 0.f, 0.f};
  if (t < K * ntp) {
    g = dp[(row * ntp + t / K) * c4 + c];
    if (K > 1) {
      const float d = (float)K;
      g = v4f{__fdiv_rn(g.x, d), __fdiv_rn(g.y, d), __fdiv_rn(g.z, d), __fdiv_rn(g.w, d)};
    }
  }
  const v4f v = y[idx];
  v4f r;
  if (act == 1) {
    r = v4f{v.x > 0.f ? g.x : 0.f, v.y > 0.f ? g.y : 0.f, v.z > 0.f ? g.z : 0.f, v.w > 0.f ? g.w : 0.f};
  } else if (act == 2) {
    r = v4f{g.x * (1.f - v.x * v.x), g.y * (1.f - v.y * v.y), g.z * (1.f - v.z * v.z), g.w * (1.f - v.w * v.w)};
  } else {
    r = g;
  }
  dz[idx] = r;
}

// ---------------------------------------------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------------------------------------------
constexpr int kTM = 128, kTN = 128, kBK = 16, kThreads = 256;
constexpr int kLd = 128 + 16;                     // LDS row stride (floats): stride % 64 == 16

struct Tens {                                     // logical [nb, nf, nt, C] channels-last view
  const float* p;
  long long sb, sf, st;
};

struct CwParams {
  Tens dz, xa, xb;
  int cout, ca, cin, ncol;                        // ncol = 9 * cin
  int nb, nf, nt;
  long long rows, rows_per_slab;
  int mtiles, ntiles, slabs;
  float* part;                                    // [slabs][cout][ncol]
};

__global__ void __launch_bounds__(kThreads) conv_wgrad_kernel(const CwParams p) {
  __shared__ __attribute__((aligned(16))) float As[2][kBK][kLd];
  __shared__ __attribute__((aligned(16))) float Bs[2][kBK][kLd];
  const int item = blockIdx.x;
  const int nt_ = item % p.ntiles;
  const int mt = (item / p.ntiles) % p.mtiles;
  const int slab = item / (p.ntiles * p.mtiles);
  const int m0 = mt * kTM, n0 = nt_ * kTN;
  const int tid = threadIdx.x;

  // loader roles: rows lr and lr + 8 of a stage, columns c4 .. c4 + 3 of both panels
  const int lr = tid >> 5, c4 = (tid & 31) * 4;
  const bool a_ok = m0 + c4 < p.cout;
  const int n = n0 + c4;
  const bool b_ok = n < p.ncol;
  const int tap = b_ok ? n / p.cin : 0, ci = b_ok ? n - tap * p.cin : 0;
  const int df = tap / 3 - 1, dt = tap % 3 - 2;     // X[f + df, t + dt] (zero outside: pad (1, 2) + crop)
  const Tens xs = ci < p.ca ? p.xa : p.xb;
  const float* bsrc = xs.p + (ci < p.ca ? ci : ci - p.ca) + df * xs.sf + dt * xs.st;
  const float* asrc = p.dz.p + m0 + c4;

  const long long r_begin = (long long)slab * p.rows_per_slab;
  const long long r_end = r_begin + p.rows_per_slab < p.rows ? r_begin + p.rows_per_slab : p.rows;
  const int nstage = (int)((r_end - r_begin + kBK - 1) / kBK);

  v4f ra[2], rb[2];
  auto load_stage = [&](int s) {
    const v4f z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long r = r_begin + (long long)s * kBK + lr + 8 * h;
      ra[h] = z;
      rb[h] = z;
      if (r < r_end) {
        const int t = (int)(r % p.nt);
        const long long bf = r / p.nt;
        const int f = (int)(bf % p.nf);
        const int b = (int)(bf / p.nf);
        if (a_ok) ra[h] = *reinterpret_cast<const v4f*>(asrc + b * p.dz.sb + f * p.dz.sf + t * p.dz.st);
        const int ff = f + df, tt = t + dt;
        if (b_ok && ff >= 0 && ff < p.nf && tt >= 0)
          rb[h] = *reinterpret_cast<const v4f*>(bsrc + b * xs.sb + f * xs.sf + t * xs.st);
      }
    }
  };
  auto store_stage = [&](int buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<v4f*>(&As[buf][lr + 8 * h][c4]) = ra[h];
      *reinterpret_cast<v4f*>(&Bs[buf][lr + 8 * h][c4]) = rb[h];
    }
  };

  const int lane = tid & 63, w = tid >> 6;
  const int wm = (w & 1) * 64, wn = (w >> 1) * 64;
  const int l16 = lane & 15, kq = lane >> 4;
  v4f acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};

  auto multiply = [&](int buf) {
    float a[4], b[4], an[4], bn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = As[buf][kq][wm + 16 * i + l16];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = Bs[buf][kq][wn + 16 * j + l16];
#pragma unroll
    for (int kk = 0; kk < kBK / 4; ++kk) {
      if (kk + 1 < kBK / 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) an[i] = As[buf][4 * (kk + 1) + kq][wm + 16 * i + l16];
#pragma unroll
        for (int j = 0; j < 4; ++j) bn[j] = Bs[buf][4 * (kk + 1) + kq][wn + 16 * j + l16];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (kk + 1 < kBK / 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = an[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = bn[j];
      }
    }
  };

  if (nstage > 0) {
    load_stage(0);
    store_stage(0);
  }
  __syncthreads();
  for (int s = 0; s < nstage; ++s) {
    if (s + 1 < nstage) load_stage(s + 1);      // in flight under this stage's MFMAs
    multiply(s & 1);
    if (s + 1 < nstage) store_stage((s + 1) & 1);
    __syncthreads();
  }

  // partial tile -> workspace; D fragment: lane (l16, kq) holds rows 4 kq + r, column l16
  float* out = p.part + (long long)slab * p.cout * p.ncol;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int nn = n0 + wn + 16 * j + l16;
      if (nn < p.ncol) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + wm + 16 * i + 4 * kq + r;
          if (m < p.cout) out[(long long)m * p.ncol + nn] = acc[i][j][r];
        }
      }
    }
}

// dw[co][ci][tap] += sum over slabs (in slab order) of part[slab][co][tap * cin + ci]
__global__ void __launch_bounds__(256)
conv_wgrad_reduce_kernel(const float* __restrict__ part, int slabs, int cout, int cin, float* __restrict__ dw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int ncol = 9 * cin;
  const long long total = (long long)cout * ncol;
  if (i >= total) return;
  const int co = (int)(i / ncol), nn = (int)(i - (long long)co * ncol);
  const int tap = nn / cin, ci = nn - tap * cin;
  float s = 0.f;
  for (int k = 0; k < slabs; ++k) s += part[(long long)k * total + i];
  dw[((long long)co * cin + ci) * 9 + tap] += s;
}

int wgrad_plan(long long rows, int mtiles, int ntiles, long long* rows_per_slab) {
  // about three rounds of two resident workgroups per CU; at least 8 stages per slab
  const int slots = 2 * fnssl::device_cus();
  const int per_slab = mtiles * ntiles;
  int slabs = (3 * slots + per_slab - 1) / per_slab;
  const long long max_slabs = (rows + 8 * kBK - 1) / (8 * kBK);
  if (slabs > max_slabs) slabs = (int)(max_slabs > 0 ? max_slabs : 1);
  if (slabs > 256) slabs = 256;
  if (slabs < 1) slabs = 1;
  long long rps = (rows + slabs - 1) / slabs;
  rps = (rps + kBK - 1) / kBK * kBK;
  slabs = (int)((rows + rps - 1) / rps);
  *rows_per_slab = rps;
  return slabs;
}

bool addressable(const float* p, long long sb, long long sf, long long st, int c, int nf, int nt) {
  // channel-contiguous, 16-byte aligned float4 loads; strides non-negative multiples of 4 floats
  return p && reinterpret_cast<uintptr_t>(p) % 16 == 0 && sb >= 0 && sf >= 0 && st >= 0 && !(sb & 3) && !(sf & 3) &&
         !(st & 3) && c > 0 && (c & 3) == 0 && (long double)(nf - 1) * sf + (long double)(nt - 1) * st + c < 4.0e9L;
}

int dgrad_chunks(int cin_g) { return (cin_g + kChunk - 1) / kChunk; }

bool dgrad_sizes_ok(int cout, int cin, int cin_g) {
  return cout >= 4 && cout <= 4096 && cout % 4 == 0 && cin > 0 && cin_g > 0 && cin_g <= cin && cin_g % 4 == 0;
}

}  // namespace

extern "C" {

size_t fnssl_conv3x3_packed_floats_backward_data(int cout, int cin, int cin_g) {
  if (!dgrad_sizes_ok(cout, cin, cin_g)) return 0;
  size_t total = 0;
  for (int k = 0; k < dgrad_chunks(cin_g); ++k) {
    const int cn = cin_g - k * kChunk < kChunk ? cin_g - k * kChunk : kChunk;
    const size_t n = fnssl_conv3x3_packed_floats(cn, cout & ~15, cout & 15);
    if (n == 0) return 0;
    total += n;
  }
  return total;
}

int fnssl_conv3x3_pack_backward_data(const float* w, int cout, int cin, int cin_g, float* packed) {
  FNSSL_REQUIRE(w && packed, "conv3x3_pack_backward_data: null pointer");
  FNSSL_REQUIRE(fnssl_conv3x3_packed_floats_backward_data(cout, cin, cin_g) > 0,
                "conv3x3_pack_backward_data: unsupported sizes (cout %d: >= 4, %% 4; cin_g %d <= cin %d, %% 4)", cout,
                cin_g, cin);
  size_t off = 0;
  for (int k = 0; k < dgrad_chunks(cin_g); ++k) {
    const int c0 = k * kChunk, cn = cin_g - c0 < kChunk ? cin_g - c0 : kChunk;
    // transposed, bin-flipped weights of this chunk: wt[i][co][df][dt] = w[co][c0 + i][2 - df][dt]
    std::vector<float> wt((size_t)cn * cout * 9);
    for (int i = 0; i < cn; ++i)
      for (int co = 0; co < cout; ++co)
        for (int df = 0; df < 3; ++df)
          for (int dt = 0; dt < 3; ++dt)
            wt[(((size_t)i * cout + co) * 3 + df) * 3 + dt] = w[(((size_t)co * cin + c0 + i) * 3 + (2 - df)) * 3 + dt];
    const int rc = fnssl_conv3x3_pack(wt.data(), cn, cout & ~15, cout & 15, packed + off);
    if (rc != FNSSL_OK) return rc;
    off += fnssl_conv3x3_packed_floats(cn, cout & ~15, cout & 15);
  }
  return FNSSL_OK;
}

int fnssl_conv3x3_act_pool_backward(const float* dp, const float* y, int nb, int nf, int nt, int c, int k, int act,
                                    float* dz, void* stream) {
  FNSSL_REQUIRE(dp && y && dz, "conv3x3_act_pool_backward: null pointer");
  FNSSL_REQUIRE(nb > 0 && nf > 0 && nt > 0 && c > 0 && c % 4 == 0 && k >= 1 && act >= 0 && act <= 2,
                "conv3x3_act_pool_backward: bad arguments (nb %d nf %d nt %d c %d k %d act %d)", nb, nf, nt, c, k, act);
  FNSSL_REQUIRE(((uintptr_t)dp | (uintptr_t)y | (uintptr_t)dz) % 16 == 0,
                "conv3x3_act_pool_backward: operands must be 16-byte aligned");
  const long long rows = (long long)nb * nf;
  const long long total = rows * nt * (c / 4);
  FNSSL_REQUIRE((total + 255) / 256 < (1ll << 31), "conv3x3_act_pool_backward: too large");
  fnssl::TimedLaunch tl("conv_act_pool_bwd", fnssl::as_stream(stream));
  return enqueue(fnssl::as_stream(stream), Kernel{act_pool_bwd_kernel, 256, 0, "act_pool_bwd_kernel"},
                 (unsigned)((total + 255) / 256), reinterpret_cast<const v4f*>(dp), reinterpret_cast<const v4f*>(y), rows, nt,
                 c / 4, k, act, reinterpret_cast<v4f*>(dz));
}

int fnssl_conv3x3_causal_backward_data(const float* dz, long long z_sb, long long z_sf, long long z_st, int cout,
                                       const float* wpack, int cin_g, int nb, int nf, int nt, float* dx, int dx_stride,
                                       void* stream) {
  FNSSL_REQUIRE(dz && wpack && dx, "conv3x3_causal_backward_data: null pointer");
  FNSSL_REQUIRE(nb > 0 && nf > 0 && nt > 0, "conv3x3_causal_backward_data: empty problem");
  FNSSL_REQUIRE(dgrad_sizes_ok(cout, cin_g, cin_g), "conv3x3_causal_backward_data: unsupported sizes (cout %d, cin_g %d)",
                cout, cin_g);
  FNSSL_REQUIRE(dx_stride >= cin_g && dx_stride % 4 == 0 && (long double)nf * nt * dx_stride * 4 < 4.0e9L,
                "conv3x3_causal_backward_data: dx row stride %d", dx_stride);
  FNSSL_REQUIRE(addressable(dz, z_sb, z_sf, z_st, cout, nf, nt),
                "conv3x3_causal_backward_data: dz must be channel-contiguous, 16-byte aligned, strides multiples of 4 "
                "floats, one utterance addressable with 32-bit offsets");
  const int ca = cout & ~15, cb = cout & 15;
  size_t off = 0;
  for (int k = 0; k < dgrad_chunks(cin_g); ++k) {
    const int c0 = k * kChunk, cn = cin_g - c0 < kChunk ? cin_g - c0 : kChunk;
    // (fewer than 16 output channels: the whole of dz is the 4-channel remainder segment B)
    const int rc = fnssl::conv3x3_anticausal_f32(dz, z_sb, z_sf, z_st, ca, cb ? dz + ca : nullptr, z_sb, z_sf, z_st, cb,
                                                 wpack + off, cn, nb, nf, nt, dx + c0, dx_stride, stream);
    if (rc != FNSSL_OK) return rc;
    off += fnssl_conv3x3_packed_floats(cn, ca, cb);
  }
  return FNSSL_OK;
}

size_t fnssl_conv3x3_weight_grads_workspace_bytes(int nb, int nf, int nt, int cout, int ca, int cb) {
  if (nb <= 0 || nf <= 0 || nt <= 0 || cout <= 0 || ca <= 0 || cb < 0) return 0;
  const int cin = ca + cb;
  long long rps;
  const int slabs = wgrad_plan((long long)nb * nf * nt, (cout + kTM - 1) / kTM, (9 * cin + kTN - 1) / kTN, &rps);
  return (size_t)slabs * cout * 9 * cin * sizeof(float) + 256;
}

int fnssl_conv3x3_weight_grads(const float* dz, long long z_sb, long long z_sf, long long z_st, int cout,
                               const float* xa, long long a_sb, long long a_sf, long long a_st, int ca, const float* xb,
                               long long b_sb, long long b_sf, long long b_st, int cb, int nb, int nf, int nt, float* dw,
                               void* workspace, size_t workspace_bytes, void* stream) {
  FNSSL_REQUIRE(dz && xa && dw, "conv3x3_weight_grads: null pointer");
  FNSSL_REQUIRE(nb > 0 && nf > 0 && nt > 0, "conv3x3_weight_grads: empty problem");
  FNSSL_REQUIRE(cout > 0 && cout % 4 == 0 && ca > 0 && ca % 4 == 0 && cb >= 0 && cb % 4 == 0,
                "conv3x3_weight_grads: channel counts (cout %d, ca %d, cb %d) must be multiples of 4", cout, ca, cb);
  FNSSL_REQUIRE(addressable(dz, z_sb, z_sf, z_st, cout, nf, nt) && addressable(xa, a_sb, a_sf, a_st, ca, nf, nt) &&
                    (cb == 0 || addressable(xb, b_sb, b_sf, b_st, cb, nf, nt)),
                "conv3x3_weight_grads: operands must be channel-contiguous, 16-byte aligned, strides multiples of 4 "
                "floats, one utterance addressable with 32-bit offsets");
  const size_t need = fnssl_conv3x3_weight_grads_workspace_bytes(nb, nf, nt, cout, ca, cb);
  if (!workspace || workspace_bytes < need) {
    fnssl::set_error("conv3x3_weight_grads: workspace %zu < %zu bytes", workspace_bytes, need);
    return FNSSL_E_WORKSPACE;
  }
  CwParams p{};
  p.dz = Tens{dz, z_sb, z_sf, z_st};
  p.xa = Tens{xa, a_sb, a_sf, a_st};
  p.xb = cb ? Tens{xb, b_sb, b_sf, b_st} : p.xa;
  p.cout = cout;
  p.ca = ca;
  p.cin = ca + cb;
  p.ncol = 9 * p.cin;
  p.nb = nb;
  p.nf = nf;
  p.nt = nt;
  p.rows = (long long)nb * nf * nt;
  p.mtiles = (cout + kTM - 1) / kTM;
  p.ntiles = (p.ncol + kTN - 1) / kTN;
  p.slabs = wgrad_plan(p.rows, p.mtiles, p.ntiles, &p.rows_per_slab);
  p.part = reinterpret_cast<float*>(workspace);
  hipStream_t st = fnssl::as_stream(stream);
  const int nitems = p.slabs * p.mtiles * p.ntiles;
  {
    fnssl::TimedLaunch tl("conv3x3_wgrad", st, 2.0 * (double)p.rows * cout * p.ncol);
    FNSSL_TRY(enqueue(st, Kernel{conv_wgrad_kernel, kThreads, 0, "conv_wgrad_kernel"}, nitems, p));
  }
  const long long total = (long long)cout * p.ncol;
  {
    fnssl::TimedLaunch tl("conv3x3_wgrad_reduce", st);
    FNSSL_TRY(enqueue(st, Kernel{conv_wgrad_reduce_kernel, 256, 0, "conv_wgrad_reduce_kernel"}, (unsigned)((total + 255) / 256),
                      p.part, p.slabs, cout, p.cin, dw));
  }
  return FNSSL_OK;
}

}  // extern "C"
