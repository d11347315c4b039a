// IPDnet2 (OnlineSpatialNet), the two ends of the network's backward: the causal encoder conv and the FreqInverse + tanh +
// decoder head.  With the Mamba block (spatialnet_train.hip) and the f-conv / full-band branches
// (spatialnet_layer_train.hip) they close the chain waveform features -> prediction -> 2 + 40 L + 4 parameter gradients.
// fp32, whole sequences from zero state.  x is the only saved state of either operator.
//
// Encoder.  y[b,t,f,o] = bias[o] + sum_{c,k} W[o,c,k] x[b,c,f,t-4+k]  (zero for negative time), so
//     dW[o,c,k] = sum_p dY[p][o] A[p][c*5+k],   A = the im2col row of x (gathered on the fly, never stored)
// is a points-as-K product on v_mfma_f32_16x16x4_f32, the operand shape of sn_wgrad_pts_kernel: lane (i, kq) feeds
// A[p0 + kq][16 mt + i] and dY[p0 + kq][16 n + i].  The rows of A are padded to KP = 80 or 160 as the forward pads them,
// and the first padded row (c*5+k = cin*5) is the constant 1: its output row is sum_p dY = dbias, so dY is read once for
// both.  A wave keeps all KP/16 x 6 output tiles in registers and walks the 32-point quarter of every 128-point tile of its
// workgroup; workgroups are persistent (tile = blockIdx.x, + gridDim.x, ...).  Order of every sum: the points of a wave's
// quarter, the tiles of the workgroup, the four waves (through LDS, in wave order), then the workgroups
// (sn_reduce_rows_kernel, in workgroup order).  No float atomics: two runs give the same bits.
// cin*5 + 1 > 160 has no matrix-pipe forward either: a plain kernel (one thread per output element, the workgroup's share
// of the points in order).  dx is its own launch and runs only when asked for.
//
// Head.  For point p = (b, t2, fc) and fine bin r: u_r = bfiP[r] + wfiP[r] x[p], v_r = tanh(u_r), d_r = bd + wdT^T v_r,
// out[b, t2, 2 (16 fc + r) + gg, m, a] = d_r[a*8 + gg*4 + m].  51 200 points at the largest configuration: a plain kernel.
// Thread (r, o) of a 256-thread workgroup owns row (r, o) of wfiP and its gradient in registers; the workgroup takes one
// point at a time (x row and du through LDS), dx[p] = wfiP^T du comes from an LDS copy of wfiP.  v is recomputed with the
// forward's tanh_fast, so the backward differentiates the function the forward computed (v = +-1 exactly where e^2u
// overflows: du and dx are exactly 0 there).
#include "spatialnet_common.h"

namespace {

constexpr int KE = 5;      // encoder taps
constexpr int DO = 16;     // dim_output
constexpr int NR = 16;     // fine bins per compressed bin
constexpr int kEncTile = 128;   // points of a tile of the encoder's dW: four waves x 8 groups of 4 points

// p -> (b, f, t): t fastest (the forward's order) or, f_fast, f fastest (the order of a frame-major dY in memory)
__device__ __forceinline__ long long split_point(long long p, int nf, int nt, int f_fast, int& f, int& t) {
  if (f_fast) return divmod(divmod(p, nf, f), nt, t);
  return divmod(divmod(p, nt, t), nf, f);
}

// ---------------------------------------------------------------------------------------------------------
// encoder, dW | dbias: part[blockIdx.x][KP][96]  (row cin*5 = dbias, the rows after it 0)
// ---------------------------------------------------------------------------------------------------------
template <int MT, int U>             // MT = KP / 16 row tiles; U groups of 4 points whose loads are in flight together
__global__ void __launch_bounds__(256, MT == 5 ? 2 : 1)       // KP 80: two workgroups per CU = 2 waves per SIMD
sn_encoder_bwd_w_kernel(const float* __restrict__ x, long long sb, long long sc, long long sf, long long st, int cin,
                        int nf, int nt, long long npts, int f_fast, const float* __restrict__ dy, long long d_sb,
                        long long d_st, long long d_sf, float* __restrict__ part) {
  constexpr int NT = H / 16;
  __shared__ __attribute__((aligned(16))) float red[3][NT][256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  // the lane's MT rows of A: (channel, tap) = (kk / 5, kk % 5), kk = 16 mt + i
  long long xoff[MT];
  int tap[MT];                       // k - 4: the frame offset of the tap;  1: not a row of x
  bool one[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int kk = 16 * mt + i, c = kk / KE, k = kk % KE;
    const bool valid = kk < cin * KE;
    one[mt] = kk == cin * KE;
    tap[mt] = valid ? k - (KE - 1) : 1;
    xoff[mt] = valid ? c * sc + (k - (KE - 1)) * st : 0;
  }
  v4f_t acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[mt][n] = v4f_t{0.f, 0.f, 0.f, 0.f};
  const long long ntiles = (npts + kEncTile - 1) / kEncTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long base = tile * kEncTile + w * (kEncTile / 4) + kq;
#pragma unroll 1
    for (int g = 0; g < kEncTile / 16; g += U) {
      float av[U][MT], bv[U][NT];
      bool ok[U], aok[U][MT];
      // every load of the U groups first (clamped addresses), the choices afterwards
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long p = base + (g + u) * 4;
        ok[u] = p < npts;
        int f, t;
        const long long b = split_point(ok[u] ? p : 0, nf, nt, f_fast, f, t);
        const long long xb = b * sb + f * sf + t * st;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          aok[u][mt] = ok[u] && tap[mt] <= 0 && t + tap[mt] >= 0;
          av[u][mt] = x[aok[u][mt] ? xb + xoff[mt] : 0];
        }
        const float* dyp = dy + b * d_sb + t * d_st + f * d_sf + i;
#pragma unroll
        for (int n = 0; n < NT; ++n) bv[u][n] = dyp[16 * n];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float bb[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) bb[n] = ok[u] ? bv[u][n] : 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const float a = one[mt] ? (ok[u] ? 1.f : 0.f) : (aok[u][mt] ? av[u][mt] : 0.f);
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[mt][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb[n], acc[mt][n], 0, 0, 0);
        }
      }
    }
  }
  // the four waves in wave order, one row tile at a time
  float* dst = part + (long long)blockIdx.x * (MT * 16 * H);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    if (w > 0) {
#pragma unroll
      for (int n = 0; n < NT; ++n) *reinterpret_cast<v4f_t*>(&red[w - 1][n][lane * 4]) = acc[mt][n];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        v4f_t v = acc[mt][n];
#pragma unroll
        for (int ww = 0; ww < 3; ++ww) v += *reinterpret_cast<const v4f_t*>(&red[ww][n][lane * 4]);
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(mt * 16 + 4 * kq + r) * H + 16 * n + i] = v[r];
      }
    }
    __syncthreads();
  }
}

// cin*5 + 1 > 160.  part[blockIdx.x][cin*5 + 1][96]: thread = output element, the workgroup's points in order.
__global__ void __launch_bounds__(256)
sn_encoder_bwd_w_plain_kernel(const float* __restrict__ x, long long sb, long long sc, long long sf, long long st, int cin,
                              int nf, int nt, long long npts, long long per_wg, const float* __restrict__ dy,
                              long long d_sb, long long d_st, long long d_sf, float* __restrict__ part) {
  const long long p_begin = blockIdx.x * per_wg;
  const long long p_end = p_begin + per_wg < npts ? p_begin + per_wg : npts;
  const int nout = (cin * KE + 1) * H;
  for (int idx = threadIdx.x; idx < nout; idx += 256) {
    const int kk = idx / H, o = idx % H, c = kk / KE, k = kk % KE;
    const bool one = kk == cin * KE;
    float acc = 0.f;
    for (long long p = p_begin; p < p_end; ++p) {
      int f, t;
      const long long b = split_point(p, nf, nt, 0, f, t);
      const float g = dy[b * d_sb + t * d_st + f * d_sf + o];
      const int tt = t + k - (KE - 1);
      const float a = one ? 1.f : (tt >= 0 ? x[b * sb + c * sc + f * sf + tt * st] : 0.f);
      acc = fmaf(a, g, acc);
    }
    part[(long long)blockIdx.x * nout + idx] = acc;
  }
}

// dx[b,c,f,s] = sum_k sum_o W[o,c,k] dY[b,s+4-k,f,o] over s+4-k < nt: thread = element of dx
__global__ void __launch_bounds__(256)
sn_encoder_bwd_x_kernel(const float* __restrict__ wT, int cin, int nf, int nt, long long nel, const float* __restrict__ dy,
                        long long d_sb, long long d_st, long long d_sf, float* __restrict__ dx, long long sb, long long sc,
                        long long sf, long long st) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nel) return;
  int s, f, c;
  const long long b = divmod(divmod(divmod(e, nt, s), nf, f), cin, c);
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < KE; ++k) {
    const int tt = s + (KE - 1) - k;
    if (tt >= nt) continue;
    const float4* g4 = reinterpret_cast<const float4*>(dy + b * d_sb + tt * d_st + f * d_sf);
    const float4* w4 = reinterpret_cast<const float4*>(wT + (long long)(c * KE + k) * H);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int o4 = 0; o4 < H / 4; ++o4) {
      const float4 g = g4[o4], wv = w4[o4];
      a0 = fmaf(wv.x, g.x, a0);
      a1 = fmaf(wv.y, g.y, a1);
      a2 = fmaf(wv.z, g.z, a2);
      a3 = fmaf(wv.w, g.w, a3);
    }
    acc += (a0 + a1) + (a2 + a3);
  }
  dx[b * sb + c * sc + f * sf + s * st] = acc;
}

// ---------------------------------------------------------------------------------------------------------
// head: dx per point, part[blockIdx.x] = dwfiP [16][16][96] | dbfiP [16][16] | dwdT [16][16] | dbd [16]
// ---------------------------------------------------------------------------------------------------------
constexpr int kHeadPart = NR * DO * H + NR * DO + DO * DO + DO;
constexpr int kHeadLds = NR * DO * H + H + NR * DO + 2 * H + NR * DO * DO + NR * DO;   // floats

__global__ void __launch_bounds__(256)
sn_head_bwd_kernel(fnssl_btf_view xv, int nt2, int nfc, long long npts, const float* __restrict__ wfiP,
                   const float* __restrict__ bfiP, const float* __restrict__ wdT, const float* __restrict__ dout,
                   float* __restrict__ dx, long long x_sb, long long x_st, long long x_sf, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const wl = lds;                       // wfiP [256 (r, o)][96]
  float* const xs = wl + NR * DO * H;          // the point's x row
  float* const dus = xs + H;                   // du [256 (r, o)]
  float* const px = dus + NR * DO;             // two half sums of dx [2][96]
  float* const red = px + 2 * H;               // dwdT per fine bin [16 r][16 o][16 j]
  float* const redd = red + NR * DO * DO;      // dbd per fine bin [16 r][16 j]
  const int tid = threadIdx.x, r = tid >> 4, o = tid & 15, rowbase = tid & 48;
  for (int q = tid; q < NR * DO * H / 4; q += 256)
    reinterpret_cast<float4*>(wl)[q] = reinterpret_cast<const float4*>(wfiP)[q];
  float wr[H], wd[DO];
  load_row(wr, wfiP + tid * H);
#pragma unroll
  for (int j = 0; j < DO; ++j) wd[j] = wdT[o * DO + j];
  const float bias = bfiP[tid];
  float gw[H], gwd[DO], gb = 0.f, gbd = 0.f;
#pragma unroll
  for (int h = 0; h < H; ++h) gw[h] = 0.f;
#pragma unroll
  for (int j = 0; j < DO; ++j) gwd[j] = 0.f;
  // this thread as (r, j = o): d_r[j] sits at element gg*8 + m*2 + a of the fine bin's 16 outputs, j = a*8 + gg*4 + m
  const int el = ((o >> 2) & 1) * 8 + (o & 3) * 2 + (o >> 3);
  __syncthreads();
  for (long long p = blockIdx.x; p < npts; p += gridDim.x) {
    int fc, t2;
    const long long b = divmod(divmod(p, nfc, fc), nt2, t2);
    if (tid < H / 4)
      reinterpret_cast<float4*>(xs)[tid] = reinterpret_cast<const float4*>(xv.p + b * xv.sb + t2 * xv.st + fc * xv.sf)[tid];
    const float dd = dout[p * (NR * DO) + r * DO + el];
    __syncthreads();
    float u = bias;
#pragma unroll
    for (int h4 = 0; h4 < H / 4; ++h4) {
      const float4 x4 = reinterpret_cast<const float4*>(xs)[h4];
      u = fmaf(wr[4 * h4], x4.x, u);
      u = fmaf(wr[4 * h4 + 1], x4.y, u);
      u = fmaf(wr[4 * h4 + 2], x4.z, u);
      u = fmaf(wr[4 * h4 + 3], x4.w, u);
    }
    const float v = tanh_fast(u);
    float dv = 0.f;
#pragma unroll
    for (int j = 0; j < DO; ++j) {
      const float ddj = __shfl(dd, rowbase + j, 64);       // d_r[j] of this thread's fine bin
      dv = fmaf(wd[j], ddj, dv);
      gwd[j] = fmaf(v, ddj, gwd[j]);
    }
    gbd += dd;
    const float du = dv * fmaf(-v, v, 1.f);
    gb += du;
#pragma unroll
    for (int h4 = 0; h4 < H / 4; ++h4) {
      const float4 x4 = reinterpret_cast<const float4*>(xs)[h4];
      gw[4 * h4] = fmaf(du, x4.x, gw[4 * h4]);
      gw[4 * h4 + 1] = fmaf(du, x4.y, gw[4 * h4 + 1]);
      gw[4 * h4 + 2] = fmaf(du, x4.z, gw[4 * h4 + 2]);
      gw[4 * h4 + 3] = fmaf(du, x4.w, gw[4 * h4 + 3]);
    }
    dus[tid] = du;
    __syncthreads();
    if (tid < 2 * H) {                                      // dx[h] = sum over (r, o) of wfiP[r][o][h] du[r][o], in two halves
      const int half = tid >= H, h = tid - half * H;
      float s = 0.f;
#pragma unroll 8
      for (int q = half * 128; q < half * 128 + 128; ++q) s = fmaf(wl[q * H + h], dus[q], s);
      px[tid] = s;
    }
    __syncthreads();
    if (tid < H) dx[b * x_sb + t2 * x_st + fc * x_sf + tid] = px[tid] + px[H + tid];
  }
  float* const row = part + (long long)blockIdx.x * kHeadPart;
  store_row(row + tid * H, gw);
  row[NR * DO * H + tid] = gb;
#pragma unroll
  for (int j = 0; j < DO; ++j) red[tid * DO + j] = gwd[j];
  redd[tid] = gbd;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int rr = 0; rr < NR; ++rr) s += red[rr * DO * DO + tid];        // tid = (o, j)
  row[NR * DO * H + NR * DO + tid] = s;
  if (tid < DO) {
    float sd = 0.f;
#pragma unroll
    for (int rr = 0; rr < NR; ++rr) sd += redd[rr * DO + tid];
    row[NR * DO * H + NR * DO + DO * DO + tid] = sd;
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
// How the encoder's dW | dbias runs for a shape, and the one description behind its workspace's size, check and carve-up:
// one row of partial sums per workgroup, nothing per point.
struct EncBwdWsLayout {
  bool mfma;                        // cin*5 taps and the row of ones fit the matrix pipe's 160 padded rows
  int kp, rows;                     // padded rows (80 or 160) and rows of a partial (kp, or cin*5 + 1 on the plain path)
  unsigned grid;
  long long per_wg;                 // plain path: points per workgroup
  WsRegion part;                    // [grid, rows, 96]
  size_t total;
  EncBwdWsLayout(long long npts, int cin) {
    const int kk = cin * KE + 1;
    mfma = kk <= 160;
    kp = kk <= 80 ? 80 : 160;
    rows = mfma ? kp : kk;
    const long long cus = fnssl::device_cus();
    if (mfma) {                     // two workgroups per CU at KP 80 (its registers allow it), one at 160
      const long long ntiles = (npts + kEncTile - 1) / kEncTile, cap = cus * (kp == 80 ? 2 : 1);
      grid = (unsigned)(ntiles < cap ? ntiles : cap);
      per_wg = 0;
    } else {
      const long long want = (npts + 63) / 64;
      grid = (unsigned)(want < cus ? want : cus);
      per_wg = (npts + grid - 1) / grid;
      grid = (unsigned)((npts + per_wg - 1) / per_wg);
    }
    part = {0, sizeof(float) * grid * rows * H};
    total = part.end();
  }
};

struct HeadBwdWsLayout {
  unsigned grid;
  WsRegion part;                    // [grid, kHeadPart]
  size_t total;
  explicit HeadBwdWsLayout(long long npts) {
    const long long cus = fnssl::device_cus();
    grid = (unsigned)(npts < cus ? npts : cus);
    part = {0, sizeof(float) * grid * kHeadPart};
    total = part.end();
  }
};

}  // namespace

extern "C" {

size_t fnssl_sn_encoder_backward_workspace_bytes(int nb, int cin, int nf, int nt) {
  if (nb <= 0 || cin <= 0 || nf <= 0 || nt <= 0) return 0;
  return EncBwdWsLayout((long long)nb * nf * nt, cin).total;
}

int fnssl_sn_encoder_backward(const float* x, long long x_sb, long long x_sc, long long x_sf, long long x_st, int nb,
                              int cin, int nf, int nt, const float* wT, const float* dout, long long d_sb, long long d_st,
                              long long d_sf, float* dwT, float* dbias, float* dx, long long dx_sb, long long dx_sc,
                              long long dx_sf, long long dx_st, void* workspace, size_t workspace_bytes, void* stream) {
  FNSSL_REQUIRE(x && dwT && dbias, "sn_encoder_backward: null pointer (x, dwT, dbias)");
  FNSSL_REQUIRE(nb > 0 && cin > 0 && nf > 0 && nt > 0, "sn_encoder_backward: empty problem");
  FNSSL_REQUIRE(cin <= (1 << 20), "sn_encoder_backward: cin %d is out of range", cin);
  FNSSL_REQUIRE(x_sb >= 0 && x_sc >= 0 && x_sf >= 0 && x_st >= 0, "sn_encoder_backward: x strides must not be negative");
  FNSSL_REQUIRE(out_ok(dout, d_sb, d_st, d_sf), "sn_encoder_backward: dout must be 16-byte aligned with strides %% 4 == 0");
  FNSSL_REQUIRE(!dx || (wT && reinterpret_cast<size_t>(wT) % 16 == 0), "sn_encoder_backward: dx needs the 16-byte aligned weights wT");
  FNSSL_REQUIRE(!dx || (dx_sb >= 0 && dx_sc >= 0 && dx_sf >= 0 && dx_st >= 0), "sn_encoder_backward: dx strides must not be negative");
  const long long npts = (long long)nb * nf * nt;
  FNSSL_REQUIRE(npts * cin < (1ll << 40), "sn_encoder_backward: too many points");
  const EncBwdWsLayout ws(npts, cin);
  FNSSL_TRY(check_workspace("sn_encoder_backward", workspace, workspace_bytes, ws.total));
  float* const part = ws.part.floats(workspace);
  hipStream_t s = fnssl::as_stream(stream);
  {
    fnssl::TimedLaunch tl("sn_encoder_bwd_w", s, 2.0 * npts * (cin * KE + 1) * H);
    if (ws.mfma) {
      // a frame-major dY is walked in its own memory order
      const int f_fast = d_sf < d_st;
      if (ws.kp == 80)
        FNSSL_TRY(enqueue(s, Kernel{sn_encoder_bwd_w_kernel<5, 4>, 256, 0, "sn_encoder_bwd_w_kernel"}, ws.grid, x, x_sb, x_sc, x_sf,
                          x_st, cin, nf, nt, npts, f_fast, dout, d_sb, d_st, d_sf, part));
      else
        FNSSL_TRY(enqueue(s, Kernel{sn_encoder_bwd_w_kernel<10, 2>, 256, 0, "sn_encoder_bwd_w_kernel"}, ws.grid, x, x_sb, x_sc, x_sf,
                          x_st, cin, nf, nt, npts, f_fast, dout, d_sb, d_st, d_sf, part));
    } else {
      FNSSL_TRY(enqueue(s, Kernel{sn_encoder_bwd_w_plain_kernel, 256, 0, "sn_encoder_bwd_w_plain_kernel"}, ws.grid, x, x_sb, x_sc,
                        x_sf, x_st, cin, nf, nt, npts, ws.per_wg, dout, d_sb, d_st, d_sf, part));
    }
  }
  {
    fnssl::TimedLaunch tl("sn_encoder_bwd_reduce", s);
    FNSSL_TRY(reduce_rows(s, part, ws.grid, (long long)ws.rows * H, cin * KE * H, dwT, H, dbias));
  }
  if (dx) {
    const long long nel = npts * cin;
    fnssl::TimedLaunch tl("sn_encoder_bwd_x", s, 2.0 * nel * KE * H);
    FNSSL_TRY(enqueue(s, Kernel{sn_encoder_bwd_x_kernel, 256, 0, "sn_encoder_bwd_x_kernel"}, blocks_of(nel), wT, cin, nf, nt, nel,
                      dout, d_sb, d_st, d_sf, dx, dx_sb, dx_sc, dx_sf, dx_st));
  }
  return FNSSL_OK;
}

size_t fnssl_sn_head_backward_workspace_bytes(int nb, int nt2, int nfc) {
  if (nb <= 0 || nt2 <= 0 || nfc <= 0) return 0;
  return HeadBwdWsLayout((long long)nb * nt2 * nfc).total;
}

int fnssl_sn_head_backward(const fnssl_btf_view* x, int nb, int nt2, int nfc, const float* wfiP, const float* bfiP,
                           const float* wdT, const float* dout, float* dx, long long x_sb, long long x_st, long long x_sf,
                           const fnssl_sn_head_grads* g, void* workspace, size_t workspace_bytes, void* stream) {
  FNSSL_REQUIRE(view_ok(x), "sn_head_backward: x must be 16-byte aligned with strides %% 4 == 0");
  FNSSL_REQUIRE(wfiP && bfiP && wdT && reinterpret_cast<size_t>(wfiP) % 16 == 0, "sn_head_backward: null / unaligned weights");
  FNSSL_REQUIRE(g && g->wfiP && g->bfiP && g->wdT && g->bd, "sn_head_backward: null gradient pointer (g)");
  FNSSL_REQUIRE(nb > 0 && nfc > 0 && nt2 > 0, "sn_head_backward: empty problem");
  FNSSL_REQUIRE(dout && reinterpret_cast<size_t>(dout) % 16 == 0, "sn_head_backward: dout must be 16-byte aligned");
  FNSSL_REQUIRE(out_ok(dx, x_sb, x_st, x_sf), "sn_head_backward: dx must be 16-byte aligned with strides %% 4 == 0");
  const long long npts = (long long)nb * nt2 * nfc;
  FNSSL_REQUIRE(npts < (1ll << 31), "sn_head_backward: too many points");
  const HeadBwdWsLayout ws(npts);
  FNSSL_TRY(check_workspace("sn_head_backward", workspace, workspace_bytes, ws.total));
  float* const part = ws.part.floats(workspace);
  hipStream_t s = fnssl::as_stream(stream);
  {
    fnssl::TimedLaunch tl("sn_head_bwd", s, 2.0 * npts * NR * (3.0 * DO * H + 2.0 * DO * DO));
    FNSSL_TRY(enqueue(s, Kernel{sn_head_bwd_kernel, 256, (size_t)kHeadLds * sizeof(float), "sn_head_bwd_kernel"}, ws.grid, *x, nt2,
                      nfc, npts, wfiP, bfiP, wdT, dout, dx, x_sb, x_st, x_sf, part));
  }
  fnssl::TimedLaunch tl("sn_head_bwd_reduce", s);
  return reduce_rows(s, part, ws.grid, kHeadPart, NR * DO * H, g->wfiP, NR * DO, g->bfiP, DO * DO, g->wdT, DO, g->bd);
}

}  // extern "C"
