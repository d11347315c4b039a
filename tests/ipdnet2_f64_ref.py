"""float64 restatement of every IPDnet2 / OnlineSpatialNet op.  TEST INFRASTRUCTURE ONLY.

Plain numpy in float64, written from the published definitions (nn.LayerNorm, CausalConv1d, grouped Conv1d + PReLU,
the squeeze / Linear-over-F / unsqueeze branch, Mamba as h_t = exp(dt A) h_{t-1} + dt B_t u_t in RECURRENT form,
FreqInverse + tanh + decoder).  It calls nothing of the library under test and nothing of ``oracle/``; the host tests in
test_ipdnet2_f64_ref_host.py pin it to the float32 oracle, to the reference's own golden outputs and to the O(T^2)
parallel float64 form.  Its purpose is the tolerance of test_gpu_ipdnet2_f64.py: the float32 oracle's own distance from
this module is the yardstick the fp32 kernels are held to.

Layouts follow the device entry points (fnssl/spatialnet.py): activations are [B, F, T, H]; Mamba sequences are
[S, T, H] with S = B * F; the Mamba state is (conv_state [S, K-1, E] = the last K-1 inputs of the depthwise conv, oldest
first, ssm_state [S, E, N]).  Weights are taken by their state_dict names (fnssl.weights.ipdnet2_param_shapes).
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

F8 = np.float64


def _d(a):
    return np.asarray(a, dtype=F8)


def silu(x):
    x = _d(x)
    return x / (1.0 + np.exp(-x))


def softplus(x):
    """log(1 + e^x) without overflow or cancellation: log1p(exp(-|x|)) + max(x, 0)."""
    x = _d(x)
    return np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0.0)


def layer_norm(x, w, b, eps=1e-5, mean_err=None):
    """nn.LayerNorm over the last axis (biased variance, eps inside the root).  ``mean_err`` (broadcastable to
    x[..., :1]) is added to the row means before they are subtracted: the model of a device whose mean carries a
    rounding error, used to turn a bound on that error into a bound on an op's output (the variance is taken about the
    exact mean: its change is second order)."""
    x = _d(x)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    if mean_err is not None:
        mu = mu + _d(mean_err)
    return (x - mu) / np.sqrt(var + eps) * _d(w) + _d(b)


def causal_conv1d(x, w, b, state=None):
    """Causal Conv1d along the last axis.  x [..., C, T], w [O, C, K], b [O]; state [..., C, K-1] = the previous
    chunk's last K-1 input frames (None: zeros).  Returns (y [..., O, T], new state)."""
    x, w = _d(x), _d(w)
    K = w.shape[2]
    prev = np.zeros(x.shape[:-1] + (K - 1,)) if state is None else _d(state)
    xp = np.concatenate([prev, x], axis=-1)
    T = x.shape[-1]
    y = sum(np.einsum("oc,...ct->...ot", w[:, :, k], xp[..., k:k + T]) for k in range(K))
    return y + _d(b)[:, None], xp[..., xp.shape[-1] - (K - 1):].copy()


def encoder(sd_w, sd_b, x, state=None):
    """The network's encoder: x [B, C, F, T] -> ([B, F, T, H], state [B, C, F, K-1])."""
    xs = _d(x).transpose(0, 2, 1, 3)                                     # [B, F, C, T]
    st = None if state is None else _d(state).transpose(0, 2, 1, 3)
    y, st = causal_conv1d(xs, sd_w, sd_b, st)
    return y.transpose(0, 1, 3, 2), st.transpose(0, 2, 1, 3)


def avgpool_f(x, k):
    x = _d(x)
    B, F, T, H = x.shape
    return x[:, :F // k * k].reshape(B, F // k, k, T, H).mean(2)


def avgpool_t(x, k):
    x = _d(x)
    B, F, T, H = x.shape
    return x[:, :, :T // k * k].reshape(B, F, T // k, k, H).mean(3)


def fconv(sd, p, x, groups=8, residual=False, pool=1, mean_err=None):
    """pool_F(x + PReLU(Conv1d_grouped('same', zeros)(LN(x)))) along F.  p + '.0' LN, '.1' conv [H, H/groups, K], '.2'
    PReLU.  x [B, F, T, H]."""
    x = _d(x)
    y = layer_norm(x, sd[p + ".0.weight"], sd[p + ".0.bias"], mean_err=mean_err)
    w, b = _d(sd[p + ".1.weight"]), _d(sd[p + ".1.bias"])
    H, cg, K = w.shape
    og, pad = H // groups, (K - 1) // 2
    B, F, T, _ = y.shape
    yp = np.pad(y, ((0, 0), (pad, K - 1 - pad), (0, 0), (0, 0)))
    out = np.empty_like(y)
    for g in range(groups):
        acc = 0.0
        for k in range(K):
            acc = acc + np.einsum("oc,bftc->bfto", w[g * og:(g + 1) * og, :, k], yp[:, k:k + F, :, g * cg:(g + 1) * cg])
        out[..., g * og:(g + 1) * og] = acc
    out += b
    out = np.where(out >= 0, out, _d(sd[p + ".2.weight"]) * out)
    if residual:
        out = x + out
    return avgpool_f(out, pool) if pool > 1 else out


def full(sd, p, x, residual=False, mean_err=None):
    """x + SiLU(unsqueeze(Linear_over_F(SiLU(squeeze(LN(x))))));  p = 'layers.N.'.  x [B, F, T, H]."""
    x = _d(x)
    y = layer_norm(x, sd[p + "norm_full.weight"], sd[p + "norm_full.bias"], mean_err=mean_err)
    s = silu(y @ _d(sd[p + "squeeze.0.weight"])[:, :, 0].T + _d(sd[p + "squeeze.0.bias"]))      # [B, F, T, Hs]
    s = np.einsum("gf,bftq->bgtq", _d(sd[p + "full.weight"]), s) + _d(sd[p + "full.bias"])[None, :, None, None]
    out = silu(s @ _d(sd[p + "unsqueeze.0.weight"])[:, :, 0].T + _d(sd[p + "unsqueeze.0.bias"]))
    return x + out if residual else out


def mamba(sd, p, x, state=None):
    """One Mamba block in recurrent form, vectorised over sequences and channels.  x [S, T, D] ->
    (out [S, T, D], (conv_state [S, K-1, E], ssm_state [S, E, N])).  p = '....mhsa.' (mamba_ssm.Mamba's names)."""
    f8 = lambda k: _d(sd[p + k])   # noqa: E731
    x = _d(x)
    S, T, _ = x.shape
    w_in = f8("in_proj.weight")
    E = w_in.shape[0] // 2
    xz = x @ w_in.T
    xi, z = xz[..., :E], xz[..., E:]
    wc, bc = f8("conv1d.weight")[:, 0, :], f8("conv1d.bias")
    K = wc.shape[1]
    prev = np.zeros((S, K - 1, E)) if state is None else _d(state[0])
    xp = np.concatenate([prev, xi], axis=1)
    u = bc + sum(xp[:, k:k + T] * wc[:, k] for k in range(K))
    u = silu(u)
    wx = f8("x_proj.weight")
    A = -np.exp(f8("A_log"))                                             # [E, N]
    N = A.shape[1]
    R = wx.shape[0] - 2 * N
    dbl = u @ wx.T
    dt = softplus(dbl[..., :R] @ f8("dt_proj.weight").T + f8("dt_proj.bias"))
    Bm, Cm = dbl[..., R:R + N], dbl[..., R + N:]
    h = np.zeros((S, E, N)) if state is None else _d(state[1]).copy()
    y = np.empty((S, T, E))
    dtu = dt * u

    def scan(sl):                                                        # the recurrence on a block of sequences, in place
        hs, buf = h[sl], np.empty_like(h[sl])
        for t in range(T):
            np.multiply(dt[sl, t, :, None], A, out=buf)
            np.exp(buf, out=buf)
            hs *= buf
            np.multiply(dtu[sl, t, :, None], Bm[sl, t, None, :], out=buf)
            hs += buf
            y[sl, t] = np.matmul(hs, Cm[sl, t, :, None])[..., 0]

    # sequences are independent: blocks of them run on a few threads (numpy releases the GIL inside its loops), so that
    # 272 sequences x 250 steps, or 4 100 x 32, stay within seconds
    nblk = min(8, -(-S // 64))
    blocks = [slice(i * S // nblk, (i + 1) * S // nblk) for i in range(nblk)]
    if nblk == 1:
        scan(blocks[0])
    else:
        with ThreadPoolExecutor(max_workers=nblk) as pool:
            list(pool.map(scan, blocks))
    y = (y + f8("D") * u) * silu(z)
    return y @ f8("out_proj.weight").T, (xp[:, xp.shape[1] - (K - 1):].copy(), h)


def mamba_block(sd, p_norm, p_mamba, x, state=None, residual=False, time_pool=1, mean_err=None):
    """pool_T(x + Mamba(LN(x))) along T for every (b, f).  x [B, F, T, H] -> ([B, F, T // pool, H], state)."""
    x = _d(x)
    B, F, T, H = x.shape
    y = layer_norm(x, sd[p_norm + ".weight"], sd[p_norm + ".bias"], mean_err=mean_err).reshape(B * F, T, H)
    y, st = mamba(sd, p_mamba + ".", y, state)
    y = y.reshape(B, F, T, H)
    if residual:
        y = x + y
    return (avgpool_t(y, time_pool) if time_pool > 1 else y), st


def head(sd, x, ratio=16):
    """FreqInverse (1x1 conv H -> ratio * out per compressed bin, fine bin f = fc * ratio + r takes outputs o * ratio +
    r), tanh, decoder Linear and the output re-ordering out[b, t, 2 f + g, m, a] = dec[b, f, t, a * 8 + g * 4 + m].
    x [B, Fc, T, H] -> [B, T, 2 * ratio * Fc, out / 4, 2]."""
    x = _d(x)
    B, Fc, T, H = x.shape
    w, b = _d(sd["freq_inverse.trans2.weight"])[:, :, 0], _d(sd["freq_inverse.trans2.bias"])
    do = w.shape[0] // ratio
    y = (x @ w.T + b).reshape(B, Fc, T, do, ratio)                        # output index o * ratio + r
    y = np.tanh(y.transpose(0, 1, 4, 2, 3).reshape(B, Fc * ratio, T, do))  # [B, F, T, do]
    y = y @ _d(sd["decoder.weight"]).T + _d(sd["decoder.bias"])
    F = Fc * ratio
    y = y.reshape(B, F, T, 2, 2, do // 4)                                 # [.., a, g, m]
    return np.ascontiguousarray(y.transpose(0, 2, 1, 4, 5, 3)).reshape(B, T, 2 * F, do // 4, 2)


def layer_forward(sd, p, x, is_first, state=None):
    """One SpatialNetLayer: fconv1 (+ F-pool 2 in the first layer), full, fconv2 (+ F-pool 8), two LN + Mamba blocks,
    each with its residual.  state = [state of block 0, state of block 1] or None."""
    x = fconv(sd, p + "fconv1", x, residual=True, pool=2 if is_first else 1)
    x = full(sd, p, x, residual=True)
    x = fconv(sd, p + "fconv2", x, residual=True, pool=8 if is_first else 1)
    st = [None, None] if state is None else list(state)
    x, st[0] = mamba_block(sd, p + "norm_mhsa", p + "mhsa", x, st[0], residual=True)
    x, st[1] = mamba_block(sd, p + "norm_tconvffn", p + "tconvffn", x, st[1], residual=True)
    return x, st


def forward(sd, x, time_ratio=5, state=None):
    """The whole network.  x [B, C, F, T] -> [B, T // ratio, 2 F, out / 4, 2]; with ``state`` (a dict, {} for the first
    chunk) also the carried state (T must then be a multiple of the time ratio)."""
    enc_state = None if not state else state.get("enc")
    y, enc_new = encoder(sd["encoder.weight"], sd["encoder.bias"], x, enc_state)
    new_state = {"enc": enc_new}
    nl = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("layers."))
    for l in range(nl):
        y, st = layer_forward(sd, "layers.%d." % l, y, l == 0, None if not state else state.get("l%d" % l))
        new_state["l%d" % l] = st
        if l == 0:
            y = avgpool_t(y, time_ratio)
    out = head(sd, y, ratio=x.shape[2] // y.shape[1])
    return (out, new_state) if state is not None else out


# ------------------------------------------------------------------------------------------------------------------ #
# The scan probe of test_gpu_ipdnet2_f64.py: a Mamba parameter set whose outputs are single inner channels.
# ------------------------------------------------------------------------------------------------------------------ #
LAST_LT1 = -16.635532                    # the largest float32 x with 1 + e^x == 1 in float32 is just below this:
                                         # e^x < 2^-24  <=>  x < -24 ln 2 = -16.63553233...


def f32_neighbours(v, k=1):
    """[v - k steps, ..., v, ..., v + k steps] in float32."""
    v = np.float32(v)
    out = [v]
    lo = hi = v
    for _ in range(k):
        lo = np.nextafter(lo, np.float32(-np.inf))
        hi = np.nextafter(hi, np.float32(np.inf))
        out = [lo] + out + [hi]
    return np.asarray(out, np.float32)


def probe_state(sd, p, half, kind, seed=0):
    """A copy of the Mamba parameters under prefix ``p`` turned into a probe (float32 arrays, as a checkpoint holds):
      out_proj one-hot: output d = inner channel 96 * half + d;  D = 0;
      A_log uniform in [ln 1e-2, ln 64];
      kind 'spread':  dt_proj.bias spread over the 192 channels across [-25, 25] (shuffled)
      kind 'exact':   dt_proj.weight = 0 and dt_proj.bias on the branch points of a fast softplus: 20 and its float32
                      neighbours, the last value with 1 + e^x > 1 in float32 and its neighbours, a sweep over [-60, 60]
      kind 'silu':    'spread' with in_proj.weight * 4 (|u|, |z| in the tens)."""
    rs = np.random.RandomState(seed)
    out = {k: np.array(v, np.float32) for k, v in sd.items() if k.startswith(p)}
    E, N = out[p + "A_log"].shape
    D = out[p + "out_proj.weight"].shape[0]
    wo = np.zeros((D, E), np.float32)
    wo[np.arange(D), half * D + np.arange(D)] = 1.0
    out[p + "out_proj.weight"] = wo
    out[p + "D"] = np.zeros(E, np.float32)
    out[p + "A_log"] = rs.uniform(np.log(1e-2), np.log(64.0), size=(E, N)).astype(np.float32)
    if kind in ("spread", "silu"):
        out[p + "dt_proj.bias"] = rs.permutation(np.linspace(-25.0, 25.0, E)).astype(np.float32)
        if kind == "silu":
            out[p + "in_proj.weight"] = out[p + "in_proj.weight"] * np.float32(4.0)
    elif kind == "exact":
        out[p + "dt_proj.weight"] = np.zeros_like(out[p + "dt_proj.weight"])
        edge = np.concatenate([f32_neighbours(20.0, 2), f32_neighbours(LAST_LT1, 3)])
        # dense where the quotient e / ((1 + e) - 1) has few significant bits, then the wide sweep
        near = np.linspace(-16.6, -9.0, 40).astype(np.float32)
        sweep = np.linspace(-60.0, 60.0, E - len(edge) - len(near)).astype(np.float32)
        out[p + "dt_proj.bias"] = rs.permutation(np.concatenate([edge, near, sweep])).astype(np.float32)
    else:
        raise ValueError(kind)
    return out


def channel_rel_err(got, want):
    """The probe's metric: per output channel (last axis), max |got - want| over every other axis divided by that
    channel's max |want|.  Returns (errors [D], scales [D])."""
    got, want = _d(got), _d(want)
    ax = tuple(range(want.ndim - 1))
    scale = np.abs(want).max(axis=ax)
    return np.abs(got - want).max(axis=ax) / scale, scale


def rms_rel_err(got, want):
    """max |got - want| over everything, relative to the rms of want."""
    got, want = _d(got), _d(want)
    return float(np.abs(got - want).max() / np.sqrt((want ** 2).mean()))
