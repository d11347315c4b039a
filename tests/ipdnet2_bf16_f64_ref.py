"""Float64 reference, flip bound, checker, legs and table of gates for the bf16 IPDnet2 kernels (csrc/spatialnet.hip,
``BF = true``).  TEST INFRASTRUCTURE ONLY: numpy float64 on top of tests/ipdnet2_f64_ref.py; nothing of the library under
test is called — with one exception: the seeded state dicts come from fnssl.weights.make_ipdnet2_state, a numpy
generator of parameter values that runs no kernel.  Imported by test_ipdnet2_bf16_f64_ref_host.py (CPU) and
test_gpu_ipdnet2_bf16_f64.py (GPU).

One product at a time.  Every bf16 product of the kernels is restated as  y = bf16_rne(W) . bf16_rne(a)  in float64, where
``a`` is either a row the device STORED (the encoder's input, xz / the pooled y in the Mamba workspace: exact, the kernel
rounded these very bits) or an intermediate only the kernel saw (a LayerNorm output, SiLU(conv + b), the squeezed row),
which the reference computes itself in float64.

Flip bound.  An in-kernel intermediate a_k is known to within eps (the fp32 error of forming it).  Rounding is monotone,
so the device's bf16(a_k^dev), a_k^dev in [a_k - eps, a_k + eps], lies in [bf16(a_k - eps), bf16(a_k + eps)]:
    flip(a_k, eps) = max(bf16(a_k + eps) - bf16(a_k), bf16(a_k) - bf16(a_k - eps))
is zero unless a bf16 midpoint lies within eps of a_k, and is then spacing(a_k) times the number of midpoints on the
worse side (exact at binade edges too), and
    |y^dev_o - y_o|  <=  delta + sum_k |bf16(W_ok)| * flip(a_k, eps).
Through a pointwise function the bound is multiplied by its Lipschitz constant (PReLU: max(1, |slope|); SiLU: 1.1),
through a pooling it is averaged, and in a chain the next operand's eps is  eps_stage + L * bound.  An element is TIGHT
when bound <= delta; every leg must be mostly tight (``leg_condition``) so that the comparison is, where it matters, the
fp32 gate ``delta`` and nothing else.

delta and eps are never taken from the kernels: delta = MARGIN x the float32 oracle's distance from this reference over
the leg's tight elements (oracle/ipdnet2_oracle.py's arithmetic under bf16 rounding, phase by phase, each phase fed by
its own float32 run of the phase before), eps = MARGIN x the oracle's distance of that intermediate from float64.  The
measured figures are the ORACLE table below (re-measured by the host test; DESIGN.md section 7 repeats them).
"""
from __future__ import annotations

import collections
import functools

import numpy as np

import ipdnet2_f64_ref as R8
from lstm_bf16_f64_ref import force_ties, fp32_block
from oracle import ipdnet2_oracle as O

F4, F8 = np.float32, np.float64
MARGIN = 8.0                 # v_exp_f32 / v_rcp_f32 against libm, and the MFMA accumulation order
MI355X_CUS = 256
H, HS, E, NST, RK, KC, XP = 96, 8, 192, 16, 6, 4, 40
SILU_LIP = 1.1               # sup |SiLU'| = 1.0998
P_NORM, P_MAMBA = "layers.1.norm_mhsa", "layers.1.mhsa"


# ------------------------------------------------------------------------------------------------------------------ #
# rounding
# ------------------------------------------------------------------------------------------------------------------ #
def bf16_rne(v):
    """fp32 values -> nearest-even bf16, as float64.  Integer arithmetic on the bits: the kept half goes up when the
    dropped half is above 0x8000, or equal to it with an odd kept mantissa."""
    a = np.ascontiguousarray(v, dtype=F4)
    u = a.reshape(-1).view(np.uint32).astype(np.uint64)
    keep, low = u >> np.uint64(16), u & np.uint64(0xFFFF)
    up = (low > 0x8000) | ((low == 0x8000) & ((keep & np.uint64(1)) == 1))
    keep = keep + up.astype(np.uint64)
    return (keep << np.uint64(16)).astype(np.uint32).view(F4).astype(F8).reshape(a.shape)


def spacing(v):
    """Distance between neighbouring bf16 values in the binade of |v| (8 significant bits), floored at the smallest
    normal binade."""
    a = np.abs(np.asarray(v, dtype=F8))
    _, e = np.frexp(a)                                         # |v| in [2^(e-1), 2^e)
    return np.ldexp(1.0, np.maximum(np.where(a == 0, -125, e), -125) - 8)


def bf16_real(v):
    """Real (float64) values -> nearest-even bf16: v / spacing is exact, rint rounds halves to even, and an even
    quotient is an even kept mantissa.  Equals bf16_rne on fp32 values (pinned by the host test)."""
    v = np.asarray(v, dtype=F8)
    s = spacing(v)
    return np.rint(v / s) * s


def q(a):
    """Operand of a product: the exact integer rounding for fp32 arrays, the real one for the reference's float64."""
    a = np.asarray(a)
    return bf16_rne(a) if a.dtype == F4 else bf16_real(a)


def flip(a, eps):
    """Largest change of bf16(a') over a' in [a - eps, a + eps] (rounding is monotone)."""
    a = np.asarray(a, dtype=F8)
    c = bf16_real(a)
    return np.maximum(bf16_real(a + eps) - c, c - bf16_real(a - eps))


def nties(a, eps):
    """flip in units of the local bf16 spacing: the number of midpoints on the worse side of a within eps."""
    return flip(a, eps) / spacing(a)


def product(w, a, eps=None):
    """w [O, K] fp32 weights, a [..., K] -> (y [..., O], bound [..., O]).  ``eps`` None: a is a stored row (fp32, exact
    operand, bound 0); else a is the reference's float64 intermediate, known to the device within eps (scalar or
    array like a)."""
    wq = bf16_rne(w)
    y = q(a) @ wq.T
    if eps is None:
        assert np.asarray(a).dtype == F4, "a stored operand is fp32"
        return y, np.zeros_like(y)
    return y, flip(a, eps) @ np.abs(wq).T


def ln_scaled(x, w, b):
    """(float64 LayerNorm output, the magnitude its fp32 error is proportional to).  y = d * rstd * w + b with d = x - mean:
    the mean is off by a few 2^-24 of the row's largest |x| (the same for every channel of the row, whatever |d|), the
    products by 2^-24 of themselves:  scale_k = |w_k| * rstd * (max |x_row| + |d_k|) + |b_k|.  An eps proportional to this,
    not one absolute figure sized for the largest outputs, keeps a midpoint from sitting next to every small output."""
    x = np.asarray(x, dtype=F8)
    mu = x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + 1e-5)
    scale = np.abs(np.asarray(w, F8)) * rstd * (np.abs(x).max(-1, keepdims=True) + np.abs(x - mu)) + np.abs(np.asarray(b, F8))
    return R8.layer_norm(x, w, b), scale


def ln_distance(x, w, b):
    """The float32 oracle's LayerNorm against float64, in units of ``ln_scaled``'s scale (outputs below 1e29 only: the
    planted fconv leg holds 1e30 in channels no product reads)."""
    r, sc = ln_scaled(x, w, b)
    return float((np.abs(O.layer_norm(x, w, b) - r) / sc)[np.abs(r) < 1e29].max())


def tie_w(w, salt=0):
    """A weight tensor with the bf16 LSTM file's tie scheme: no element bf16-representable, one of every eight on an
    exact tie (low half 0x8000) with the kept mantissa even or odd by a hash of the index."""
    w = np.ascontiguousarray(w, dtype=F4)
    bits = w.reshape(-1).view(np.uint32).astype(np.int64)
    idx = np.arange(bits.size, dtype=np.int64) + 8 * int(salt)
    return force_ties(bits, idx).astype(np.uint32).view(F4).reshape(w.shape)


def tie_state(sd, names):
    sd = collections.OrderedDict(sd)
    for i, n in enumerate(names):
        sd[n] = tie_w(sd[n], 1000 * i + 1)
    return sd


# ------------------------------------------------------------------------------------------------------------------ #
# checker
# ------------------------------------------------------------------------------------------------------------------ #
Cmp = collections.namedtuple("Cmp", "key ref bound pos rule")    # rule "abs": delta + bound per element; "rms": fp32 rule
MIN_SHARE, MIN_TIGHT = 1.0 / 3.0, 10000


def leg_condition(cs, delta, what=""):
    """The condition on a leg (``cs``: the comparisons of its calls that share one gate), from the reference alone: at
    least 1/3 of the elements tight, at least 10 000 tight elements, every output channel (last axis) and every position of
    a point in its 16-point tile with a tight element.  -> (tight share, tight elements)."""
    tight = np.concatenate([(c.bound <= delta).reshape(-1, c.bound.shape[-1]) for c in cs])
    pos = np.concatenate([np.broadcast_to(c.pos, c.bound.shape).reshape(-1, c.bound.shape[-1]) for c in cs])
    share, n = float(tight.mean()), int(tight.sum())
    assert share >= MIN_SHARE, "%s: only %.1f %% of the elements are tight" % (what, 100 * share)
    assert n >= MIN_TIGHT, "%s: only %d tight elements" % (what, n)
    assert tight.any(axis=0).all(), "%s: an output channel has no tight element" % what
    assert set(np.unique(pos[tight])) == set(np.unique(pos)), "%s: a tile position has no tight element" % what
    return share, n


def stats(c, got, delta):
    got = np.asarray(got, dtype=F8)
    assert got.shape == c.ref.shape, (c.key, got.shape, c.ref.shape)
    if c.rule == "rms":
        return {"rms": R8.rms_rel_err(got, c.ref), "finite": bool(np.isfinite(got).all())}
    err = np.abs(got - c.ref)
    tight = c.bound <= delta
    return {"tight_max": float(err[tight].max()) if tight.any() else 0.0, "share": float(tight.mean()),
            "excess": float((err - c.bound).max()), "viol": int((err > delta + c.bound).sum()),
            "worst": float((err / (delta + c.bound)).max()) if delta > 0 else float(err.max()),
            "finite": bool(np.isfinite(got).all())}


def check(c, got, delta, report=print):
    """|got - ref| <= delta + bound on EVERY element (rule "abs"), or max |got - ref| / rms(ref) <= delta (rule "rms",
    the all-fp32 scan: the rule of test_gpu_ipdnet2_f64.py).  Figures are printed before they are asserted."""
    s = stats(c, got, delta)
    if c.rule == "rms":
        report("%-40s rms-rel %.3e (gate %.3e)" % (c.key, s["rms"], delta))
        assert s["finite"] and s["rms"] <= delta, "%s: %.3e > %.3e" % (c.key, s["rms"], delta)
        return s
    report("%-40s tight %.1f %%: max %.3e (delta %.3e); all: max (err - bound) %.3e, worst err / (delta + bound) %.3f"
           % (c.key, 100 * s["share"], s["tight_max"], delta, s["excess"], s["worst"]))
    assert s["finite"], "%s: non-finite output" % c.key
    assert s["viol"] == 0, "%s: %d elements outside delta + bound (tight max %.3e, delta %.3e, max excess %.3e)" % (
        c.key, s["viol"], s["tight_max"], delta, s["excess"])
    return s


# ------------------------------------------------------------------------------------------------------------------ #
# rounding hooks of the float32 oracle runners (the host test's mutants replace them)
# ------------------------------------------------------------------------------------------------------------------ #
class Rounding:
    """qa: operand -> bf16 (fp32 array), qw: weight -> bf16, wmod(name, W [O, K] rounded) -> the matrix the product uses."""

    def __init__(self, qa=O.bf16_round, qw=O.bf16_round, wmod=None):
        self.qa, self.qw, self.wmod = qa, qw, wmod

    def w(self, name, w2d):
        w2d = self.qw(np.ascontiguousarray(w2d, dtype=F4))
        return w2d if self.wmod is None else self.wmod(name, w2d)


RNE = Rounding()


def _mm(a, w):
    return (a @ w.T).astype(F4)


# ------------------------------------------------------------------------------------------------------------------ #
# encoder  (sn_encoder_mfma_kernel<KP, true, PIPE>): x is the direct operand, bound 0 everywhere
# ------------------------------------------------------------------------------------------------------------------ #
def encoder_inputs(seed, cin, nb, nf, nt):
    x = fp32_block(seed, (nb, cin, nf, nt), 1.0)
    w = tie_w(np.random.RandomState(seed + 1).uniform(-1, 1, (H, cin, 5)).astype(F4) * F4(0.1), 1)
    b = (np.random.RandomState(seed + 2).standard_normal(H) * 0.1).astype(F4)
    return x, w, b


def encoder_ref(x, w, b, state=None, key="encoder"):
    """x [B, C, F, T] fp32, state [B, C, F, 4] fp32 (the carried frames are operands like x) -> Cmp on [B, F, T, 96]."""
    y, _ = R8.encoder(bf16_rne(w), b, bf16_rne(x), None if state is None else bf16_rne(state))
    B, F, T, _ = y.shape
    p = (np.arange(B * F * T).reshape(B, F, T, 1)) % 16
    return Cmp(key, y, np.zeros_like(y), p, "abs")


def oracle_encoder(x, w, b, state=None, rnd=RNE):
    """The float32 oracle's causal conv (ipdnet2_oracle.causal_conv1d's arithmetic) with the rounding hooks:
    -> (out [B, F, T, 96], new state [B, C, F, 4])."""
    x = np.asarray(x, dtype=F4)
    B, C, F, T = x.shape
    xs = x.transpose(0, 2, 1, 3).reshape(B * F, C, T)
    prev = np.zeros((B * F, C, 4), F4) if state is None else np.asarray(state, F4).transpose(0, 2, 1, 3).reshape(B * F, C, 4)
    xp = np.concatenate([prev, xs], axis=-1)
    wm = rnd.w("encoder", np.asarray(w, F4).reshape(H, C * 5)).reshape(H, C, 5)
    y = np.zeros((B * F, H, T), F4)
    for k in range(5):
        y += np.einsum("oc,bct->bot", wm[:, :, k], rnd.qa(xp[:, :, k:k + T])).astype(F4)
    y = (y + np.asarray(b, F4)[None, :, None]).astype(F4)
    st = xp[:, :, -4:].reshape(B, F, C, 4).transpose(0, 2, 1, 3)
    return y.transpose(0, 2, 1).reshape(B, F, T, H), np.ascontiguousarray(st)


# ------------------------------------------------------------------------------------------------------------------ #
# Mamba block, phase by phase.  MambaWsLayout (csrc/spatialnet.hip) restated: floats, in this order, no padding.
# ------------------------------------------------------------------------------------------------------------------ #
def mamba_ws_layout(npts):
    """{region: (first float, floats per point)} and the total in bytes of fnssl_sn_mamba's workspace."""
    lay, off = collections.OrderedDict(), 0
    for name, width in (("xz", 2 * E), ("dbl", XP), ("y", E)):
        lay[name] = (off, width)
        off += npts * width
    return lay, 4 * off


def mamba_state_dict(seed):
    from fnssl import weights as W
    sd = W.make_ipdnet2_state(seed, num_layers=2)
    return tie_state(sd, [P_MAMBA + ".in_proj.weight", P_MAMBA + ".x_proj.weight", P_MAMBA + ".out_proj.weight"])


def pool32(y, tp):
    """The kernel's fp32 time pooling, restated exactly (sn_mamba_out_mfma_kernel): the tp frames are added in frame
    order starting from 0.f, then ONE multiplication by float32(1 / tp).  y [S, T, C] fp32 -> [S, T // tp, C] fp32."""
    y = np.asarray(y, dtype=F4)
    S, T, C = y.shape
    n = T // tp
    v = y[:, :n * tp].reshape(S, n, tp, C)
    acc = np.zeros((S, n, C), F4)
    for i in range(tp):
        acc = (acc + v[:, :, i]).astype(F4)
    return (acc * (F4(1.0) / F4(tp))).astype(F4)


def _conv_u(sd, xi, taps, f, scale=False):
    """SiLU(conv4(xi) + b) with the 3 carried frames ``taps`` [S, 3, E] (None: zeros) in arithmetic ``f`` (F4 / F8).
    -> (u, new taps), or with ``scale`` (u, sum_k |w_k xi_k| + |b|): the magnitude the fp32 error of u is proportional to."""
    wc, bc = np.asarray(sd[P_MAMBA + ".conv1d.weight"], f)[:, 0, :], np.asarray(sd[P_MAMBA + ".conv1d.bias"], f)
    S, T, _ = xi.shape
    prev = np.zeros((S, KC - 1, E), f) if taps is None else np.asarray(taps, f)
    xp = np.concatenate([prev, np.asarray(xi, f)], axis=1)
    u = np.zeros((S, T, E), f) + bc
    for k in range(KC):
        u += xp[:, k:k + T] * wc[:, k]
    act = O.silu(u) if f is F4 else R8.silu(u)
    if scale:
        return act, np.abs(bc) + sum(np.abs(xp[:, k:k + T] * wc[:, k]) for k in range(KC))
    return act, xp[:, xp.shape[1] - (KC - 1):].copy()


def scan64(sd, xz, dbl, state=None):
    """The float64 selective scan driven by stored xz [S, T, 384] and dbl [S, T, >= 38]: -> (y gated [S, T, E], ssm
    state [S, E, N]).  state = (taps [S, 3, E], ssm [S, E, N]) or None."""
    f8 = lambda k: np.asarray(sd[P_MAMBA + "." + k], dtype=F8)   # noqa: E731
    xz, dbl = np.asarray(xz, F8), np.asarray(dbl, F8)
    S, T, _ = xz.shape
    u, _ = _conv_u(sd, xz[..., :E], None if state is None else state[0], F8)
    z = xz[..., E:]
    dt = R8.softplus(dbl[..., :RK] @ f8("dt_proj.weight").T + f8("dt_proj.bias"))
    Bm, Cm = dbl[..., RK:RK + NST], dbl[..., RK + NST:RK + 2 * NST]
    A = -np.exp(f8("A_log"))
    h = np.zeros((S, E, NST)) if state is None else np.asarray(state[1], F8).copy()
    y = np.empty((S, T, E))
    dtu = dt * u
    for t in range(T):
        h = np.exp(dt[:, t, :, None] * A) * h + dtu[:, t, :, None] * Bm[:, t, None, :]
        y[:, t] = np.matmul(h, Cm[:, t, :, None])[..., 0]
    return (y + f8("D") * u) * R8.silu(z), h


def oracle_mamba(sd, x, state=None, time_pool=1, residual=True, rnd=RNE):
    """ipdnet2_oracle.mamba's float32 arithmetic, cut into the device's phases, with the rounding hooks and the device's
    order at the pooled out_proj (pool, then round).  x [S, T, 96] -> dict(xz, dbl, y, out, taps, ssm): what the device
    leaves in its workspace, its output and its state."""
    f4 = lambda k: np.asarray(sd[P_MAMBA + "." + k], dtype=F4)   # noqa: E731
    x = np.asarray(x, dtype=F4)
    S, T, _ = x.shape
    ln = O.layer_norm(x, sd[P_NORM + ".weight"], sd[P_NORM + ".bias"])
    xz = _mm(rnd.qa(ln), rnd.w("in_proj", f4("in_proj.weight")))
    u, taps = _conv_u(sd, xz[..., :E], None if state is None else state[0], F4)
    dbl = _mm(rnd.qa(u), rnd.w("x_proj", f4("x_proj.weight")))
    dt = O.softplus(_mm(dbl[..., :RK], f4("dt_proj.weight")) + f4("dt_proj.bias"))
    Bm, Cm = dbl[..., RK:RK + NST], dbl[..., RK + NST:]
    A = -np.exp(f4("A_log"))
    h = np.zeros((S, E, NST), F4) if state is None else np.asarray(state[1], F4).copy()
    y = np.zeros((S, T, E), F4)
    for t in range(T):
        dA = np.exp(dt[:, t, :, None] * A[None])
        h = (dA * h + (dt[:, t, :, None] * Bm[:, t, None, :]) * u[:, t, :, None]).astype(F4)
        y[:, t] = (h * Cm[:, t, None, :]).sum(-1, dtype=F4) + f4("D") * u[:, t]
    y = (y * O.silu(xz[..., E:])).astype(F4)
    out = _mm(rnd.qa(pool32(y, time_pool)), rnd.w("out_proj", f4("out_proj.weight")))
    if residual:
        out = (out + pool32(x, time_pool)).astype(F4)
    dblp = np.zeros((S, T, XP), F4)
    dblp[..., :RK + 2 * NST] = dbl
    return dict(xz=xz, dbl=dblp, y=y, out=out, taps=taps, ssm=h)


def mamba_refs(sd, rec, eps, fused, key=""):
    """The four comparisons of one fnssl_sn_mamba call.  rec: x [S, T, 96] fp32 (the sampled sequences), seqs (their
    numbers in the call), nt, state_in (taps, ssm) or None, time_pool, residual, and what the device stored: xz, dbl, y.
    eps = (eps of the LN output, eps of SiLU(conv + b) relative to sum |w_k xi_k| + |b| of its element: most of u is far
    below 1, where an absolute eps sized for the largest elements would put a midpoint next to every small one).  fused: the call ran sn_mamba_convx_mfma_kernel (tiles of 13
    frames of one sequence; tile position = frame % 13 + 3), else conv + xproj (position = point % 16)."""
    f4 = lambda k: np.asarray(sd[P_MAMBA + "." + k], dtype=F4)   # noqa: E731
    x, xz, dbl, ydev = rec["x"], rec["xz"], rec["dbl"], rec["y"]
    S, T, _ = x.shape
    tp = rec.get("time_pool", 1)
    pt = (np.asarray(rec["seqs"], np.int64)[:, None] * T + np.arange(T)[None, :])[..., None]
    ln, lsc = ln_scaled(x, sd[P_NORM + ".weight"], sd[P_NORM + ".bias"])
    y1, b1 = product(f4("in_proj.weight"), ln, eps[0] * lsc)
    st = rec.get("state_in")
    u, uscale = _conv_u(sd, np.asarray(xz, F4)[..., :E], None if st is None else st[0], F8, scale=True)
    y2, b2 = product(f4("x_proj.weight"), u, eps[1] * uscale)
    pos2 = (np.arange(T) % 13 + 3)[None, :, None] if fused else pt % 16
    y3, ssm = scan64(sd, xz, dbl, st)
    y4, b4 = product(f4("out_proj.weight"), pool32(ydev, tp))
    if rec.get("residual", True):
        n = T // tp
        y4 = y4 + np.asarray(x, F8)[:, :n * tp].reshape(S, n, tp, H).mean(2)
    pt4 = (np.asarray(rec["seqs"], np.int64)[:, None] * (T // tp) + np.arange(T // tp)[None, :])[..., None]
    return [Cmp(key + "in_proj", y1, b1, pt % 16, "abs"), Cmp(key + "x_proj", y2, b2, pos2, "abs"),
            Cmp(key + "scan", y3, None, None, "rms"), Cmp(key + "scan_ssm", ssm, None, None, "rms"),
            Cmp(key + "out_proj", y4, b4, pt4 % 16, "abs")]


def mamba_got(stored):
    return [stored["xz"], stored["dbl"][..., :RK + 2 * NST], stored["y"], stored["ssm"], stored["out"]]


# ------------------------------------------------------------------------------------------------------------------ #
# fconv  (sn_fconv_mfma_kernel<POOL, true>): flip bound from the LN output, through PReLU, residual and the F-pooling
# ------------------------------------------------------------------------------------------------------------------ #
FCONV_P = "layers.0.fconv1"
PLANT = 1e30


def fconv_state_dict(seed, planted=False):
    """planted: the LayerNorm bias of the first four channels of every group is 1e30 and the conv weights of those
    input channels are zero, so the true product ignores them; the kernel's padding lanes (k = 60..63 of a group's
    64-wide patch) read exactly these four values of the row two bins down against weights that must be zero."""
    from fnssl import weights as W
    sd = collections.OrderedDict(W.make_ipdnet2_state(seed, num_layers=1))
    w = tie_w(sd[FCONV_P + ".1.weight"], 3)
    if planted:
        w[:, :4, :] = 0.0
        b = sd[FCONV_P + ".0.bias"].copy()
        b.reshape(8, 12)[:, :4] = PLANT
        sd[FCONV_P + ".0.bias"] = b
    sd[FCONV_P + ".1.weight"] = w
    return sd


def fconv_ref(sd, x, pool, eps, residual=True, key="fconv"):
    p = FCONV_P
    x = np.asarray(x, dtype=F4)
    B, F, T, _ = x.shape
    ln, lsc = ln_scaled(x, sd[p + ".0.weight"], sd[p + ".0.bias"])
    w, b = np.asarray(sd[p + ".1.weight"], F4), np.asarray(sd[p + ".1.bias"], F8)
    lnp = np.pad(ln, ((0, 0), (2, 2), (0, 0), (0, 0)))
    epp = np.pad(eps * lsc, ((0, 0), (2, 2), (0, 0), (0, 0)))
    live = np.pad(np.ones((1, F, 1, 1)), ((0, 0), (2, 2), (0, 0), (0, 0)))        # the padding rows are exact zeros
    y, bd = np.empty((B, F, T, H)), np.empty((B, F, T, H))
    for g in range(8):
        patch = np.concatenate([lnp[:, k:k + F, :, 12 * g:12 * g + 12] for k in range(5)], axis=-1)     # k = tap * 12 + ci
        lv = np.concatenate([np.broadcast_to(live[:, k:k + F], (B, F, T, 12)) for k in range(5)], axis=-1)
        ep = np.concatenate([epp[:, k:k + F, :, 12 * g:12 * g + 12] for k in range(5)], axis=-1)
        wg = w[12 * g:12 * g + 12].transpose(0, 2, 1).reshape(12, 60)
        wq = bf16_rne(wg)
        y[..., 12 * g:12 * g + 12] = q(patch) @ wq.T
        ok = np.abs(patch) < 1e29                                    # the planted 1e30 meet zero weights: no flip counts
        fl = np.where(ok, flip(np.where(ok, patch, 0.0), np.where(ok, ep, 0.0)), 0.0) * lv
        bd[..., 12 * g:12 * g + 12] = fl @ np.abs(wq).T
    y = y + b
    slope = np.asarray(sd[p + ".2.weight"], F8)
    y = np.where(y >= 0, y, slope * y)
    bd = bd * np.maximum(1.0, np.abs(slope))
    if residual:
        y = y + np.asarray(x, F8)
    if pool > 1:
        y, bd = R8.avgpool_f(y, pool), R8.avgpool_f(bd, pool)
    pos = ((np.arange(F // pool) * pool) % 16).reshape(1, -1, 1, 1)
    return Cmp(key, y, bd, pos, "abs")


def oracle_fconv(sd, x, pool, residual=True, rnd=RNE):
    """ipdnet2_oracle.fconv's float32 arithmetic with the rounding hooks (+ residual and F-pooling)."""
    p = FCONV_P
    x = np.asarray(x, dtype=F4)
    B, F, T, _ = x.shape
    ln = O.layer_norm(x, sd[p + ".0.weight"], sd[p + ".0.bias"])
    w = np.asarray(sd[p + ".1.weight"], F4)
    lnp = rnd.qa(np.pad(ln, ((0, 0), (2, 2), (0, 0), (0, 0))))
    y = np.zeros((B, F, T, H), F4)
    for g in range(8):
        wg = rnd.w("fconv", w[12 * g:12 * g + 12].transpose(0, 2, 1).reshape(12, 60)).reshape(12, 5, 12)
        for k in range(5):
            y[..., 12 * g:12 * g + 12] += _mm(lnp[:, k:k + F, :, 12 * g:12 * g + 12], wg[:, k, :])
    y = (y + np.asarray(sd[p + ".1.bias"], F4)).astype(F4)
    y = np.where(y >= 0, y, np.asarray(sd[p + ".2.weight"], F4) * y).astype(F4)
    if residual:
        y = (x + y).astype(F4)
    return O.avgpool_f(y, pool) if pool > 1 else y


# ------------------------------------------------------------------------------------------------------------------ #
# full  (sn_full_mfma_kernel<NF, true>): three chained products; isolating weights so that each stage meets generic
# weights once while the other two pass their operand on exactly
# ------------------------------------------------------------------------------------------------------------------ #
FULL_P = "layers.0."
SQ_CH = (5, 17, 29, 41, 53, 65, 77, 95)          # one-hot squeeze: squeezed channel c = LN channel SQ_CH[c]


def full_state_dict(seed, nf, probe):
    """probe 'S': squeeze generic | Linear over F identity, bias 0 | unsqueeze one-hot 1.0, bias 0
             'F': squeeze one-hot, bias 0 | Linear over F generic | unsqueeze one-hot, bias 0
             'U': squeeze one-hot, bias 0 | identity, bias 0 | unsqueeze generic (K = 8: the zero half of its 32-wide k-step)
             'G': all three generic (exempt from the tight-share condition).
    Generic tensors carry the tie scheme; identity / one-hot tensors are exact by construction and carry none."""
    from fnssl import weights as W
    sd = collections.OrderedDict((k, v) for k, v in W.make_ipdnet2_state(seed, num_layers=1, num_freqs=2 * nf).items()
                                 if k.startswith(FULL_P))
    p = FULL_P
    onehot_s = np.zeros((HS, H, 1), F4)
    onehot_s[np.arange(HS), SQ_CH, 0] = 1.0
    onehot_u = np.zeros((H, HS, 1), F4)
    onehot_u[np.arange(H), np.arange(H) % HS, 0] = 1.0
    if probe in ("S", "G"):
        sd[p + "squeeze.0.weight"] = tie_w(sd[p + "squeeze.0.weight"], 1)
    else:
        sd[p + "squeeze.0.weight"], sd[p + "squeeze.0.bias"] = onehot_s, np.zeros(HS, F4)
    if probe in ("F", "G"):
        sd[p + "full.weight"] = tie_w(sd[p + "full.weight"], 2)
    else:
        sd[p + "full.weight"], sd[p + "full.bias"] = np.eye(nf, dtype=F4), np.zeros(nf, F4)
    if probe in ("U", "G"):
        sd[p + "unsqueeze.0.weight"] = tie_w(sd[p + "unsqueeze.0.weight"], 3)
    else:
        sd[p + "unsqueeze.0.weight"], sd[p + "unsqueeze.0.bias"] = onehot_u, np.zeros(H, F4)
    return sd


def full_ref(sd, x, eps, residual=True, key="full", parts=False):
    """eps = (LN output, SiLU(squeeze + b), Linear-over-F output): the fp32 error of forming each from exact operands;
    the chain adds L * (bound of the stage before)."""
    p = FULL_P
    x = np.asarray(x, dtype=F4)
    B, F, T, _ = x.shape
    w = lambda n: np.asarray(sd[p + n], F4)      # noqa: E731
    ln, lsc = ln_scaled(x, w("norm_full.weight"), w("norm_full.bias"))
    y1, b1 = product(w("squeeze.0.weight")[:, :, 0], ln, eps[0] * lsc)
    a2 = R8.silu(y1 + w("squeeze.0.bias").astype(F8))                       # [B, F, T, 8]
    e2 = eps[1] + SILU_LIP * b1
    y2, b2 = product(w("full.weight"), a2.transpose(0, 2, 3, 1), e2.transpose(0, 2, 3, 1))     # over F: [B, T, 8, G]
    a3 = y2.transpose(0, 3, 1, 2) + w("full.bias").astype(F8)[None, :, None, None]
    e3 = eps[2] + b2.transpose(0, 3, 1, 2)
    y3, b3 = product(w("unsqueeze.0.weight")[:, :, 0], a3, e3)
    out = R8.silu(y3 + w("unsqueeze.0.bias").astype(F8))
    if residual:
        out = out + np.asarray(x, F8)
    c = Cmp(key, out, SILU_LIP * b3, (np.arange(F) % 16).reshape(1, -1, 1, 1), "abs")
    return (c, a2, b1, a3, b2.transpose(0, 3, 1, 2)) if parts else c


def oracle_full(sd, x, residual=True, rnd=RNE, parts=False):
    """ipdnet2_oracle.full's float32 arithmetic with the rounding hooks."""
    p = FULL_P
    x = np.asarray(x, dtype=F4)
    w = lambda n: np.asarray(sd[p + n], F4)      # noqa: E731
    ln = O.layer_norm(x, w("norm_full.weight"), w("norm_full.bias"))
    s = O.silu(np.einsum("bfth,qh->bftq", rnd.qa(ln), rnd.w("squeeze", w("squeeze.0.weight")[:, :, 0])).astype(F4) +
               w("squeeze.0.bias"))
    wf = rnd.w("over_f", w("full.weight"))
    s2 = (np.einsum("bftq,gf->bgtq", rnd.qa(s), wf).astype(F4) + w("full.bias")[None, :, None, None]).astype(F4)
    out = O.silu(np.einsum("bftq,hq->bfth", rnd.qa(s2), rnd.w("unsqueeze", w("unsqueeze.0.weight")[:, :, 0])).astype(F4) +
                 w("unsqueeze.0.bias"))
    if residual:
        out = (x + out).astype(F4)
    return (out, s, s2) if parts else out


# ------------------------------------------------------------------------------------------------------------------ #
# the legs
# ------------------------------------------------------------------------------------------------------------------ #
# Persistent grids (csrc/spatialnet.hip): encoder cus * 2 workgroups * 8 waves * 16 points per pass; in_proj cus * 16
# waves * 16 points; conv + x_proj cus * 4 * 8 tiles of 13 frames; carried x_proj cus * 4 * 8 * 16 points; out_proj cus *
# 2 * 8 * 16 outputs; fconv / full min(blocks, cus) workgroups of 256 / nf frames.
def sizes(cus):
    nseq = cus * 16 + 4                      # 16 frames each: in_proj, out_proj (cus * 256 points a pass) and the fused
    return {"enc_nt": cus * 16 + 1,          # conv + x_proj (2 tiles a sequence: > cus * 32 tiles) all start a second pass
            "wide_nseq": nseq, "wide_nt": 16,
            "carry_nt": cus * 512 // nseq + 1,                   # carried x_proj kernel past one pass
            "f16_nt": 16 * cus + 5}                              # fconv / full at 16 bins: cus blocks + a partial one


def wide_sample(cus, nt, per_pass):
    """Sequences a multi-pass Mamba leg checks: the first 32, the 16 either side of every pass boundary of a grid that
    takes ``per_pass`` points, the last 32 (x_proj has 38 outputs a point: fewer sequences leave under 10 000 tight)."""
    nseq = sizes(cus)["wide_nseq"]
    s = set(range(32)) | set(range(nseq - 32, nseq))
    for pp in per_pass:
        k = pp
        while k < nseq * nt:
            s |= set(range(max(0, k // nt - 16), min(nseq, k // nt + 17)))
            k += pp
    return sorted(s)


ENC_SEED, MAMBA_SEED, FCONV_SEED, FULL_SEED = 5100, 5200, 5300, 5400
ENC_CINS = (10, 16, 17, 30, 32)              # K = 50 (of 80), 80 (exact), 85 (of 160), 150 (of 160), 160
ENC_CHUNKS = (9, 1, 13)
# name -> (nb, nf, nt, time_pool, chunks or None)
MAMBA_LEGS = collections.OrderedDict([
    ("m_small", (3, 16, 35, 1, None)),                 # 35 = 2 * 13 + 9: a ragged third conv + x_proj tile
    ("m_short", (6, 16, 9, 3, None)),                  # nt < 13; pool 3: the run-time trip count
    ("m_pool5", (17, 16, 250, 5, None)),               # 250 = 19 * 13 + 3
    ("m_carry", (3, 16, 35, 1, (4, 1, 30))),           # conv + xproj kernels, carried taps and state
])
# name -> (nb, nf, nt, pool, planted): 5 frames an utterance; 4 utterances so that the pooled legs keep 10 000 tight
FCONV_LEGS = collections.OrderedDict([
    ("fc256p2", (4, 256, 5, 2, False)), ("fc128p8", (4, 128, 5, 8, False)), ("fc16", (4, 16, 5, 1, False)),
    ("fc32", (4, 32, 5, 1, False)), ("fc16_ragged", (1, 16, 37, 1, False)), ("fc16_planted", (1, 16, 37, 1, True)),
])
FULL_NT = {16: 37, 64: 9, 128: 5}            # 16 / 4 / 2 frames per workgroup: a partial last workgroup each


@functools.lru_cache(maxsize=None)
def enc_case(cin, nb, nf, nt):
    return encoder_inputs(ENC_SEED + cin, cin, nb, nf, nt)


@functools.lru_cache(maxsize=None)
def mamba_case(name, cus=MI355X_CUS):
    """(sd, x [S, T, 96] fp32 (every sequence of the call), the sequences the leg checks, (nb, nf, nt, pool, chunks))."""
    sd = mamba_state_dict(MAMBA_SEED)
    if name in MAMBA_LEGS:
        nb, nf, nt, tp, chunks = MAMBA_LEGS[name]
        x = fp32_block(MAMBA_SEED + 10 + len(name) + nt, (nb * nf, nt, H), 1.0)
        # the 272 x 250 leg RUNS at its full size and COMPARES three of its 17 utterances (first, middle, last: 48 sequences,
        # among them 262, where in_proj's second grid pass starts on 256 CUs); sequences are independent
        seqs = [s for b in (0, 8, 16) for s in range(16 * b, 16 * b + 16)] if name == "m_pool5" else list(range(nb * nf))
        return sd, x, seqs, (nb, nf, nt, tp, chunks)
    z = sizes(cus)
    nseq = z["wide_nseq"]
    if name == "m_wide":
        nt, pp, chunks = z["wide_nt"], (cus * 256,), None
    else:                                                                  # m_wide_carry
        nt, pp, chunks = z["carry_nt"], (cus * 512, cus * 256), (z["carry_nt"],)
    x = fp32_block(MAMBA_SEED + 30 + nt, (nseq, nt, H), 1.0)
    return sd, x, wide_sample(cus, nt, pp), (1, nseq, nt, 1, chunks)


def wide_carry_state(nseq):
    """The carried state both sides of m_wide_carry start from."""
    rs = np.random.RandomState(MAMBA_SEED + 77)
    return (rs.standard_normal((nseq, 3, E)).astype(F4), (rs.standard_normal((nseq, E, NST)) * 0.3).astype(F4))


def oracle_mamba_leg(name, rnd=RNE, cus=MI355X_CUS):
    """The oracle standing in for the device: the records (one per call) of a leg, on the leg's sampled sequences."""
    sd, x, seqs, (nb, nf, nt, tp, chunks) = mamba_case(name, cus)
    xs = x[seqs]
    recs, st, t0 = [], None, 0
    if name == "m_wide_carry":
        full_st = wide_carry_state(nb * nf)
        st = (full_st[0][seqs], full_st[1][seqs])
    for n in (chunks or (nt,)):
        xc = np.ascontiguousarray(xs[:, t0:t0 + n])
        o = oracle_mamba(sd, xc, st, tp, True, rnd)
        recs.append(dict(o, x=xc, seqs=seqs, state_in=st, time_pool=tp, residual=True))
        st = (o["taps"], o["ssm"]) if chunks else None
        t0 += n
    return recs


@functools.lru_cache(maxsize=None)
def fconv_case(name, cus=MI355X_CUS):
    if name == "fc16_multi":
        nb, nf, nt, pool, planted = 1, 16, sizes(cus)["f16_nt"], 1, False
    else:
        nb, nf, nt, pool, planted = FCONV_LEGS[name]
    return fconv_state_dict(FCONV_SEED, planted), fp32_block(FCONV_SEED + nf + nt, (nb, nf, nt, H), 1.0), pool


@functools.lru_cache(maxsize=None)
def full_case(nf, probe, cus=MI355X_CUS, multi=False):
    nt = sizes(cus)["f16_nt"] if multi else FULL_NT[nf]
    return full_state_dict(FULL_SEED + nf, nf, probe), fp32_block(FULL_SEED + nf + nt + ord(probe), (1, nf, nt, H), 1.0)


# ------------------------------------------------------------------------------------------------------------------ #
# the gates
# ------------------------------------------------------------------------------------------------------------------ #
# ORACLE[key]: the float32 oracle's measured distance (max abs; "scan" keys: max / rms) from this reference on the leg's own
# inputs at 256 CUs (``measure``); "eps_ln" / "eps_u": of the LN output / SiLU(conv + b) in units of their error scales
# (ln_scaled, _conv_u), "eps_s" / "eps_f": of SiLU(squeeze + b) / the Linear over F's output where no operand before them
# can flip (absolute; 0: the isolating weights make the stage exact).  The kernels get MARGIN x each figure.  The host test
# re-measures every figure and fails when one is more than 2 x off.
ORACLE = {
    "enc10": 1.76e-07, "enc16": 2.24e-07, "enc17": 2.09e-07, "enc30": 3.90e-07, "enc32": 3.24e-07,
    "enc10_nt3": 8.94e-08, "enc30_carry": 3.90e-07, "enc10_carry": 1.76e-07, "enc10_multi": 2.31e-07,
    "m_small.eps_ln": 1.05e-07, "m_small.eps_u": 1.81e-07, "m_small.in_proj": 4.47e-07, "m_small.x_proj": 6.80e-08,
    "m_small.scan": 3.57e-06, "m_small.scan_ssm": 6.64e-06, "m_small.out_proj": 2.38e-07, "m_short.eps_ln": 1.17e-07,
    "m_short.eps_u": 1.65e-07, "m_short.in_proj": 3.28e-07, "m_short.x_proj": 2.79e-08, "m_short.scan": 3.02e-06,
    "m_short.scan_ssm": 8.65e-06, "m_short.out_proj": 3.25e-07, "m_pool5.eps_ln": 1.23e-07, "m_pool5.eps_u": 1.94e-07,
    "m_pool5.in_proj": 5.07e-07, "m_pool5.x_proj": 1.04e-07, "m_pool5.scan": 8.54e-06, "m_pool5.scan_ssm": 9.32e-06,
    "m_pool5.out_proj": 2.44e-07, "m_carry.eps_ln": 1.05e-07, "m_carry.eps_u": 1.81e-07, "m_carry.in_proj": 4.47e-07,
    "m_carry.x_proj": 2.98e-08, "m_carry.scan": 3.60e-06, "m_carry.scan_ssm": 7.70e-06, "m_carry.out_proj": 2.38e-07,
    "m_wide.eps_ln": 1.09e-07, "m_wide.eps_u": 1.76e-07, "m_wide.in_proj": 3.76e-07, "m_wide.x_proj": 3.32e-08,
    "m_wide.scan": 3.87e-06, "m_wide.scan_ssm": 6.17e-06, "m_wide.out_proj": 2.20e-07,
    "m_wide_carry.eps_ln": 1.14e-07, "m_wide_carry.eps_u": 1.68e-07, "m_wide_carry.in_proj": 4.66e-07,
    "m_wide_carry.x_proj": 1.08e-07, "m_wide_carry.scan": 5.50e-06, "m_wide_carry.scan_ssm": 6.09e-06,
    "m_wide_carry.out_proj": 2.30e-07, "fc256p2.eps_ln": 1.28e-07, "fc256p2": 2.46e-07, "fc128p8.eps_ln": 1.05e-07,
    "fc128p8": 1.56e-07, "fc16.eps_ln": 9.19e-08, "fc16": 3.20e-07, "fc32.eps_ln": 1.15e-07, "fc32": 3.02e-07,
    "fc16_ragged.eps_ln": 1.13e-07, "fc16_ragged": 2.76e-07, "fc16_planted.eps_ln": 1.02e-07,
    "fc16_planted": 2.91e-07, "fc16_multi.eps_ln": 1.13e-07, "fc16_multi": 2.83e-07, "full16S.eps_ln": 1.01e-07,
    "full16S.eps_s": 2.92e-07, "full16S.eps_f": 0.00e+00, "full16S": 2.29e-07, "full16F.eps_ln": 1.09e-07,
    "full16F.eps_s": 2.45e-07, "full16F.eps_f": 8.57e-08, "full16F": 1.49e-07, "full16U.eps_ln": 9.85e-08,
    "full16U.eps_s": 2.34e-07, "full16U.eps_f": 0.00e+00, "full16U": 2.00e-07, "full64S.eps_ln": 9.15e-08,
    "full64S.eps_s": 1.86e-07, "full64S.eps_f": 0.00e+00, "full64S": 2.09e-07, "full64F.eps_ln": 1.14e-07,
    "full64F.eps_s": 2.30e-07, "full64F.eps_f": 1.08e-07, "full64F": 1.93e-07, "full64U.eps_ln": 1.07e-07,
    "full64U.eps_s": 2.45e-07, "full64U.eps_f": 0.00e+00, "full64U": 2.20e-07, "full128S.eps_ln": 1.03e-07,
    "full128S.eps_s": 1.75e-07, "full128S.eps_f": 0.00e+00, "full128S": 2.20e-07, "full128F.eps_ln": 9.64e-08,
    "full128F.eps_s": 2.45e-07, "full128F.eps_f": 2.24e-07, "full128F": 2.01e-07, "full128U.eps_ln": 1.09e-07,
    "full128U.eps_s": 2.45e-07, "full128U.eps_f": 0.00e+00, "full128U": 2.67e-07, "full16G.eps_ln": 9.83e-08,
    "full16G.eps_s": 2.35e-07, "full16G.eps_f": 3.73e-08, "full16G": 1.26e-07, "full16S_multi.eps_ln": 1.06e-07,
    "full16S_multi.eps_s": 2.40e-07, "full16S_multi.eps_f": 0.00e+00, "full16S_multi": 2.33e-07,
}


def delta(key):
    return MARGIN * ORACLE[key]


def measure(c, got, key):
    """The oracle's distance for one comparison, over the elements no flip can reach (bound = 0).  These are all but a
    handful of the tight ones; a tight element with 0 < bound <= delta may hold a flip of the oracle's own, which is
    not fp32 arithmetic error and would feed the gate back into itself."""
    got = np.asarray(got, dtype=F8)
    if c.rule == "rms":
        return R8.rms_rel_err(got, c.ref)
    return float(np.abs(got - c.ref)[c.bound == 0].max())


# ------------------------------------------------------------------------------------------------------------------ #
# one driver for the host test (stored = the oracle's arrays) and the GPU test (stored = the device's)
# ------------------------------------------------------------------------------------------------------------------ #
# name -> (cin, nb, nf, nt, chunks); nt None: sizes(cus)["enc_nt"]
ENC_LEGS = collections.OrderedDict(
    [("enc%d" % c, (c, 2, 16, 23, None)) for c in ENC_CINS] +
    [("enc10_nt3", (10, 3, 16, 3, None)),                       # the non-pipelined kernel without carried frames
     ("enc30_carry", (30, 2, 16, 23, ENC_CHUNKS)), ("enc10_carry", (10, 2, 16, 23, ENC_CHUNKS)),
     ("enc10_multi", (10, 1, 16, None, None))])
MAMBA_ALL = list(MAMBA_LEGS) + ["m_wide", "m_wide_carry"]
FCONV_ALL = list(FCONV_LEGS) + ["fc16_multi"]
FULL_ALL = [(nf, p, False) for nf in (16, 64, 128) for p in "SFU"] + [(16, "G", False), (16, "S", True)]


def full_name(nf, probe, multi):
    return "full%d%s%s" % (nf, probe, "_multi" if multi else "")


def enc_spec(name, cus=MI355X_CUS):
    cin, nb, nf, nt, chunks = ENC_LEGS[name]
    return cin, nb, nf, nt or sizes(cus)["enc_nt"], chunks


def oracle_enc_leg(name, rnd=RNE, cus=MI355X_CUS):
    cin, nb, nf, nt, chunks = enc_spec(name, cus)
    x, w, b = enc_case(cin, nb, nf, nt)
    out, st, t0 = [], None, 0
    for n in (chunks or (nt,)):
        o, st = oracle_encoder(x[..., t0:t0 + n], w, b, st if chunks else None, rnd)
        out.append((o, st))
        t0 += n
    return out


def enc_cmps(name, stored, cus=MI355X_CUS):
    """stored: [(out, state_out)] per call.  The carried frames are the previous call's stored state (asserted to be the
    input's last four frames, bit for bit)."""
    cin, nb, nf, nt, chunks = enc_spec(name, cus)
    x, w, b = enc_case(cin, nb, nf, nt)
    res, st, t0 = [], None, 0
    for i, n in enumerate(chunks or (nt,)):
        res.append((name, encoder_ref(x[..., t0:t0 + n], w, b, st, "%s[%d]" % (name, i)), stored[i][0]))
        t0 += n
        if chunks:
            st = np.asarray(stored[i][1], F4)
            want = np.concatenate([np.zeros((nb, cin, nf, 4), F4), x[..., :t0]], axis=-1)[..., -4:]
            assert np.array_equal(st, want), "%s: carried frames after call %d are not the input's last four" % (name, i)
    return res


def mamba_eps(name, table=None):
    t = ORACLE if table is None else table
    return MARGIN * t[name + ".eps_ln"], MARGIN * t[name + ".eps_u"]


def mamba_cmps(name, recs, cus=MI355X_CUS, table=None):
    sd = mamba_case(name, cus)[0]
    res = []
    for i, r in enumerate(recs):
        for c, got in zip(mamba_refs(sd, r, mamba_eps(name, table), r["state_in"] is None or not r.get("carry", True),
                                     "%s[%d]." % (name, i)), mamba_got(r)):
            res.append(("%s.%s" % (name, c.key.split(".")[-1]), c, got))
    return res


def mamba_measure_eps(name, recs, cus=MI355X_CUS):
    sd = mamba_case(name, cus)[0]
    e_ln = e_u = 0.0
    for r in recs:
        e_ln = max(e_ln, ln_distance(r["x"], sd[P_NORM + ".weight"], sd[P_NORM + ".bias"]))
        st = r["state_in"]
        taps = None if st is None else st[0]
        u8, sc = _conv_u(sd, r["xz"][..., :E], taps, F8, scale=True)
        e_u = max(e_u, float((np.abs(_conv_u(sd, r["xz"][..., :E], taps, F4)[0] - u8) / sc).max()))
    return {name + ".eps_ln": e_ln, name + ".eps_u": e_u}


def multi_frames(cus):
    """Frames a multi-pass fconv / full leg (16 bins, 16 frames a workgroup, ``cus`` workgroups a pass) checks: the first
    two workgroups, the last two of the first pass and the second pass (one partial workgroup of 5 frames).  Frames are
    independent, so the device runs them all and the reference only these."""
    nt = sizes(cus)["f16_nt"]
    return np.asarray(sorted(set(range(32)) | set(range(16 * cus - 32, nt))))


def leg_frames(name, cus=MI355X_CUS):
    multi = name[2] if isinstance(name, tuple) else name == "fc16_multi"
    return multi_frames(cus) if multi else None


def fconv_cmps(name, stored, cus=MI355X_CUS, table=None):
    sd, x, pool = fconv_case(name, cus)
    if leg_frames(name, cus) is not None:
        x = x[:, :, leg_frames(name, cus)]
    eps = MARGIN * (ORACLE if table is None else table)[name + ".eps_ln"]
    return [(name, fconv_ref(sd, x, pool, eps, key=name), stored)]


def fconv_measure_eps(name, cus=MI355X_CUS):
    sd, x, _ = fconv_case(name, cus)
    if leg_frames(name, cus) is not None:
        x = x[:, :, leg_frames(name, cus)]
    return {name + ".eps_ln": ln_distance(x, sd[FCONV_P + ".0.weight"], sd[FCONV_P + ".0.bias"])}


def full_eps(name, table=None):
    t = ORACLE if table is None else table
    return tuple(MARGIN * t[name + k] for k in (".eps_ln", ".eps_s", ".eps_f"))


def full_cmps(nf, probe, multi, stored, cus=MI355X_CUS, table=None):
    name = full_name(nf, probe, multi)
    sd, x = full_case(nf, probe, cus, multi)
    if multi:
        x = x[:, :, multi_frames(cus)]
    return [(name, full_ref(sd, x, full_eps(name, table), key=name), stored)]


def full_measure_eps(nf, probe, multi, cus=MI355X_CUS):
    """In dependency order: the LN output; SiLU(squeeze + b) where no operand of the squeeze can flip; the Linear over F's
    output where none of its operands can (each uses the figures measured before it)."""
    name = full_name(nf, probe, multi)
    sd, x = full_case(nf, probe, cus, multi)
    if multi:
        x = x[:, :, multi_frames(cus)]
    _, s, s2 = oracle_full(sd, x, parts=True)
    w = lambda n: np.asarray(sd[FULL_P + n], F4)      # noqa: E731
    e_ln = ln_distance(x, w("norm_full.weight"), w("norm_full.bias"))
    _, a2, b1, _, _ = full_ref(sd, x, (MARGIN * e_ln, 0.0, 0.0), parts=True)
    e_s = float(np.abs(s - a2)[b1 == 0].max())
    _, _, _, a3, b2 = full_ref(sd, x, (MARGIN * e_ln, MARGIN * e_s, 0.0), parts=True)
    return {name + ".eps_ln": e_ln, name + ".eps_s": e_s, name + ".eps_f": float(np.abs(s2 - a3)[b2 == 0].max())}


@functools.lru_cache(maxsize=None)
def oracle_stored(name, rnd=RNE, cus=MI355X_CUS):
    """The oracle's arrays for leg ``name`` in the form its *_cmps takes (name: a string, or a FULL_ALL tuple)."""
    fr = leg_frames(name, cus)
    if isinstance(name, tuple):
        sd, x = full_case(name[0], name[1], cus, name[2])
        return oracle_full(sd, x if fr is None else x[:, :, fr], rnd=rnd)
    if name in ENC_LEGS:
        return oracle_enc_leg(name, rnd, cus)
    if name in MAMBA_ALL:
        return oracle_mamba_leg(name, rnd, cus)
    sd, x, pool = fconv_case(name, cus)
    return oracle_fconv(sd, x if fr is None else x[:, :, fr], pool, rnd=rnd)


def cmps(name, stored, cus=MI355X_CUS, table=None):
    """[(gate key, Cmp, got)] of a leg.  ``table``: where the eps figures are read (None: the committed ORACLE)."""
    if isinstance(name, tuple):
        return full_cmps(name[0], name[1], name[2], stored, cus, table)
    if name in ENC_LEGS:
        return enc_cmps(name, stored, cus)
    if name in MAMBA_ALL:
        return mamba_cmps(name, stored, cus, table)
    return fconv_cmps(name, stored, cus, table)


def measure_eps(name, stored, cus=MI355X_CUS):
    if isinstance(name, tuple):
        return full_measure_eps(name[0], name[1], name[2], cus)
    if name in MAMBA_ALL:
        return mamba_measure_eps(name, stored, cus)
    if name in ENC_LEGS:
        return {}
    return fconv_measure_eps(name, cus)


ALL_LEGS = list(ENC_LEGS) + MAMBA_ALL + FCONV_ALL + FULL_ALL


def is_exempt(name):
    """The generic-weights full leg asserts only delta + bound (a three-product chain leaves ~0.3 % tight)."""
    return isinstance(name, tuple) and name[1] == "G"


def measure_leg(name, cus=MI355X_CUS):
    """Every figure of a leg's rows in ORACLE, measured: the eps first, then the distances with the bounds formed from
    the eps just measured (passed on explicitly: ORACLE is not touched), each the maximum over the leg's calls."""
    stored = oracle_stored(name, RNE, cus)
    out = measure_eps(name, stored, cus)
    for key, c, got in cmps(name, stored, cus, table=out):
        out[key] = max(out.get(key, 0.0), measure(c, got, key))
    return out


def check_leg(name, stored, cus=MI355X_CUS, report=print):
    """The leg's condition on the reference (before anything is compared), then every comparison.  -> {key: stats}."""
    todo = cmps(name, stored, cus)
    res = {}
    if not is_exempt(name):
        for key in sorted({k for k, c, _ in todo if c.rule == "abs"}):
            share, n = leg_condition([c for k, c, _ in todo if k == key], delta(key), key)
            res[key + " tight"] = (share, n)
    for key, c, got in todo:
        res[c.key] = check(c, got, delta(key), report)
    return res
