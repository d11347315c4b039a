"""Autograd restatement of the f-conv branch, the full-band branch and a whole IPDnet2 SpatialNetLayer for the training
tests.  TEST INFRASTRUCTURE ONLY.

torch on the CPU, float64 (the reference) or float32 (the yardstick), written from the branches' definitions:

    f-conv   pool_F(residual x + PReLU(bias + Conv1d_{k5, 8 groups, zero 'same'}(LN(x)))) along F
    full     residual x + SiLU(Wu v + bu),  v[f] = sum_f2 Wf[f, f2] s[f2] + bf[f],  s = SiLU(Ws LN(x) + bs)
    layer    fconv1 (F pooled by 2 in the first layer), full, fconv2 (pooled by 8), two LN + Mamba blocks
             (mamba_train_ref.forward), each with its residual; the second block pools T by ``time_pool``

It calls nothing of the library under test and nothing of ``oracle/``; test_layer_train_ref_host.py pins its float64 forward
to ipdnet2_f64_ref and its float64 gradients to finite differences.

The gate of test_gpu_layer_train.py: per gradient tensor, err = max|got - f64| / max|f64|, held to GATE = 8 x the float32
restatement's own err on the same inputs, taken per tensor as the LARGEST over all legs of the
group (f-conv, full, layer).  GATE_F32 below holds those float32 figures as measured on the host; the host test
re-measures them.  None is chosen from what the kernels give.

THE PReLU KINK.  A pre-activation a within rounding of zero makes float32, float64 and the kernel take different branches,
and one flipped element moves dx by ~3e-2 of its maximum.  ``leg_inputs`` therefore evaluates a in float64 and re-draws,
until min|a| >= A_MARGIN, the rows that feed a small a (branch legs) or the whole frame (layer legs: fconv1, full and
fconv2 are all frame-local).  This is a condition on the inputs; every element of every tensor is still compared.

``mutant``: a deliberately wrong backward (the forward's values are unchanged, bit for bit), to show that the gates see the
mistakes these backwards can make.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import mamba_train_ref as MR

H, HS, NG, CG, KF = 96, 8, 8, 12, 5
TC = MR.TC
GATE = 8.0
A_MARGIN = 1e-4          # min |a| of every leg; the float32 restatement's max|a32 - a64| is 4.9e-7 (host test: <= 1e-6)
A_ROUNDS = 50

FCONV_PARAMS = ("0.weight", "0.bias", "1.weight", "1.bias", "2.weight")
FULL_PARAMS = ("norm_full.weight", "norm_full.bias", "squeeze.0.weight", "squeeze.0.bias", "full.weight", "full.bias",
               "unsqueeze.0.weight", "unsqueeze.0.bias")
LAYER_PARAMS = (tuple("fconv1." + n for n in FCONV_PARAMS) + FULL_PARAMS + tuple("fconv2." + n for n in FCONV_PARAMS) +
                ("norm_mhsa.weight", "norm_mhsa.bias") + tuple("mhsa." + n for n in MR.PARAMS) +
                ("norm_tconvffn.weight", "norm_tconvffn.bias") + tuple("tconvffn." + n for n in MR.PARAMS))
TENSORS = {"fconv": ("x",) + FCONV_PARAMS, "full": ("x",) + FULL_PARAMS, "layer": ("x",) + LAYER_PARAMS}
GROUPS = ("fconv", "full", "layer")

MUTANTS = {"fconv": ("tap_flip", "prelu_neg", "pool_scale", "ln_xhat_term", "residual_drop"),
           "full": ("wf_not_transposed", "silu_sigma", "dbf_unsummed"),
           "layer": ()}


# ------------------------------------------------------------------------------------------------------------------ #
# legs
# ------------------------------------------------------------------------------------------------------------------ #
def legs(group: str):
    """The leg table of a group.  f-conv / full: (name, nb, nf, nt, pool, residual, layout, special); layer: (name, nb,
    nf, nt, is_first, time_pool, layout, None).  layout: 'frame' = frame-major storage ([B, T, F, H] in memory, the
    library's native layout), 'plain' = a contiguous [B, F, T, H] tensor.  special: None, 'point_lo' / 'point_hi' (dout
    zero except one point at f = 0 / f = nf - 1), 'mean100' (x rows of mean 100)."""
    out = []
    if group == "fconv":
        for res in (True, False):
            sfx = "res" if res else "branch"
            out.append(("f8_1frame_" + sfx, 1, 8, 1, 1, res, "plain" if res else "frame", None))   # both paddings in one window
            out.append(("f16_6frames_" + sfx, 2, 16, 3, 1, res, "frame" if res else "plain", None))   # ragged last block
        out.append(("f32_pool2", 1, 32, 5, 2, True, "plain", None))
        out.append(("f128_pool8", 2, 128, 3, 8, True, "frame", None))
        out.append(("f256_pool2", 1, 256, 2, 2, True, "plain", None))                     # one frame = one 256-point block
        out.append(("f16_17frames", 1, 16, 17, 1, True, "frame", None))                   # frames no multiple of 256 / nf
        out.append(("f256_300blocks", 3, 256, 100, 2, True, "frame", None))               # more blocks than CUs
        out.append(("f16_real", 2, 16, 250, 1, True, "frame", None))                      # layers 1-7 at real length
        out.append(("f16_point_lo", 1, 16, 3, 1, True, "frame", "point_lo"))
        out.append(("f16_point_hi", 1, 16, 3, 1, True, "frame", "point_hi"))
    elif group == "full":
        for i, nf in enumerate((8, 16, 32, 64, 128, 256)):
            for res in (True, False):
                out.append(("f%d_%s" % (nf, "res" if res else "branch"), 2, nf, 3, 1, res,
                            "frame" if (i + res) % 2 else "plain", None))
        out.append(("f16_17frames", 1, 16, 17, 1, True, "frame", None))
        out.append(("f16_real", 2, 16, 250, 1, True, "frame", None))
        out.append(("f128_300frames", 2, 128, 150, 1, True, "frame", None))               # the dWf reduction crosses workgroups
        out.append(("f16_mean100", 2, 16, 3, 1, True, "plain", "mean100"))                # LayerNorm cancellation
    elif group == "layer":
        out.append(("later_layer", 2, 16, TC + 3, False, 1, "frame", None))
        out.append(("first_layer", 1, 64, 6, True, 1, "plain", None))                     # full at 32, fconv2 32 -> 4 bins
        out.append(("later_layer_tpool5", 2, 16, 12, False, 5, "frame", None))            # dx of frames 10, 11 exactly 0
    else:
        raise KeyError(group)
    return out


def leg_seed(group: str, name: str) -> int:
    return MR.leg_seed(group + ":" + name)


def full_weight(nf: int):
    """full.weight [nf, nf] and full.bias [nf] for any nf: U(+-1/sqrt(nf)) like nn.Linear's default, seeded by nf (a
    state dict holds them for its own num_freqs only)."""
    rs = np.random.RandomState(7000 + nf)
    b = nf ** -0.5
    return rs.uniform(-b, b, (nf, nf)).astype(np.float32), rs.uniform(-b, b, (nf,)).astype(np.float32)


def leg_params(group: str, leg, sd):
    """The parameters of a leg as float32 arrays under TENSORS[group]'s names, out of an IPDnet2 state dict with at least
    two layers (fnssl.weights.make_ipdnet2_state(0, num_layers=2)): f-conv legs use layers.0.fconv1, full legs layers.0's
    norm_full / squeeze / unsqueeze with full_weight(nf), layer legs layers.0 (first) or layers.1 with full_weight."""
    f4 = lambda k: np.array(sd[k], np.float32)   # noqa: E731
    if group == "fconv":
        return {n: f4("layers.0.fconv1." + n) for n in FCONV_PARAMS}
    if group == "full":
        p = {n: f4("layers.0." + n) for n in FULL_PARAMS}
        p["full.weight"], p["full.bias"] = full_weight(leg[2])
        return p
    pre = "layers.0." if leg[4] else "layers.1."
    p = {n: f4(pre + n) for n in LAYER_PARAMS}
    p["full.weight"], p["full.bias"] = full_weight(leg[2] // 2 if leg[4] else leg[2])
    return p


# ------------------------------------------------------------------------------------------------------------------ #
# the restatements
# ------------------------------------------------------------------------------------------------------------------ #
class _ScaleGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        ctx.k = k
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.k, None


def _same_value(value, wrong):
    """``value``'s bits with ``wrong``'s gradient: value + (wrong - wrong) adds an exact zero."""
    return value.detach() + (wrong - wrong.detach())


def layer_norm(x, w, b, mutant=None):
    """nn.LayerNorm over the last axis, spelled out so that the mutant can cut rstd's dependence on x (which is where the
    x^ mean(dl x^) term of the backward comes from) without touching a value."""
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    if mutant == "ln_xhat_term":
        rstd = rstd.detach()
    return xc * rstd * w + b


def silu(z, mutant=None):
    if mutant == "silu_sigma":                               # SiLU' = sigma (1 + z (1 - sigma)) replaced by sigma
        return _same_value(F.silu(z), z * torch.sigmoid(z).detach())
    return F.silu(z)


def fconv_pre(p, x, mutant=None, pre=""):
    """The PReLU's input a [B, F, T, H] = bias + grouped conv along F of LN(x)."""
    B, Fq, T, _ = x.shape
    ln = layer_norm(x, p[pre + "0.weight"], p[pre + "0.bias"], mutant)
    z = ln.permute(0, 2, 3, 1).reshape(B * T, H, Fq)
    w, b = p[pre + "1.weight"], p[pre + "1.bias"]
    if mutant == "tap_flip":                                 # d ln through the conv with the taps NOT flipped
        a = F.conv1d(z.detach(), w, b, padding=KF // 2, groups=NG)
        wrong = F.conv1d(z, w.detach().flip(-1), None, padding=KF // 2, groups=NG)
        a = a + (wrong - wrong.detach())
    else:
        a = F.conv1d(z, w, b, padding=KF // 2, groups=NG)
    return a.reshape(B, T, H, Fq).permute(0, 3, 1, 2)


def fconv_forward(p, x, residual=True, pool=1, mutant=None, pre=""):
    """p: dict of torch tensors under FCONV_PARAMS' names (behind ``pre``); x [B, F, T, H]."""
    B, Fq, T, _ = x.shape
    a = fconv_pre(p, x, mutant, pre)
    slope = p[pre + "2.weight"]
    act = torch.where(a >= 0, a, slope * a)
    if mutant == "prelu_neg":                                # the negative branch differentiated as 1 (d slope kept)
        act = _same_value(act, a + slope * torch.where(a >= 0, torch.zeros_like(a), a).detach())
    out = act
    if residual:
        out = (x.detach() if mutant == "residual_drop" else x) + act
    if pool > 1:
        if mutant == "pool_scale":                           # the spread without its 1 / pool
            out = _ScaleGrad.apply(out, float(pool))
        out = out.reshape(B, Fq // pool, pool, T, H).mean(2)
    return out


def full_forward(p, x, residual=True, mutant=None):
    """p: dict of torch tensors under FULL_PARAMS' names; x [B, F, T, H]."""
    ln = layer_norm(x, p["norm_full.weight"], p["norm_full.bias"])
    s = silu(ln @ p["squeeze.0.weight"][:, :, 0].T + p["squeeze.0.bias"], mutant)          # [B, F, T, 8]
    wf, bf = p["full.weight"], p["full.bias"]
    if mutant == "wf_not_transposed":                        # ds formed with Wf instead of Wf^T
        v = torch.einsum("gf,bftq->bgtq", wf, s.detach())
        wrong = torch.einsum("fg,bftq->bgtq", wf.detach(), s)
        v = v + (wrong - wrong.detach())
    else:
        v = torch.einsum("gf,bftq->bgtq", wf, s)
    if mutant == "dbf_unsummed":                             # d bf from squeeze channel 0 alone
        v = v + bf.detach()[None, :, None, None]
        pad = torch.zeros_like(v)
        pad[..., 0] = 1.0
        v = v + (bf - bf.detach())[None, :, None, None] * pad
    else:
        v = v + bf[None, :, None, None]
    u = silu(v @ p["unsqueeze.0.weight"][:, :, 0].T + p["unsqueeze.0.bias"], mutant)
    return x + u if residual else u


def _mamba_params(p, norm, mamba):
    out = {"norm.weight": p[norm + ".weight"], "norm.bias": p[norm + ".bias"]}
    out.update({n: p[mamba + "." + n] for n in MR.PARAMS})
    return out


def layer_forward(p, x, is_first=False, time_pool=1):
    """p: dict of torch tensors under LAYER_PARAMS' names; x [B, F, T, H] -> [B, F', T // time_pool, H]."""
    y = fconv_forward(p, x, True, 2 if is_first else 1, pre="fconv1.")
    y = full_forward(p, y, True)
    y = fconv_forward(p, y, True, 8 if is_first else 1, pre="fconv2.")
    y = MR.forward(_mamba_params(p, "norm_mhsa", "mhsa"), y, True, 1)
    return MR.forward(_mamba_params(p, "norm_tconvffn", "tconvffn"), y, True, time_pool)


def leg_forward(group, leg, p, x, mutant=None):
    if group == "fconv":
        return fconv_forward(p, x, leg[5], leg[4], mutant)
    if group == "full":
        return full_forward(p, x, leg[5], mutant)
    assert mutant is None
    return layer_forward(p, x, leg[4], leg[5])


class _one_thread:
    """ONE torch thread while the restatement runs: the float32 figures are dominated by the sums over all points, and
    torch splits those by its thread count (mamba_train_ref.gradients).  Pinned, the table is the same on every host."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


def _tensors(p_np, dtype, grad):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=grad) for k, v in p_np.items()}


def pre_activations(group, leg, p_np, x_np, dtype=torch.float64):
    """Every PReLU input of the leg ([a] for an f-conv leg, [a of fconv1, a of fconv2] for a layer leg, [] for full), as
    numpy float64 arrays [B, F, T, H]."""
    if group == "full":
        return []
    with _one_thread(), torch.no_grad():
        p, x = _tensors(p_np, dtype, False), torch.tensor(np.asarray(x_np), dtype=dtype)
        if group == "fconv":
            out = [fconv_pre(p, x)]
        else:
            first = leg[4]
            y = full_forward(p, fconv_forward(p, x, True, 2 if first else 1, pre="fconv1."), True)
            out = [fconv_pre(p, x, pre="fconv1."), fconv_pre(p, y, pre="fconv2.")]
    return [a.numpy().astype(np.float64) for a in out]


def leg_inputs(group, leg, p_np):
    """(x [B, F, T, H], dout) of a leg: float32 arrays, the same on the host and on the device, with no PReLU input
    within A_MARGIN of zero (module docstring)."""
    name, nb, nf, nt = leg[:4]
    rs = np.random.RandomState(leg_seed(group, name))
    x = rs.standard_normal((nb, nf, nt, H)).astype(np.float32)
    if leg[7] == "mean100":
        x += np.float32(100.0)
    if group == "layer":
        oshape = (nb, nf // 16 if leg[4] else nf, nt // leg[5], H)
    else:
        oshape = (nb, nf // leg[4], nt, H)
    dout = rs.standard_normal(oshape).astype(np.float32)
    if leg[7] in ("point_lo", "point_hi"):
        keep = np.zeros_like(dout)
        f = 0 if leg[7] == "point_lo" else nf - 1
        keep[0, f, 1] = dout[0, f, 1]
        dout = keep
    for _ in range(A_ROUNDS):
        small = [np.abs(a).min(-1) < A_MARGIN for a in pre_activations(group, leg, p_np, x)]      # [B, F', T] each
        if not any(s.any() for s in small):
            return x, dout
        if group == "layer":                                 # the whole frame: every branch before the Mambas is frame-local
            bad = np.zeros((nb, nt), bool)
            for s in small:
                bad |= s.any(1)
            idx = np.argwhere(bad)
            for b, t in idx:
                x[b, :, t] = rs.standard_normal((nf, H)).astype(np.float32)
        else:                                                # the rows the 5 taps reach
            for b, f, t in np.argwhere(small[0]):
                lo, hi = max(0, f - KF // 2), min(nf, f + KF // 2 + 1)
                x[b, lo:hi, t] = rs.standard_normal((hi - lo, H)).astype(np.float32)
    raise AssertionError("%s/%s: PReLU inputs within %g of zero after %d rounds" % (group, name, A_MARGIN, A_ROUNDS))


def gradients(group, leg, p_np, x_np, dout_np, dtype=torch.float64, mutant=None):
    """(out, {tensor name: gradient}) as numpy float64 arrays; the cotangent of out is dout."""
    with _one_thread():
        p = _tensors(p_np, dtype, True)
        x = torch.tensor(np.asarray(x_np), dtype=dtype, requires_grad=True)
        out = leg_forward(group, leg, p, x, mutant)
        (out * torch.tensor(np.asarray(dout_np), dtype=dtype)).sum().backward()
    g = {"x": x.grad}
    g.update({k: v.grad for k, v in p.items()})
    return out.detach().numpy().astype(np.float64), {k: v.detach().numpy().astype(np.float64) for k, v in g.items()}


rel_err = MR.rel_err


def leg_errors(group, leg, sd, dtype=torch.float32, mutant=None):
    """{tensor: rel_err of the ``dtype`` restatement's gradient against float64} for one leg."""
    p = leg_params(group, leg, sd)
    x, dout = leg_inputs(group, leg, p)
    _, want = gradients(group, leg, p, x, dout, torch.float64)
    _, got = gradients(group, leg, p, x, dout, dtype, mutant)
    return {k: rel_err(got[k], want[k]) for k in TENSORS[group]}


def measure_gate_table(group, sd):
    """Per tensor, the largest float32-vs-float64 rel_err over all legs of the group (what GATE_F32 commits)."""
    worst = {k: 0.0 for k in TENSORS[group]}
    for leg in legs(group):
        for k, v in leg_errors(group, leg, sd).items():
            worst[k] = max(worst[k], v)
    return worst


def gate(group: str, name: str) -> float:
    return GATE * GATE_F32[group][name]


# measure_gate_table(group, make_ipdnet2_state(0, num_layers=2)) on the host (torch CPU on one thread, float32 against float64)
GATE_F32 = {
    "fconv": {
        "x": 1.76e-07,
        "0.weight": 7.75e-07,
        "0.bias": 5.70e-07,
        "1.weight": 8.23e-07,
        "1.bias": 7.71e-07,
        "2.weight": 5.31e-07,
    },
    "full": {
        "x": 4.34e-07,
        "norm_full.weight": 6.09e-06,
        "norm_full.bias": 1.65e-06,
        "squeeze.0.weight": 7.04e-06,
        "squeeze.0.bias": 2.22e-06,
        "full.weight": 6.91e-06,
        "full.bias": 9.09e-07,
        "unsqueeze.0.weight": 6.48e-06,
        "unsqueeze.0.bias": 5.53e-07,
    },
    "layer": {
        "x": 1.73e-07,
        "fconv1.0.weight": 2.15e-07,
        "fconv1.0.bias": 1.75e-07,
        "fconv1.1.weight": 1.74e-07,
        "fconv1.1.bias": 2.11e-07,
        "fconv1.2.weight": 2.32e-07,
        "norm_full.weight": 3.32e-07,
        "norm_full.bias": 3.19e-07,
        "squeeze.0.weight": 6.65e-07,
        "squeeze.0.bias": 3.52e-07,
        "full.weight": 4.78e-07,
        "full.bias": 6.54e-07,
        "unsqueeze.0.weight": 5.90e-07,
        "unsqueeze.0.bias": 1.91e-07,
        "fconv2.0.weight": 2.11e-07,
        "fconv2.0.bias": 1.60e-07,
        "fconv2.1.weight": 2.65e-07,
        "fconv2.1.bias": 2.38e-07,
        "fconv2.2.weight": 1.81e-07,
        "norm_mhsa.weight": 8.63e-07,
        "norm_mhsa.bias": 6.69e-07,
        "mhsa.in_proj.weight": 6.28e-07,
        "mhsa.conv1d.weight": 5.07e-07,
        "mhsa.conv1d.bias": 4.98e-07,
        "mhsa.x_proj.weight": 7.70e-07,
        "mhsa.dt_proj.weight": 1.33e-06,
        "mhsa.dt_proj.bias": 7.70e-07,
        "mhsa.A_log": 1.00e-06,
        "mhsa.D": 4.57e-07,
        "mhsa.out_proj.weight": 5.81e-07,
        "norm_tconvffn.weight": 5.29e-07,
        "norm_tconvffn.bias": 7.63e-07,
        "tconvffn.in_proj.weight": 9.35e-07,
        "tconvffn.conv1d.weight": 4.17e-07,
        "tconvffn.conv1d.bias": 3.89e-07,
        "tconvffn.x_proj.weight": 9.56e-07,
        "tconvffn.dt_proj.weight": 9.33e-07,
        "tconvffn.dt_proj.bias": 6.73e-07,
        "tconvffn.A_log": 6.54e-07,
        "tconvffn.D": 4.86e-07,
        "tconvffn.out_proj.weight": 7.80e-07,
    },
}
