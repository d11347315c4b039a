"""Autograd restatement of the IPDnet2 encoder, head, whole network and PIT-MSE training step for the training tests.
TEST INFRASTRUCTURE ONLY.

torch on the CPU, float64 (the reference) or float32 (the yardstick), written from the operators' definitions:

    encoder  y[b,f,t,o] = bias[o] + sum_{c,k} W[o,c,k] x[b,c,f,t-4+k], zero for negative time (F.conv1d on a left-padded signal)
    head     u_r[o] = b[o*16+r] + sum_h W[o*16+r, h] x[p][h];  v_r = tanh(u_r);  d_r = bd + Wd v_r;
             out[b, t, 2 (16 fc + r) + gg, m, a] = d_r[a*8 + gg*4 + m]
    net      encoder, L layers (layer_train_ref.layer_forward; time pooled by 5 after layer 0), head
    step     PIT-MSE of the prediction, cut to the targets' frames, against the targets (two tracks)

It imports layer_train_ref and mamba_train_ref and calls nothing of the library under test and nothing of ``oracle/``;
test_net_train_ref_host.py pins its float64 forward to ipdnet2_f64_ref and the float64 gradients of the encoder and the
head to finite differences.

The gate of test_gpu_net_train.py: per gradient tensor, err = max|got - f64| / max|f64|, held to GATE = 8 x the float32
restatement's own err on the same inputs, taken per tensor as the LARGEST over all legs of the
group (encoder, head, net).  GATE_F32 below holds those float32 figures as measured on the host on one torch thread; the
host test re-measures them.  None is chosen from what the kernels give.

THE PReLU KINK (layer_train_ref).  No PReLU input of a net leg may lie within A_MARGIN of zero.  A plain draw of the
smallest network leaves ~5 such elements per frame and whole-input re-draws cannot converge; the network is causal in time, so
``net_input`` draws the input ONE FRAME AT A TIME, in order: frame t is re-drawn until every layer-0 pre-activation of
frame t clears the margin and, for t = 4 (mod 5), every later layer's pre-activation of pooled frame (t + 1) / 5 - 1 does
(evaluated in float64 on the prefix <= t).  A frame of 2 x 128 or 1 x 256 bins holds ~37 000 layer-0 pre-activations, ~5 of
them inside the margin, so a whole-frame re-draw clears it with probability e^-5; from the second draw on only the bins
of frame t within two taps of an offending element are drawn again (the f-conv reaches 2 bins, the encoder none; the
full-band branch moves everything a little, so every draw is checked whole).  At most MAX_DRAWS draws per frame.

``mutant``: a deliberately wrong backward (the forward's values are unchanged, bit for bit).
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import layer_train_ref as LR
import mamba_train_ref as MR

H, KE, DO, NR, RATIO = 96, 5, 16, 16, 5
GATE = 8.0
A_MARGIN = LR.A_MARGIN
MAX_DRAWS = 200
PERM_GAP = 1e-3

GROUPS = ("encoder", "head", "net")
HEAD_PARAMS = ("freq_inverse.trans2.weight", "freq_inverse.trans2.bias", "decoder.weight", "decoder.bias")
MUTANTS = {"encoder": ("dx_taps_not_flipped", "dw_k_reversed"),
           "head": ("one_minus_v", "gather_a_gg_swapped", "decoder_not_transposed"),
           "net": ("time_pool_no_fifth",)}

rel_err = MR.rel_err
_one_thread = LR._one_thread


# ------------------------------------------------------------------------------------------------------------------ #
# legs
# ------------------------------------------------------------------------------------------------------------------ #
def legs(group: str):
    """encoder: (name, nb, cin, nf, nt, x layout, dout layout, special, x requires grad); x layout 'plain' = contiguous
    [B, C, F, T], 'tstride' = stored [B, C, T, F] (time stride nf); dout layout 'frame' / 'plain' as in layer_train_ref;
    special: None, 'point_t0' / 'point_tlast' (dout zero except one (b, f) point at t = 0 / nt - 1).
    head: (name, nb, nfc, nt2, x layout, special); special: None, 'element_last' (dout zero except the element
    (t2, 2f + gg, m, a) = (last, last, 3, 1)), 'saturated'.
    net: (name, num_layers, num_freqs, dim_input, nb, nt, kind); kind 'dout' (a random cotangent) or 'step' (the cotangent
    of the PIT-MSE loss against targets one pooled frame shorter than the prediction)."""
    if group == "encoder":
        return [("one_frame", 1, 4, 8, 1, "plain", "frame", None, True),          # every tap but the last is padding
                ("nt3", 1, 4, 8, 3, "plain", "plain", None, True),                # nt < 4
                ("cin10_kp80", 2, 10, 16, 7, "plain", "plain", None, True),       # the shipped cin
                ("cin30_kp160", 1, 30, 16, 6, "plain", "frame", None, False),     # 15 microphones
                ("cin34_plain", 1, 34, 8, 5, "plain", "frame", None, True),       # 170 > 160: the plain path
                ("cin10_tstride", 1, 10, 16, 17, "tstride", "frame", None, True),
                ("many_tiles", 3, 10, 256, 100, "plain", "frame", None, False),   # more tiles than workgroups
                ("ragged", 1, 10, 3, 5, "plain", "plain", None, True),            # 15 points
                ("point_t0", 1, 10, 8, 6, "plain", "frame", "point_t0", True),
                ("point_tlast", 1, 10, 8, 6, "plain", "frame", "point_tlast", True)]
    if group == "head":
        return [("one_point", 1, 1, 1, "frame", None),
                ("fc16", 2, 16, 3, "plain", None),                                # the shipped compressed width
                ("ragged40", 1, 8, 5, "frame", None),
                ("many", 3, 16, 60, "frame", None),                               # the reduction crosses workgroups
                ("element_last", 1, 2, 2, "plain", "element_last"),
                ("saturated", 1, 4, 3, "frame", "saturated")]
    if group == "net":
        return [("l2_f128_nt10", 2, 128, 4, 2, 10, "dout"),
                ("l2_f128_nt12", 2, 128, 4, 2, 12, "dout"),                       # frames 10, 11 reach no pooled frame
                ("l3_f256_nt5", 3, 256, 10, 1, 5, "dout"),
                ("step", 2, 128, 4, 2, 10, "step")]
    raise KeyError(group)


def leg_seed(group: str, name: str) -> int:
    return MR.leg_seed("net_train:" + group + ":" + name)


def net_cfg(leg):
    """The keyword arguments of fnssl.weights.make_ipdnet2_state / ipdnet2_param_shapes for a net leg."""
    return {"num_layers": leg[1], "num_freqs": leg[2], "dim_input": leg[3]}


def net_param_names(num_layers: int):
    out = ["encoder.weight", "encoder.bias"]
    for l in range(num_layers):
        out += ["layers.%d.%s" % (l, n) for n in LR.LAYER_PARAMS]
    return tuple(out) + HEAD_PARAMS


def tensors(group: str, leg):
    """The gradient tensors a leg compares."""
    if group == "encoder":
        return ("weight", "bias") + (("x",) if leg[8] else ())
    if group == "head":
        return ("x",) + HEAD_PARAMS
    return net_param_names(leg[1])


def _uniform(rs, bound, shape):
    return rs.uniform(-bound, bound, shape).astype(np.float32)


def leg_params(group: str, leg, sd=None):
    """The parameters of a leg as float32 arrays.  encoder: U(+-1/sqrt(5 cin)) like nn.Conv1d's default, seeded by cin;
    head: the same ranges as fnssl.weights gives them, seeded here; net: the leg's state dict ``sd``
    (make_ipdnet2_state(0, **net_cfg(leg)))."""
    if group == "encoder":
        cin = leg[2]
        rs = np.random.RandomState(7100 + cin)
        b = (cin * KE) ** -0.5
        return {"weight": _uniform(rs, b, (H, cin, KE)), "bias": _uniform(rs, b, (H,))}
    if group == "head":
        rs = np.random.RandomState(7200)
        return {"freq_inverse.trans2.weight": _uniform(rs, H ** -0.5, (NR * DO, H, 1)),
                "freq_inverse.trans2.bias": _uniform(rs, 0.1, (NR * DO,)),
                "decoder.weight": _uniform(rs, 0.25, (DO, DO)), "decoder.bias": _uniform(rs, 0.1, (DO,))}
    return {n: np.array(sd[n], np.float32) for n in net_param_names(leg[1])}


# ------------------------------------------------------------------------------------------------------------------ #
# the restatements
# ------------------------------------------------------------------------------------------------------------------ #
def _conv(xs, w, b):
    return F.conv1d(F.pad(xs, (KE - 1, 0)), w, b)


def encoder_forward(w, b, x, mutant=None):
    """x [B, C, F, T] -> [B, F, T, 96]."""
    B, C, Fq, T = x.shape
    xs = x.permute(0, 2, 1, 3).reshape(B * Fq, C, T)
    if mutant == "dx_taps_not_flipped":                      # dx through the conv with the taps NOT flipped (dW, db kept)
        y = _conv(xs.detach(), w, b)
        wrong = _conv(xs, w.detach().flip(-1), None)
        y = y + (wrong - wrong.detach())
    elif mutant == "dw_k_reversed":                          # dW with k running the wrong way (dx, db kept)
        y = _conv(xs, w.detach(), b)
        wrong = _conv(xs.detach(), w.flip(-1), None)
        y = y + (wrong - wrong.detach())
    else:
        y = _conv(xs, w, b)
    return y.reshape(B, Fq, H, T).permute(0, 1, 3, 2)


class _TanhOneMinusV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u):
        v = torch.tanh(u)
        ctx.save_for_backward(v)
        return v

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return g * (1.0 - v)


def head_forward(p, x, mutant=None):
    """p: dict of torch tensors under HEAD_PARAMS' names; x [B, Fc, T, 96] -> [B, T, 2 * 16 Fc, 4, 2]."""
    B, Fc, T, _ = x.shape
    w, b = p["freq_inverse.trans2.weight"][:, :, 0], p["freq_inverse.trans2.bias"]
    wd, bd = p["decoder.weight"], p["decoder.bias"]
    u = (x @ w.T + b).reshape(B, Fc, T, DO, NR)                               # output index o * 16 + r
    u = u.permute(0, 1, 4, 2, 3).reshape(B, Fc * NR, T, DO)                   # fine bin f = 16 fc + r: u_r[o]
    v = _TanhOneMinusV.apply(u) if mutant == "one_minus_v" else torch.tanh(u)
    if mutant == "decoder_not_transposed":                   # dv formed with Wd instead of Wd^T
        d = v.detach() @ wd.T + bd
        wrong = v @ wd.detach()
        d = d + (wrong - wrong.detach())
    else:
        d = v @ wd.T + bd                                                     # d_r[j], j = a*8 + gg*4 + m
    d6 = d.reshape(B, Fc * NR, T, 2, 2, DO // 4)                              # [.., a, gg, m]
    out = d6.permute(0, 2, 1, 4, 5, 3)                                        # [b, t, f, gg, m, a]
    if mutant == "gather_a_gg_swapped":                      # the gather reads (a, gg) where (gg, a) is stored
        wrong = d6.permute(0, 2, 1, 3, 5, 4)
        out = out.detach() + (wrong - wrong.detach())
    return out.reshape(B, T, 2 * Fc * NR, DO // 4, 2)


def _layer_params(p, l):
    return {n: p["layers.%d.%s" % (l, n)] for n in LR.LAYER_PARAMS}


def time_pool(y, ratio=RATIO, mutant=None):
    B, Fq, T, _ = y.shape
    if mutant == "time_pool_no_fifth":                       # the spread without its 1 / 5
        y = LR._ScaleGrad.apply(y, float(ratio))
    return y[:, :, :T // ratio * ratio].reshape(B, Fq, T // ratio, ratio, H).mean(3)


def net_forward(p, x, num_layers, mutant=None, pre=None):
    """p: dict of torch tensors under the state dict's names; x [B, C, F, T] -> [B, T // 5, 2F, 4, 2].  ``pre``: a list that
    receives every PReLU input (fconv1's and fconv2's of every layer, [B, F', T', 96])."""
    y = encoder_forward(p["encoder.weight"], p["encoder.bias"], x)
    for l in range(num_layers):
        pl = _layer_params(p, l)
        if pre is not None:
            first = l == 0
            y1 = LR.full_forward(pl, LR.fconv_forward(pl, y, True, 2 if first else 1, pre="fconv1."), True)
            pre += [LR.fconv_pre(pl, y, pre="fconv1."), LR.fconv_pre(pl, y1, pre="fconv2.")]
        y = LR.layer_forward(pl, y, l == 0, 1)
        if l == 0:
            y = time_pool(y, RATIO, mutant)
    return head_forward(p, y)


def pit_mse(pred, gt):
    """pred, gt [nb, nt, 2F, nm1, 2]: per frame the better of the two track permutations (ties: the identity); the mean of
    the squared differences.  Returns (loss, per frame the two permutation errors [nb * nt, 2])."""
    nb, nt = pred.shape[:2]
    pr, g = pred.reshape(nb * nt, -1, 2), gt.reshape(nb * nt, -1, 2)
    e_id = ((pr - g) ** 2).sum((1, 2))
    e_sw = ((pr.flip(-1) - g) ** 2).sum((1, 2))
    e = torch.stack([e_id, e_sw], 1)
    best = torch.where(e_sw.detach() < e_id.detach(), e_sw, e_id)
    return best.sum() / pred.numel(), e


# ------------------------------------------------------------------------------------------------------------------ #
# inputs
# ------------------------------------------------------------------------------------------------------------------ #
def _t(p_np, dtype, grad=False):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=grad) for k, v in p_np.items()}


def net_input(leg, p_np, rs):
    """x [nb, dim_input, nf, nt] float32, drawn frame by frame (module docstring).  Returns (x, the most draws a frame took)."""
    _, nl, nf, cin, nb, nt, _ = leg
    p = _t(p_np, torch.float64)
    pl0 = _layer_params(p, 0)
    x = np.zeros((nb, cin, nf, nt), np.float32)
    worst = 0
    def reach(mask, bad, span):
        """mask [nb, nf] |= the input bins within two taps of a bad element; bad [nb, F'] at a resolution of ``span`` bins"""
        for b, f in np.argwhere(bad):
            mask[b, max(0, (f - 2) * span):(f + 3) * span] = True

    with _one_thread(), torch.no_grad():
        for t in range(nt):
            mask = np.ones((nb, nf), bool)                                    # the first draw: the whole frame
            for draw in range(1, MAX_DRAWS + 1):
                fresh = rs.standard_normal((nb, cin, nf)).astype(np.float32)
                x[:, :, :, t] = np.where(mask[:, None, :], fresh, x[:, :, :, t])
                mask[:] = False
                lo = max(0, t - (KE - 1))
                xe = np.zeros((nb, cin, nf, KE), np.float64)                  # frames t-4 .. t, zero before time 0
                xe[:, :, :, KE - (t + 1 - lo):] = x[:, :, :, lo:t + 1]
                y = encoder_forward(p["encoder.weight"], p["encoder.bias"], torch.tensor(xe))[:, :, KE - 1:]
                y1 = LR.full_forward(pl0, LR.fconv_forward(pl0, y, True, 2, pre="fconv1."), True)
                a1, a2 = LR.fconv_pre(pl0, y, pre="fconv1."), LR.fconv_pre(pl0, y1, pre="fconv2.")
                reach(mask, (a1.abs().amin(-1)[:, :, 0] < A_MARGIN).numpy(), 1)
                reach(mask, (a2.abs().amin(-1)[:, :, 0] < A_MARGIN).numpy(), 2)
                if not mask.any() and t % RATIO == RATIO - 1 and nl > 1:      # the later layers' pooled frame (t + 1) / 5 - 1
                    pre = []
                    net_forward(p, torch.tensor(x[:, :, :, :t + 1].astype(np.float64)), nl, pre=pre)
                    j = (t + 1) // RATIO - 1
                    for v in pre[2:]:
                        reach(mask, (v[:, :, j].abs().amin(-1) < A_MARGIN).numpy(), 16)
                if not mask.any():
                    break
            else:
                raise AssertionError("%s: frame %d has a PReLU input within %g of zero after %d draws" % (leg[0], t, A_MARGIN, MAX_DRAWS))
            worst = max(worst, draw)
    return x, worst


@functools.lru_cache(maxsize=None)
def _cached_inputs(group, name, sd_key):
    leg = [l for l in legs(group) if l[0] == name][0]
    rs = np.random.RandomState(leg_seed(group, name))
    p = leg_params(group, leg, _SD[sd_key] if sd_key is not None else None)
    if group == "encoder":
        _, nb, cin, nf, nt = leg[:5]
        x = rs.standard_normal((nb, cin, nf, nt)).astype(np.float32)
        dout = rs.standard_normal((nb, nf, nt, H)).astype(np.float32)
        if leg[7] in ("point_t0", "point_tlast"):
            keep = np.zeros_like(dout)
            t = 0 if leg[7] == "point_t0" else nt - 1
            keep[0, 3, t] = dout[0, 3, t]
            dout = keep
        return p, x, dout
    if group == "head":
        _, nb, nfc, nt2 = leg[:4]
        x = rs.standard_normal((nb, nfc, nt2, H)).astype(np.float32)
        dout = rs.standard_normal((nb, nt2, 2 * NR * nfc, DO // 4, 2)).astype(np.float32)
        if leg[5] == "element_last":
            keep = np.zeros_like(dout)
            keep[0, -1, -1, 3, 1] = dout[0, -1, -1, 3, 1]
            dout = keep
        if leg[5] == "saturated":
            # per point p: x scaled so that max|u| is 20 (p = 0 mod 3), max|u| is 100 (1 mod 3), or MIN|u| is 20 (2 mod 3:
            # every one of the point's 256 tanh saturates in float32, where e^2u >= 2^25)
            w = p["freq_inverse.trans2.weight"][:, :, 0].astype(np.float64)
            xf = x.reshape(-1, H).astype(np.float64)
            for i in range(xf.shape[0]):
                for _ in range(60):                                            # the bias shifts u: a few fixed-point rounds
                    u = np.abs(w @ xf[i] + p["freq_inverse.trans2.bias"])
                    xf[i] *= (20.0 / u.max(), 100.0 / u.max(), 20.0 / u.min() * 1.0001)[i % 3]
            x = xf.reshape(x.shape).astype(np.float32)
        return p, x, dout
    _, nl, nf, cin, nb, nt, kind = leg
    x, draws = net_input(leg, p, rs)
    nt2 = nt // RATIO
    if kind == "dout":
        return p, x, rs.standard_normal((nb, nt2, 2 * nf, DO // 4, 2)).astype(np.float32)
    # step: targets in [-1, 1], one pooled frame shorter than the prediction, re-drawn per frame until the two permutation
    # errors of that frame differ by more than PERM_GAP of their sum (float64)
    with _one_thread(), torch.no_grad():
        pred = net_forward(_t(p, torch.float64), torch.tensor(x.astype(np.float64)), nl)[:, :nt2 - 1]
    gt = np.zeros((nb, nt2 - 1, 2 * nf, DO // 4, 2), np.float32)
    for b in range(nb):
        for t in range(nt2 - 1):
            for _ in range(MAX_DRAWS):
                gt[b, t] = rs.uniform(-1.0, 1.0, gt.shape[2:]).astype(np.float32)
                _, e = pit_mse(pred[b:b + 1, t:t + 1], torch.tensor(gt[b:b + 1, t:t + 1].astype(np.float64)))
                if abs(float(e[0, 0] - e[0, 1])) > PERM_GAP * float(e.sum()):
                    break
            else:
                raise AssertionError("step: no targets with a permutation gap for frame (%d, %d)" % (b, t))
    return p, x, gt


_SD = {}


def leg_inputs(group, leg, sd=None):
    """(parameters, x, dout) of a leg as float32 arrays (step leg: the targets in dout's place): the same on the host and
    on the device, computed once per leg and shared — never modified.  ``sd``: a net leg's state dict."""
    key = None
    if group == "net":
        key = tuple(sorted(net_cfg(leg).items()))
        _SD.setdefault(key, sd)
    return _cached_inputs(group, leg[0], key)


def pre_activations(leg, p_np, x_np, dtype=torch.float64):
    """Every PReLU input of a net leg on its whole input: 2 per layer, numpy float64 arrays."""
    with _one_thread(), torch.no_grad():
        pre = []
        net_forward(_t(p_np, dtype), torch.tensor(np.asarray(x_np), dtype=dtype), leg[1], pre=pre)
    return [a.numpy().astype(np.float64) for a in pre]


def perm_errors(leg, p_np, x_np, gt_np):
    """The step leg's two permutation errors per frame, float64: [nb * frames, 2]."""
    with _one_thread(), torch.no_grad():
        pred = net_forward(_t(p_np, torch.float64), torch.tensor(np.asarray(x_np, np.float64)), leg[1])
        _, e = pit_mse(pred[:, :gt_np.shape[1]], torch.tensor(np.asarray(gt_np, np.float64)))
    return e.numpy()


# ------------------------------------------------------------------------------------------------------------------ #
# gradients and gates
# ------------------------------------------------------------------------------------------------------------------ #
def leg_forward(group, leg, p, x, mutant=None):
    if group == "encoder":
        return encoder_forward(p["weight"], p["bias"], x, mutant)
    if group == "head":
        return head_forward(p, x, mutant)
    return net_forward(p, x, leg[1], mutant)


def gradients(group, leg, p_np, x_np, dout_np, dtype=torch.float64, mutant=None):
    """(out, {tensor name: gradient}) as numpy float64 arrays.  The cotangent of out is dout; on the step leg ``dout_np``
    holds the targets, the scalar is the PIT-MSE loss of out cut to their frames, and out is (prediction, loss)."""
    with _one_thread():
        p = _t(p_np, dtype, True)
        x = torch.tensor(np.asarray(x_np), dtype=dtype, requires_grad=True)
        out = leg_forward(group, leg, p, x, mutant)
        d = torch.tensor(np.asarray(dout_np), dtype=dtype)
        if group == "net" and leg[6] == "step":
            loss, e = pit_mse(out[:, :d.shape[1]], d)
            if dtype == torch.float64:                       # the condition on the inputs, checked where they are used
                gap = ((e[:, 0] - e[:, 1]).abs() / e.sum(1)).detach()
                assert float(gap.min()) > PERM_GAP, "step: a frame's permutation errors are within %g of their sum" % PERM_GAP
            loss.backward()
        else:
            (out * d).sum().backward()
    g = {"x": x.grad}
    g.update({k: v.grad for k, v in p.items()})
    return out.detach().numpy().astype(np.float64), {k: g[k].detach().numpy().astype(np.float64) for k in tensors(group, leg) + ("x",)
                                                       if g[k] is not None}


def leg_errors(group, leg, sd=None, dtype=torch.float32, mutant=None):
    """{tensor: rel_err of the ``dtype`` restatement's gradient against float64} for one leg."""
    p, x, dout = leg_inputs(group, leg, sd)
    _, want = gradients(group, leg, p, x, dout, torch.float64)
    _, got = gradients(group, leg, p, x, dout, dtype, mutant)
    return {k: rel_err(got[k], want[k]) for k in tensors(group, leg)}


def measure_gate_table(group, sd_of=None):
    """Per tensor, the largest float32-vs-float64 rel_err over all legs of the group (what GATE_F32 commits).  ``sd_of``:
    leg -> state dict, for the net group."""
    worst = {}
    for leg in legs(group):
        for k, v in leg_errors(group, leg, sd_of(leg) if sd_of else None).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


def gate(group: str, name: str) -> float:
    return GATE * GATE_F32[group][name]


# measure_gate_table(group, ...) on the host (torch CPU on one thread, float32 against float64)
GATE_F32 = {
    "encoder": {
        "weight": 7.81e-06,
        "bias": 5.56e-06,
        "x": 2.75e-07,
    },
    "head": {
        "x": 8.90e-07,
        "freq_inverse.trans2.weight": 3.69e-06,
        "freq_inverse.trans2.bias": 2.26e-06,
        "decoder.weight": 4.07e-07,
        "decoder.bias": 2.04e-07,
    },
    "net": {
        "encoder.weight": 1.28e-06,
        "encoder.bias": 1.58e-06,
        "layers.0.fconv1.0.weight": 6.71e-07,
        "layers.0.fconv1.0.bias": 4.59e-07,
        "layers.0.fconv1.1.weight": 5.20e-07,
        "layers.0.fconv1.1.bias": 6.77e-07,
        "layers.0.fconv1.2.weight": 5.03e-07,
        "layers.0.norm_full.weight": 4.94e-07,
        "layers.0.norm_full.bias": 4.26e-07,
        "layers.0.squeeze.0.weight": 8.39e-07,
        "layers.0.squeeze.0.bias": 4.51e-07,
        "layers.0.full.weight": 5.68e-07,
        "layers.0.full.bias": 5.79e-07,
        "layers.0.unsqueeze.0.weight": 5.90e-07,
        "layers.0.unsqueeze.0.bias": 8.06e-07,
        "layers.0.fconv2.0.weight": 5.20e-07,
        "layers.0.fconv2.0.bias": 6.74e-07,
        "layers.0.fconv2.1.weight": 8.70e-07,
        "layers.0.fconv2.1.bias": 6.72e-07,
        "layers.0.fconv2.2.weight": 7.96e-07,
        "layers.0.norm_mhsa.weight": 7.31e-07,
        "layers.0.norm_mhsa.bias": 6.80e-07,
        "layers.0.mhsa.in_proj.weight": 1.31e-06,
        "layers.0.mhsa.conv1d.weight": 9.33e-07,
        "layers.0.mhsa.conv1d.bias": 7.73e-07,
        "layers.0.mhsa.x_proj.weight": 8.47e-07,
        "layers.0.mhsa.dt_proj.weight": 7.02e-07,
        "layers.0.mhsa.dt_proj.bias": 4.89e-07,
        "layers.0.mhsa.A_log": 9.91e-07,
        "layers.0.mhsa.D": 1.01e-06,
        "layers.0.mhsa.out_proj.weight": 6.53e-07,
        "layers.0.norm_tconvffn.weight": 7.12e-07,
        "layers.0.norm_tconvffn.bias": 7.32e-07,
        "layers.0.tconvffn.in_proj.weight": 8.68e-07,
        "layers.0.tconvffn.conv1d.weight": 9.68e-07,
        "layers.0.tconvffn.conv1d.bias": 6.70e-07,
        "layers.0.tconvffn.x_proj.weight": 9.85e-07,
        "layers.0.tconvffn.dt_proj.weight": 1.74e-06,
        "layers.0.tconvffn.dt_proj.bias": 1.20e-06,
        "layers.0.tconvffn.A_log": 1.16e-06,
        "layers.0.tconvffn.D": 8.78e-07,
        "layers.0.tconvffn.out_proj.weight": 7.85e-07,
        "layers.1.fconv1.0.weight": 5.79e-07,
        "layers.1.fconv1.0.bias": 5.86e-07,
        "layers.1.fconv1.1.weight": 8.15e-07,
        "layers.1.fconv1.1.bias": 5.59e-07,
        "layers.1.fconv1.2.weight": 7.42e-07,
        "layers.1.norm_full.weight": 1.07e-06,
        "layers.1.norm_full.bias": 7.73e-07,
        "layers.1.squeeze.0.weight": 1.21e-06,
        "layers.1.squeeze.0.bias": 6.10e-07,
        "layers.1.full.weight": 5.47e-07,
        "layers.1.full.bias": 4.64e-07,
        "layers.1.unsqueeze.0.weight": 9.55e-07,
        "layers.1.unsqueeze.0.bias": 6.07e-07,
        "layers.1.fconv2.0.weight": 1.34e-06,
        "layers.1.fconv2.0.bias": 7.25e-07,
        "layers.1.fconv2.1.weight": 4.99e-07,
        "layers.1.fconv2.1.bias": 4.68e-07,
        "layers.1.fconv2.2.weight": 6.06e-07,
        "layers.1.norm_mhsa.weight": 9.00e-07,
        "layers.1.norm_mhsa.bias": 8.69e-07,
        "layers.1.mhsa.in_proj.weight": 7.23e-07,
        "layers.1.mhsa.conv1d.weight": 7.19e-07,
        "layers.1.mhsa.conv1d.bias": 5.08e-07,
        "layers.1.mhsa.x_proj.weight": 1.60e-06,
        "layers.1.mhsa.dt_proj.weight": 1.53e-06,
        "layers.1.mhsa.dt_proj.bias": 1.19e-06,
        "layers.1.mhsa.A_log": 1.85e-06,
        "layers.1.mhsa.D": 5.36e-07,
        "layers.1.mhsa.out_proj.weight": 6.62e-07,
        "layers.1.norm_tconvffn.weight": 1.47e-06,
        "layers.1.norm_tconvffn.bias": 6.76e-07,
        "layers.1.tconvffn.in_proj.weight": 1.12e-06,
        "layers.1.tconvffn.conv1d.weight": 1.29e-06,
        "layers.1.tconvffn.conv1d.bias": 9.10e-07,
        "layers.1.tconvffn.x_proj.weight": 1.84e-06,
        "layers.1.tconvffn.dt_proj.weight": 4.99e-06,
        "layers.1.tconvffn.dt_proj.bias": 2.98e-06,
        "layers.1.tconvffn.A_log": 1.26e-06,
        "layers.1.tconvffn.D": 7.11e-07,
        "layers.1.tconvffn.out_proj.weight": 6.43e-07,
        "freq_inverse.trans2.weight": 3.47e-07,
        "freq_inverse.trans2.bias": 1.96e-07,
        "decoder.weight": 7.50e-07,
        "decoder.bias": 9.24e-08,
        "layers.2.fconv1.0.weight": 5.86e-07,
        "layers.2.fconv1.0.bias": 4.97e-07,
        "layers.2.fconv1.1.weight": 4.99e-07,
        "layers.2.fconv1.1.bias": 2.84e-07,
        "layers.2.fconv1.2.weight": 4.42e-07,
        "layers.2.norm_full.weight": 5.82e-07,
        "layers.2.norm_full.bias": 6.32e-07,
        "layers.2.squeeze.0.weight": 9.73e-07,
        "layers.2.squeeze.0.bias": 6.92e-07,
        "layers.2.full.weight": 8.20e-07,
        "layers.2.full.bias": 3.94e-07,
        "layers.2.unsqueeze.0.weight": 3.58e-07,
        "layers.2.unsqueeze.0.bias": 2.59e-07,
        "layers.2.fconv2.0.weight": 5.25e-07,
        "layers.2.fconv2.0.bias": 4.89e-07,
        "layers.2.fconv2.1.weight": 4.82e-07,
        "layers.2.fconv2.1.bias": 2.55e-07,
        "layers.2.fconv2.2.weight": 6.51e-07,
        "layers.2.norm_mhsa.weight": 1.22e-06,
        "layers.2.norm_mhsa.bias": 9.63e-07,
        "layers.2.mhsa.in_proj.weight": 8.93e-07,
        "layers.2.mhsa.conv1d.weight": 8.40e-07,
        "layers.2.mhsa.conv1d.bias": 8.66e-07,
        "layers.2.mhsa.x_proj.weight": 9.13e-07,
        "layers.2.mhsa.dt_proj.weight": 6.40e-07,
        "layers.2.mhsa.dt_proj.bias": 1.09e-06,
        "layers.2.mhsa.A_log": 0.00e+00,
        "layers.2.mhsa.D": 7.45e-07,
        "layers.2.mhsa.out_proj.weight": 3.76e-07,
        "layers.2.norm_tconvffn.weight": 4.93e-07,
        "layers.2.norm_tconvffn.bias": 8.56e-07,
        "layers.2.tconvffn.in_proj.weight": 4.36e-07,
        "layers.2.tconvffn.conv1d.weight": 8.03e-07,
        "layers.2.tconvffn.conv1d.bias": 7.02e-07,
        "layers.2.tconvffn.x_proj.weight": 5.84e-07,
        "layers.2.tconvffn.dt_proj.weight": 1.00e-06,
        "layers.2.tconvffn.dt_proj.bias": 1.28e-06,
        "layers.2.tconvffn.A_log": 0.00e+00,
        "layers.2.tconvffn.D": 5.35e-07,
        "layers.2.tconvffn.out_proj.weight": 5.38e-07,
    },
}
