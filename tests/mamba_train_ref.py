"""Autograd restatement of one IPDnet2 Mamba block for the training tests.  TEST INFRASTRUCTURE ONLY.

torch on the CPU, float64 (the reference) or float32 (the yardstick), written from the block's definition in RECURRENT
form: LN -> in_proj -> depthwise causal conv + SiLU -> x_proj -> dt_proj + softplus -> h_t = exp(dt_t A) h_{t-1} + dt_t u_t B_t,
ys_t = C_t . h_t + D u_t -> gate by SiLU(z) -> out_proj -> residual -> time pooling.  It calls nothing of the library
under test and nothing of ``oracle/``; test_mamba_train_ref_host.py pins its forward to ipdnet2_f64_ref.mamba_block and its
float64 gradients to finite differences.

The gate of test_gpu_mamba_train.py: per gradient tensor, err = max|got - f64| / max|f64|, held to GATE = 8 x the float32
restatement's own err on the same inputs (DESIGN.md section 7's rule for the IPDnet2 kernels), taken per tensor as the
LARGEST over all legs so that one lucky leg does not set it.  GATE_F32 below holds those float32 figures as measured on
the host; the host test re-measures them.

``mutant``: a deliberately wrong backward (the forward is unchanged), to show that the gate sees the mistakes a reverse
scan can make.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

H, E, NST, RK, KC = 96, 192, 16, 6, 4
TC = 8                                  # fnssl_sn_mamba_backward_chunk() of the library the tables were measured for
GATE = 8.0

PARAMS = ("in_proj.weight", "conv1d.weight", "conv1d.bias", "x_proj.weight", "dt_proj.weight", "dt_proj.bias", "A_log", "D",
          "out_proj.weight")
TENSORS = ("x", "norm.weight", "norm.bias") + PARAMS        # the 12 gradients of a leg

MUTANTS = ("carry_cut", "ddt_decay", "conv_tap", "softplus_branch", "pool_scale")


def legs(tc: int = TC):
    """The leg table.  (name, nb, nf, nt, pool, residual, layout, dt_proj.bias shift); layout: 'frame' = frame-major
    storage ([B, T, F, H] in memory, the library's native layout), 'plain' = a contiguous [B, F, T, H] tensor."""
    out = []
    for nt in (1, 3, 4, 5):                                           # single step, fewer frames than conv taps, 30 points
        for res in (True, False):                                     # against 16-point tiles, strided views
            for lay in ("frame", "plain"):
                out.append(("short_nt%d_%s_%s" % (nt, "res" if res else "branch", lay), 2, 3, nt, 1, res, lay, 0.0))
    for nt in (tc - 1, tc, tc + 1, 2 * tc + 3):                       # checkpoint hand-over, last partial chunk
        out.append(("chunk_nt%d" % nt, 2, 3, nt, 1, True, "frame", 0.0))
    for nt in (5, 12):                                                # frames 10, 11 of nt 12: dx exactly 0; 1 / pool
        out.append(("pooled_nt%d" % nt, 2, 3, nt, 5, True, "frame", 0.0))
    for pool in (1, 5):                                               # config 5's per-utterance shape, 250-step carry
        out.append(("real_pool%d" % pool, 2, 16, 250, pool, True, "frame", 0.0))
    out.append(("many_seq", 33, 16, 16, 1, True, "frame", 0.0))       # more workgroups than CUs, partials over many rows
    for shift in (25.0, -20.0):                                       # dtv > 20; 1 + e^dtv == 1; decays that underflow
        out.append(("softplus_%+d" % shift, 2, 16, 32, 1, True, "frame", shift))
    return out


def leg_seed(name: str) -> int:
    return int(np.frombuffer(name.encode().ljust(64, b"\0")[:64], np.uint32).sum() % (1 << 30))


def block_params(sd, p_norm="layers.0.norm_mhsa", p_mamba="layers.0.mhsa", bias_shift=0.0):
    """The 11 parameters of one block out of an IPDnet2 state dict (fnssl.weights.make_ipdnet2_state), as float32 arrays
    under this module's names."""
    out = {"norm.weight": np.array(sd[p_norm + ".weight"], np.float32), "norm.bias": np.array(sd[p_norm + ".bias"], np.float32)}
    for n in PARAMS:
        out[n] = np.array(sd[p_mamba + "." + n], np.float32)
    if bias_shift:
        out["dt_proj.bias"] = (out["dt_proj.bias"] + np.float32(bias_shift)).astype(np.float32)
    return out


def leg_inputs(leg):
    """(x [B, F, T, H], dout [B, F, T // pool, H]) of a leg: float32 arrays, the same on the host and on the device."""
    name, nb, nf, nt, pool = leg[:5]
    rs = np.random.RandomState(leg_seed(name))
    x = rs.standard_normal((nb, nf, nt, H)).astype(np.float32)
    dout = rs.standard_normal((nb, nf, nt // pool, H)).astype(np.float32)
    return x, dout


def softplus(x):
    """log(1 + e^x) as log1p(exp(-|x|)) + max(x, 0): no overflow, no threshold; its autograd derivative is the sigmoid."""
    return torch.log1p(torch.exp(-x.abs())) + torch.clamp(x, min=0.0)


class _ScaleGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        ctx.k = k
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.k, None


class _SoftplusWrongBranch(torch.autograd.Function):
    """softplus whose derivative above 20 is e^x, the derivative of the forward kernel's OTHER special branch (1 + e^x == 1).
    (The sigmoid itself is within 2.1e-9 of the identity branch's 1 above 20: no gate can see that one, see
    test_mamba_train_ref_host.py.)"""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return softplus(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.where(x > 20.0, torch.exp(x), torch.sigmoid(x))


def forward(params, x, residual=True, pool=1, mutant=None, tc=TC):
    """params: dict of torch tensors under TENSORS' names; x [B, F, T, H].  Returns pool_T(residual * x + block(x))."""
    assert mutant is None or mutant in MUTANTS, mutant
    B, Fq, T, _ = x.shape
    ln = F.layer_norm(x, (H,), params["norm.weight"], params["norm.bias"], 1e-5)
    xz = ln @ params["in_proj.weight"].T
    xi, z = xz[..., :E], xz[..., E:]
    wc = params["conv1d.weight"][:, 0, :]
    xp = F.pad(xi, (0, 0, KC - 1, 0))
    pre = params["conv1d.bias"]
    for k in range(KC):
        tap = xp[:, :, k:k + T]
        if mutant == "conv_tap" and k == 0:                 # dxi loses the tap that reaches three frames ahead
            tap = tap.detach()
        pre = pre + wc[:, k] * tap
    u = F.silu(pre)
    dbl = u @ params["x_proj.weight"].T
    dtv = dbl[..., :RK] @ params["dt_proj.weight"].T + params["dt_proj.bias"]
    dt = _SoftplusWrongBranch.apply(dtv) if mutant == "softplus_branch" else softplus(dtv)
    Bm, Cm = dbl[..., RK:RK + NST], dbl[..., RK + NST:]
    A = -torch.exp(params["A_log"])
    h = torch.zeros((B, Fq, E, NST), dtype=x.dtype, device=x.device)
    ys = []
    for t in range(T):
        dtt = dt[:, :, t, :, None]
        decay = torch.exp((dtt.detach() if mutant == "ddt_decay" else dtt) * A)
        hp = h.detach() if (mutant == "carry_cut" and t > 0 and t % tc == 0) else h
        h = decay * hp + (dtt * u[:, :, t, :, None]) * Bm[:, :, t, None, :]
        ys.append((h * Cm[:, :, t, None, :]).sum(-1))
    ysv = torch.stack(ys, 2) + params["D"] * u
    y = ysv * F.silu(z)
    out = y @ params["out_proj.weight"].T
    if residual:
        out = x + out
    if pool > 1:
        if mutant == "pool_scale":                          # the broadcast without its 1 / pool
            out = _ScaleGrad.apply(out, float(pool))
        out = out[:, :, :T // pool * pool].reshape(B, Fq, T // pool, pool, H).mean(3)
    return out


def gradients(params_np, x_np, dout_np, residual=True, pool=1, dtype=torch.float64, mutant=None, tc=TC):
    """(out, {tensor name: gradient}) as numpy float64 arrays; the cotangent of out is dout."""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in params_np.items()}
    x = torch.tensor(np.asarray(x_np), dtype=dtype, requires_grad=True)
    # ONE thread: the float32 figures are dominated by the sums over all points (d gamma, d beta, the weight gradients), and
    # torch splits those sums by its thread count — 9e-7 with 8 threads, 4e-6 with one, something else on every other host.
    # Pinned, the yardstick is the sequential float32 restatement and the same number wherever it is measured.
    nth = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = forward(p, x, residual, pool, mutant, tc)
        (out * torch.tensor(np.asarray(dout_np), dtype=dtype)).sum().backward()
    finally:
        torch.set_num_threads(nth)
    g = {"x": x.grad}
    g.update({k: v.grad for k, v in p.items()})
    return out.detach().numpy().astype(np.float64), {k: v.detach().numpy().astype(np.float64) for k, v in g.items()}


def rel_err(got, want):
    """The gate's metric: max|got - want| / max|want|.  A reference that is identically zero (dA_log of a one-frame
    sequence: h_0 = 0) admits only exact zeros."""
    want, got = np.asarray(want, np.float64), np.asarray(got, np.float64)
    scale = np.abs(want).max()
    if scale == 0.0:
        return 0.0 if not got.any() else float("inf")
    return float(np.abs(got - want).max() / scale)


def leg_errors(sd, leg, dtype=torch.float32, mutant=None, tc=TC):
    """{tensor: rel_err of the ``dtype`` restatement's gradient against float64} for one leg."""
    name, nb, nf, nt, pool, res, _, shift = leg
    p = block_params(sd, bias_shift=shift)
    x, dout = leg_inputs(leg)
    _, want = gradients(p, x, dout, res, pool, torch.float64)
    _, got = gradients(p, x, dout, res, pool, dtype, mutant, tc)
    return {k: rel_err(got[k], want[k]) for k in TENSORS}


def measure_gate_table(sd, tc=TC):
    """Per tensor, the largest float32-vs-float64 rel_err over all legs (what GATE_F32 commits)."""
    worst = {k: 0.0 for k in TENSORS}
    for leg in legs(tc):
        for k, v in leg_errors(sd, leg).items():
            worst[k] = max(worst[k], v)
    return worst


def gate(name: str) -> float:
    return GATE * GATE_F32[name]


# measure_gate_table(make_ipdnet2_state(0, num_layers=1)) on the host (torch CPU on one thread, float32 against float64)
GATE_F32 = {
    "x": 6.01e-07,
    "norm.weight": 4.21e-06,
    "norm.bias": 3.17e-06,
    "in_proj.weight": 6.48e-07,
    "conv1d.weight": 8.55e-07,
    "conv1d.bias": 5.89e-07,
    "x_proj.weight": 1.15e-06,
    "dt_proj.weight": 2.20e-06,
    "dt_proj.bias": 1.20e-06,
    "A_log": 1.06e-06,
    "D": 6.91e-07,
    "out_proj.weight": 7.24e-07,
}
