"""The fp32 IPDnet2 kernels (csrc/spatialnet.hip) against the float64 restatement tests/ipdnet2_f64_ref.py: the
fast-math branches of the selective scan observed per inner channel (C1), every op at the smallest size that needs a
second pass of its persistent grid (C2), carried state over hundreds of chunks / frames (C3) and LayerNorm on rows far
from zero mean (C4).  fp32 precision only (the bf16 mode has its own restated-rounding oracle in test_gpu_ipdnet2.py).

Tolerances.  None is chosen from what the kernels give.  For C1 - C3 the yardstick is the float32 numpy oracle
(oracle/ipdnet2_oracle.py: libm transcendentals at 0.5 ulp, numpy summation order) measured against the same float64
reference ON THE SAME INPUTS on the host; the kernel gets GATE = 8 x that figure.  Why 8: the kernel's exp, log, divide
and reciprocal are the hardware's (documented at 1 - 2 ulp against libm's 0.5), a scan step chains four of them, and the
sum over the 16 states runs in another order; a first-order mistake (wrong constant, dropped term, branch taken on the
wrong side) costs 1e-4 relative or more, two orders of magnitude outside the gate.  The measured oracle figures are the
ORACLE_* tables below, next to the tests that use them (DESIGN.md section 7 repeats them).  No channel, frame or
sequence is excluded from any comparison."""
import functools

import numpy as np
import pytest

import ipdnet2_f64_ref as R8
from conftest import rs_randn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GATE = 8.0
P_NORM, P_MAMBA = "layers.1.norm_mhsa", "layers.1.mhsa"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def report(what, got, gate):
    """Every figure is printed before it is asserted (pytest -s / the captured output of a failing test)."""
    print("%-64s %.3e  (gate %.3e)" % (what, got, gate))
    return got <= gate


# ================================================================================================================== #
# C1.  Scan fast-math edges, per inner channel.
# ================================================================================================================== #
# The float32 oracle against the float64 reference on exactly these inputs (S = 3, T = 250), per-channel metric
# (R8.channel_rel_err): worst channel of the output / of the final SSM state / of the carried conv taps; the median
# output channel for orientation.  The kernel's gate is GATE x the worst channel of the same row.
#                      (kind, half):   out worst   out median   ssm worst   taps worst
ORACLE_C1 = {
    ("spread", 0): (4.95e-6, 6.93e-7, 9.42e-6, 6.16e-7),
    ("spread", 1): (6.97e-6, 8.02e-7, 9.42e-6, 6.16e-7),
    ("exact", 0): (8.76e-6, 8.82e-7, 1.32e-5, 6.16e-7),
    ("exact", 1): (7.12e-6, 7.41e-7, 1.32e-5, 6.16e-7),
    ("silu", 0): (3.83e-6, 6.86e-7, 4.48e-6, 6.16e-7),
    ("silu", 1): (2.74e-6, 6.91e-7, 4.48e-6, 6.16e-7),
}
# Smallest channel scale of the reference: 4.0e-12 (spread), 2.3e-27 (exact: dt = e^-60), 1.8e-9 (silu) for the output,
# 1.1e-26 for the SSM state: all normal float32 numbers (c1_reference asserts it).
C1_SEED, C1_S, C1_T = 3100, 3, 250                                        # 250 = 19 * 13 + 3: a ragged conv + x_proj tile


@functools.lru_cache(maxsize=None)
def c1_case(kind, half):
    from fnssl import weights as W
    sd = dict(W.make_ipdnet2_state(C1_SEED, num_layers=2))
    sd.update(R8.probe_state(sd, P_MAMBA + ".", half, kind, seed=C1_SEED + 1))
    x = rs_randn(C1_SEED + 2, (1, C1_S, C1_T, 96))
    return sd, x


@functools.lru_cache(maxsize=None)
def c1_reference(kind, half):
    sd, x = c1_case(kind, half)
    want, (taps, ssm) = R8.mamba_block(sd, P_NORM, P_MAMBA, x)
    # every channel's scale must be a normal float32 (the probe's ranges were chosen for that; none is skipped)
    tiny = float(np.finfo(np.float32).tiny)
    assert np.abs(want).max(axis=(0, 1, 2)).min() > tiny and np.abs(ssm).max(axis=(0, 2)).min() > tiny
    for a in (want, taps, ssm):
        a.setflags(write=False)
    return want, taps, ssm


def c1_errors(out, taps, ssm, ref):
    """(worst output channel, worst SSM-state channel, worst conv-tap channel) of one run against the reference."""
    want, wtaps, wssm = ref
    e_out, _ = R8.channel_rel_err(out, want)
    e_ssm, _ = R8.channel_rel_err(np.transpose(ssm, (0, 2, 1)), np.transpose(wssm, (0, 2, 1)))
    e_taps, _ = R8.channel_rel_err(taps, wtaps)
    return float(e_out.max()), float(e_ssm.max()), float(e_taps.max()), int(e_out.argmax())


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("kind", ["spread", "exact", "silu"])
def test_scan_fast_math_edges_per_channel(dev, monkeypatch, kind, half):
    """softplus on both sides of 20 and of the last x with 1 + e^x > 1, the few-bit quotient above it, a decay that
    underflows (dt up to 60, A down to -64) and SiLU at |x| in the tens — each inner channel observed alone through a
    one-hot out_proj with D = 0, on the three launch paths of the block."""
    from fnssl import spatialnet as sn
    sd, x = c1_case(kind, half)
    ref = c1_reference(kind, half)
    o_out, _, o_ssm, o_taps = ORACLE_C1[(kind, half)]
    w, keep = sn.pack_mamba(sd, P_NORM, P_MAMBA, dev)
    xs = to_dev(x, dev)

    def whole():
        st = sn.mamba_state(1, C1_S, dev)
        out = sn.mamba(xs, w, residual=False, state=st)
        return out.cpu().numpy(), st[0].cpu().numpy(), st[1].cpu().numpy()

    def chunked():                                                        # separate conv kernel, scan with have_u
        st = sn.mamba_state(1, C1_S, dev)
        parts, t0 = [], 0
        for n in (4, 1, 245):
            parts.append(sn.mamba(xs[:, :, t0:t0 + n].contiguous(), w, residual=False, state=st, carry=t0 > 0))
            t0 += n
        return torch.cat(parts, 2).cpu().numpy(), st[0].cpu().numpy(), st[1].cpu().numpy()

    runs = [("fused conv + x_proj", whole()), ("chunks 4 + 1 + 245", chunked())]
    monkeypatch.setenv("FNSSL_SN_SCALAR", "1")
    runs.append(("scalar kernels", whole()))
    monkeypatch.delenv("FNSSL_SN_SCALAR")
    ok = True
    for name, (out, taps, ssm) in runs:
        e_out, e_ssm, e_taps, worst = c1_errors(out, taps, ssm, ref)
        tag = "C1 %s half %d, %s: " % (kind, half, name)
        ok &= report(tag + "output, worst channel (%d)" % (96 * half + worst), e_out, GATE * o_out)
        ok &= report(tag + "final SSM state, worst channel", e_ssm, GATE * o_ssm)
        ok &= report(tag + "carried conv taps, worst channel", e_taps, GATE * o_taps)
    del keep
    assert ok, "a channel is outside 8 x the float32 oracle's own distance from float64 (figures above)"


# ================================================================================================================== #
# C2.  Every op at a multi-pass, ragged size.
# ================================================================================================================== #
# Persistent grids (csrc/spatialnet.hip, the fnssl_sn_* launchers), points per pass on a device of `cus` CUs:
#   encoder               mfma_grid(npts, 2): cus * 2 workgroups * 8 waves * 16 points
#   fconv / full          min(nblk, cus) workgroups of 256 / nf frames
#   mamba in_proj         mfma_grid(npts, 1, 16): cus * 16 waves * 16 points
#   mamba conv + x_proj   mfma_grid(tiles * 16, 4): cus * 4 * 8 tiles of 13 frames of one sequence
#   mamba x_proj (carry)  mfma_grid(npts, 4): cus * 4 * 8 * 16 points
#   mamba out_proj        mfma_grid(nout, 2): cus * 2 * 8 * 16 outputs
#   head                  mfma_grid(npts, 1): cus * 8 * 16 points
# Each case is the smallest count that leaves a partial second pass.  The float32 oracle's max |o - f64| / rms(f64) on
# the same inputs at 256 CUs (the MI355X) — the kernel's gate is GATE x this:
ORACLE_C2 = {
    "encoder10": 7.61e-7, "encoder30": 1.05e-6,
    "fconv256p2": 4.74e-7, "fconv128p8": 6.29e-7, "fconv16": 5.32e-7,
    "full128": 2.63e-7, "full16": 2.54e-7,
    "mamba_pool5": 7.94e-7, "mamba_wide": 6.00e-6, "mamba_wide_ssm": 1.70e-5,
    "mamba_carry": 7.14e-6, "mamba_carry_ssm": 8.14e-6,
    "head": 1.06e-6,
}
C2_SEED = 3200


def c2_sizes(cus):
    """Shapes of the C2 cases on a device with ``cus`` compute units."""
    nseq_wide = cus * 16 + 4                  # 2 conv + x_proj tiles per sequence at 14 .. 26 frames: > cus * 32 tiles
    return {
        "enc_nt": cus * 2 * 8 * 16 // 256 + 1,                # one utterance, 256 bins
        "f256_nt": cus + 1, "f128_nt": 2 * cus + 1, "f16_nt": 16 * cus + 5,
        "m_nb": -(-(cus * 16 * 16 + 1) // (16 * 250)),        # utterances of 16 bins x 250 frames past one in_proj pass
        "wide_nseq": nseq_wide,
        "wide_nt": -(-(cus * 2 * 8 * 16 + 1) // nseq_wide),   # out_proj past one pass (16 frames: tiles of 13 + 3)
        "carry_nt": cus * 4 * 8 * 16 // nseq_wide + 1,        # carried x_proj kernel past one pass
        "head_nt": cus * 8 * 16 // 8 + 1,                     # 8 compressed bins (a 128-bin network): half a tile over
    }


@functools.lru_cache(maxsize=None)
def c2_state():
    from fnssl import weights as W
    return W.make_ipdnet2_state(C2_SEED, num_layers=2, dim_input=30)


def c2_inputs(name, cus):
    """(input arrays of case ``name``) — shared by the test and by the host measurement of ORACLE_C2."""
    z = c2_sizes(cus)
    if name.startswith("encoder"):
        cin = int(name[7:])
        return (rs_randn(C2_SEED + cin, (1, cin, 256, z["enc_nt"])), rs_randn(C2_SEED + cin + 1, (96, cin, 5), 0.1),
                rs_randn(C2_SEED + cin + 2, (96,), 0.1))
    if name in ("fconv256p2", "fconv128p8", "fconv16", "full128", "full16"):
        nf = {"fconv256p2": 256, "fconv128p8": 128, "fconv16": 16, "full128": 128, "full16": 16}[name]
        nt = z["f256_nt"] if nf == 256 else (z["f128_nt"] if nf == 128 else z["f16_nt"])
        return (rs_randn(C2_SEED + 10 + nf + len(name), (1, nf, nt, 96)),)
    if name == "mamba_pool5":
        return (rs_randn(C2_SEED + 40, (z["m_nb"], 16, 250, 96)),)
    if name == "mamba_wide":
        return (rs_randn(C2_SEED + 41, (1, z["wide_nseq"], z["wide_nt"], 96)),)
    if name == "mamba_carry":                                             # a carried state both sides start from
        n = z["wide_nseq"]
        return (rs_randn(C2_SEED + 42, (1, n, z["carry_nt"], 96)), rs_randn(C2_SEED + 43, (n, 3, 192)),
                rs_randn(C2_SEED + 44, (n, 192, 16), 0.3))
    if name == "head":
        return (rs_randn(C2_SEED + 50, (1, 8, z["head_nt"], 96)),)
    raise KeyError(name)


def c2_reference(M, name, inp, sd):
    """Case ``name`` evaluated with module ``M`` (ipdnet2_f64_ref here; the float32 oracle in the host measurement goes
    through its own functions).  Returns a tuple of arrays in the order of the device results."""
    if name.startswith("encoder"):
        return (M.encoder(inp[1], inp[2], inp[0])[0],)
    if name.startswith("fconv"):
        pool = {"fconv256p2": 2, "fconv128p8": 8, "fconv16": 1}[name]
        return (M.fconv(sd, "layers.0.fconv1", inp[0], residual=True, pool=pool),)
    if name.startswith("full"):
        return (M.full(sd, "layers.0." if name == "full128" else "layers.1.", inp[0], residual=True),)
    if name == "mamba_pool5":
        return (M.mamba_block(sd, P_NORM, P_MAMBA, inp[0], residual=True, time_pool=5)[0],)
    if name == "mamba_wide":
        y, st = M.mamba_block(sd, P_NORM, P_MAMBA, inp[0])            # no residual: the input would dilute the branch
        return y, st[1]
    if name == "mamba_carry":
        y, st = M.mamba_block(sd, P_NORM, P_MAMBA, inp[0], state=(inp[1], inp[2]))
        return y, st[1]
    if name == "head":
        return (M.head(sd, inp[0]),)
    raise KeyError(name)


def c2_device(name, inp, sd, dev):
    from fnssl import spatialnet as sn
    x = to_dev(inp[0], dev)
    if name.startswith("encoder"):
        wT = to_dev(inp[1], dev).permute(1, 2, 0).contiguous()
        return (sn.encoder(x, wT, to_dev(inp[2], dev)),)
    if name.startswith("fconv"):
        w, keep = sn.pack_fconv(sd, "layers.0.fconv1", dev)
        pool = {"fconv256p2": 2, "fconv128p8": 8, "fconv16": 1}[name]
        return (sn.fconv(x, w, residual=True, pool=pool),)
    if name.startswith("full"):
        w, keep, _ = sn.pack_full(sd, "layers.0." if name == "full128" else "layers.1.", dev)
        return (sn.full(x, w, residual=True),)
    if name == "head":
        ptrs, keep = sn.pack_head(sd, dev)
        return (sn.head(x, ptrs),)
    w, keep = sn.pack_mamba(sd, P_NORM, P_MAMBA, dev)
    if name == "mamba_pool5":
        return (sn.mamba(x, w, residual=True, time_pool=5),)
    if name == "mamba_wide":
        st = sn.mamba_state(1, x.shape[1], dev)
        return sn.mamba(x, w, residual=False, state=st), st[1]
    st = (to_dev(inp[1], dev), to_dev(inp[2], dev))
    return sn.mamba(x, w, residual=False, state=st, carry=True), st[1]


C2_CASES = ["encoder10", "encoder30", "fconv256p2", "fconv128p8", "fconv16", "full128", "full16", "mamba_pool5",
            "mamba_wide", "mamba_carry", "head"]


@pytest.mark.parametrize("name", C2_CASES)
def test_every_op_at_multi_pass_ragged_size_vs_float64(dev, name):
    """The matrix-pipe kernels with more work than one pass of their persistent grid holds, against the float64
    reference (the existing "matrix pipe == scalar kernels" tests compare two device paths with each other)."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    sd = c2_state()
    inp = c2_inputs(name, cus)
    got = [g.cpu().numpy() for g in c2_device(name, inp, sd, dev)]
    want = c2_reference(R8, name, inp, sd)
    ok = True
    for g, w, key in zip(got, want, (name, name + "_ssm")):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        ok &= report("C2 %s %s on %d CUs" % (key, tuple(w.shape), cus), R8.rms_rel_err(g, w), GATE * ORACLE_C2[key])
    assert ok, "outside 8 x the float32 oracle's own distance from float64 (figures above)"


# ================================================================================================================== #
# C3.  Long carried state.
# ================================================================================================================== #
# The float32 oracle against float64, max |o - f64| / rms(f64):
#   the 2-layer 256-bin network, one utterance of 300 frames (oracle: whole signal)
ORACLE_C3_NET = 1.27e-6
#   the LN + Mamba block driven one frame at a time (oracle: mamba_step), S = 5, at frames 1, 2, 50, 250:
#   worst of the four frames for the output / the SSM state / the conv taps
ORACLE_C3_STEP = (1.34e-6, 1.07e-5, 1.81e-6)
C3_SEED = 3300


def c3_net_case():
    from fnssl import weights as W
    return W.make_ipdnet2_state(C3_SEED, num_layers=2), rs_randn(C3_SEED + 1, (1, 10, 256, 300), 0.7)


def c3_step_case():
    from fnssl import weights as W
    return W.make_ipdnet2_state(C3_SEED + 2, num_layers=2), rs_randn(C3_SEED + 3, (1, 5, 250, 96))


C3_FRAMES = (1, 2, 50, 250)


def c3_step_reference(sd, x):
    """The float64 block stepped one frame at a time; {frame: (out [S, H], taps, ssm)} at C3_FRAMES (1-based)."""
    st, keep = None, {}
    for t in range(x.shape[2]):
        y, st = R8.mamba_block(sd, P_NORM, P_MAMBA, x[:, :, t:t + 1], st)
        if t + 1 in C3_FRAMES:
            keep[t + 1] = (y[0, :, 0].copy(), st[0].copy(), st[1].copy())
    return keep


def test_network_streamed_in_60_chunks_vs_float64_and_vs_whole(dev):
    from test_gpu_ipdnet2 import build_net
    sd, x = c3_net_case()
    sd_, net = build_net(dev, C3_SEED, num_layers=2)
    assert all(np.array_equal(sd[k], sd_[k]) for k in sd)
    xd = to_dev(x, dev)
    whole = net(xd)
    st, outs = None, []
    for t0 in range(0, 300, 5):
        o, st = net.forward_stream(xd[..., t0:t0 + 5], st)
        outs.append(o)
    got = torch.cat(outs, 1)
    assert tuple(got.shape) == (1, 60, 512, 4, 2)
    want = R8.forward(sd, x)
    ok = report("C3 network, 60 chunks of 5 vs float64", R8.rms_rel_err(got.cpu().numpy(), want), GATE * ORACLE_C3_NET)
    ok &= report("C3 network, whole vs float64", R8.rms_rel_err(whole.cpu().numpy(), want), GATE * ORACLE_C3_NET)
    # the device's own whole-signal forward, at the 1e-5 of the 3-chunk test (test_gpu_ipdnet2.py)
    ok &= report("C3 network, 60 chunks vs the device's whole-signal forward (abs)", (got - whole).abs().max().item(), 1e-5)
    assert ok


def test_mamba_stepped_250_frames_vs_float64_step_reference(dev):
    from fnssl import spatialnet as sn
    sd, x = c3_step_case()
    ref = c3_step_reference(sd, x)
    w, keep = sn.pack_mamba(sd, P_NORM, P_MAMBA, dev)
    xs = to_dev(x, dev)
    st = sn.mamba_state(1, 5, dev)
    ok = True
    for t in range(x.shape[2]):
        o = sn.mamba(xs[:, :, t:t + 1], w, residual=False, state=st, carry=t > 0)
        if t + 1 in C3_FRAMES:
            wo, wt, ws = ref[t + 1]
            for what, g, r, gate in (("output", o[0, :, 0], wo, ORACLE_C3_STEP[0]), ("SSM state", st[1], ws, ORACLE_C3_STEP[1]),
                                     ("conv taps", st[0], wt, ORACLE_C3_STEP[2])):
                ok &= report("C3 stepped block, frame %d, %s" % (t + 1, what), R8.rms_rel_err(g.cpu().numpy(), r), GATE * gate)
    del keep
    assert ok


# ================================================================================================================== #
# C4.  LayerNorm away from zero mean: rows of mean 100, standard deviation 0.1.
# ================================================================================================================== #
# Gate, derived (not borrowed from the 8 x rule).  The inputs are float32 and exact for both sides.  A float32 mean of n
# values near m = 100 is a sum of positives: each addition rounds its partial sum by at most 2^-24 relative, so an
# element that passes through d additions contributes d * 2^-24 of itself to the error of the sum, and the mean is off by
# at most (mean depth + 1 for the division by n) * max|x| * 2^-24.  The mean depth is log2(n) for a tree and (n + 1) / 2
# for a plain loop, the deepest order a kernel would use; with that
#     mean_err(n) = ((n + 1) / 2 + 1) * max|x| * 2^-24          (n = 96: 49.5 * 6.0e-6 = 3.0e-4 = 3.0e-3 sigma)
# — one rounding of the mean (100 * 2^-24 absolute, 6e-5 relative to sigma = 0.1) times the number of roundings.  x - mean is then
# exact to one rounding (Sterbenz), the variance taken about a mean that is off by 3e-3 sigma changes by 1e-5 relative,
# so to first order the device's LayerNorm is the exact one with every row's mean shifted by up to mean_err.  The
# float64 reference evaluates exactly that model (ipdnet2_f64_ref.layer_norm(mean_err=...)): stand-alone, the bound is
# element-wise |LN(mean + mean_err) - LN|; for a fused site the op is evaluated with the rows' means shifted by +mean_err
# in every row and by +-mean_err in two random sign patterns, and the largest output change is the gate.  All the
# roundings aligned in the worst direction is 10 - 30 x what a real sum shows, so no further factor is applied.  What the
# gate excludes: a one-pass variance E[x^2] - mean^2 is off by ~1e4 * 2^-24 / 0.01 = 6 % per rounding, 20 x the gate.
C4_SEED, C4_MEAN, C4_STD = 3400, 100.0, 0.1
LN_ROUNDOFF = 16 * 2.0 ** -24            # the handful of float32 operations after the statistics, relative to |y| + |b|


def c4_rows(seed, shape):
    return (C4_MEAN + C4_STD * rs_randn(seed, shape).astype(np.float64)).astype(np.float32)


def c4_mean_err(x):
    n = x.shape[-1]
    return ((n + 1) / 2 + 1) * float(np.abs(x).max()) * 2.0 ** -24


def c4_shift_patterns(x):
    """Row-mean shifts of magnitude mean_err(n): all rows up, and two random sign patterns."""
    d = c4_mean_err(x)
    rs = np.random.RandomState(C4_SEED + 9)
    shape = x.shape[:-1] + (1,)
    return [np.full(shape, d)] + [d * rs.choice([-1.0, 1.0], size=shape) for _ in range(2)]


@pytest.mark.parametrize("h", [96, 200])
def test_layernorm_alone_on_rows_of_mean_100(dev, h):
    from fnssl import spatialnet as sn
    x = c4_rows(C4_SEED + h, (37, h))
    w, b = (1.0 + 0.3 * rs_randn(C4_SEED + h + 1, (h,))).astype(np.float32), rs_randn(C4_SEED + h + 2, (h,))
    got = sn.layernorm(to_dev(x, dev), to_dev(w, dev), to_dev(b, dev)).cpu().numpy()
    want = R8.layer_norm(x, w, b)
    bound = np.abs(R8.layer_norm(x, w, b, mean_err=c4_mean_err(x)) - want) + LN_ROUNDOFF * (np.abs(want) + np.abs(b))
    err = np.abs(got - want)
    print("C4 LayerNorm h %d: max err %.3e, max err / bound %.3f, mean_err %.3e" % (h, err.max(), (err / bound).max(),
                                                                                    c4_mean_err(x)))
    assert (err <= bound).all(), "LayerNorm h %d: %d elements outside the mean-rounding bound" % (h, int((err > bound).sum()))


@pytest.mark.parametrize("scalar", [False, True], ids=["matrix_pipe", "scalar"])
@pytest.mark.parametrize("site", ["fconv", "full", "mamba"])
def test_fused_layernorm_sites_on_rows_of_mean_100(dev, monkeypatch, site, scalar):
    from fnssl import spatialnet as sn
    sd = c2_state()
    x = c4_rows(C4_SEED + 20 + len(site), (2, 16, 13, 96))
    if site == "fconv":
        ref = lambda me: R8.fconv(sd, "layers.1.fconv1", x, mean_err=me)   # noqa: E731
        w, keep = sn.pack_fconv(sd, "layers.1.fconv1", dev)
        run = lambda: sn.fconv(to_dev(x, dev), w, residual=False)          # noqa: E731
    elif site == "full":
        ref = lambda me: R8.full(sd, "layers.1.", x, mean_err=me)          # noqa: E731
        w, keep, _ = sn.pack_full(sd, "layers.1.", dev)
        run = lambda: sn.full(to_dev(x, dev), w, residual=False)           # noqa: E731
    else:
        ref = lambda me: R8.mamba_block(sd, P_NORM, P_MAMBA, x, mean_err=me)[0]   # noqa: E731
        w, keep = sn.pack_mamba(sd, P_NORM, P_MAMBA, dev)
        run = lambda: sn.mamba(to_dev(x, dev), w, residual=False)          # noqa: E731
    want = ref(None)
    gate = max(float(np.abs(ref(me) - want).max()) for me in c4_shift_patterns(x))
    gate += LN_ROUNDOFF * float(np.abs(want).max())
    if scalar:
        monkeypatch.setenv("FNSSL_SN_SCALAR", "1")
    got = run().cpu().numpy()
    if scalar:
        monkeypatch.delenv("FNSSL_SN_SCALAR")
    del keep
    err = float(np.abs(got - want).max())
    assert report("C4 %s (%s), max abs err (output max %.3g)" % (site, "scalar" if scalar else "matrix pipe",
                                                                 np.abs(want).max()), err, gate)
