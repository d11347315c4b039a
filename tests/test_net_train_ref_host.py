"""Host checks of tests/net_train_ref.py, the autograd restatement behind test_gpu_net_train.py: its float64 forward against
the numpy restatement (ipdnet2_f64_ref.encoder / head / forward), the float64 gradients of the encoder and the head against
Richardson-extrapolated central differences, the conditions on the inputs (no PReLU input near zero, the permutation gap of
the step leg, the saturated head leg), the committed gate tables re-measured, and mutants of the backward against the gates
(each must miss a gate on at least one leg).  No GPU, nothing of the library but its deterministic weight generator."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fn-ssl_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import ipdnet2_f64_ref as R8                                        # noqa: E402
import net_train_ref as R                                           # noqa: E402
from fnssl import weights as W                                      # noqa: E402


@functools.lru_cache(maxsize=None)
def _sd(cfg):
    return W.make_ipdnet2_state(0, **dict(cfg))


def sd_of(leg):
    return _sd(tuple(sorted(R.net_cfg(leg).items())))


def leg_sd(group, leg):
    return sd_of(leg) if group == "net" else None


@pytest.fixture(scope="module")
def f32_errors():
    """{group: {leg name: {tensor: err of the float32 restatement}}} — computed once, shared."""
    return {g: {leg[0]: R.leg_errors(g, leg, leg_sd(g, leg)) for leg in R.legs(g)} for g in R.GROUPS}


def _t64(p):
    return {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in p.items()}


def test_leg_tables_cover_the_shapes_they_name():
    enc = {l[0]: l for l in R.legs("encoder")}
    assert len(enc) == 10 and enc["many_tiles"][1:5] == (3, 10, 256, 100) and enc["cin34_plain"][2] * 5 > 160
    assert enc["ragged"][1] * enc["ragged"][3] * enc["ragged"][4] % 16 != 0
    assert {l[8] for l in R.legs("encoder")} == {True, False}                    # dx both wanted and not wanted
    head = {l[0]: l for l in R.legs("head")}
    assert len(head) == 6 and head["ragged40"][1] * head["ragged40"][2] * head["ragged40"][3] == 40
    assert {l[4] for l in R.legs("head")} == {"frame", "plain"}
    net = {l[0]: l for l in R.legs("net")}
    assert len(net) == 4
    for leg in R.legs("net"):
        assert len(R.tensors("net", leg)) == 2 + 40 * leg[1] + 4


@pytest.mark.parametrize("name", ["one_frame", "cin10_kp80", "cin34_plain"])
def test_encoder_forward_is_the_float64_restatement(name):
    leg = [l for l in R.legs("encoder") if l[0] == name][0]
    p, x, _ = R.leg_inputs("encoder", leg)
    want = R8.encoder(p["weight"], p["bias"], x)[0]
    got = R.encoder_forward(*(torch.tensor(p[k], dtype=torch.float64) for k in ("weight", "bias")),
                            torch.tensor(x, dtype=torch.float64)).numpy()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", ["one_point", "fc16", "ragged40"])
def test_head_forward_is_the_float64_restatement(name):
    leg = [l for l in R.legs("head") if l[0] == name][0]
    p, x, _ = R.leg_inputs("head", leg)
    want = R8.head(p, x)
    got = R.head_forward(_t64(p), torch.tensor(x, dtype=torch.float64)).numpy()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", ["l2_f128_nt12", "l3_f256_nt5"])
def test_net_forward_is_the_float64_restatement(name):
    leg = [l for l in R.legs("net") if l[0] == name][0]
    p, x, _ = R.leg_inputs("net", leg, sd_of(leg))
    want = R8.forward(sd_of(leg), x)
    got = R.net_forward(_t64(p), torch.tensor(x, dtype=torch.float64), leg[1]).numpy()
    assert got.shape == want.shape == (leg[4], leg[5] // 5, 2 * leg[2], 4, 2)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_pit_mse_is_the_step_reference():
    import ipdnet_step_ref as SR
    rs = np.random.RandomState(11)
    pred, gt = rs.standard_normal((2, 3, 16, 4, 2)), rs.uniform(-1, 1, (2, 3, 16, 4, 2))
    pt = torch.tensor(pred, requires_grad=True)
    loss, _ = R.pit_mse(pt, torch.tensor(gt))
    loss.backward()
    want_loss, _, want_d = SR.pit_mse(pred.reshape(6, -1, 2), gt.reshape(6, -1, 2))
    assert abs(float(loss.detach()) - want_loss) <= 1e-14 * want_loss
    assert np.abs(pt.grad.numpy().reshape(6, -1, 2) - want_d).max() <= 1e-15


FD_LEGS = {"encoder": ("fd", 1, 3, 2, 7, "plain", "plain", None, True), "head": ("fd", 1, 1, 2, "plain", None)}


@pytest.mark.parametrize("group", ["encoder", "head"])
def test_float64_gradients_are_the_finite_differences(group):
    """Per tensor, three random directions v: <grad, v> against the Richardson-extrapolated central difference of the loss
    <out, dout> along v (both operators are smooth: no kink to step over)."""
    leg = FD_LEGS[group]
    rs = np.random.RandomState(5)
    p = {k: v.astype(np.float64) for k, v in R.leg_params(group, leg).items()}
    if group == "encoder":
        x, dout = rs.standard_normal((1, 3, 2, 7)), rs.standard_normal((1, 2, 7, R.H))
    else:
        x, dout = rs.standard_normal((1, 1, 2, R.H)), rs.standard_normal((1, 2, 32, 4, 2))
    _, g = R.gradients(group, leg, p, x, dout)

    def out_of(pp, xx):
        return R.leg_forward(group, leg, _t64(pp), torch.tensor(xx)).numpy()

    def central(name, base, v, h):
        hi, lo = dict(p), dict(p)
        if name == "x":
            d = out_of(p, x + h * v) - out_of(p, x - h * v)
        else:
            hi[name], lo[name] = base + h * v, base - h * v
            d = out_of(hi, x) - out_of(lo, x)
        return float((d * dout).sum()) / (2 * h)

    for name in R.tensors(group, leg):
        base = x if name == "x" else p[name]
        for _ in range(3):
            v = rs.standard_normal(base.shape)
            h = 1e-4 * max(1e-3, np.abs(base).max())
            fd = (4.0 * central(name, base, v, h / 2) - central(name, base, v, h)) / 3.0      # Richardson: O(h^4)
            an = float((g[name] * v).sum())
            scale = float(np.abs(g[name]).max() * np.abs(v).sum() / v.size ** 0.5)
            print("%-8s %-28s analytic %+.9e  finite difference %+.9e" % (group, name, an, fd))
            assert abs(an - fd) <= 1e-6 * max(abs(an), scale), (name, an, fd)


def test_no_net_leg_has_a_prelu_input_near_zero():
    """min|a| >= A_MARGIN in float64 on every net leg (2 L pre-activations each), and the float32 restatement's a within
    A_MARGIN / 10 of it: the margin is >= 10 x the rounding it guards against."""
    for leg in R.legs("net"):
        p, x, _ = R.leg_inputs("net", leg, sd_of(leg))
        a64 = R.pre_activations(leg, p, x)
        a32 = R.pre_activations(leg, p, x, torch.float32)
        assert len(a64) == 2 * leg[1]
        lo = min(np.abs(a).min() for a in a64)
        d = max(np.abs(u - v).max() for u, v in zip(a32, a64))
        print("%-14s min|a| %.3e  max|a32 - a64| %.3e" % (leg[0], lo, d))
        assert lo >= R.A_MARGIN and d <= R.A_MARGIN / 10, leg[0]


def test_step_leg_has_its_permutation_gap_and_a_longer_prediction():
    leg = [l for l in R.legs("net") if l[6] == "step"][0]
    p, x, gt = R.leg_inputs("net", leg, sd_of(leg))
    assert gt.shape[1] == leg[5] // 5 - 1 and np.abs(gt).max() <= 1.0
    e = R.perm_errors(leg, p, x, gt)
    gap = np.abs(e[:, 0] - e[:, 1]) / e.sum(1)
    print("step: permutation gaps", gap)
    assert (gap > R.PERM_GAP).all()
    _, g = R.gradients("net", leg, p, x, gt)
    # one frame of targets: a later layer's dA_log is identically zero (h starts at 0), everything else is reached
    zero = [k for k in R.tensors("net", leg) if not np.abs(g[k]).max() > 0]
    assert zero == ["layers.1.mhsa.A_log", "layers.1.tconvffn.A_log"], zero


def test_saturated_head_leg_reaches_20_and_100():
    leg = [l for l in R.legs("head") if l[5] == "saturated"][0]
    p, x, _ = R.leg_inputs("head", leg)
    u = np.abs(x.reshape(-1, R.H).astype(np.float64) @ p["freq_inverse.trans2.weight"][:, :, 0].T.astype(np.float64)
               + p["freq_inverse.trans2.bias"])
    assert np.allclose(u[0::3].max(1), 20.0, rtol=1e-3) and np.allclose(u[1::3].max(1), 100.0, rtol=1e-3)
    assert (u[2::3].min(1) >= 19.9).all()                    # e^2u overflows 2^25 at u = 8.7: every tanh of the point is +-1
    _, g = R.gradients("head", leg, p, x, R.leg_inputs("head", leg)[2])
    assert all(np.isfinite(v).all() for v in g.values())
    assert np.abs(g["x"].reshape(-1, R.H)[2::3]).max() <= 1e-9 * np.abs(g["x"]).max()


def test_tail_frames_reach_nothing():
    """nt = 12: frames 10 and 11 reach no pooled frame, so the prediction and every gradient are those of the first 10
    frames' network — the x-gradient of the tail is exactly zero."""
    leg = [l for l in R.legs("net") if l[0] == "l2_f128_nt12"][0]
    p, x, dout = R.leg_inputs("net", leg, sd_of(leg))
    _, g = R.gradients("net", leg, p, x, dout)
    assert (g["x"][:, :, :, 10:] == 0).all() and (g["x"][:, :, :, :10] != 0).any()


@pytest.mark.parametrize("group", R.GROUPS)
def test_committed_gate_table_is_what_float32_measures_here(f32_errors, group):
    """Within a factor 2 (the project's reading of 'equal' for a measured float32 figure, test_mamba_train_ref_host.py)."""
    names = sorted({k for leg in R.legs(group) for k in R.tensors(group, leg)})
    assert sorted(R.GATE_F32[group]) == names
    for k in names:
        v, c = max(e[k] for e in f32_errors[group].values() if k in e), R.GATE_F32[group][k]
        print("%-8s %-36s committed %.3e  measured %.3e" % (group, k, c, v))
        assert 0.5 * c <= v <= 2.0 * c, "%s: committed %.3e, measured %.3e" % (k, c, v)


@pytest.mark.parametrize("group", R.GROUPS)
def test_float32_restatement_passes_its_own_gate_with_room(f32_errors, group):
    for name, e in f32_errors[group].items():
        for k, v in e.items():
            assert v <= R.gate(group, k) / 4, (name, k, v)


MUTANT_LEGS = {"dx_taps_not_flipped": ("cin10_kp80", "nt3"), "dw_k_reversed": ("cin10_kp80", "one_frame"),
               "one_minus_v": ("fc16",), "gather_a_gg_swapped": ("fc16", "element_last"),
               "decoder_not_transposed": ("fc16",), "time_pool_no_fifth": ("l2_f128_nt10",)}


@pytest.mark.parametrize("group,mutant", [(g, m) for g in R.GROUPS for m in R.MUTANTS[g]])
def test_gate_sees_the_mutant(group, mutant):
    """float64 with one mistake in the backward: some tensor of some leg must miss its gate, and the forward is untouched."""
    worst = 0.0
    for leg in [l for l in R.legs(group) if l[0] in MUTANT_LEGS[mutant]]:
        sd = leg_sd(group, leg)
        e = R.leg_errors(group, leg, sd, torch.float64, mutant)
        for k, v in e.items():
            worst = max(worst, v / R.gate(group, k))
        p, x, dout = R.leg_inputs(group, leg, sd)
        assert np.array_equal(R.gradients(group, leg, p, x, dout, mutant=mutant)[0], R.gradients(group, leg, p, x, dout)[0])
    print("%-24s worst err / gate %.3g" % (mutant, worst))
    assert worst > 1.0, "no tensor of any leg misses its gate under mutant %s (worst err / gate %.3g)" % (mutant, worst)
