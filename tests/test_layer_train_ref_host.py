"""Host checks of tests/layer_train_ref.py, the autograd restatement behind test_gpu_layer_train.py: its float64 forward
against the numpy restatement (ipdnet2_f64_ref.fconv / full / layer_forward), its float64 gradients against Richardson-
extrapolated central differences, the kink condition of every leg's inputs, the committed gate tables re-measured and
their independence of the host's thread count, and mutants of the backward against the gates (each must miss a gate on at
least one leg).  No GPU, nothing of the library but its deterministic weight generator."""
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
import layer_train_ref as R                                         # noqa: E402
from fnssl import weights as W                                      # noqa: E402


@pytest.fixture(scope="module")
def sd():
    return W.make_ipdnet2_state(0, num_layers=2)


@pytest.fixture(scope="module")
def f32_errors(sd):
    """{group: {leg name: {tensor: err of the float32 restatement}}} — computed once, shared."""
    return {g: {leg[0]: R.leg_errors(g, leg, sd) for leg in R.legs(g)} for g in R.GROUPS}


def _t64(p):
    return {k: torch.tensor(v, dtype=torch.float64) for k, v in p.items()}


def test_leg_tables_cover_the_shapes_they_name():
    for g, n in (("fconv", 12), ("full", 16), ("layer", 3)):
        legs = R.legs(g)
        assert len({l[0] for l in legs}) == len(legs) == n, g
    fc = {l[0]: l for l in R.legs("fconv")}
    assert fc["f256_300blocks"][1] * fc["f256_300blocks"][3] == 300 and fc["f16_real"][1:4] == (2, 16, 250)
    assert sorted({l[2] for l in R.legs("full")}) == [8, 16, 32, 64, 128, 256]
    assert len(R.LAYER_PARAMS) == 40 and len(R.TENSORS["layer"]) == 41


@pytest.mark.parametrize("pool,residual", [(1, False), (1, True), (2, True), (8, True)])
def test_fconv_forward_is_the_float64_restatement(sd, pool, residual):
    x = np.random.RandomState(3).standard_normal((2, 16, 3, R.H))
    want = R8.fconv(sd, "layers.0.fconv1", x, residual=residual, pool=pool)
    p = R.leg_params("fconv", None, sd)
    got = R.fconv_forward(_t64(p), torch.tensor(x), residual, pool).numpy()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("residual", [False, True])
def test_full_forward_is_the_float64_restatement(sd, residual):
    x = np.random.RandomState(4).standard_normal((2, 16, 3, R.H))
    want = R8.full(sd, "layers.1.", x, residual=residual)
    p = {n: np.array(sd["layers.1." + n], np.float32) for n in R.FULL_PARAMS}
    got = R.full_forward(_t64(p), torch.tensor(x), residual).numpy()
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_layer_forward_is_the_float64_restatement(sd):
    x = np.random.RandomState(5).standard_normal((1, 16, 6, R.H))
    want = R8.layer_forward(sd, "layers.1.", x, False)
    want = want[0] if isinstance(want, tuple) else want
    p = {n: np.array(sd["layers.1." + n], np.float32) for n in R.LAYER_PARAMS}
    got = R.layer_forward(_t64(p), torch.tensor(x), False, 1).numpy()
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


FD_LEGS = {"fconv": [("fd", 1, 8, 2, 1, True, "plain", None), ("fd_pool2", 1, 8, 2, 2, True, "plain", None)],
           "full": [("fd", 1, 8, 2, 1, True, "plain", None)]}


@pytest.mark.parametrize("group,leg", [(g, l) for g in FD_LEGS for l in FD_LEGS[g]], ids=lambda v: v if isinstance(v, str) else v[0])
def test_float64_gradients_are_the_finite_differences(sd, group, leg):
    """1 x 8 x 2 kink-free inputs; per tensor, three random directions v: <grad, v> against the Richardson-extrapolated
    central difference of the loss <out, dout> along v."""
    p = {k: v.astype(np.float64) for k, v in R.leg_params(group, leg, sd).items()}
    x, dout = (a.astype(np.float64) for a in R.leg_inputs(group, leg, p))
    _, g = R.gradients(group, leg, p, x, dout)
    rs = np.random.RandomState(5)

    def out_of(pp, xx):
        return R.leg_forward(group, leg, _t64(pp), torch.tensor(xx)).numpy()

    def central(name, base, v, h):
        # the difference is taken per output element BEFORE the sum with dout (mamba_train_ref's host test)
        hi, lo = dict(p), dict(p)
        if name == "x":
            d = out_of(p, x + h * v) - out_of(p, x - h * v)
        else:
            hi[name], lo[name] = base + h * v, base - h * v
            d = out_of(hi, x) - out_of(lo, x)
        return float((d * dout).sum()) / (2 * h)

    for name in R.TENSORS[group]:
        base = x if name == "x" else p[name]
        for _ in range(3):
            v = rs.standard_normal(base.shape)
            # small enough that no PReLU input (|a| >= 1e-4) changes sign along the step
            h = 1e-5 * max(1e-3, np.abs(base).max())
            fd = (4.0 * central(name, base, v, h / 2) - central(name, base, v, h)) / 3.0      # Richardson: O(h^4)
            an = float((g[name] * v).sum())
            scale = float(np.abs(g[name]).max() * np.abs(v).sum() / v.size ** 0.5)
            print("%-6s %-20s analytic %+.9e  finite difference %+.9e" % (group, name, an, fd))
            assert abs(an - fd) <= 1e-6 * max(abs(an), scale), (name, an, fd)


@pytest.mark.parametrize("group", ["fconv", "layer"])
def test_no_leg_has_a_prelu_input_near_zero(sd, group):
    """min|a| >= A_MARGIN in float64 on every leg, and the float32 restatement's a within 1e-6 of it: the margin is >= 100 x
    the rounding it guards against."""
    for leg in R.legs(group):
        p = R.leg_params(group, leg, sd)
        x, _ = R.leg_inputs(group, leg, p)
        a64 = R.pre_activations(group, leg, p, x)
        a32 = R.pre_activations(group, leg, p, x, torch.float32)
        lo = min(np.abs(a).min() for a in a64)
        d = max(np.abs(u - v).max() for u, v in zip(a32, a64))
        print("%-6s %-20s min|a| %.3e  max|a32 - a64| %.3e" % (group, leg[0], lo, d))
        assert lo >= R.A_MARGIN and d <= 1e-6, leg[0]


@pytest.mark.parametrize("group", R.GROUPS)
def test_committed_gate_table_is_what_float32_measures_here(f32_errors, group):
    """Within a factor 2 (the project's reading of 'equal' for a measured float32 figure, test_mamba_train_ref_host.py)."""
    assert sorted(R.GATE_F32[group]) == sorted(R.TENSORS[group])
    for k in R.TENSORS[group]:
        v, c = max(e[k] for e in f32_errors[group].values()), R.GATE_F32[group][k]
        print("%-6s %-28s committed %.3e  measured %.3e" % (group, k, c, v))
        assert 0.5 * c <= v <= 2.0 * c, "%s: committed %.3e, measured %.3e" % (k, c, v)


@pytest.mark.parametrize("group", R.GROUPS)
def test_float32_restatement_passes_its_own_gate_with_room(f32_errors, group):
    for name, e in f32_errors[group].items():
        for k in R.TENSORS[group]:
            assert e[k] <= R.gate(group, k) / 4, (name, k, e[k])


def test_table_does_not_move_with_the_thread_count(sd):
    """The restatement pins torch to one thread while it runs, so the figures are the same bits at 1, 2 and 5 threads."""
    picks = [("fconv", "f16_real"), ("full", "f128_300frames"), ("layer", "later_layer")]
    before = torch.get_num_threads()
    seen = []
    try:
        for n in (1, 2, 5):
            torch.set_num_threads(n)
            seen.append([R.leg_errors(g, [l for l in R.legs(g) if l[0] == name][0], sd) for g, name in picks])
            assert torch.get_num_threads() == n
    finally:
        torch.set_num_threads(before)
    assert seen[0] == seen[1] == seen[2]


MUTANT_LEGS = {"tap_flip": ("f16_6frames_res", "f8_1frame_res"), "prelu_neg": ("f16_6frames_res",),
               "pool_scale": ("f32_pool2", "f128_pool8"), "ln_xhat_term": ("f16_6frames_branch",),
               "residual_drop": ("f16_6frames_res",),
               "wf_not_transposed": ("f16_res", "f8_branch"), "silu_sigma": ("f16_res",), "dbf_unsummed": ("f16_res",)}


@pytest.mark.parametrize("group,mutant", [(g, m) for g in R.GROUPS for m in R.MUTANTS[g]])
def test_gate_sees_the_mutant(sd, group, mutant):
    """float64 with one mistake in the backward: some tensor of some leg must miss its gate."""
    worst = 0.0
    for leg in [l for l in R.legs(group) if l[0] in MUTANT_LEGS[mutant]]:
        e = R.leg_errors(group, leg, sd, torch.float64, mutant)
        for k in R.TENSORS[group]:
            print("%-18s %-20s %-20s err %.3e  gate %.3e" % (mutant, leg[0], k, e[k], R.gate(group, k)))
            worst = max(worst, e[k] / R.gate(group, k))
    assert worst > 1.0, "no tensor of any leg misses its gate under mutant %s (worst err / gate %.3g)" % (mutant, worst)


@pytest.mark.parametrize("group", ["fconv", "full"])
def test_mutants_leave_the_forward_alone(sd, group):
    name = "f32_pool2" if group == "fconv" else "f16_res"
    leg = [l for l in R.legs(group) if l[0] == name][0]
    p = R.leg_params(group, leg, sd)
    x, dout = R.leg_inputs(group, leg, p)
    want, _ = R.gradients(group, leg, p, x, dout)
    for m in R.MUTANTS[group]:
        got, _ = R.gradients(group, leg, p, x, dout, mutant=m)
        assert np.array_equal(got, want), m
