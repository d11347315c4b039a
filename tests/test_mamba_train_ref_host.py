"""Host checks of tests/mamba_train_ref.py, the autograd restatement behind test_gpu_mamba_train.py: its forward against
the float64 numpy restatement (ipdnet2_f64_ref.mamba_block), its float64 gradients against central finite differences,
the committed gate table re-measured, and mutants of its backward against the gate (the gate must see each of them on
at least one leg).  No GPU, nothing of the library but its deterministic weight generator."""
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
import mamba_train_ref as R                                         # noqa: E402
from fnssl import weights as W                                      # noqa: E402


@pytest.fixture(scope="module")
def sd():
    return W.make_ipdnet2_state(0, num_layers=1)


@pytest.fixture(scope="module")
def f32_errors(sd):
    """{leg name: {tensor: err of the float32 restatement}} — computed once, shared."""
    return {leg[0]: R.leg_errors(sd, leg) for leg in R.legs()}


def test_leg_table_covers_the_shapes_it_names():
    legs = {l[0]: l for l in R.legs()}
    assert len(legs) == len(R.legs()) == 16 + 4 + 2 + 2 + 1 + 2
    assert sorted(l[3] for l in R.legs() if l[0].startswith("chunk")) == [R.TC - 1, R.TC, R.TC + 1, 2 * R.TC + 3]
    assert legs["many_seq"][1] * legs["many_seq"][2] == 528 and legs["real_pool5"][3:5] == (250, 5)


@pytest.mark.parametrize("pool,residual", [(1, False), (1, True), (5, True)])
def test_forward_is_the_float64_restatement(sd, pool, residual):
    rs = np.random.RandomState(3)
    x = rs.standard_normal((2, 3, 12, R.H))
    want, _ = R8.mamba_block(sd, "layers.0.norm_mhsa", "layers.0.mhsa", x, residual=residual, time_pool=pool)
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in R.block_params(sd).items()}
    got = R.forward(p, torch.tensor(x), residual, pool).numpy()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("pool", [1, 2])
def test_float64_gradients_are_the_finite_differences(sd, pool):
    """2 sequences x 5 frames; per tensor, three random directions v: <grad, v> against the central difference of the
    loss <out, dout> along v."""
    rs = np.random.RandomState(5)
    p = {k: v.astype(np.float64) for k, v in R.block_params(sd).items()}
    x = rs.standard_normal((1, 2, 5, R.H))
    dout = rs.standard_normal((1, 2, 5 // pool, R.H))
    _, g = R.gradients(p, x, dout, True, pool)

    def out_of(pp, xx):
        t = {k: torch.tensor(v, dtype=torch.float64) for k, v in pp.items()}
        return R.forward(t, torch.tensor(xx), True, pool).numpy()

    def central(name, base, v, h):
        # the difference is taken per output element BEFORE the sum with dout: the loss itself is ~1e2 and would bury a
        # gradient of 1e-5 in its rounding
        hi, lo = dict(p), dict(p)
        if name == "x":
            d = out_of(p, x + h * v) - out_of(p, x - h * v)
        else:
            hi[name], lo[name] = base + h * v, base - h * v
            d = out_of(hi, x) - out_of(lo, x)
        return float((d * dout).sum()) / (2 * h)

    for name in R.TENSORS:
        base = x if name == "x" else p[name]
        for _ in range(3):
            v = rs.standard_normal(base.shape)
            h = 2e-3 * max(1e-3, np.abs(base).max())
            fd = (4.0 * central(name, base, v, h / 2) - central(name, base, v, h)) / 3.0      # Richardson: O(h^4)
            an = float((g[name] * v).sum())
            scale = float(np.abs(g[name]).max() * np.abs(v).sum() / v.size ** 0.5)
            print("%-16s analytic %+.9e  finite difference %+.9e" % (name, an, fd))
            assert abs(an - fd) <= 1e-6 * max(abs(an), scale), (name, an, fd)


def test_committed_gate_table_is_what_float32_measures_here(f32_errors):
    """The project's reading of 'equal' for a measured float32 figure (test_ipdnet2_bf16_f64_ref_host.py): within a
    factor 2.  The reference pins itself to one thread, so the figures do not move with the host's thread count (which
    alone moved norm.weight by 4.6 x); what is left to the window is the host's vector width and math library."""
    assert sorted(R.GATE_F32) == sorted(R.TENSORS)
    for k in R.TENSORS:
        v, c = max(e[k] for e in f32_errors.values()), R.GATE_F32[k]
        print("%-16s committed %.3e  measured %.3e" % (k, c, v))
        assert 0.5 * c <= v <= 2.0 * c, "%s: committed %.3e, measured %.3e" % (k, c, v)


def test_float32_restatement_passes_its_own_gate_with_room(f32_errors):
    for name, e in f32_errors.items():
        for k in R.TENSORS:
            assert e[k] <= R.gate(k) / 4, (name, k, e[k])


def _mutant_legs(mutant):
    pick = {"carry_cut": ("chunk_nt%d" % (R.TC + 1), "chunk_nt%d" % (2 * R.TC + 3)),
            "ddt_decay": ("chunk_nt%d" % R.TC, "short_nt5_res_frame"),
            "conv_tap": ("short_nt4_res_frame", "chunk_nt%d" % R.TC),
            "softplus_branch": ("softplus_+25",),
            "pool_scale": ("pooled_nt5", "pooled_nt12")}[mutant]
    return [l for l in R.legs() if l[0] in pick]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_gate_sees_the_mutant(sd, mutant):
    """float64 with one mistake in the backward: some tensor of some leg must miss its gate."""
    worst = 0.0
    for leg in _mutant_legs(mutant):
        e = R.leg_errors(sd, leg, torch.float64, mutant)
        for k in R.TENSORS:
            print("%-16s %-22s %-16s err %.3e  gate %.3e" % (mutant, leg[0], k, e[k], R.gate(k)))
            worst = max(worst, e[k] / R.gate(k))
    assert worst > 1.0, "no tensor of any leg misses its gate under mutant %s (worst err / gate %.3g)" % (mutant, worst)


def test_mutants_leave_the_forward_alone(sd):
    leg = [l for l in R.legs() if l[0] == "pooled_nt12"][0]
    p = R.block_params(sd)
    x, dout = R.leg_inputs(leg)
    want, _ = R.gradients(p, x, dout, True, 5)
    for m in R.MUTANTS:
        got, _ = R.gradients(p, x, dout, True, 5, mutant=m)
        assert np.array_equal(got, want), m


def test_sigmoid_above_20_is_below_every_gate():
    """Why the softplus mutant is the wrong-branch one: the forward kernel's identity branch (dtv > 20) has derivative 1,
    and the plain sigmoid there differs from 1 by less than 2.1e-9 — a derivative 'forced to sigmoid' on that branch is
    the same gradient to every gate of the table, so no test could tell it apart."""
    assert 1.0 - 1.0 / (1.0 + np.exp(-20.0)) < 2.1e-9 < min(R.gate(k) for k in R.TENSORS)
