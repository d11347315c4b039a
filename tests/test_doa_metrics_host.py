"""Host-side checks of the DOA evaluation (no GPU): the float64 restatement (tests/doa_metric_ref.py) reproduces the real
reference's golden results (tests/golden/g20_doa_metrics.npz); its assignment against an exhaustive search and — where
scipy is installed — against ``linear_sum_assignment`` itself, ties included; the two new entry points are declared,
exported and validate their arguments before touching the device; the drop-in classes construct without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import doa_metric_ref as R
from conftest import load_golden
from fnssl import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fnssl_doa_metrics", "fnssl_ipd2doa_tracks")


def _close(got, want, what):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape and (np.isnan(got) == np.isnan(want)).all(), (what, got, want)
    ok = np.isnan(want) | (np.abs(got - want) <= 1e-5 * np.abs(want) + 1e-7)
    assert ok.all(), (what, got, want)


def _k(ref):
    return np.stack([ref["K_gt"], ref["K_est"], ref["K_corr"]])


@pytest.mark.parametrize("name", list(R.G20_SINGLE))
def test_restatement_reproduces_g20_single(name):
    g = load_golden("g20_doa_metrics")
    doa_gt, vad_gt, doa_est, vad_est = R.g20_single_inputs(name)
    ref = R.get_metric(R.degrees(doa_gt), vad_gt, R.degrees(doa_est), vad_est, "single", ("ele", "azi"), 5, True, (2 / 3, 2 / 3))
    _close(ref["ACC"], g[name + "_ACC"], name)
    _close([ref["MAE"]["ele"], ref["MAE"]["azi"]], g[name + "_MAE"], name)
    assert (_k(ref) == g[name + "_K"]).all()


@pytest.mark.parametrize("name", list(R.G20_MULTI_NAMES))
def test_restatement_reproduces_g20_multiple(name):
    g = load_golden("g20_doa_metrics")
    ref = R.get_metric(*R.g20_multi_inputs(name), "multiple", ("azi",), R.G20_AE_TH, True, R.G20_VAD_TH)
    _close([ref["ACC"], ref["MDR"], ref["FAR"], ref["MAE"]["azi"], ref["RMSE"]["azi"]], g[name + "_metric"], name)
    assert (_k(ref) == g[name + "_K"]).all()
    assert ref["gap"] > 1e-3 and ref["tie_safe"]


@pytest.mark.parametrize("name", list(R.G20_MICS))
def test_restatement_reproduces_g20_pred2doa(name):
    g = load_golden("g20_doa_metrics")
    mic, c = R.G20_MICS[name], R.G20_PRED[name]
    pred, doa_gt, vad_gt = R.g20_pred(mic, c["nb"], c["nt"], c["seed"])
    idx, doa, vad, scores = R.pred2doa(pred, mic)
    assert (idx == g[name + "_idx"]).all()
    _close(vad, g[name + "_vad"], name)
    top = np.sort(scores, axis=-1)
    assert ((top[..., -1] - top[..., -2]) > 1e-4 * np.abs(scores).max()).all()
    ref = R.get_metric(R.degrees(doa_gt), vad_gt, R.degrees(doa.astype(np.float32)), g[name + "_vad"], "multiple", ("azi",), 10, True,
                       (0.001, 0.5))
    _close([ref["ACC"], ref["MDR"], ref["FAR"], ref["MAE"]["azi"], ref["RMSE"]["azi"]], g[name + "_metric"], name)
    assert (_k(ref) == g[name + "_K"]).all()


def test_judge_assignment_cases():
    """3 x 2: two valid pairs survive; 4 x 3: the reference's position-for-row slip erases one of two valid pairs."""
    ref = R.get_metric(*R.judge_case(10), "multiple", ("azi",), 10, False)
    assert ref["K_gt"][0] == 6 and ref["K_est"][0] == 4 and ref["K_corr"][0] == 2
    gt, vg, est, ve = R.erase_case()
    az = R.azi_error(est[0, 0, 1][None, :].astype(np.float64), gt[0, 0, 1][:, None].astype(np.float64))
    cost = np.where(az > 10, 10000.0, az)
    rows, cols = R.lsap(cost)
    assert rows == [1, 2, 3] and cols == [1, 2, 0]
    assert sum(cost[r, c] != 10000 for r, c in zip(rows, cols)) == 2                  # two valid pairs ...
    assert R.judge_assignment(cost, rows, cols, 10000.0, 10) == [10, 10, 10, 0]      # ... one survives
    assert R.get_metric(gt, vg, est, ve, "multiple", ("azi",), 10, True, (0.001, 0.5))["K_corr"][0] == 1


def _random_costs(n):
    rng = np.random.RandomState(7)
    for k in range(n):
        r, c = rng.randint(1, 5, 2)
        if k % 2:
            yield rng.choice([1.0, 2.0, 2.5, 3.0, 10000.0, 10000.0], (r, c))           # tie-heavy
        else:
            yield np.where(rng.rand(r, c) < 0.4, 10000.0, rng.uniform(0, 10, (r, c)).astype(np.float32).astype(np.float64))


def test_lsap_restatement_is_optimal():
    for cost in _random_costs(2000):
        rows, cols = R.lsap(cost)
        tot, optimal, _gap = R.assign_exhaustive(cost)
        assert sorted(zip(rows, cols)) in optimal, (cost, rows, cols)
        assert rows == sorted(rows) and len(set(cols)) == len(cols) == min(cost.shape)


def test_assignment_against_scipy():
    """The exhaustive optimum equals linear_sum_assignment's total cost on 2000 random <= 4 x 4 matrices, and the
    restatement of its algorithm returns the SAME pairs, exact ties included."""
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    for cost in _random_costs(2000):
        r, c = lsa(cost)
        tot, _optimal, _gap = R.assign_exhaustive(cost)
        assert abs(cost[r, c].sum() - tot) <= 1e-9 * max(1.0, tot)
        rows, cols = R.lsap(cost)
        assert list(r) == rows and list(c) == cols, (cost, r, c, rows, cols)


def test_degrees_are_formed_by_true_division():
    """``x * 180 / np.pi`` on an fp32 tensor is an fp32 multiply and an fp32 DIVIDE on the host (what the kernel restates) —
    not a multiply by the reciprocal."""
    import torch
    x = (np.random.RandomState(3).rand(100000) * 3.2).astype(np.float32)
    got = (torch.from_numpy(x) * 180 / np.pi).numpy()
    assert (got == (x * np.float32(180)) / np.float32(np.pi)).all()


def test_symbols_declared_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fnssl.h")).read()
    declared = set(re.findall(r"\b(fnssl_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.fnssl_abi_version() == 19


def _metrics(lib, ptr=64, strides=True, shape=(2, 5, 2, 2), mode=1, ae=1, use_vad=1, large=10000.0, out=64):
    """Every pointer is the never-dereferenced address 64: each call must fail validation before any launch."""
    p = lambda v: C.c_void_p(v) if v else None                                       # noqa: E731
    s4 = (C.c_longlong * 4)(40, 8, 4, 1) if strides else None
    s3 = (C.c_longlong * 3)(20, 4, 1) if strides else None
    nb, nt, ns_gt, ns_est = shape
    rc = lib.fnssl_doa_metrics(p(ptr), s4, p(ptr), s3, p(ptr), s4, p(ptr), s3, nb, nt, ns_gt, ns_est, mode, ae, 10.0, 0.001, 0.5,
                               use_vad, 0, large, 1e-5, p(out), p(out), p(out), p(out), p(out), None)
    return rc, lib.fnssl_last_error().decode()


def test_doa_metrics_validates_before_launch():
    lib = _lib.load()
    for kw, word in (({"shape": (2, 5, 5, 2)}, "sources"), ({"shape": (2, 5, 2, 5)}, "sources"), ({"shape": (2, 5, 0, 2)}, "sources"),
                     ({"shape": (0, 5, 2, 2)}, "utterances"), ({"shape": (2, 0, 2, 2)}, "utterances"),
                     ({"ptr": 0}, "null"), ({"out": 0}, "null"), ({"strides": False}, "null"),
                     ({"mode": 2}, "unknown source mode"), ({"mode": -1}, "unknown source mode"),
                     ({"mode": 0, "shape": (2, 5, 2, 1)}, "single"),
                     ({"ae": 0}, "angle-error"), ({"ae": 8}, "angle-error"), ({"large": 100.0}, "large_number")):
        rc, msg = _metrics(lib, **kw)
        assert rc != 0 and word in msg, (kw, rc, msg)


def test_ipd2doa_tracks_validates_before_launch():
    lib = _lib.load()
    p = lambda v: C.c_void_p(v) if v else None                                       # noqa: E731

    def call(pred=64, bank=64, out=64, nb=2, np_=3, nt=4, nf2=512, ncand=180, nsrc=1, ntrack=2):
        rc = lib.fnssl_ipd2doa_tracks(p(pred), 1, 1, 1, 1, 1, p(bank), nb, np_, nt, nf2, ncand, nsrc, ntrack, 1, p(out), p(out), p(out),
                                      None)
        return rc, lib.fnssl_last_error().decode()
    for kw, word in (({"pred": 0}, "null"), ({"bank": 0}, "null"), ({"out": 0}, "null"), ({"ntrack": 0}, "tracks"),
                     ({"nb": 0}, "bad sizes"), ({"nsrc": 0}, "bad sizes"), ({"np_": 64}, "LDS")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    assert call(nt=0)[0] == 0                                                         # nothing to do, nothing launched


def test_drop_in_classes_construct_without_a_device():
    import Module as fn_module
    from IPDnet import Module as ip_module
    m = fn_module.getMetric(source_mode='single')
    assert m.source_mode == 'single' and m.inf == 10000 and m.eps == 1e-5
    with pytest.raises(ValueError):
        fn_module.getMetric(invalid_source_idx=2)
    pd = ip_module.PredDOA(mic_location=R.G20_MICS["mic4"], dev='cpu')
    assert tuple(pd.bank.shape) == (1, 180, 512, 3) and pd.max_track == 2
    bank, azi = R.template_bank(R.G20_MICS["mic4"])
    assert np.abs(pd.bank.numpy()[0].astype(np.float64) - bank).max() < 1e-6
    assert np.abs(pd.azi_candidate.numpy() - azi).max() < 1e-6
    with pytest.raises(ValueError):
        ip_module.PredDOA(mic_location=R.G20_MICS["mic2"], max_num_sources=2)
    with pytest.raises(NotImplementedError):
        pd.pred2DOA_track(None, None, time_pool_size=2)
