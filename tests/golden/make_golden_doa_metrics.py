#!/usr/bin/env python3
"""G20: DOA evaluation results from the REAL reference (build container only: needs /root/reference and scipy).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_doa_metrics.py

Imports the reference's own ``FN-SSL/Lightning/Module.py`` and ``IPDnet/Module.py`` (``soundfile`` / ``webrtcvad`` are
stubbed like in make_golden_ipdnet_step.py) and runs, on inputs drawn from seeds (tests/doa_metric_ref.py):

  (a) FN-SSL ``PredDOA(device='cpu').evaluate`` -> ``getMetric('single')``, 1 and 2 sources, radians in;
  (b) IPDnet ``getMetric('multiple')`` called directly, in degrees: 2 x 2 with a silent utterance (NaN) and segments without an
      estimate, rectangular 1 x 2, 2 x 1, 3 x 2, 2 x 3, errors one fp32 step below / at / above ``ae_TH`` and VADs at the
      thresholds, the 3 x 2 ``judge_assignment`` case and the 4 x 3 case in which it erases a valid pair;
  (c) IPDnet ``PredDOA(dev='cpu').pred2DOA`` + ``evaluate`` on noisy DP-IPDs for a 2- and a 4-microphone array.

Only results are stored, and only data is written.  The integer counts stored beside the reference's metrics come from the
float64 restatement, AFTER the script has asserted that the restatement reproduces every metric of the reference.

The script asserts that the fixture is well-posed (conditions, not measurements; no case is left out):
  * every stored argmax beats the runner-up by more than 1e-4 of the spectrum's largest value;
  * in every assignment the best total and the nearest DIFFERENT total are more than 1e-3 degrees apart, and assignments
    that tie exactly agree on their valid pairs.  Exact ties cannot be excluded: with more ground truths than estimates an
    estimate that is invalid for every free row costs 10000 whichever takes it.  Those ties are not decided by rounding
    but by the steps of linear_sum_assignment, which tests/doa_metric_ref.lsap restates and this script checks against
    scipy's answer on every matrix it meets;
  * no azimuth error of a random case lies within 1e-3 degrees of ``ae_TH`` and no VAD within 1e-6 of its threshold (the
    threshold case is exact in fp32 by construction instead).
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
for name in ("soundfile", "webrtcvad"):
    sys.modules.setdefault(name, types.ModuleType(name))
try:
    import matplotlib.pyplot  # noqa: F401  (FN-SSL's Module.py imports it for visDOA)
except Exception:
    mpl = types.ModuleType("matplotlib")
    mpl.pyplot = types.ModuleType("matplotlib.pyplot")
    sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, mpl.pyplot

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy.optimize import linear_sum_assignment  # noqa: E402

import doa_metric_ref as R  # noqa: E402


def load_reference(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FN = load_reference("/root/reference/FN-SSL/Lightning/Module.py", "ref_fnssl_module")
IP = load_reference("/root/reference/IPDnet/Module.py", "ref_ipdnet_module")


def check_lsap_against_scipy():
    """R.assign is called for every cost matrix of the fixture; make each of those calls compare with scipy's pairs."""
    inner = R.lsap

    def checked(cost):
        rows, cols = inner(cost)
        r, c = linear_sum_assignment(np.asarray(cost, dtype=np.float64))
        assert list(r) == rows and list(c) == cols, (cost, rows, cols, r, c)
        return rows, cols
    R.lsap = checked


def well_posed(ref, name, random_case):
    # "gap": the nearest DIFFERENT total; exactly tied optima are allowed only when they agree on their valid pairs, i.e.
    # differ in which row takes a 10000-cost estimate (unavoidable with more ground truths than estimates).  Those ties are
    # decided by linear_sum_assignment's steps, and the stored 3 x 2 / 4 x 3 counts depend on R.lsap following them: that is
    # why check_lsap_against_scipy() compares every matrix of the fixture with scipy's own pairs.
    assert ref["gap"] > 1e-3 and ref["tie_safe"], (name, ref["gap"], ref["tie_safe"])
    if random_case:
        assert ref["th_margin"] > 1e-3 and ref["vad_margin"] > 1e-6, (name, ref["th_margin"], ref["vad_margin"])


def close(a, b, name):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    assert a.shape == b.shape and (np.isnan(a) == np.isnan(b)).all(), (name, a, b)
    ok = np.isnan(a) | (np.abs(a - b) <= 1e-5 * np.abs(b) + 1e-7)
    assert ok.all(), (name, a, b)


def counts(ref):
    return np.stack([ref["K_gt"], ref["K_est"], ref["K_corr"]]).astype(np.int32)


def main():
    check_lsap_against_scipy()
    arrs = {}
    T = torch.from_numpy
    # ---- (a) FN-SSL 'single' through PredDOA.evaluate ----
    fn_pred = FN.PredDOA(device="cpu")
    for name in R.G20_SINGLE:
        doa_gt, vad_gt, doa_est, vad_est = R.g20_single_inputs(name)
        setting = {'ae_mode': ['ele', 'azi'], 'ae_TH': 5, 'useVAD': True, 'vad_TH': [2 / 3, 2 / 3], 'metric_unfold': False}
        got = fn_pred.evaluate(pred={'doa': T(doa_est), 'vad_sources': T(vad_est)}, gt={'doa': T(doa_gt), 'vad_sources': T(vad_gt)},
                               metric_setting=setting)
        ref = R.get_metric(R.degrees(doa_gt), vad_gt, R.degrees(doa_est), vad_est, "single", ("ele", "azi"), 5, True, (2 / 3, 2 / 3))
        assert ref["th_margin"] > 1e-3 and ref["vad_margin"] > 1e-6, (name, ref["th_margin"], ref["vad_margin"])
        close(ref["ACC"], got["ACC"].numpy(), name)
        close([ref["MAE"]["ele"], ref["MAE"]["azi"]], got["MAE"].numpy(), name)
        arrs[name + "_ACC"] = got["ACC"].numpy().astype(np.float32)
        arrs[name + "_MAE"] = got["MAE"].numpy().astype(np.float32)                      # (ele, azi): the reference's order
        arrs[name + "_K"] = counts(ref)
        print(name, "ACC %.4f MAE" % float(got["ACC"]), got["MAE"].numpy(), "K", counts(ref).sum(axis=1))
    # ---- (b) IPDnet 'multiple', direct calls in degrees ----
    ip_metric = IP.getMetric(source_mode='multiple', metric_unfold=True)
    for name in R.G20_MULTI_NAMES:
        doa_gt, vad_gt, doa_est, vad_est = R.g20_multi_inputs(name)
        got = ip_metric(T(doa_gt), T(vad_gt), T(doa_est), T(vad_est), ae_mode=['azi'], ae_TH=R.G20_AE_TH, useVAD=True,
                        vad_TH=list(R.G20_VAD_TH))
        got = np.array([float(g) for g in got], np.float32)                              # ACC, MDR, FAR, MAE, RMSE
        ref = R.get_metric(doa_gt, vad_gt, doa_est, vad_est, "multiple", ("azi",), R.G20_AE_TH, True, R.G20_VAD_TH)
        well_posed(ref, name, name in R.G20_MULTI)
        close([ref["ACC"], ref["MDR"], ref["FAR"], ref["MAE"]["azi"], ref["RMSE"]["azi"]], got, name)
        arrs[name + "_metric"] = got
        arrs[name + "_K"] = counts(ref)
        print(name, got, "K", counts(ref).sum(axis=1))
    assert np.isnan(arrs["multi_2x2_metric"][:3]).all() and np.isnan(arrs["multi_2x3_metric"][:3]).all()
    assert arrs["multi_erase_K"][2, 0] == 1 and arrs["multi_judge_K"][2, 0] == 2
    assert list(arrs["multi_threshold_K"][:, 0]) == [5, 4, 3], arrs["multi_threshold_K"]
    # ---- (c) IPDnet pred2DOA + evaluate ----
    for name, mic in R.G20_MICS.items():
        c = R.G20_PRED[name]
        pred, doa_gt, vad_gt = R.g20_pred(mic, c["nb"], c["nt"], c["seed"])
        pd = IP.PredDOA(dev='cpu', mic_location=mic.astype(np.float64))
        pred_batch, _ = pd.pred2DOA(T(pred), [T(doa_gt), T(vad_gt)])
        metric = pd.evaluate(pred_batch=pred_batch, gt_batch=[T(doa_gt), T(vad_gt)])
        got = np.array([float(metric[k]) for k in ("ACC", "MDR", "FAR", "MAE", "RMSE")], np.float32)
        doa_est, vad_est = pred_batch[0].numpy(), pred_batch[1].numpy()
        nb, nt, nf2, nmic, ntrack = pred.shape
        idx = np.empty((nb, nt, ntrack), np.int32)
        for r in range(ntrack):                                                           # the spectrum of each track
            trk, _ = pd.pred2DOA_track(pred_batch[2][:, :, :, r], None)
            ss = trk[2].numpy().reshape(nb, nt, -1)
            idx[:, :, r] = ss.argmax(-1)
            top = np.sort(ss, axis=-1)
            assert ((top[..., -1] - top[..., -2]) > 1e-4 * np.abs(ss).max()).all(), name
            assert (trk[0].numpy()[:, :, :, 0] == doa_est[:, :, :, r]).all() and (trk[1].numpy()[:, :, 0] == vad_est[:, :, r]).all()
        ridx, rdoa, rvad, _ = R.pred2doa(pred, mic)
        assert (ridx == idx).all(), name
        close(rvad, vad_est, name)
        assert np.abs(vad_est.astype(np.float64) - 0.5).min() > 1e-4, name              # estimated VADs away from vad_TH[1]
        ref = R.get_metric(R.degrees(doa_gt), vad_gt, R.degrees(doa_est), vad_est, "multiple", ("azi",), 10, True, (0.001, 0.5))
        well_posed(ref, name, True)
        close([ref["ACC"], ref["MDR"], ref["FAR"], ref["MAE"]["azi"], ref["RMSE"]["azi"]], got, name)
        arrs[name + "_idx"], arrs[name + "_vad"], arrs[name + "_metric"], arrs[name + "_K"] = idx, vad_est, got, counts(ref)
        print(name, got, "K", counts(ref).sum(axis=1), "active estimates %d / %d" % ((vad_est > 0.5).sum(), vad_est.size))
    out = os.path.join(HERE, "g20_doa_metrics.npz")
    np.savez_compressed(out, **arrs)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
