#!/usr/bin/env python3
"""G21: IPDnet2 evaluation results from the REAL reference (build container only: needs /root/reference and scipy).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ipdnet2_eval.py

Imports the reference's own ``IPDnet2/Module.py`` (``soundfile`` / ``webrtcvad`` stubbed as in make_golden_doa_metrics.py)
and CALLS, on inputs drawn from seeds (tests/ipdnet2_eval_ref.py: a 2- and a 5-microphone array, 2 utterances x 6 frames x
2 sources, distances 0.3 - 3 m, noisy DP-IPDs, a silent utterance, frames with one active source, activities on both
sides of 0.4 * 0.2919):

  (a) ``DPIPD2(...).forward(source_doa, source_distance)`` with numpy float32 DOAs / distances and a float64 table, as
      run_IPDnet2.py:290-296 hands them -> the near-field targets [cos | sin] of bins 1..256, float32;
  (b) ``PredDOA(dev='cpu').pred2DOA`` / ``pred2DOA_track`` -> the MSE spectrum's argmin and the MSE activities;
  (c) ``PredDOA.evaluate`` -> ``getMetric`` with IPDnet2's rules -> ACC, MDR, FAR, MAE, RMSE.

run_IPDnet2.py itself cannot be imported (it opens datasets at import), so its gating and Bessel fill are not taken from
it: tests check them against the float64 restatement, and this script checks the restatement's Bessel table against
``scipy.special.jn``.

Only results are stored, and only data is written.  The integer counts stored beside the reference's metrics come from the
float64 restatement, AFTER the script has asserted that the restatement reproduces every metric of the reference.

The script asserts that the fixture is well-posed (conditions, not measurements; no case is left out):
  * every argmin beats the runner-up by more than 1e-4 of the spectrum's largest value;
  * no activity lies within 1e-4 of 0.4 * 0.2919 and no label VAD within 1e-6 of its threshold;
  * in every assignment the best total and the nearest different total are more than 1e-3 degrees apart, exactly tied optima
    agree on their valid pairs, and no azimuth error lies within 1e-3 degrees of ``ae_TH`` (the rules of
    make_golden_doa_metrics.py).

It also prints the largest difference between the reference's targets and a float64 evaluation of the same formula from the
same fp32 inputs.  Measured on the three cases: 4.45e-07 (mic2), 2.86e-07 (mic5), 4.62e-07 (mic5_silent); the largest,
4.62e-07, is the figure tests/test_gpu_ipdnet2_eval.py derives its target tolerance from (the fp32 source position is
what it measures: an fp32 step of a 3 m coordinate is 2.4e-07 m, a few 1e-07 rad of phase at 8 kHz).
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

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy.optimize import linear_sum_assignment  # noqa: E402
from scipy.special import jn  # noqa: E402

import doa_metric_ref as R  # noqa: E402
import ipdnet2_eval_ref as R2  # noqa: E402


def load_reference(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


IP2 = load_reference("/root/reference/IPDnet2/Module.py", "ref_ipdnet2_module")


def check_lsap_against_scipy():
    inner = R.lsap

    def checked(cost):
        rows, cols = inner(cost)
        r, c = linear_sum_assignment(np.asarray(cost, dtype=np.float64))
        assert list(r) == rows and list(c) == cols, (cost, rows, cols, r, c)
        return rows, cols
    R.lsap = checked


def close(a, b, name):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    assert a.shape == b.shape and (np.isnan(a) == np.isnan(b)).all(), (name, a, b)
    ok = np.isnan(a) | (np.abs(a - b) <= 1e-5 * np.abs(b) + 1e-7)
    assert ok.all(), (name, a, b)


def one_case(name, arrs):
    """Runs the reference on case ``name``, asserts the conditions, stores the results; returns the target difference."""
    T = torch.from_numpy
    k = list(range(1, 257))
    if True:
        d = R2.g21_inputs(name)
        mic = d["mic"]
        assert mic.dtype == np.float64 and d["doa"].dtype == np.float32 and d["distance"].dtype == np.float32
        # the Bessel table of the restatement against scipy
        bess = np.concatenate([np.concatenate((jn(0, 2 * np.pi * np.linspace(0, 8000, 257)[k] / 340 * dist), np.zeros(256)))[:, None]
                               for dist in np.sqrt(np.sum((mic[1:] - mic[0]) ** 2, axis=1))], axis=1)
        assert np.abs(R2.bessel_target(mic) - bess).max() < 1e-12, name
        # ---- (a) near-field targets ----
        gen = IP2.DPIPD2(ndoa_candidate=[1, R2.RES_PHI], mic_location=mic, nf=257, fre_max=8000.0, ch_mode='M', speed=340)
        _tmpl, ipd = gen(source_doa=d["doa"], source_distance=d["distance"])
        tgt = np.concatenate((ipd.real[:, :, k, :, :], ipd.imag[:, :, k, :, :]), axis=2).astype(np.float32)
        diff = np.abs(tgt.astype(np.float64) - R2.nearfield_targets(d["doa"], d["distance"], mic)).max()
        far = np.abs(tgt.astype(np.float64) - R2.farfield_targets(d["doa"], mic)).max()
        print(name, "targets %s: |reference - float64| max %.3g; |near - far field| max %.3g" % (tgt.shape, diff, far))
        assert far > 0.01, name                                                  # the near field matters at these distances
        # ---- (b) MSE search ----
        pd = IP2.PredDOA(dev='cpu', mic_location=mic)
        gt_batch = [T(d["azi_deg"]), T(tgt).view(-1, *tgt.shape[2:]), mic, T(d["distance"]), T(d["vad"])]
        pred_batch, _ = pd.pred2DOA(T(d["pred"]), gt_batch)
        doa_est, vad_est = pred_batch[0].numpy(), pred_batch[1].numpy()
        nb, nt, nf2, nm1, ntrack = d["pred"].shape
        idx = np.empty((ntrack, nb, nt), np.int32)
        for r in range(ntrack):
            trk, _ = pd.pred2DOA_track(pred_batch[2][:, :, :, r], None)
            ss = trk[2].numpy().reshape(nb, nt, -1)
            idx[r] = ss.argmin(-1)
            low = np.sort(ss, axis=-1)
            assert ((low[..., 1] - low[..., 0]) > 1e-4 * np.abs(ss).max()).all(), (name, (low[..., 1] - low[..., 0]).min(), ss.max())
            assert (trk[0].numpy()[:, :, :, 0] == doa_est[:, :, :, r]).all() and (trk[1].numpy()[:, :, 0] == vad_est[:, :, r]).all()
        bank, azi = R2.candidate_bank(mic)
        ridx, rvad, _ss, _ = R2.mse_search(d["pred"], bank)
        assert (ridx[..., 0] == idx).all(), name
        close(rvad[..., 0].transpose(1, 2, 0), vad_est, name)
        assert (azi[idx].astype(np.float32).transpose(1, 2, 0) == doa_est[:, :, 1, :]).all(), name
        act = vad_est.astype(np.float64)
        assert np.abs(act - 0.4 * 0.2919).min() > 1e-4, (name, np.abs(act - 0.4 * 0.2919).min())
        assert (act < 0.4 * 0.2919).any() and (act > 0.4 * 0.2919).any(), name
        # ---- (c) evaluation ----
        metric = pd.evaluate(pred_batch=pred_batch, gt_batch=gt_batch, idx=None)
        got = np.array([float(metric[m]) for m in ("ACC", "MDR", "FAR", "MAE", "RMSE")], np.float32)
        ref = R2.evaluate(doa_est, vad_est, d["azi_deg"], d["vad"])
        assert ref["gap"] > 1e-3 and ref["tie_safe"], (name, ref["gap"], ref["tie_safe"])
        assert ref["th_margin"] > 1e-3 and ref["vad_margin"] > 1e-6, (name, ref["th_margin"], ref["vad_margin"])
        close(R2.metric_vector(ref), got, name)
        counts = np.stack([ref["K_gt"], ref["K_est"], ref["K_corr"]]).astype(np.int32)
        arrs[name + "_targets"], arrs[name + "_idx"], arrs[name + "_vad"] = tgt, idx, vad_est
        arrs[name + "_metric"], arrs[name + "_K"] = got, counts
        print(name, got, "K", counts.tolist(), "active estimates %d / %d" % (ref["active_est"].sum(), vad_est.size))
    return diff


def main():
    check_lsap_against_scipy()
    arrs = {}
    worst = max(one_case(name, arrs) for name in R2.G21_CASES)
    silent = arrs["mic5_silent_K"]
    assert silent[0, 1] == 0 and silent[0, 0] > 0, silent                        # the + 1e-6 rule: that utterance gives 0, not NaN
    assert np.isfinite(arrs["mic5_silent_metric"]).all()
    print("largest |reference targets - float64|: %.3g" % worst)
    out = os.path.join(HERE, "g21_ipdnet2_eval.npz")
    np.savez_compressed(out, **arrs)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
