"""GPU tests of IPDnet2's evaluation on device: ``fnssl_ipd2doa_mse_tracks`` (csrc/doa.hip), ``fnssl_ipdnet2_targets``
(csrc/ipdnet_step.hip), ``fnssl_doa_metrics_ex`` (csrc/metrics.hip), their tensor fronts, the drop-in ``getMetric`` /
``DPIPD2`` / ``PredDOA`` of IPDnet2/Module.py and ``MyModel.validation_step`` / ``test_step`` of IPDnet2/run_step.py — against
the real reference's golden results (G21, tests/golden/make_golden_ipdnet2_eval.py) and the float64 restatement
(tests/ipdnet2_eval_ref.py).

Tolerances.
  * Search: indices are exact on G21 (the fixture keeps every argmin 1e-4 of the spectrum's maximum clear of the runner-up).
    On random inputs a score is a sum of <= 2048 non-negative fp32 terms (32 per lane, a six-level butterfly): 38 roundings
    of 6e-8, 2.3e-6 relative, inside the 1e-6 + 1e-5 |s| class tests/test_gpu_doa.py uses; the chosen candidate is a
    minimum within twice that, and the activity is held to 1e-4 |v| + 1e-6 of float64.
  * Targets against G21: G21_TARGET_DIFF = 4.62e-07 is the largest difference the golden script printed between the
    reference's targets and the float64 formula; the test allows 4 x that = 1.848e-06, which covers a kernel that rounds at
    other points of the same chain.
  * Targets against float64: the fp32 source position (sin / cos, two products: 3 roundings of 2^-24 relative) moves a
    path difference by at most b * 3 * 2^-24 for a microphone b from the reference microphone, whatever the distance, i.e.
    (2 pi f / c) * b * 1.8e-7 = 1.6e-6 rad at 8 kHz and b = 6 cm, plus 6e-8 for the fp32 result: 2e-6.
  * Metrics: counts exact, ratios within rtol 1e-5 (the order of fp32 sums, as tests/test_gpu_doa_metrics.py derives).
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import doa_metric_ref as R  # noqa: E402
import ipdnet2_eval_ref as R2  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G21_TARGET_DIFF = 4.62e-07                       # printed by tests/golden/make_golden_ipdnet2_eval.py
TARGET_ATOL_G21 = 4 * G21_TARGET_DIFF            # 1.848e-06
TARGET_ATOL_F64 = 2e-6                           # derived in the module docstring
MULTI = ("ACC", "MDR", "FAR", "MAE", "RMSE")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


def _load(rel, name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "fn-ssl_amd", *rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def module2():
    return _load(("IPDnet2", "Module.py"), "fnssl_ipdnet2_module_eval")


def run_step():
    return _load(("IPDnet2", "run_step.py"), "fnssl_ipdnet2_run_step_eval")


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def close(got, want, what, rtol=1e-5):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    print("CHECK %s: got %s want %s" % (what, got, want))
    assert got.shape == want.shape and (np.isnan(got) == np.isnan(want)).all(), (what, got, want)
    ok = np.isnan(want) | (np.abs(got - want) <= rtol * np.abs(want))
    assert ok.all(), (what, got, want)


def counts_of(gm):
    k = gm.last_counts
    return np.stack([k["K_gt"].cpu().numpy(), k["K_est"].cpu().numpy(), k["K_corr"].cpu().numpy()])


# --------------------------------------------------------------------------- the MSE search
@pytest.mark.parametrize("name", list(R2.G21_CASES))
def test_g21_search_and_metrics_through_preddoa(dev, name):
    """The reference's own indices (exact), activities and five metrics, through the drop-in PredDOA.forward."""
    g = load_golden("g21_ipdnet2_eval")
    d = R2.g21_inputs(name)
    M2 = module2()
    pd = M2.PredDOA(mic_location=d["mic"], dev="cuda:0")
    pred = to_dev(d["pred"], dev)
    gt_batch = [to_dev(d["azi_deg"], dev), to_dev(g[name + "_targets"], dev).view(-1, *g[name + "_targets"].shape[2:]), d["mic"],
                to_dev(d["distance"], dev), to_dev(d["vad"], dev)]
    pred_batch, _ = pd.pred2DOA(pred, gt_batch)
    doa, vad, pred_ipd = pred_batch
    nb, nt, nf2, nm1, ntrack = d["pred"].shape
    assert doa.shape == (nb, nt, 2, 2) and vad.shape == (nb, nt, 2) and pred_ipd.shape == (nb * nm1, nt, nf2, ntrack) and doa.is_cuda
    _bank, azi = R2.candidate_bank(d["mic"])
    want_azi = azi[g[name + "_idx"]].astype(np.float32).transpose(1, 2, 0)
    np.testing.assert_array_equal(doa[:, :, 1, :].cpu().numpy(), want_azi)
    np.testing.assert_array_equal(doa[:, :, 0, :].cpu().numpy(), np.full_like(want_azi, np.float32(np.pi / 2)))
    err = np.abs(vad.cpu().numpy().astype(np.float64) - g[name + "_vad"])
    print("CHECK %s activities: max abs err %.3g" % (name, err.max()))
    assert (err <= 1e-4 * np.abs(g[name + "_vad"]) + 1e-6).all()
    # one track at a time, the reference's re-batched layout
    for r in range(ntrack):
        trk, _ = pd.pred2DOA_track(pred_ipd[:, :, :, r], None)
        assert trk[0].shape == (nb, nt, 2, 1) and trk[1].shape == (nb, nt, 1) and trk[2].shape == (nb, nt, 1, 360)
        assert torch.equal(trk[0][..., 0], doa[..., r]) and torch.equal(trk[1][..., 0], vad[..., r])
        np.testing.assert_array_equal(trk[2].reshape(nb, nt, -1).argmin(-1).cpu().numpy(), g[name + "_idx"][r])
    metric = pd(pred, gt_batch, None)
    assert list(metric) == list(MULTI) and all(v.is_cuda and v.numel() == 1 for v in metric.values())
    np.testing.assert_array_equal(counts_of(pd.getmetric), g[name + "_K"])
    close([float(metric[k]) for k in MULTI], g[name + "_metric"], name)
    again = pd.evaluate(pred_batch=pred_batch, gt_batch=gt_batch, idx=3, dir_name="unused/")       # no dumps are written
    assert all(torch.equal(again[k], metric[k]) for k in MULTI) and not os.path.exists("unused")


def _random_problem(np_, nf2, ncand, ntrack, seed):
    rng = np.random.RandomState(seed)
    pred = np.tanh(rng.standard_normal((2, 3, nf2, np_, ntrack))).astype(np.float32)
    bank = rng.uniform(-1, 1, (1, ncand, nf2, np_)).astype(np.float32)
    return pred, bank


def _check_against_float64(pred, bank, idx, vad, ss, nsrc):
    """idx / vad [ntrack, nb, nt, nsrc], ss [ntrack, nb, nt, ncand] of the device against float64 scores of the same fp32
    inputs; from the second source on the float64 residual follows the DEVICE's choices, so only the arithmetic differs."""
    ntrack, nb, nt = idx.shape[:3]
    flat = bank.astype(np.float64).reshape(bank.shape[1], -1)
    res = pred.astype(np.float64).transpose(4, 0, 1, 2, 3).reshape(ntrack, nb, nt, -1)
    worst = 0.0
    for s in range(nsrc):
        sc = ((res[..., None, :] - flat) ** 2).mean(axis=-1)
        if s == 0:
            assert (np.abs(ss - sc) <= 1e-6 + 1e-5 * np.abs(sc)).all(), np.abs(ss - sc).max()
        low = sc.min(axis=-1)
        chosen = np.take_along_axis(sc, idx[..., s:s + 1], axis=-1)[..., 0]
        worst = max(worst, (chosen - low).max())
        assert (chosen <= low + 2 * (1e-6 + 1e-5 * np.abs(low))).all(), (s, (chosen - low).max())
        assert (np.abs(vad[..., s] - chosen) <= 1e-4 * np.abs(chosen) + 1e-6).all(), (s, np.abs(vad[..., s] - chosen).max())
        res = res - flat[idx[..., s]]
    return worst


@pytest.mark.parametrize("nsrc", [1, 2])
@pytest.mark.parametrize("ntrack", [1, 2])
@pytest.mark.parametrize("ncand", [360, 7])
@pytest.mark.parametrize("nf2", [512, 20])
@pytest.mark.parametrize("np_", [1, 4])
def test_search_against_float64(dev, np_, nf2, ncand, ntrack, nsrc):
    """nf2 * np = 20 or 80 is no multiple of 64 or 256; 7 candidates are fewer than one per lane and no multiple of the 4
    waves; 2 x 3 frames and two tracks are more than one workgroup in both grid dimensions."""
    from fnssl import metrics as M
    pred, bank = _random_problem(np_, nf2, ncand, ntrack, 4100 + np_ + nf2 + ncand + 10 * ntrack)
    idx, vad, ss = M.localize_tracks_mse(to_dev(pred, dev), to_dev(bank, dev), nsrc, "UnkNum")
    assert idx.shape == (ntrack, 2, 3, nsrc) and vad.shape == idx.shape and ss.shape == (ntrack, 2, 3, 1, ncand)
    assert idx.dtype == torch.int32 and idx.is_cuda
    idx, vad, ss = idx.cpu().numpy(), vad.cpu().numpy(), ss.cpu().numpy()[:, :, :, 0, :]
    assert (idx >= 0).all() and (idx < ncand).all()
    worst = _check_against_float64(pred, bank, idx, vad, ss, nsrc)
    print("CHECK search np %d nf2 %d ncand %d tracks %d nsrc %d: chosen candidate at most %.3g above the float64 minimum"
          % (np_, nf2, ncand, ntrack, nsrc, worst))
    _i, ones, _s = M.localize_tracks_mse(to_dev(pred, dev), to_dev(bank, dev), nsrc, "KNum")
    assert (ones == 1).all() and np.array_equal(_i.cpu().numpy(), idx)


def test_search_tie_and_nan_rules(dev):
    from fnssl import metrics as M
    pred, bank = _random_problem(4, 20, 7, 2, 4201)
    bank[0, 5] = bank[0, 2]                                                 # two identical rows: the lower index wins
    pred[:, :, :, :, 0] = bank[0, 2] + 0.01 * pred[:, :, :, :, 0]
    idx, vad, ss = M.localize_tracks_mse(to_dev(pred, dev), to_dev(bank, dev), 1, "UnkNum")
    ss = ss.cpu().numpy()[:, :, :, 0, :]
    assert (ss[0, :, :, 2] == ss[0, :, :, 5]).all() and (ss[0].argmin(-1) == 2).all()
    assert (idx.cpu().numpy()[0, :, :, 0] == 2).all()
    # a NaN score counts as the minimum and the first one wins
    nanbank = bank.copy()
    nanbank[0, 3, 7, 1] = np.nan
    nanbank[0, 6, 0, 0] = np.nan
    idx2, vad2, ss2 = M.localize_tracks_mse(to_dev(pred, dev), to_dev(nanbank, dev), 2, "UnkNum")
    ss2 = ss2.cpu().numpy()[:, :, :, 0, :]
    assert np.isnan(ss2[..., 3]).all() and np.isnan(ss2[..., 6]).all() and np.isfinite(ss2[..., [0, 1, 2, 4, 5]]).all()
    assert (idx2.cpu().numpy()[..., 0] == 3).all() and np.isnan(vad2.cpu().numpy()[..., 0]).all()
    assert (idx2.cpu().numpy()[..., 1] == 0).all()                           # the residual is NaN now: every score is, index 0
    nanpred = pred.copy()
    nanpred[1, 2, 11, 3, 1] = np.nan                                        # one frame of one track
    idx3, vad3, ss3 = M.localize_tracks_mse(to_dev(nanpred, dev), to_dev(bank, dev), 1, "UnkNum")
    idx3, vad3, ss3 = idx3.cpu().numpy()[..., 0], vad3.cpu().numpy()[..., 0], ss3.cpu().numpy()[:, :, :, 0, :]
    assert idx3[1, 1, 2] == 0 and np.isnan(vad3[1, 1, 2]) and np.isnan(ss3[1, 1, 2]).all()
    keep = np.ones(idx3.shape, bool)
    keep[1, 1, 2] = False
    assert (idx3[keep] == idx.cpu().numpy()[..., 0][keep]).all() and np.isfinite(ss3[keep]).all()
    assert torch.equal(M.localize_tracks_mse(to_dev(nanpred, dev), to_dev(bank, dev), 1, "KNum")[1], torch.ones_like(vad))


@pytest.mark.parametrize("nsrc", [1, 2])
def test_search_layouts_tracks_and_determinism(dev, nsrc):
    """The forward's [nb, nt, 2nf, nmic - 1, ntrack] output as a permuted view, its contiguous copy, one call per track and a
    second run all give the same bits."""
    from fnssl import metrics as M
    rng = np.random.RandomState(4301)
    base = to_dev(np.tanh(rng.standard_normal((2, 3, 2, 4, 512))).astype(np.float32), dev)
    view = base.permute(0, 1, 4, 3, 2)
    assert not view.is_contiguous()
    bank = to_dev(R2.candidate_bank(R2.G21_MICS["mic5"])[0].astype(np.float32)[None], dev)
    a = M.localize_tracks_mse(view, bank, nsrc, "UnkNum")
    b = M.localize_tracks_mse(view.contiguous(), bank, nsrc, "UnkNum")
    c = M.localize_tracks_mse(view, bank, nsrc, "UnkNum")
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    for r in range(2):
        one = M.localize_tracks_mse(view[..., r:r + 1], bank, nsrc, "UnkNum")
        for x, y in zip(a, one):
            assert torch.equal(x[r], y[0])
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- near-field targets
@pytest.mark.parametrize("name", list(R2.G21_CASES))
def test_g21_targets(dev, name):
    """fnssl_ipdnet2_targets on the fixture's fp32 DOAs / distances and float64 table against the reference's own targets,
    at 4 x the difference the golden script printed (1.848e-06); through the kernel front and through DPIPD2.forward."""
    from fnssl import ipdnet_step
    g = load_golden("g21_ipdnet2_eval")
    d = R2.g21_inputs(name)
    geo = ipdnet_step.ipdnet2_geometry(d["mic"], dev)
    got = ipdnet_step.ipdnet2_targets(to_dev(d["doa"], dev), to_dev(d["distance"], dev), None, geo["mic"], None)
    err = np.abs(got.cpu().numpy().astype(np.float64) - g[name + "_targets"])
    print("CHECK %s targets: max abs err vs the reference %.3g (allowed %.4g)" % (name, err.max(), TARGET_ATOL_G21))
    assert got.shape == g[name + "_targets"].shape and err.max() <= TARGET_ATOL_G21
    gen = module2().DPIPD2([1, 360], d["mic"], nf=257, fre_max=8000, ch_mode='M', speed=340, dev="cuda:0")
    template, ipd = gen(source_doa=d["doa"], source_distance=d["distance"])
    assert template.shape == (1, 360, 257, d["mic"].shape[0] - 1) and template.dtype == torch.complex64 and template.is_cuda
    assert ipd.shape == (2, 6, 257, d["mic"].shape[0] - 1, 2) and ipd.dtype == torch.complex64
    assert torch.equal(torch.cat((ipd.real[:, :, 1:], ipd.imag[:, :, 1:]), dim=2), got)
    assert (ipd[:, :, 0] == 1).all()
    bank, _azi = R2.candidate_bank(d["mic"])
    tb = torch.cat((template.real[0, :, 1:], template.imag[0, :, 1:]), dim=1).cpu().numpy()
    assert np.abs(tb - bank).max() < 2e-6 and (template[:, :, 0] == 1).all()


@pytest.mark.parametrize("nmic", [2, 5])
@pytest.mark.parametrize("nsrc", [1, 2])
def test_targets_against_float64_gating_and_far_field(dev, nsrc, nmic):
    from fnssl import ipdnet_step
    mic = R2.G21_MICS["mic2" if nmic == 2 else "mic5"]
    rng = np.random.RandomState(4400 + 10 * nmic + nsrc)
    nb, nt = 2, 5
    azi = rng.uniform(-np.pi, np.pi, (nb, nt, nsrc))
    doa = np.stack((np.full_like(azi, np.pi / 2), azi), axis=2).astype(np.float32)
    geo = ipdnet_step.ipdnet2_geometry(mic, dev)
    ns = geo["non_source"]
    assert np.abs(ns.cpu().numpy() - R2.bessel_target(mic)).max() < 1e-7
    far = ipdnet_step.ipdnet_targets(to_dev(doa, dev), None, geo["mic"].float(), None).cpu().numpy().astype(np.float64)
    b = np.sqrt(((mic[1:] - mic[0]) ** 2).sum(axis=1)).max()
    k = 2 * np.pi * 8000.0 / 340.0
    for dist_m in (0.3, 50.0):
        dist = np.full((nb, nt, nsrc), dist_m, np.float32)
        got = ipdnet_step.ipdnet2_targets(to_dev(doa, dev), to_dev(dist, dev), None, geo["mic"], ns)
        assert got.shape == (nb, nt, 512, nmic - 1, nsrc)
        got = got.cpu().numpy().astype(np.float64)
        err = np.abs(got - R2.nearfield_targets(doa, dist, mic)).max()
        gap = np.abs(got - far).max()
        print("CHECK targets nmic %d nsrc %d at %g m: max abs err vs float64 %.3g, |near - far field| max %.3g" % (nmic, nsrc, dist_m, err, gap))
        assert err <= TARGET_ATOL_F64
        assert np.abs(got - R2.farfield_targets(doa, mic)).max() >= gap - 4e-6
        if dist_m == 50.0:
            assert gap <= k * b * b / dist_m + 4e-6          # the second-order term of the path difference, k b^2 / (2 d), twice
        elif nmic == 5:
            assert gap > 0.05                                # clearly not the far field at 0.3 m
    # gating: vad > 0 keeps the target, vad <= 0 takes the non-source column, a NaN VAD gives NaN
    dist = rng.uniform(0.3, 3.0, (nb, nt, nsrc)).astype(np.float32)
    vad = np.empty((nb, nt, nsrc), np.float32)
    vad[0, :, 0] = vad[1, :, nsrc - 1] = [-1.0, 0.0, 1e-9, 1.0, np.nan]
    if nsrc == 2:
        vad[0, :, 1], vad[1, :, 0] = 1.0, 0.0
    args = (to_dev(doa, dev), to_dev(dist, dev))
    open_ = ipdnet_step.ipdnet2_targets(*args, None, geo["mic"], ns).cpu().numpy()
    gated = ipdnet_step.ipdnet2_targets(*args, to_dev(vad, dev), geo["mic"], ns, vad_th=0.0).cpu().numpy()
    table = ns.cpu().numpy()
    for bi in range(nb):
        for t in range(nt):
            for s in range(nsrc):
                v, got = vad[bi, t, s], gated[bi, t, :, :, s]
                if np.isnan(v):
                    assert np.isnan(got).all(), (bi, t, s)
                elif v > 0:
                    np.testing.assert_array_equal(got, open_[bi, t, :, :, s])
                else:
                    np.testing.assert_array_equal(got, table)
    want = R2.gate_targets(R2.nearfield_targets(doa, dist, mic), vad, R2.bessel_target(mic), 0.0)
    assert (np.isnan(want) == np.isnan(gated)).all() and np.nanmax(np.abs(gated - want)) <= TARGET_ATOL_F64
    again = ipdnet_step.ipdnet2_targets(*args, to_dev(vad, dev), geo["mic"], ns, vad_th=0.0).cpu().numpy()
    assert np.array_equal(again, gated, equal_nan=True)


# --------------------------------------------------------------------------- the metrics options
def _g21_metric_inputs(name, dev):
    g = load_golden("g21_ipdnet2_eval")
    d = R2.g21_inputs(name)
    _bank, azi = R2.candidate_bank(d["mic"])
    idx = g[name + "_idx"]
    doa_est = np.stack((np.full(idx.shape, np.pi / 2), azi[idx]), axis=0).astype(np.float32).transpose(2, 3, 0, 1)   # radians
    doa_gt = np.stack((d["azi_deg"], d["azi_deg"]), axis=2)                                                           # degrees
    vad_est = (g[name + "_vad"] / np.float32(0.2919)).astype(np.float32)
    return g, d, [to_dev(a, dev) for a in (doa_gt, d["vad"], doa_est, vad_est)], (doa_gt, d["vad"], doa_est, vad_est)


@pytest.mark.parametrize("name", list(R2.G21_CASES))
def test_metrics_options_on_g21(dev, name):
    from fnssl import metrics as M
    g, d, t, host = _g21_metric_inputs(name, dev)
    kw = dict(source_mode="multiple", ae_mode=("azi",), ae_TH=5, useVAD=True, vad_TH=(0.001, 0.4), radians=(False, True))
    m, kg, ke, kc = M.doa_metrics(*t, est_below=True, ratio_eps=1e-6, **kw)
    np.testing.assert_array_equal(np.stack([kg.cpu().numpy(), ke.cpu().numpy(), kc.cpu().numpy()]), g[name + "_K"])
    m = m.cpu().numpy()
    close([m[0], m[1], m[2], m[3], m[6]], g[name + "_metric"], name)
    # est_below flips exactly the gated set: the estimates active in frames with an active ground truth
    doa_gt, vad_gt, doa_est, vad_est = host
    for below in (True, False):
        ref = R2.get_metric2(doa_gt, vad_gt, R.degrees(doa_est), vad_est, est_below=below)
        mm, kg, ke, kc = M.doa_metrics(*t, est_below=below, ratio_eps=1e-6, **kw)
        np.testing.assert_array_equal(np.stack([kg.cpu().numpy(), ke.cpu().numpy(), kc.cpu().numpy()]),
                                      np.stack([ref["K_gt"], ref["K_est"], ref["K_corr"]]))
        mm = mm.cpu().numpy()
        want = R2.metric_vector(ref)
        close(mm[:3], want[:3], "%s est_below=%s ACC MDR FAR" % (name, below))
        # MAE / RMSE against FLOAT64 errors: the kernel forms an error as the reference does, in fp32 around 180 + error
        # (degrees of the estimate, est - gt + 180, the remainder: three roundings of half an fp32 step of 360, 1.5e-5 each)
        assert abs(mm[3] - want[3]) <= 1e-4 and abs(mm[6] - want[4]) <= 1e-4, (name, below, mm, want)
    some = (vad_gt > 0.001).any(axis=2, keepdims=True)
    n_below, n_above = ((vad_est < np.float32(0.4)) & some).sum(), ((vad_est > np.float32(0.4)) & some).sum()
    assert n_below + n_above == some.sum() * 2 and n_below > 0 and n_above > 0
    ref_b, ref_a = (R2.get_metric2(doa_gt, vad_gt, R.degrees(doa_est), vad_est, est_below=x) for x in (True, False))
    assert ref_b["K_est"].sum() == n_below and ref_a["K_est"].sum() == n_above
    # ratio_eps: 0 leaves a silent utterance's 0 / 0 = NaN, 1e-6 turns it into 0
    m0 = M.doa_metrics(*t, est_below=True, ratio_eps=0.0, **kw)[0].cpu().numpy()
    silent = (g[name + "_K"][0] == 0).any()
    assert silent == (name == "mic5_silent") and np.isnan(m0[:3]).all() == silent and np.isfinite(m[:3]).all()
    if not silent:
        close(m0[:3], m[:3], name + " without ratio_eps", rtol=1e-5)
    a = M.doa_metrics(*t, est_below=True, ratio_eps=1e-6, **kw)
    b = M.doa_metrics(*t, est_below=True, ratio_eps=1e-6, **kw)
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))       # two runs, the same bits


def test_old_metrics_entry_is_the_new_one_with_the_old_meaning(dev):
    """fnssl_doa_metrics on a G20 case: the golden values as before, and the same bits as fnssl_doa_metrics_ex with
    est_below = 0, ratio_eps = 0 and one unit for both sides (NaNs of the silent utterance included)."""
    import ctypes as C

    from fnssl import _lib
    from fnssl import metrics as M
    g = load_golden("g20_doa_metrics")
    name = "multi_2x2"
    t = [to_dev(a, dev) for a in R.g20_multi_inputs(name)]
    m, kg, ke, kc = M.doa_metrics(t[0], t[1], t[2], t[3], "multiple", ("azi",), R.G20_AE_TH, True, R.G20_VAD_TH, False)
    np.testing.assert_array_equal(np.stack([kg.cpu().numpy(), ke.cpu().numpy(), kc.cpu().numpy()]), g[name + "_K"])
    mh = m.cpu().numpy()
    close([mh[0], mh[1], mh[2], mh[3], mh[6]], g[name + "_metric"], name)
    assert np.isnan(mh[:3]).all()
    lib = _lib.load()
    out = torch.empty(9, dtype=torch.float32, device=dev)
    per = torch.empty((4, 9), dtype=torch.float32, device=dev)
    cnt = torch.empty((3, 4), dtype=torch.int32, device=dev)
    st = lambda x, n: (C.c_longlong * n)(*x.stride())                                 # noqa: E731
    p = lambda x: C.c_void_p(x.data_ptr())                                            # noqa: E731
    with torch.cuda.device(dev):
        rc = lib.fnssl_doa_metrics_ex(p(t[0]), st(t[0], 4), p(t[1]), st(t[1], 3), p(t[2]), st(t[2], 4), p(t[3]), st(t[3], 3), 4, 8, 2, 2,
                                      1, 1, float(R.G20_AE_TH), float(R.G20_VAD_TH[0]), float(R.G20_VAD_TH[1]), 1, 0, 0, 0, 0.0,
                                      10000.0, 1e-5, p(out), p(per), p(cnt[0]), p(cnt[1]), p(cnt[2]),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.fnssl_last_error()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == mh.tobytes()
    np.testing.assert_array_equal(cnt.cpu().numpy(), g[name + "_K"])
    # the tensor front takes the _ex path for a (gt, est) pair of units: same bits again
    m2 = M.doa_metrics(t[0], t[1], t[2], t[3], "multiple", ("azi",), R.G20_AE_TH, True, R.G20_VAD_TH, (False, False))[0]
    assert m2.cpu().numpy().tobytes() == mh.tobytes()


# --------------------------------------------------------------------------- end to end
def _batch(nt_targets, seed=4501, nb=2, nsrc=2):
    rng = np.random.RandomState(seed)
    mic = R2.G21_MICS["mic5"]
    sig = (rng.standard_normal((nb, 16000, 5)) * 0.05).astype(np.float32)             # 1 s: 51 frames, 10 after the network
    azi = rng.uniform(-170.0, 170.0, (nb, nt_targets, nsrc)).astype(np.float32)
    vad = (rng.rand(nb, nt_targets, nsrc) < 0.8).astype(np.float32)
    vad[:, :4, 0] = 1.0                                                               # every utterance has active ground truth
    vad[:, :4, 1] = 1.0
    dist = rng.uniform(0.5, 3.0, (nb, nt_targets, nsrc)).astype(np.float32)
    geo = np.repeat(mic[None], nb, axis=0)
    T = torch.from_numpy
    return [T(sig), T(azi), T(vad), T(geo), T(dist)]


@pytest.fixture(scope="module")
def model(dev):
    from fnssl import weights as W
    m = run_step().MyModel(device="cuda:0")
    m.arch.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in W.make_ipdnet2_state(4601).items()})
    return m.to(dev).eval()


@pytest.mark.parametrize("nt_targets", [10, 8, 12])
def test_validation_and_test_step_end_to_end(dev, model, nt_targets):
    """2 utterances of 1 s on the 5-microphone array: the prediction has 10 frames; targets of 10 (equal), 8 (prediction
    longer: it is cut) and 12 frames (prediction shorter: every utterance's targets are cut)."""
    from fnssl import ipdnet_step
    M2 = module2()
    batch = [x.to(dev) for x in _batch(nt_targets)]
    nt = min(10, nt_targets)
    loss = model.validation_step(batch, 0)
    valid = model.last_metrics
    assert loss.is_cuda and loss.shape == () and torch.isfinite(loss)
    assert list(valid) == list(MULTI) and all(v.is_cuda and v.numel() == 1 for v in valid.values())
    # the same tensors by hand
    pred, gt = model._forward_aligned(batch)
    assert pred.shape == (2, nt, 512, 4, 2) and gt[0].shape == (2, nt, 2) and gt[1].shape == (2 * nt, 512, 4, 2)
    assert gt[-1].shape == (2, nt, 2) and gt[-2].shape == (2, nt, 2) and isinstance(gt[-3], np.ndarray) and gt[-3].dtype == np.float64
    want = ipdnet_step.pit_mse(pred, gt[1])[0]
    assert abs(float(loss) - float(want)) <= 1e-6 * abs(float(want))
    by_hand = M2.PredDOA(mic_location=gt[-3], dev="cuda:0")(pred_batch=pred, gt_batch=gt, idx=None)
    assert all(torch.equal(by_hand[k], valid[k]) for k in MULTI)
    vals = {k: float(valid[k]) for k in MULTI}
    print("CHECK end to end nt_targets %d: loss %.6g metrics %s" % (nt_targets, float(loss), vals))
    assert all(np.isfinite(v) for v in vals.values()) and abs(vals["ACC"] + vals["MDR"] - 1.0) <= 1e-6
    # the targets are the kernel's, cut per utterance
    full = model.data_preprocess(batch[0], batch[1], batch[3], batch[2], batch[4])
    assert full[0].shape == (2, 10, 256, 51) and full[2].shape == (2 * nt_targets, 512, 4, 2)
    assert torch.equal(full[2].view(2, nt_targets, 512, 4, 2)[:, :nt].reshape(2 * nt, 512, 4, 2), gt[1])
    # test_step: same loss, same metrics, and cal_loss's permuted prediction
    loss_t = model.test_step(batch, 7)
    assert torch.equal(loss_t, loss) and all(torch.equal(model.last_metrics[k], valid[k]) for k in MULTI)
    l3, ipd_gt, pred_perm = model.cal_loss(pred_batch=pred, gt_batch=gt, mode='test')
    D = 512 * 4
    assert torch.equal(l3, loss) and ipd_gt.shape == (2 * nt, 2, D) and pred_perm.shape == (2 * nt, 2, D)
    flat = pred.reshape(2 * nt, D, 2).permute(0, 2, 1)
    same = (pred_perm == flat).all(dim=2).all(dim=1)
    swapped = (pred_perm == flat.flip(1)).all(dim=2).all(dim=1)
    assert (same | swapped).all()
    e_id = ((flat - ipd_gt) ** 2).sum(dim=(1, 2))
    e_sw = ((flat.flip(1) - ipd_gt) ** 2).sum(dim=(1, 2))
    clear = (e_id - e_sw).abs() > 1e-4 * (e_id + e_sw)
    assert (same[clear] == (e_id < e_sw)[clear]).all()
    assert abs(float(((pred_perm - ipd_gt) ** 2).mean()) - float(loss)) <= 1e-5 * float(loss)
    # two runs give the same bits
    again = model.validation_step(batch, 0)
    assert torch.equal(again, loss) and all(torch.equal(model.last_metrics[k], valid[k]) for k in MULTI)


def test_predict_step_and_forward_only_training(dev, model):
    batch = [x.to(dev) for x in _batch(10)]
    out = model.predict_step(batch[0].permute(0, 2, 1), 0)
    assert out.shape == (10, 512, 4, 2) and torch.isfinite(out).all()
    assert torch.equal(out, model._forward_aligned(batch)[0][0])
    model.train()
    try:
        with pytest.raises(Exception, match="(?i)forward-only|eval"):
            model.training_step(batch, 0)
    finally:
        model.eval()
