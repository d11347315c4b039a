"""GPU tests of the DOA evaluation (csrc/metrics.hip, ``fnssl_ipd2doa_tracks`` of csrc/doa.hip, fnssl/metrics.py, the
drop-in ``getMetric`` / ``PredDOA`` classes and the two modules' ``validation_step`` / ``test_step``): the real reference's
golden results (G20, tests/golden/make_golden_doa_metrics.py), the float64 restatement (tests/doa_metric_ref.py) at the
real validation sizes, layouts, source counts, determinism and the end-to-end steps.

Tolerances.  Counts are integers and exact.  Every azimuth / elevation error and every decision is formed by the
reference's fp32 operations in its order, so a metric differs from the reference's only by the ORDER of its fp32 sums:
a lane adds at most ceil(nt / 64) terms, a six-level butterfly closes the utterance, and the batch stage repeats that
over utterances — at most (13 + 6) + (1 + 6) = 26 roundings of 6e-8 on a sum of non-negative terms, 1.6e-6, against the
reference's own sequential or pairwise order of the same size; rtol 1e-5 covers both.  'aziele' goes through cos / sin /
acos, which are the device's own: it is held to the float64 restatement with its own written bound (see the test)."""
import numpy as np
import pytest

from conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import doa_metric_ref as R  # noqa: E402

MICS4 = np.array([[0.04, 0.0, 0.0], [0.0, 0.04, 0.0], [-0.04, 0.0, 0.0], [0.0, -0.04, 0.02]])
MICS8 = np.stack([0.05 * np.cos(np.arange(8) * np.pi / 4), 0.05 * np.sin(np.arange(8) * np.pi / 4),
                  0.01 * (np.arange(8) % 2)], axis=1)
MULTI = ("ACC", "MDR", "FAR", "MAE", "RMSE")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def close(got, want, what, rtol=1e-5):
    """NaNs in the same places; everything else within rtol of the reference."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    print("CHECK %s: got %s want %s" % (what, got, want))
    assert got.shape == want.shape and (np.isnan(got) == np.isnan(want)).all(), (what, got, want)
    ok = np.isnan(want) | (np.abs(got - want) <= rtol * np.abs(want))
    assert ok.all(), (what, got, want)


def run(dev, inputs, mode, ae_mode=("azi",), ae_TH=10, vad_TH=(0.001, 0.5), radians=False, useVAD=True):
    """fnssl.metrics.doa_metrics (-> fnssl_doa_metrics) on host arrays; returns (metrics [9], counts [3, nb]) as numpy."""
    from fnssl import metrics as M
    t = [to_dev(a, dev) for a in inputs]
    m, kg, ke, kc = M.doa_metrics(t[0], t[1], t[2], t[3], mode, ae_mode, ae_TH, useVAD, vad_TH, radians)
    assert m.is_cuda and kg.is_cuda and kg.dtype == torch.int32
    return m.cpu().numpy(), np.stack([kg.cpu().numpy(), ke.cpu().numpy(), kc.cpu().numpy()])


def multi_vector(m, mode="azi"):
    s = {"azi": 0, "ele": 1, "aziele": 2}[mode]
    return [m[0], m[1], m[2], m[3 + s], m[6 + s]]


def ref_multi_vector(ref, mode="azi"):
    return [ref["ACC"], ref["MDR"], ref["FAR"], ref["MAE"][mode], ref["RMSE"][mode]]


def ref_counts(ref):
    return np.stack([ref["K_gt"], ref["K_est"], ref["K_corr"]])


# --------------------------------------------------------------------------- G20: the real reference
@pytest.mark.parametrize("name", list(R.G20_SINGLE))
def test_g20_single_through_preddoa_evaluate(dev, name):
    """(a) FN-SSL PredDOA.evaluate -> getMetric('single'), radians in, ae_mode ['ele', 'azi']."""
    import Module as fn_module
    g = load_golden("g20_doa_metrics")
    doa_gt, vad_gt, doa_est, vad_est = (to_dev(a, dev) for a in R.g20_single_inputs(name))
    pd = fn_module.PredDOA(device="cuda:0").to(dev)
    setting = {'ae_mode': ['ele', 'azi'], 'ae_TH': 5, 'useVAD': True, 'vad_TH': [2 / 3, 2 / 3], 'metric_unfold': False}
    got = pd.evaluate(pred={'doa': doa_est, 'vad_sources': vad_est}, gt={'doa': doa_gt, 'vad_sources': vad_gt}, metric_setting=setting)
    assert set(got) == {"ACC", "MAE"} and got["ACC"].is_cuda and got["ACC"].shape == () and got["MAE"].shape == (2,)
    k = pd.getmetric.last_counts
    np.testing.assert_array_equal(np.stack([k["K_gt"].cpu().numpy(), k["K_est"].cpu().numpy(), k["K_corr"].cpu().numpy()]), g[name + "_K"])
    close(got["ACC"].cpu().numpy(), g[name + "_ACC"], name + " ACC")
    close(got["MAE"].cpu().numpy(), g[name + "_MAE"], name + " MAE (ele, azi)")
    unfolded, keys = pd.evaluate(pred={'doa': doa_est, 'vad_sources': vad_est}, gt={'doa': doa_gt, 'vad_sources': vad_gt},
                                 metric_setting=dict(setting, metric_unfold=True))
    assert keys == ["ACC", "MAE"] and len(unfolded) == 3 and all(isinstance(v, float) for v in unfolded)


@pytest.mark.parametrize("name", list(R.G20_MULTI_NAMES))
def test_g20_multiple_direct(dev, name):
    """(b) IPDnet getMetric('multiple') in degrees: square and rectangular source counts, silent utterances (NaN), segments
    without an estimate, errors one fp32 step below / at / above ae_TH, VADs at the thresholds, judge_assignment."""
    from IPDnet import Module as ip_module
    g = load_golden("g20_doa_metrics")
    t = [to_dev(a, dev) for a in R.g20_multi_inputs(name)]
    gm = ip_module.getMetric(source_mode='multiple', metric_unfold=True)
    got = gm(t[0], t[1], t[2], t[3], ae_mode=['azi'], ae_TH=R.G20_AE_TH, useVAD=True, vad_TH=list(R.G20_VAD_TH))
    assert len(got) == 5 and all(v.is_cuda and v.numel() == 1 for v in got)
    k = gm.last_counts
    np.testing.assert_array_equal(np.stack([k["K_gt"].cpu().numpy(), k["K_est"].cpu().numpy(), k["K_corr"].cpu().numpy()]), g[name + "_K"])
    close([float(v) for v in got], g[name + "_metric"], name)


@pytest.mark.parametrize("name", list(R.G20_MICS))
def test_g20_pred2doa_and_evaluate(dev, name):
    """(c) IPDnet PredDOA.pred2DOA + evaluate on noisy DP-IPDs: DOA indices exact, 'UnkNum' VADs within 1e-5."""
    from IPDnet import Module as ip_module
    g = load_golden("g20_doa_metrics")
    mic, c = R.G20_MICS[name], R.G20_PRED[name]
    pred, doa_gt, vad_gt = R.g20_pred(mic, c["nb"], c["nt"], c["seed"])
    pd = ip_module.PredDOA(mic_location=mic, dev="cuda:0").to(dev)
    gt = [to_dev(doa_gt, dev), to_dev(vad_gt, dev)]
    pred_batch, gt_out = pd.pred2DOA(to_dev(pred, dev), gt)
    doa, vad, ipd = pred_batch
    nb, nt, nf2, nm1, ntrack = pred.shape
    assert doa.shape == (nb, nt, 2, 2) and vad.shape == (nb, nt, 2) and ipd.shape == (nb * nm1, nt, nf2, ntrack)
    np.testing.assert_array_equal(ipd.cpu().numpy(), pred.transpose(0, 3, 1, 2, 4).reshape(nb * nm1, nt, nf2, ntrack))
    azi = np.linspace(0, np.pi, 180)
    np.testing.assert_array_equal(doa.cpu().numpy()[:, :, 1, :], azi[g[name + "_idx"]].astype(np.float32))
    np.testing.assert_array_equal(doa.cpu().numpy()[:, :, 0, :], np.float32(np.pi / 2))
    err = np.abs(vad.cpu().numpy() - g[name + "_vad"]).max()
    print("CHECK %s UnkNum VAD vs reference: max abs err %.3g (tol 1e-5)" % (name, err))
    assert err <= 1e-5
    metric = pd.evaluate(pred_batch=pred_batch, gt_batch=gt_out)
    assert list(metric) == list(MULTI) and all(v.is_cuda and v.shape == (1,) for v in metric.values())
    k = pd.getmetric.last_counts
    np.testing.assert_array_equal(np.stack([k["K_gt"].cpu().numpy(), k["K_est"].cpu().numpy(), k["K_corr"].cpu().numpy()]), g[name + "_K"])
    close([float(metric[m]) for m in MULTI], g[name + "_metric"], name)
    again = pd(to_dev(pred, dev), gt, None)                                                 # forward = pred2DOA + evaluate
    for m in MULTI:
        assert torch.equal(again[m], metric[m])
    with pytest.raises(RuntimeError, match="tar_useVAD"):
        pd.evaluate(pred_batch=pred_batch, gt_batch=[gt[0], to_dev(pred.reshape(nb * nt, nf2, nm1, ntrack), dev)])


# --------------------------------------------------------------------------- real sizes against float64
def test_ipdnet_validation_size_against_float64(dev):
    """IPDnet's validation batch at config-3 geometry: 64 utterances x 25 segments, 2 tracks against 2 ground truths,
    radians in (as evaluate hands them over), ae_TH 10, vad_TH [0.001, 0.5].  No float64 error within 1e-3 degrees of
    ae_TH, no VAD within 1e-6 of a threshold (offending entries are redrawn by the generator)."""
    inputs = R.draw_metric_inputs(64, 25, 2, 2, 3101, 10, (0.001, 0.5), radians=True, silent_utt=(7,), no_est_seg=((3, 4), (9, 0)))
    ref = R.get_metric(R.degrees(inputs[0]), inputs[1], R.degrees(inputs[2]), inputs[3], "multiple", ("azi", "ele"), 10, True, (0.001, 0.5))
    assert ref["th_margin"] > 1e-3 and ref["vad_margin"] > 1e-6 and ref["gap"] > 1e-3 and ref["tie_safe"]
    m, k = run(dev, inputs, "multiple", ("azi", "ele"), 10, (0.001, 0.5), radians=True)
    np.testing.assert_array_equal(k, ref_counts(ref))
    assert np.isnan(ref["ACC"])                                                            # utterance 7 is silent
    close(multi_vector(m, "azi"), ref_multi_vector(ref, "azi"), "config 3, azi")
    close(multi_vector(m, "ele"), ref_multi_vector(ref, "ele"), "config 3, ele")
    # without the silent utterance the means are numbers
    inputs = R.draw_metric_inputs(64, 25, 2, 2, 3102, 10, (0.001, 0.5), radians=True)
    ref = R.get_metric(R.degrees(inputs[0]), inputs[1], R.degrees(inputs[2]), inputs[3], "multiple", ("azi",), 10, True, (0.001, 0.5))
    assert ref["th_margin"] > 1e-3 and ref["gap"] > 1e-3 and ref["tie_safe"] and np.isfinite(ref["ACC"])
    m, k = run(dev, inputs, "multiple", ("azi",), 10, (0.001, 0.5), radians=True)
    np.testing.assert_array_equal(k, ref_counts(ref))
    close(multi_vector(m), ref_multi_vector(ref), "config 3, no silent utterance")


@pytest.mark.parametrize("ns", [1, 2])
def test_fnssl_validation_size_against_float64(dev, ns):
    """FN-SSL's validation batch at config 2: 32 utterances x 25 segments, 'single', ae_TH 5, vad_TH 2/3."""
    inputs = R.draw_metric_inputs(32, 25, ns, ns, 3200 + ns, 5, (2 / 3, 2 / 3), radians=True)
    ref = R.get_metric(R.degrees(inputs[0]), inputs[1], R.degrees(inputs[2]), inputs[3], "single", ("azi", "ele"), 5, True, (2 / 3, 2 / 3))
    assert ref["th_margin"] > 1e-3 and ref["vad_margin"] > 1e-6
    m, k = run(dev, inputs, "single", ("azi", "ele"), 5, (2 / 3, 2 / 3), radians=True)
    np.testing.assert_array_equal(k, ref_counts(ref))
    close([m[0], m[3], m[4]], [ref["ACC"], ref["MAE"]["azi"], ref["MAE"]["ele"]], "config 2, %d sources" % ns)
    assert (m[[1, 2, 5, 6, 7, 8]] == 0).all()


def test_localisation_at_validation_size_against_float64(dev):
    """64 utterances x 25 segments x 2 tracks, 8 microphones (7 reference pairs, 180 candidates): float64 scores, every
    chosen candidate a maximum within rounding (tests/test_gpu_doa.py's rule: s64[idx] >= max - 2 (1e-6 + 1e-5 |max|)),
    the 'UnkNum' ratio within 1e-4 |r| + 1e-6 of float64."""
    from IPDnet import Module as ip_module
    from fnssl import metrics as M
    pred, _doa_gt, _vad_gt = R.g20_pred(MICS8, 64, 25, 3301)
    pd = ip_module.PredDOA(mic_location=MICS8, dev="cuda:0").to(dev)
    idx, vad, ss = M.localize_tracks(to_dev(pred, dev), pd.bank, 1, "UnkNum")
    idx, vad, ss = idx.cpu().numpy()[..., 0], vad.cpu().numpy()[..., 0], ss.cpu().numpy()[:, :, :, 0, :]
    assert idx.shape == (2, 64, 25) and (idx >= 0).all() and (idx < 180).all()
    bank64, _ = R.template_bank(MICS8)
    assert np.abs(pd.bank.cpu().numpy()[0].astype(np.float64) - bank64).max() < 1e-6
    # float64 scores of the DEVICE's (fp32) bank, so that only the accumulation differs
    flat = pd.bank.cpu().numpy()[0].astype(np.float64).reshape(180, -1)
    x = pred.astype(np.float64).transpose(4, 0, 1, 2, 3).reshape(2, 64, 25, -1)
    scores = x @ flat.T / (7 * 512 / 2)
    tol = 1e-6 + 1e-5 * np.abs(scores)
    assert (np.abs(ss - scores) <= tol).all(), np.abs(ss - scores).max()
    top = scores.max(axis=-1)
    chosen = np.take_along_axis(scores, idx[..., None], axis=-1)[..., 0]
    short = top - chosen
    print("CHECK localisation: chosen candidate at most %.3g below the float64 maximum; %d of %d differ from the float64 argmax"
          % (short.max(), int((scores.argmax(-1) != idx).sum()), idx.size))
    assert (short <= 2 * (1e-6 + 1e-5 * np.abs(top))).all()
    win = flat[idx]
    ratio = (win * x).sum(-1) / (win * win).sum(-1)
    assert (np.abs(vad - ratio) <= 1e-4 * np.abs(ratio) + 1e-6).all(), np.abs(vad - ratio).max()


# --------------------------------------------------------------------------- the tracks entry
def _eval_forward_view(dev, nb, nt, nm1, ntrack, seed):
    """What the network's forward hands over: [nb, nt, 2nf, nmic - 1, ntrack] as a permuted view of [nb, nt, ntrack, nmic - 1, 2nf]."""
    base = torch.from_numpy(np.tanh(np.random.RandomState(seed).standard_normal((nb, nt, ntrack, nm1, 512))).astype(np.float32)).to(dev)
    view = base.permute(0, 1, 4, 3, 2)
    assert not view.is_contiguous()
    return view


@pytest.mark.parametrize("mode", ["UnkNum", "KNum"])
def test_tracks_entry_equals_per_track_calls(dev, mode):
    from fnssl import doa as fdoa
    from fnssl import metrics as M
    from IPDnet import Module as ip_module
    pd = ip_module.PredDOA(mic_location=MICS4, dev="cuda:0").to(dev)
    view = _eval_forward_view(dev, 5, 7, 3, 3, 41)
    for pred in (view, view.contiguous()):
        idx, vad, ss = M.localize_tracks(pred, pd.bank, 1, mode)
        assert idx.shape == (3, 5, 7, 1) and ss.shape == (3, 5, 7, 1, 180)
        for r in range(3):
            i1, v1, s1 = fdoa.localize(pred[..., r], pd.bank, 5, 1, "unkNum" if mode == "UnkNum" else "kNum")
            assert torch.equal(idx[r], i1) and torch.equal(vad[r], v1) and torch.equal(ss[r], s1), r
    # two sources per track go through the same kernel
    idx, vad, ss = M.localize_tracks(view, pd.bank, 2, mode)
    for r in range(3):
        i1, v1, s1 = fdoa.localize(view[..., r], pd.bank, 5, 2, "unkNum" if mode == "UnkNum" else "kNum")
        assert torch.equal(idx[r], i1) and torch.equal(vad[r], v1) and torch.equal(ss[r], s1), r


# --------------------------------------------------------------------------- source counts, layouts, determinism
@pytest.mark.parametrize("ns_gt,ns_est", [(g, e) for g in range(1, 5) for e in range(1, 5)])
def test_source_counts_against_float64(dev, ns_gt, ns_est):
    inputs = R.draw_metric_inputs(6, 9, ns_gt, ns_est, 4000 + 10 * ns_gt + ns_est, 10, (0.001, 0.5), silent_utt=(4,) if ns_gt == 2 else ())
    ref = R.get_metric(*inputs, "multiple", ("azi", "ele"), 10, True, (0.001, 0.5))
    assert ref["th_margin"] > 1e-3 and ref["gap"] > 1e-3 and ref["tie_safe"]
    m, k = run(dev, inputs, "multiple", ("azi", "ele"), 10, (0.001, 0.5))
    np.testing.assert_array_equal(k, ref_counts(ref))
    close(multi_vector(m, "azi"), ref_multi_vector(ref, "azi"), "%d x %d azi" % (ns_gt, ns_est))
    close(multi_vector(m, "ele"), ref_multi_vector(ref, "ele"), "%d x %d ele" % (ns_gt, ns_est))
    if ns_gt == ns_est:
        ref = R.get_metric(*inputs, "single", ("azi",), 10, True, (0.001, 0.5))
        m, k = run(dev, inputs, "single", ("azi",), 10, (0.001, 0.5))
        np.testing.assert_array_equal(k, ref_counts(ref))
        close([m[0], m[3]], [ref["ACC"], ref["MAE"]["azi"]], "%d sources, single" % ns_gt)
    # useVAD = False: every entry active, the VAD tensors are not read
    ref = R.get_metric(*inputs, "multiple", ("azi",), 10, False)
    assert ref["gap"] > 1e-3 and ref["tie_safe"]
    from fnssl import metrics as M
    mm, kg, ke, kc = M.doa_metrics(to_dev(inputs[0], dev), None, to_dev(inputs[2], dev), None, "multiple", ("azi",), 10, False)
    np.testing.assert_array_equal(np.stack([kg.cpu().numpy(), ke.cpu().numpy(), kc.cpu().numpy()]), ref_counts(ref))
    close(multi_vector(mm.cpu().numpy()), ref_multi_vector(ref), "%d x %d, useVAD False" % (ns_gt, ns_est))


def test_judge_assignment_as_written(dev):
    """3 ground truths x 2 estimates with the first assigned pair invalid: two valid pairs survive.  4 x 3: the
    reference's ``final_assignment[i]`` erases row 1's valid pair — one correct source, not two."""
    m, k = run(dev, R.judge_case(10), "multiple", ("azi",), 10, useVAD=False)
    assert k[:, 0].tolist() == [6, 4, 2]
    ref = R.get_metric(*R.judge_case(10), "multiple", ("azi",), 10, False)
    close(multi_vector(m), ref_multi_vector(ref), "judge 3 x 2")
    m, k = run(dev, R.erase_case(), "multiple", ("azi",), 10)
    assert k[:, 0].tolist() == [4, 3, 1]
    ref = R.get_metric(*R.erase_case(), "multiple", ("azi",), 10, True, (0.001, 0.5))
    close(multi_vector(m), ref_multi_vector(ref), "erase 4 x 3")
    assert abs(m[3] - 7.0 / (1 + 1e-5)) <= 1e-5 * 7                                        # the 7-degree pair survived


def _aziele_inputs(seed, nb=8, nt=25, ns=2):
    """Degrees; every estimate is its own ground truth moved by 2 .. 8 degrees in azimuth and up to 3 in elevation
    (elevations 60 .. 120), the ground truths of a segment 40 degrees apart: every angular error is above 1.7 degrees."""
    rng = np.random.RandomState(seed)
    ele = rng.uniform(60, 120, (nb, nt, ns))
    azi = rng.uniform(10, 40, (nb, nt, 1)) + 40 * np.arange(ns)[None, None, :] + rng.uniform(-5, 5, (nb, nt, ns))
    doa_gt = np.stack((ele, azi), axis=2).astype(np.float32)
    d_azi = rng.uniform(2, 8, (nb, nt, ns)) * rng.choice([-1, 1], (nb, nt, ns))
    doa_est = np.stack((ele + rng.uniform(-3, 3, (nb, nt, ns)), azi + d_azi), axis=2).astype(np.float32)
    vad = np.ones((nb, nt, ns), np.float32)
    return doa_gt, vad, doa_est, vad.copy()


def test_aziele_against_float64(dev):
    """'aziele' (the clamped acos form) against float64.  Its cos / sin / acos are the device's fp32 functions.  With every
    angular error above 1.7 degrees (0.03 rad), acos is evaluated where d(angle) = d(aux) / sin(angle) <= 34 d(aux); a
    handful of fp32 roundings enter aux (<= 3e-7 together), so a term is off by at most 1e-5 rad of >= 0.03 rad: 3.4e-4
    relative.  Bound: rtol 1e-3 on MAE / RMSE.  Counts are exact (they depend on the azimuth error only)."""
    inputs = _aziele_inputs(4400)
    ref = R.get_metric(*inputs, "multiple", ("azi", "aziele"), 10, True, (0.001, 0.5))
    assert ref["th_margin"] > 1e-3 and ref["gap"] > 1e-3 and ref["tie_safe"] and ref["K_corr"].sum() > 300
    m, k = run(dev, inputs, "multiple", ("azi", "aziele"), 10, (0.001, 0.5))
    np.testing.assert_array_equal(k, ref_counts(ref))
    close(multi_vector(m, "azi"), ref_multi_vector(ref, "azi"), "aziele case, azi")
    close([m[5], m[8]], [ref["MAE"]["aziele"], ref["RMSE"]["aziele"]], "aziele MAE, RMSE", rtol=1e-3)
    ref1 = R.get_metric(*inputs, "single", ("aziele",), 10, True, (0.001, 0.5))
    m1, k1 = run(dev, inputs, "single", ("aziele",), 10, (0.001, 0.5))
    np.testing.assert_array_equal(k1, ref_counts(ref1))
    close([m1[0]], [ref1["ACC"]], "aziele single ACC")
    close([m1[5]], [ref1["MAE"]["aziele"]], "aziele single MAE", rtol=1e-3)


def test_layouts_give_the_same_bits(dev):
    """Strided and non-contiguous inputs: DOAs stored [ns, 2, nb, nt] and permuted, VADs as every second column of a wider
    tensor — the same bits as contiguous copies."""
    from fnssl import metrics as M
    inputs = R.draw_metric_inputs(9, 11, 3, 2, 4500, 10, (0.001, 0.5), radians=True)
    c = [to_dev(a, dev) for a in inputs]
    want = M.doa_metrics(*c, "multiple", ("azi", "ele"), 10, True, (0.001, 0.5), True)
    s = []
    for a in (c[0], c[2]):
        s.append(a.permute(3, 2, 0, 1).contiguous().permute(2, 3, 1, 0))
    for a in (c[1], c[3]):
        wide = torch.full((a.shape[0], a.shape[1], 2 * a.shape[2] + 1), float("nan"), device=dev)
        wide[:, :, 1::2] = a
        s.append(wide[:, :, 1::2])
    assert not any(t.is_contiguous() for t in s)
    got = M.doa_metrics(s[0], s[2], s[1], s[3], "multiple", ("azi", "ele"), 10, True, (0.001, 0.5), True)
    for g, w in zip(got, want):
        assert not torch.isnan(w.float()).any() and torch.equal(g, w)
    got1 = M.doa_metrics(s[0][..., :2], s[2][..., :2], s[1], s[3], "single", ("azi",), 10, True, (0.001, 0.5), True)
    want1 = M.doa_metrics(c[0][..., :2].contiguous(), c[1][..., :2].contiguous(), c[2], c[3], "single", ("azi",), 10, True, (0.001, 0.5), True)
    for g, w in zip(got1, want1):
        assert torch.equal(g, w)


def test_two_runs_give_the_same_bits(dev):
    from fnssl import metrics as M
    inputs = [to_dev(a, dev) for a in R.draw_metric_inputs(64, 25, 2, 2, 4600, 10, (0.001, 0.5), radians=True)]
    for mode in ("multiple", "single"):
        a = M.doa_metrics(*inputs, mode, ("azi", "ele", "aziele"), 10, True, (0.001, 0.5), True)
        b = M.doa_metrics(*inputs, mode, ("azi", "ele", "aziele"), 10, True, (0.001, 0.5), True)
        for x, y in zip(a, b):
            assert np.array_equal(x.cpu().numpy().view(np.int32), y.cpu().numpy().view(np.int32)), mode


def test_wrapper_refuses_what_the_kernel_cannot_do(dev):
    from fnssl import metrics as M
    inputs = [to_dev(a, dev) for a in R.draw_metric_inputs(2, 3, 2, 2, 4700, 10, (0.001, 0.5))]
    with pytest.raises(RuntimeError, match="source_mode"):
        M.doa_metrics(*inputs, "both")
    with pytest.raises(Exception, match="Angle error mode unrecognized"):
        M.doa_metrics(*inputs, "multiple", ("polar",))
    five = torch.zeros(2, 3, 2, 5, device=dev)
    with pytest.raises(RuntimeError, match="sources"):
        M.doa_metrics(five, torch.zeros(2, 3, 5, device=dev), inputs[2], inputs[3], "multiple")
    with pytest.raises(RuntimeError, match="device tensor"):
        M.doa_metrics(inputs[0].cpu(), inputs[1], inputs[2], inputs[3], "multiple")


# --------------------------------------------------------------------------- end to end
def test_ipdnet_validation_and_test_step(dev):
    """IPDnet MyModel on G19's four-microphone batch: validation_step returns the loss it returned before the metrics were
    wired in (the loss of the training path's own chain), last_metrics equals get_metric called separately, test_step
    agrees, nothing falls back."""
    import ipdnet_step_ref as S
    import ipdnet_train_ref as T
    from IPDnet.FixedAarryIPDnet import IPDnet
    from IPDnet.train_step import MyModel
    from fnssl import ops
    from fnssl import weights as W
    net = IPDnet(8, 256, 2, True)
    net.load_state_dict(T.state_tensors(W.make_ipdnet_state(1900, 8, 256, 2, True)))
    model = MyModel(arch=net, mic_pos=torch.from_numpy(S.G19_MICS), device="cuda:0").to(dev).eval()
    mic_sig, dp, doa, _ = S.g19_batch()
    batch = (torch.from_numpy(mic_sig).to(dev), {"doa": torch.from_numpy(doa).to(dev), "dp_signal": torch.from_numpy(dp).to(dev)})
    fallbacks = ops.cluster_fallbacks(dev)
    with torch.no_grad():
        loss = model.validation_step(batch, 0)
        metrics = model.last_metrics
        data = model.data_preprocess(batch[0], batch[1])
        pred = model(data[0])
        want_loss = model.cal_loss(pred_batch=pred, gt_batch=data[1:])
        want = model.get_metric(pred_batch=pred, gt_batch=data[1:], idx=None)
        loss_t = model.test_step(batch, 3)
    assert loss.shape == () and np.isfinite(loss.item())
    assert abs(loss.item() - want_loss.item()) <= 1e-6 * abs(want_loss.item()) and abs(loss_t.item() - loss.item()) <= 1e-6 * abs(loss.item())
    assert list(metrics) == list(MULTI)
    for m in MULTI:
        assert metrics[m].is_cuda and metrics[m].shape == (1,) and torch.equal(metrics[m], want[m]), m
        assert torch.equal(model.last_metrics[m], want[m])
    vals = {m: float(metrics[m]) for m in MULTI}
    print("CHECK IPDnet validation_step on G19: loss %.6g metrics %s" % (loss.item(), vals))
    assert 0.0 <= vals["ACC"] <= 1.0 and abs(vals["ACC"] + vals["MDR"] - 1.0) <= 1e-6 and vals["FAR"] >= 0.0
    k = model.get_metric.getmetric.last_counts
    v = data[-1].cpu().numpy()
    np.testing.assert_array_equal(k["K_gt"].cpu().numpy(), (v > np.float32(0.001)).sum(axis=(1, 2)))
    # against the float64 restatement fed with the device's own DOAs and VADs
    pb, _ = model.get_metric.pred2DOA(pred, list(data[1:]))
    ref = R.get_metric(R.degrees(data[1].cpu().numpy()), v, R.degrees(pb[0].cpu().numpy()), pb[1].cpu().numpy(), "multiple", ("azi",), 10,
                       True, (0.001, 0.5))
    np.testing.assert_array_equal(np.stack([k[n].cpu().numpy() for n in ("K_gt", "K_est", "K_corr")]), ref_counts(ref))
    close([vals[m] for m in MULTI], ref_multi_vector(ref), "G19 metrics vs float64")
    with pytest.raises(RuntimeError, match="tar_useVAD"):
        MyModel(arch=net, mic_pos=torch.from_numpy(S.G19_MICS), device="cuda:0", tar_useVAD=False).to(dev).eval().validation_step(batch, 0)
    assert ops.cluster_fallbacks(dev) == fallbacks


def test_fnssl_validation_and_test_step(dev):
    """FN-SSL MyModel on a batch (waveforms, {'doa', 'vad_sources'}): the steps return the loss cal_loss gives and fill
    last_metrics with ACC and MAE, equal to get_metric called separately; nothing falls back."""
    import predict_step as ps
    from fnssl import ops
    from fnssl import weights as W
    sd = W.make_fnssl_state(3)
    mics = np.array(((-0.04, 0.0, 0.0), (0.04, 0.0, 0.0), (0.0, 0.05, 0.0)))
    model = ps.MyModel(device="cuda:0", mic_location=mics)
    model.arch.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(dev).eval()
    rs = np.random.RandomState(11)
    nb, nseg = 2, 2
    sig = torch.from_numpy((rs.standard_normal((nb, 512 + 25 * 256, 3)) * 0.05).astype(np.float32)).to(dev)
    # ground-truth azimuths halfway between two of the 37 candidates (5 k + 2.5 degrees): whatever the network predicts, every
    # azimuth error is 2.5 + 5 j degrees, 2.5 away from ae_TH = 5, so no decision of the comparison below hangs on rounding
    azi = (5.0 * rs.randint(2, 33, (nb, nseg, 1)) + 2.5) * np.pi / 180
    doa = np.stack((np.full((nb, nseg, 1), np.pi / 2), azi), axis=2).astype(np.float32)
    vad = (rs.rand(nb, nseg, 12, 1) < 0.8).astype(np.float32)

    def gt():
        return {"doa": torch.from_numpy(doa).to(dev), "vad_sources": torch.from_numpy(vad).to(dev)}
    fallbacks = ops.cluster_fallbacks(dev)
    loss = model.validation_step((sig, gt()), 0)
    metrics = model.last_metrics
    with torch.no_grad():
        in_batch, gt_batch = model.data_preprocess(sig, gt())
        pred = model(in_batch)
        want_loss = model.cal_loss(pred_batch=pred, gt_batch=gt_batch)
        want = model.get_metric(pred_batch=pred, gt_batch=gt_batch)
    assert loss.shape == () and np.isfinite(loss.item()) and torch.equal(loss, want_loss)
    assert set(metrics) == {"ACC", "MAE"} and metrics["ACC"].is_cuda
    assert torch.equal(metrics["ACC"], want["ACC"]) and torch.equal(metrics["MAE"], want["MAE"])
    loss_t = model.test_step((sig, gt()), 1)
    assert torch.equal(loss_t, loss) and torch.equal(model.last_metrics["ACC"], want["ACC"])
    # the float64 restatement on the device's own DOAs
    pb, _ = model.get_metric.predgt2DOA(pred_batch=pred, gt_batch=None)
    ref = R.get_metric(R.degrees(doa), gt_batch["vad_sources"].cpu().numpy(), R.degrees(pb["doa"].cpu().numpy()),
                       pb["vad_sources"].cpu().numpy(), "single", ("azi",), 5, True, (2 / 3, 2 / 3))
    k = model.get_metric.getmetric.last_counts
    np.testing.assert_array_equal(np.stack([k[n].cpu().numpy() for n in ("K_gt", "K_est", "K_corr")]), ref_counts(ref))
    print("CHECK FN-SSL validation_step: loss %.6g ACC %s MAE %s" % (loss.item(), metrics["ACC"].item(), metrics["MAE"].cpu().numpy()))
    assert ref["K_gt"].sum() > 0 and ref["th_margin"] > 2.4, ref["th_margin"]
    close([metrics["ACC"].item(), metrics["MAE"][0].item()], [ref["ACC"], ref["MAE"]["azi"]], "FN-SSL metrics vs float64")
    assert ops.cluster_fallbacks(dev) == fallbacks
