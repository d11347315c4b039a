"""Host-side checks of IPDnet2's evaluation (no GPU): the float64 restatement (tests/ipdnet2_eval_ref.py) reproduces what the
real reference computed (tests/golden/g21_ipdnet2_eval.npz); the three new entry points are declared, exported and validate
their arguments before touching the device; the tensor fronts refuse bad shapes / dtypes / CPU tensors; the drop-in
classes construct without a device."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import ipdnet2_eval_ref as R2
from conftest import assert_close, load_golden
from fnssl import _lib, ipdnet_step
from fnssl import metrics as fmetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fnssl_ipd2doa_mse_tracks", "fnssl_ipdnet2_targets", "fnssl_doa_metrics_ex")
# the largest |reference targets - float64| tests/golden/make_golden_ipdnet2_eval.py printed
G21_TARGET_DIFF = 4.62e-07


def _load(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "fn-ssl_amd", *rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_symbols_declared_exported_and_abi_unchanged():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fnssl.h")).read()
    declared = set(re.findall(r"\b(fnssl_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.fnssl_abi_version() == 19 and _lib.ABI_VERSION == 19


def test_metrics_ex_argtypes_are_the_old_ones_plus_three():
    """fnssl_doa_metrics(..., radians, ...) = fnssl_doa_metrics_ex(..., radians, radians, est_below = 0, ratio_eps = 0, ...):
    the same argument list with `radians` doubled and (int, float) after it."""
    lib = _lib.load()
    old, new = list(lib.fnssl_doa_metrics.argtypes), list(lib.fnssl_doa_metrics_ex.argtypes)
    at = 18                                                                # position of `radians`
    assert old[at] is C.c_int and old[at - 1] is C.c_int and old[at + 1] is C.c_float
    assert new == old[:at] + [C.c_int, C.c_int, C.c_int, C.c_float] + old[at + 1:]
    header = open(os.path.join(ROOT, "include", "fnssl.h")).read()

    def params(name):
        body = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        return [re.sub(r"\s+", " ", p).strip() for p in body.split(",")]
    po, pn = params("fnssl_doa_metrics"), params("fnssl_doa_metrics_ex")
    assert len(po) == len(old) and len(pn) == len(new)
    assert pn == po[:at] + ["int gt_radians", "int est_radians", "int est_below", "float ratio_eps"] + po[at + 1:]


def test_restatement_reproduces_the_golden_fixture():
    g = load_golden("g21_ipdnet2_eval")
    for name in R2.G21_CASES:
        d = R2.g21_inputs(name)
        mic = d["mic"]
        tgt = g[name + "_targets"]
        assert tgt.dtype == np.float32 and tgt.shape == (2, 6, 512, mic.shape[0] - 1, 2)
        ref = R2.nearfield_targets(d["doa"], d["distance"], mic)
        diff = np.abs(tgt.astype(np.float64) - ref).max()
        assert diff < G21_TARGET_DIFF + 0.005e-07, (name, diff)             # the printed figure's last digit
        assert np.abs(ref - R2.farfield_targets(d["doa"], mic)).max() > 0.01, name          # the near field is visible
        bank, azi = R2.candidate_bank(mic)
        idx, vad, ss, _ = R2.mse_search(d["pred"], bank)
        np.testing.assert_array_equal(idx[..., 0], g[name + "_idx"])
        assert_close(vad[..., 0].transpose(1, 2, 0), g[name + "_vad"], 1e-5, 1e-7, name + " activity")
        low = np.sort(ss, axis=-1)
        assert ((low[..., 1] - low[..., 0]) > 1e-4 * ss.max()).all(), name
        doa_est = np.stack((np.full(idx[..., 0].shape, np.pi / 2), azi[idx[..., 0]]), axis=0).astype(np.float32).transpose(2, 3, 0, 1)
        m = R2.evaluate(doa_est, g[name + "_vad"], d["azi_deg"], d["vad"])
        assert_close(R2.metric_vector(m), g[name + "_metric"].astype(np.float64), 1e-5, 1e-7, name + " metrics")
        np.testing.assert_array_equal(np.stack([m["K_gt"], m["K_est"], m["K_corr"]]), g[name + "_K"])
        assert m["gap"] > 1e-3 and m["tie_safe"] and m["th_margin"] > 1e-3 and m["vad_margin"] > 1e-6
        act = g[name + "_vad"].astype(np.float64)
        assert (act < 0.4 * 0.2919).any() and (act > 0.4 * 0.2919).any() and np.abs(act - 0.4 * 0.2919).min() > 1e-4
    k = g["mic5_silent_K"]
    assert k[0, 1] == 0 and k[0, 0] > 0 and np.isfinite(g["mic5_silent_metric"]).all()      # K_gt + 1e-6: 0, not NaN
    m = R2.evaluate(doa_est, g["mic5_silent_vad"], d["azi_deg"], d["vad"], ratio_eps=0.0)
    assert np.isnan(m["ACC"]) and np.isnan(m["MDR"]) and np.isnan(m["FAR"])


def test_restatement_gating_and_bessel_table():
    mic = R2.G21_MICS["mic5"]
    ns = R2.bessel_target(mic)
    assert ns.shape == (512, 4) and (ns[256:] == 0).all()
    assert_close(ipdnet_step.non_source_target(mic), ns.astype(np.float32), 0, 1e-7, "library table")
    try:
        from scipy.special import jn
    except Exception:
        jn = None
    if jn is not None:
        assert np.abs(R2.bessel_target(mic, lambda x: jn(0, x)) - ns).max() < 1e-12
    d = R2.g21_inputs("mic5")
    ipd = R2.nearfield_targets(d["doa"], d["distance"], mic)
    vad = np.array([-1.0, 0.0, 1e-9, 1.0, np.nan])
    out = R2.gate_targets(ipd[:1, :5, :, :, :1], vad.reshape(1, 5, 1), ns, 0.0)
    for t, kind in enumerate(("fill", "fill", "keep", "keep", "nan")):
        got = out[0, t, :, :, 0]
        if kind == "fill":
            np.testing.assert_array_equal(got, ns)
        elif kind == "keep":
            np.testing.assert_array_equal(got, ipd[0, t, :, :, 0])
        else:
            assert np.isnan(got).all()
    assert R2.argmin_first(np.array([3.0, 1.0, np.nan, 1.0, np.nan])) == 2 and R2.argmin_first(np.array([3.0, 1.0, 1.0])) == 1


def test_search_validates_before_launch():
    lib = _lib.load()
    p = C.c_void_p(64)                                                     # never dereferenced: every call fails validation
    err = lambda: lib.fnssl_last_error().decode()                                    # noqa: E731
    keys = ("pred", "sb", "sp", "st", "sk", "sr", "bank", "nb", "np", "nt", "nf2", "ncand", "nsrc", "ntrack", "unk", "ss", "idx",
            "vad", "stream")
    base = dict(pred=p, sb=4096, sp=2, st=2048, sk=8, sr=1, bank=p, nb=2, np=4, nt=3, nf2=512, ncand=360, nsrc=1, ntrack=2, unk=1,
                ss=p, idx=p, vad=p, stream=None)
    s = lambda **kw: lib.fnssl_ipd2doa_mse_tracks(*[{**base, **kw}[k] for k in keys])   # noqa: E731
    for name in ("pred", "bank", "ss", "idx", "vad"):
        assert s(**{name: None}) == -1 and "null" in err(), name
    assert s(nsrc=0) == -1 and "sources" in err()
    assert s(nsrc=5) == -1 and "sources" in err()
    assert s(np=0) == -1 and s(np=64) == -1 and "microphone" in err()
    assert s(ntrack=0) == -1 and s(ntrack=65536) == -1 and "tracks" in err()
    assert s(nb=0) == -1 and s(nf2=0) == -1 and s(ncand=0) == -1 and s(nt=-1) == -1
    # (nf2 * np + ncand) * 4 bytes <= 60 KiB = 15360 floats
    assert s(nf2=3750, np=4, ncand=361) == -1 and "LDS" in err()
    assert s(nf2=512, np=63, ncand=360) == -1 and "LDS" in err()
    assert s(nf2=1 << 20, np=63, ncand=1 << 20) == -1 and "LDS" in err()
    assert s(nt=0, pred=None, bank=None, ss=None, idx=None, vad=None) == 0  # nothing to do


def test_targets_and_metrics_ex_validate_before_launch():
    lib = _lib.load()
    p = C.c_void_p(64)
    err = lambda: lib.fnssl_last_error().decode()                                    # noqa: E731
    keys = ("doa", "dist", "vad", "nb", "nseg", "nsrc", "mic", "nmic", "ns", "bin0", "nf", "nbins", "fmax", "speed", "th", "ipd", "stream")
    base = dict(doa=p, dist=p, vad=p, nb=1, nseg=2, nsrc=2, mic=p, nmic=5, ns=p, bin0=1, nf=256, nbins=257, fmax=8000.0, speed=340.0,
                th=0.0, ipd=p, stream=None)
    t = lambda **kw: lib.fnssl_ipdnet2_targets(*[{**base, **kw}[k] for k in keys])    # noqa: E731
    for name in ("doa", "dist", "mic", "ipd"):
        assert t(**{name: None}) == -1 and "null" in err(), name
    assert t(ns=None) == -1 and "null" in err()                            # a VAD gate needs the non-source target
    assert t(nsrc=0) == -1 and "sources" in err()
    assert t(nsrc=5) == -1 and "sources" in err()
    assert t(nmic=1) == -1 and "microphones" in err()
    assert t(nmic=65) == -1 and "microphones" in err()
    assert t(nb=0) == -1 and t(nseg=0) == -1
    assert t(nf=257) == -1 and "bins" in err()
    assert t(speed=0.0) == -1 and t(fmax=-1.0) == -1
    assert t(th=float("nan")) == -1 and "NaN" in err()

    st4, st3 = (C.c_longlong * 4)(8, 4, 2, 1), (C.c_longlong * 3)(4, 2, 1)
    mkeys = ("dg", "sg", "vg", "svg", "de", "se", "ve", "sve", "nb", "nt", "ng", "ne", "mode", "ae", "ae_th", "thg", "the", "use_vad",
             "gt_rad", "est_rad", "below", "ratio_eps", "large", "eps", "metrics", "per_utt", "kg", "ke", "kc", "stream")
    mbase = dict(dg=p, sg=st4, vg=p, svg=st3, de=p, se=st4, ve=p, sve=st3, nb=2, nt=6, ng=2, ne=2, mode=1, ae=1, ae_th=5.0, thg=0.001,
                 the=0.4, use_vad=1, gt_rad=0, est_rad=1, below=1, ratio_eps=1e-6, large=10000.0, eps=1e-5, metrics=p, per_utt=p, kg=p,
                 ke=p, kc=p, stream=None)
    m = lambda **kw: lib.fnssl_doa_metrics_ex(*[{**mbase, **kw}[k] for k in mkeys])   # noqa: E731
    for name in ("dg", "de", "sg", "se", "vg", "ve", "metrics", "per_utt", "kg", "ke", "kc"):
        assert m(**{name: None}) == -1 and "null" in err(), name
    assert m(ng=0) == -1 and m(ne=5) == -1 and "sources" in err()
    assert m(mode=2) == -1 and m(ae=0) == -1 and m(large=100.0) == -1
    assert m(ratio_eps=-1e-6) == -1 and "ratio_eps" in err()
    assert m(ratio_eps=float("nan")) == -1


def test_tensor_fronts_refuse_before_touching_the_device():
    pred, bank = torch.zeros(2, 3, 20, 4, 2), torch.zeros(1, 7, 20, 4)
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        fmetrics.localize_tracks_mse(pred, bank)
    with pytest.raises(RuntimeError, match="source_num_mode"):
        fmetrics.localize_tracks_mse(pred, bank, 1, "unkNum")
    doa, dist, vad = torch.zeros(2, 3, 2, 2), torch.ones(2, 3, 2), torch.ones(2, 3, 2)
    mic, ns = torch.zeros(5, 3, dtype=torch.float64), torch.zeros(512, 4)
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        ipdnet_step.ipdnet2_targets(doa, dist, vad, mic, ns)
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        fmetrics.doa_metrics(torch.zeros(2, 3, 2, 2), vad, torch.zeros(2, 3, 2, 2), vad, est_below=True, ratio_eps=1e-6)
    with pytest.raises(RuntimeError, match="source_mode"):
        fmetrics.doa_metrics(doa, vad, doa, vad, "both", est_below=True)
    # on meta tensors the shape and dtype checks can be reached without a device: is_cuda is what _need_dev asks
    if not torch.cuda.is_available():
        return
    dev = torch.device("cuda:0")
    g = lambda x: x.to(dev)                                                          # noqa: E731
    with pytest.raises(RuntimeError, match="float32"):
        fmetrics.localize_tracks_mse(g(pred).double(), g(bank))
    with pytest.raises(RuntimeError, match="does not match"):
        fmetrics.localize_tracks_mse(g(pred), g(torch.zeros(1, 7, 20, 3)))
    with pytest.raises(RuntimeError, match=r"1\.\.4"):
        fmetrics.localize_tracks_mse(g(pred), g(bank), 5)
    with pytest.raises(RuntimeError, match="LDS"):
        fmetrics.localize_tracks_mse(g(torch.zeros(1, 1, 4000, 4, 1)), g(torch.zeros(1, 7, 4000, 4)))
    with pytest.raises(RuntimeError, match="float64"):
        ipdnet_step.ipdnet2_targets(g(doa), g(dist), g(vad), g(mic).float(), g(ns))
    with pytest.raises(RuntimeError, match="distance"):
        ipdnet_step.ipdnet2_targets(g(doa), g(torch.ones(2, 3, 1)), g(vad), g(mic), g(ns))
    with pytest.raises(RuntimeError, match="non_source"):
        ipdnet_step.ipdnet2_targets(g(doa), g(dist), g(vad), g(mic), g(torch.zeros(512, 3)))
    with pytest.raises(RuntimeError, match="microphones"):
        ipdnet_step.ipdnet2_targets(g(doa), g(dist), None, g(torch.zeros(1, 3, dtype=torch.float64)), None)


def test_drop_ins_construct_without_a_device():
    mod = _load(("IPDnet2", "Module.py"), "fnssl_ipdnet2_module_host")
    for name in ("STFT", "getMetric", "DPIPD2", "PredDOA"):
        assert hasattr(mod, name), name
    mic = R2.G21_MICS["mic5"]
    pd = mod.PredDOA(mic_location=mic, dev="cpu")
    assert pd.max_track == 2 and pd.max_num_sources == 1 and pd.gerdpipd.ndoa_candidate == [1, 360] and pd.gerdpipd.speed == 340
    assert pd.gerdpipd.mic_location.dtype == np.float64
    with pytest.raises(NotImplementedError):
        pd.pred2DOA_track(torch.zeros(4, 3, 512), None, time_pool_size=2)
    with pytest.raises(ValueError):
        mod.PredDOA(mic_location=None)
    with pytest.raises(ValueError):
        mod.DPIPD2([1, 360], mic, ch_mode='MM')
    with pytest.raises(ValueError):
        mod.getMetric(invalid_source_idx=2)
    import inspect
    assert list(inspect.signature(mod.PredDOA.evaluate).parameters)[:4] == ["self", "pred_batch", "gt_batch", "vad_TH"]
    assert inspect.signature(mod.PredDOA.evaluate).parameters["vad_TH"].default == [0.001, 0.4]
    assert inspect.signature(mod.PredDOA.__init__).parameters["res_phi"].default == 360
    # the geometry cache: one bank and one Bessel table per (array, grid, device)
    g1 = ipdnet_step.ipdnet2_geometry(mic, "cpu")
    g2 = ipdnet_step.ipdnet2_geometry(mic.copy(), "cpu")
    assert g1 is g2 and g1["bank"].shape == (1, 360, 512, 4) and g1["mic"].dtype == torch.float64
    bank, azi = R2.candidate_bank(mic)
    assert_close(g1["bank"][0].numpy(), bank.astype(np.float32), 0, 2e-6, "candidate bank")
    assert_close(g1["azi"].numpy(), azi.astype(np.float32), 0, 0, "azimuth grid")
    step = _load(("IPDnet2", "run_step.py"), "fnssl_ipdnet2_run_step_host")
    model = step.MyModel(device="cpu")
    assert isinstance(model, torch.nn.Module) and type(model.arch).__name__ == "OnlineSpatialNet"
    opt = model.configure_optimizers()
    assert type(opt["optimizer"]).__name__ == "AdamW" and opt["optimizer"].defaults["lr"] == 0.0005
    assert opt["lr_scheduler"]["scheduler"].gamma == 0.975 and opt["lr_scheduler"]["monitor"] == "valid/loss"
    with pytest.raises(ValueError):
        step.MyModel(ch_mode='MM')
    with pytest.raises(ValueError):
        step.MyModel(win_shift_ratio=0.5)
