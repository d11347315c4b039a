"""GPU tests of the scene finish (csrc/scene.hip: fnssl_anf_coherence / _factor / _mean / _mix, fnssl_scene_power / _finish;
fnssl/scene.py, the surface under the reference's names) against the float64 restatements of tests/scene_ref.py and golden
G23, recorded from the reference's own Dataset.py.

Gates: per case the device may be at most 8 x as far from float64 (max abs over the output) as the float32
restatement of scene_ref is; those distances are the table ``scene_ref.GATE``, measured on a CPU and re-measured by
tests/test_scene_ref_host.py.  ``acoustic_power`` is also held exactly (integer-valued inputs whose window sums are exact in
fp32), the finish is restated from the parts the DEVICE stored, and the VADs are compared exactly outside the samples a
float32 evaluation may decide either way.  Every figure is printed before it is asserted.  Run with -m gpu on an MI355X."""
import functools
import types

import numpy as np
import pytest

import scene_ref as R
from conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


def up(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def held(what, got, want, gate_key):
    dist = float(np.abs(np.asarray(got, dtype=np.float64) - want).max())
    bound = R.GATE_FACTOR * R.GATE[gate_key]
    print("%s: device %.3e from float64, float32 restatement %.3e, bound %.3e, peak %.3e"
          % (what, dist, R.GATE[gate_key], bound, float(np.abs(want).max())))
    assert dist <= bound, (what, dist, bound)


@functools.lru_cache(maxsize=None)
def coherence_f64(m):
    return R.coherence(R.MICS[m])


# ------------------------------------------------------------------------------------------------------------------------
# coherence and factor
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.FACTOR_M)
def test_factor_reproduces_the_coherence(dev, m):
    from fnssl import ops
    dc = coherence_f64(m)
    dc_dev = ops.anf_coherence(up(R.MICS[m], dev, np.float64)[None], R.FS)
    assert dc_dev.shape == (1, m, m, 129) and dc_dev.dtype == torch.float64
    d = float(np.abs(dc_dev[0].cpu().numpy() - dc).max())
    print("coherence M = %d: %.3e from numpy's" % (m, d))
    assert d <= 1e-13                                                       # double sin and a division, |x| < 5
    c, status = ops.anf_factor(dc_dev)
    assert c.shape == (1, m, m, 129) and c.dtype == torch.float32 and int(status[0]) == -1
    c = c[0].cpu().numpy()
    assert (c[:, :, 0] == 0).all()                                          # bin 0's slot is unused
    for q in range(m):
        assert (c[q, :q, :] == 0).all() and (c[q, q, 1:] > 0).all()         # upper, positive pivots
    res, bound = R.factor_residual(c, dc), R.GATE_FACTOR * R.GATE["factor/%d" % m]
    print("factor M = %d: |C^T C - DC| %.3e, scipy's factor in float32 %.3e, bound %.3e" % (m, res, R.GATE["factor/%d" % m], bound))
    assert res <= bound


def test_factor_raises_on_the_twelve_microphone_ring_and_recovers(dev):
    from fnssl import ops, scene
    with pytest.raises(np.linalg.LinAlgError, match="bin 1 "):
        ops.anf_factor(ops.anf_coherence(up(R.RING12, dev, np.float64)[None], R.FS))
    with pytest.raises(np.linalg.LinAlgError, match="bin 1 "):
        scene.gen_diffuse_noise(np.zeros(12 * 640), 0.04, R.FS, R.RING12)
    _, status = ops.anf_factor(ops.anf_coherence(up(np.stack([R.MICS[8], R.ring(8, 0.05) * 2]), dev, np.float64), R.FS))
    assert status.cpu().tolist() == [-1, -1]
    # an item of a batch that fails is named; the others are factorised
    pos = up(np.stack([np.random.RandomState(1).uniform(-0.3, 0.3, (12, 3)), R.RING12]), dev, np.float64)   # (smallest pivot 9e-4)
    _, status = ops.anf_factor(ops.anf_coherence(pos, R.FS), sync=False)
    assert status.cpu().tolist() == [-1, 1]
    with pytest.raises(np.linalg.LinAlgError, match=r"bin 1 .*item 1"):
        ops.anf_factor(ops.anf_coherence(pos, R.FS))


# ------------------------------------------------------------------------------------------------------------------------
# mix
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", R.MIX_L)
@pytest.mark.parametrize("m", R.MIX_M)
def test_mix_signals_held_to_float64(dev, m, length):
    from fnssl import scene
    x = R.mix_case(m, length).astype(np.float32)
    got = scene.mix_signals(x, coherence_f64(m))
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (R.out_len(length), m)
    held("mix M = %d L = %d" % (m, length), got, R.mix_signals(x.astype(np.float64), coherence_f64(m)), "mix/%d/%d" % (m, length))


@pytest.mark.parametrize("length", [1000, 1087])
@pytest.mark.parametrize("m", [2, 4])
def test_gen_diffuse_noise_against_the_reference_golden(dev, m, length):
    """Golden G23(a): NoiseDataset.gen_diffuse_noise of the reference on a vector of mean 0.3."""
    from fnssl import scene
    g = load_golden("g23_scene")
    key = "a_%d_%d" % (m, length)
    v, t = g[key + "_noise"], float(g[key + "_T"])
    assert abs(float(v.mean()) - 0.3) < 0.05
    got = scene.gen_diffuse_noise(v, t, R.FS, g[key + "_mic_pos"])
    assert got.shape == (R.out_len(length), m)
    held("gen_diffuse_noise M = %d L = %d (golden)" % (m, length), got, g[key + "_out"], "diffuse/%d/%d" % (m, length))
    held("gen_diffuse_noise M = %d L = %d (scene_ref)" % (m, length), got,
         R.gen_diffuse_noise(v.astype(np.float64), t, R.FS, R.MICS[m]), "diffuse/%d/%d" % (m, length))
    on_dev = scene.gen_diffuse_noise(up(v, dev), t, R.FS, up(g[key + "_mic_pos"], dev, np.float64))
    assert on_dev.is_cuda and np.array_equal(on_dev.cpu().numpy(), got)


def test_mix_bits_do_not_depend_on_the_launch_geometry(dev):
    from fnssl import ops, scene
    m, length = 3, 4097
    x = up(R.mix_case(m, length), dev)[None]
    c, _ = ops.anf_factor(up(coherence_f64(m), dev, np.float64)[None])
    base = ops.anf_mix(x, c)
    assert base.shape == (1, 4160, m)
    for tile in (4, 16, 1, 65):
        assert torch.equal(ops.anf_mix(x, c, _tile_hops=tile), base), tile
    assert torch.equal(ops.anf_mix(x, c), base)
    # a strided view is read in place
    xt = x[0].t().contiguous().t()[None]
    assert xt.stride() != x.stride() and torch.equal(ops.anf_mix(xt, c), base)
    # a batch of three microphone sets against the three single calls
    length = 1000
    pos = np.stack([R.MICS[4], R.MICS[4] * 1.7, R.MICS[4][::-1] * 0.6])
    v = np.stack([R.diffuse_case(4, length)[0] + 0.1 * i for i in range(3)]).astype(np.float32)
    t = R.diffuse_case(4, length)[1]
    batch = scene.gen_diffuse_noise(up(v, dev), t, R.FS, up(pos, dev, np.float64))
    assert batch.shape == (3, 1024, 4)
    for i in range(3):
        single = scene.gen_diffuse_noise(up(v[i], dev), t, R.FS, up(pos[i], dev, np.float64))
        assert single.shape == (1024, 4) and torch.equal(batch[i], single), i
    assert not torch.equal(batch[0], batch[1])


# ------------------------------------------------------------------------------------------------------------------------
# acoustic_power
# ------------------------------------------------------------------------------------------------------------------------
def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


@pytest.mark.parametrize("n", [512, 767, 768, 5000])
def test_acoustic_power_is_exact_on_integer_signals(dev, n):
    """Integer values in {-3 .. 3} with loud and silent stretches: every block and window sum is exact in fp32, so the device
    equals the float64 reference rounded to fp32 within 1 ulp (the division by the window count)."""
    from fnssl import ops, scene
    x = R.integer_power_case(n)
    assert min(R.threshold_margin(x[:, i]) for i in range(3)) > 0.1        # a condition on the inputs, not a tolerance
    want = [np.float32(R.acoustic_power(x[:, i])) for i in range(3)]
    got = ops.scene_power(up(x, dev)).cpu().numpy()
    rs = np.random.RandomState(n)
    a = rs.randint(-2, 3, size=x.shape).astype(np.float64)
    got2 = ops.scene_power([up(a, dev), up(x - a, dev)]).cpu().numpy()     # two integer summands of the same signal
    longer = ops.scene_power([up(np.vstack([x, 9 * np.ones((70, 3))]), dev)], n).cpu().numpy()   # rows past n are not read
    for i in range(3):
        print("n = %d channel %d: device %r, float64 rounded %r" % (n, i, got[i], want[i]))
        assert ulps(got[i], want[i]) <= 1 and ulps(got2[i], want[i]) <= 1 and longer[i] == got[i]
    one = scene.acoustic_power(x[:, 1])
    assert one.dtype == np.float32 and one == got[1]


def test_acoustic_power_random_leg(dev):
    from fnssl import ops
    x = R.power_case().astype(np.float32)
    x64 = x.astype(np.float64)
    assert min(R.threshold_margin(x64[:, i]) for i in range(8)) > 0.1
    want = np.array([R.acoustic_power(x64[:, i]) for i in range(8)])
    held("acoustic_power [5000, 8]", ops.scene_power(up(x, dev)).cpu().numpy(), want, "power/random")


# ------------------------------------------------------------------------------------------------------------------------
# finish
# ------------------------------------------------------------------------------------------------------------------------
def vads_agree(what, got_sources, got_any, ref):
    """Exact outside the samples where |mean - threshold| <= 64 x 2^-24 x mean_m sum |terms|; those are at most 1 %."""
    und = R.vad_undecided(ref["vmean"], ref["vth"], ref["vabs"])
    print("%s: %d of %d VAD samples undecided in float32, %.1f %% active" % (what, int(und.sum()), und.size, 100 * ref["vad_sources"].mean()))
    assert und.mean() <= 0.01
    got_sources = np.asarray(got_sources).astype(bool)
    assert got_sources.shape == ref["vad_sources"].shape
    assert np.array_equal(got_sources[~und], ref["vad_sources"][~und])
    assert np.array_equal(np.asarray(got_any).astype(bool), got_sources.any(axis=1))


@pytest.mark.parametrize("name", list(R.FINISH_CASES))
def test_finish_restated_from_what_the_device_stored(dev, name):
    from fnssl import ops
    mic, dp, noise, snr, n, vads = R.finish_case(name)
    d = lambda seq: [up(a, dev) for a in seq]
    p = ops.scene_power(d(dp), n)
    pn = ops.scene_power(d([noise]))
    fin = ops.scene_finish(d(mic), up(noise, dev), p, pn, snr, n, d(vads) if vads is not None else None)
    p64, pn64 = p.cpu().numpy().astype(np.float64), pn.cpu().numpy().astype(np.float64)
    ref = R.finish(mic, dp, noise, snr, n, vads)
    for label, got, want in (("P", p64, ref["P"]), ("Pn", pn64, ref["Pn"])):
        rel = float(np.abs(got / want - 1).max())
        print("%s %s: device %.3e (relative) from float64" % (name, label, rel))
        assert rel <= 32 * 2.0 ** -24                                      # a tree of <= 512 + windows positive fp32 terms
    stored = R.finish(mic, dp, noise, snr, n, vads, powers=(p64, pn64))    # float64 from the DEVICE's power vectors
    g = float(fin["g"].cpu()[0])
    print("%s g: device %r, float64 from the stored powers %r" % (name, g, float(stored["g"])))
    assert abs(g / float(stored["g"]) - 1) <= 16 * 2.0 ** -24              # 2 (M - 1) additions, 4 divisions, 2 roots
    assert fin["mic"].shape == (n, 3)
    held("finish " + name, fin["mic"].cpu().numpy(), stored["mic"], "finish/" + name)
    if vads is None:
        assert "vad" not in fin
    else:
        assert np.array_equal(fin["vmax"].cpu().numpy().astype(np.float64), stored["vmax"])
        assert fin["vad_sources"].dtype == torch.uint8 and fin["vad"].dtype == torch.uint8
        vads_agree("finish " + name, fin["vad_sources"].cpu().numpy(), fin["vad"].cpu().numpy(), stored)


# ------------------------------------------------------------------------------------------------------------------------
# simulate
# ------------------------------------------------------------------------------------------------------------------------
def golden_scene(t60, conv=lambda a: a, **over):
    g = load_golden("g23_scene")
    key = "b_%g" % t60
    t60_, snr, fs, seed, n = g[key + "_scalars"]
    sc = types.SimpleNamespace(
        room_sz=g[key + "_room_sz"].tolist(), T60=float(t60_), beta=g[key + "_beta"].astype(np.float64), SNR=float(snr), fs=float(fs),
        noise_signal=conv(g[key + "_noise_signal"]), source_signal=conv(g[key + "_source_signal"]),
        array_setup=types.SimpleNamespace(mic_orV=None, mic_pattern="omni"), mic_pos=conv(g[key + "_mic_pos"]),
        timestamps=g[key + "_timestamps"], traj_pts=conv(g[key + "_traj_pts"]), t=np.arange(int(n)) / float(fs), c=343.0)
    sc.source_vad = conv(g[key + "_source_vad"].astype(np.float32))
    for k, v in over.items():
        if v is None and k == "source_vad":
            del sc.source_vad
        else:
            setattr(sc, k, v)
    return sc, int(seed), g, key


@functools.lru_cache(maxsize=None)
def scene_f64(t60):
    return R.simulate_case(t60)


@pytest.mark.parametrize("t60", [0, 0.2])
def test_simulate_against_the_reference_golden(dev, t60):
    """Golden G23(b): AcousticScene.simulate of the reference over rir_ref as gpuRIR.  T60 = 0 is the direct path alone;
    T60 = 0.2 has image sources to 40 ms and the fitted tail to 133 ms, its noise drawn from the same generator and seeds."""
    from fnssl import scene
    sc, seed, g, key = golden_scene(t60)
    mic, parts = scene.simulate(sc, seed=seed, keep=True)
    n = R.SCENE_N
    assert isinstance(mic, np.ndarray) and mic.dtype == np.float32 and mic.shape == (n, 2)
    held("simulate T60 = %g" % t60, mic, g[key + "_mic_signals"], "simulate/%g" % t60)
    assert sc.mic_vad_sources.shape == (n, 2) and sc.mic_vad_sources.dtype == bool and sc.mic_vad.shape == (n,)
    vads_agree("simulate T60 = %g" % t60, sc.mic_vad_sources, sc.mic_vad, scene_f64(t60))
    assert sc.dp_mic_signals_sources.shape == (n, 2, 2)
    held("dp_mic_signals_sources T60 = %g" % t60, sc.dp_mic_signals_sources, scene_f64(t60)["dp_sources"], "simulate_dp/%g" % t60)
    nism, ns = R.rir_ref.sample_counts(0.04 if t60 else 0.1, 40.0 / 60.0 * t60 if t60 else 0.1, R.FS)
    assert tuple(parts["rirs"][0].shape) == (3, 2, ns) and tuple(parts["dp_rirs"][0].shape) == (3, 2, 1600)
    if t60 == 0:                                                           # no tail: the full path IS the direct path
        assert all(torch.equal(a, b) for a, b in zip(parts["mic_signals_sources"], parts["dp_mic_signals_sources"]))
    else:
        assert ns > nism and float(parts["rirs"][0][:, :, nism:].abs().max()) > 0


def test_simulate_numpy_and_device_tensor_scenes_agree(dev):
    from fnssl import scene
    host, seed, _, _ = golden_scene(0.2)
    on_dev, _, _, _ = golden_scene(0.2, lambda a: up(a, dev))
    a = scene.simulate(host, seed=seed)
    b = scene.simulate(on_dev, seed=seed)
    assert isinstance(b, torch.Tensor) and b.is_cuda and np.array_equal(a, b.cpu().numpy())
    for name in ("mic_vad_sources", "mic_vad", "dp_mic_signals_sources"):
        h, d = getattr(host, name), getattr(on_dev, name)
        assert isinstance(h, np.ndarray) and d.is_cuda and np.array_equal(h, d.cpu().numpy()), name
    assert on_dev.mic_vad.dtype == torch.bool
    # without source_vad no VAD attribute appears, and the signals are the same
    plain, _, _, _ = golden_scene(0.2, source_vad=None)
    assert np.array_equal(scene.simulate(plain, seed=seed), a) and not hasattr(plain, "mic_vad")
    with pytest.raises(RuntimeError, match="ROCm device tensor or a numpy array"):
        scene.simulate(golden_scene(0.2, lambda a_: torch.from_numpy(a_))[0])


def test_simulate_noise_seeds_and_rirs(dev):
    from fnssl import rir, scene
    pts = load_golden("g23_scene")["b_0.2_traj_pts"].copy()
    pts[:, :, 1] = pts[:, :, 0]                                            # both sources walk the same path
    n = R.SCENE_N
    # noise_signal None: the reference's shape from numpy's stream; an explicit seed leaves the stream alone
    sc, _, _, _ = golden_scene(0.2, noise_signal=None, traj_pts=pts)
    np.random.seed(5)
    a, pa = scene.simulate(sc, seed=7, keep=True)
    np.random.seed(5)
    assert sc.noise_signal.shape == (n, 2) and np.array_equal(sc.noise_signal, np.random.standard_normal((n, 2)))
    # seed None: one np.random.randint first
    sc2, _, _, _ = golden_scene(0.2, noise_signal=None, traj_pts=pts)
    np.random.seed(5)
    _, p2 = scene.simulate(sc2, keep=True)
    np.random.seed(5)
    assert p2["seed"] == int(np.random.randint(0, 2 ** 31 - 1)) and np.array_equal(sc2.noise_signal, np.random.standard_normal((n, 2)))
    # the same seed gives the same bits, another seed another tail
    sc3, _, _, _ = golden_scene(0.2, noise_signal=sc.noise_signal, traj_pts=pts)
    b, pb = scene.simulate(sc3, seed=7, keep=True)
    assert np.array_equal(a, b)
    sc4, _, _, _ = golden_scene(0.2, noise_signal=sc.noise_signal, traj_pts=pts)
    assert not np.array_equal(scene.simulate(sc4, seed=8), a)
    # sources get different tails on the same image-source part, and the RIRs are those of simulateRIR called directly
    tdiff, tmax = rir.att2t_SabineEstimator(12, 0.2), rir.att2t_SabineEstimator(40, 0.2)
    nism, ns = R.rir_ref.sample_counts(tdiff, tmax, R.FS)
    r0, r1 = pa["rirs"]
    assert torch.equal(r0[:, :, :nism], r1[:, :, :nism]) and not torch.equal(r0[:, :, nism:], r1[:, :, nism:])
    for s, r in enumerate(pa["rirs"]):
        direct = rir.simulateRIR(sc.room_sz, sc.beta, up(pts[:, :, s], dev), up(sc.mic_pos, dev), rir.t2n(tdiff, sc.room_sz), tmax, sc.fs,
                                 Tdiff=tdiff, seed=7 + s)
        assert torch.equal(direct, r), s


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_limit(dev):
    from fnssl import ops
    with pytest.raises(RuntimeError, match=r"nfft = 512 \(only 256 is built\)"):
        ops.anf_coherence(up(R.MICS[2], dev, np.float64)[None], R.FS, nfft=512)
    with pytest.raises(RuntimeError, match=r"17 microphones \(1 .. 16\)"):
        ops.anf_coherence(torch.zeros((1, 17, 3), dtype=torch.float64, device=dev), R.FS)
    with pytest.raises(RuntimeError, match=r"17 microphones \(1 .. 16\)"):
        ops.anf_mix(torch.zeros((1, 100, 17), device=dev), torch.zeros((1, 17, 17, 129), device=dev))
    with pytest.raises(RuntimeError, match="511 samples"):
        ops.scene_power(torch.zeros((511, 2), device=dev))
    with pytest.raises(RuntimeError, match="expected a ROCm device tensor"):
        ops.scene_power(torch.zeros((1024, 2)))
    with pytest.raises(RuntimeError, match="expected a ROCm device tensor"):
        ops.anf_mix(torch.zeros((1, 100, 2)), torch.zeros((1, 2, 2, 129)))
    with pytest.raises(RuntimeError, match="what anf_factor returned"):
        ops.anf_mix(torch.zeros((1, 100, 2), device=dev), torch.zeros((1, 2, 2, 129), device=dev))
