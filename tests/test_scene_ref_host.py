"""CPU tests that pin the scene-finish reference of tests/scene_ref.py (the yardstick of tests/test_gpu_scene.py): its float64
``mix_signals`` against the scipy call sequence the reference's Dataset.py makes (stft / cholesky / istft), the output shape
and the 1.5 overlap constant, golden G23 recorded from the real Dataset.py, ``acoustic_power`` against the strided-window
form, the gate table re-measured, and mutants of the model that must each be told apart by the gates."""
import numpy as np
import pytest
import scipy.linalg
import scipy.signal

import scene_ref as R


def scipy_mix_signals(noise, DC):
    """The reference's call sequence, stage by stage: K/2 zeros either side, scipy.signal.stft (hann, 75 % overlap), per bin
    k >= 1 the upper factor and N^T conj(C), scipy.signal.istft, the K/2 crop."""
    M, K = noise.shape[1], (DC.shape[2] - 1) * 2
    x = np.vstack([np.zeros([K // 2, M]), noise, np.zeros([K // 2, M])]).transpose()
    _, _, N = scipy.signal.stft(x, window="hann", nperseg=K, noverlap=0.75 * K, nfft=K)
    X = np.zeros(N.shape, dtype=complex)
    for k in range(1, K // 2 + 1):
        C = scipy.linalg.cholesky(DC[:, :, k])
        X[:, k, :] = np.dot(N[:, k, :].transpose(), np.conj(C)).transpose()
    _, y = scipy.signal.istft(X, window="hann", nperseg=K, noverlap=0.75 * K, nfft=K)
    return y.transpose()[K // 2:-K // 2, :]


@pytest.mark.parametrize("length", [1024, 1025, 1057, 1087, 1000])
@pytest.mark.parametrize("m", [1, 4])
def test_mix_signals_equals_the_scipy_call_sequence(m, length):
    """L = 0, 1, 33, 63 mod 64 (and the issue's 1000): same values within 1e-12 of the peak, and the reference's own shape
    [L + ((-L) mod 64), M]."""
    x, dc = R.mix_case(m, length), R.coherence(R.MICS[m])
    want, got = scipy_mix_signals(x, dc), R.mix_signals(x, dc)
    assert want.shape == got.shape == (length + (-length) % 64, m)
    peak = np.abs(want).max()
    assert peak > 1.0 and np.abs(got - want).max() <= 1e-12 * peak


def test_reference_shapes_named_in_the_model():
    for length, rows in ((1000, 1024), (1055, 1088), (1087, 1088)):
        assert scipy_mix_signals(R.mix_case(4, length), R.coherence(R.MICS[4])).shape == (rows, 4)


@pytest.mark.parametrize("length", [1, 64, 1000, 1087, 4097])
def test_overlap_constant_holds_on_every_kept_sample(length):
    s = R.overlap_sum(length)
    assert s.shape == (R.out_len(length),) and np.abs(s - 1.5).max() < 1e-14


def test_coherence_matches_its_formula():
    pos = R.MICS[4]
    dc = R.coherence(pos)
    assert dc.shape == (4, 4, 129) and (dc[:, :, 0] == 1).all() and (dc[np.arange(4), np.arange(4)] == 1).all()
    d = np.linalg.norm(pos[1] - pos[3])
    k = 77
    x = 2 * np.pi * R.FS * k / 256 * d / 343.0
    assert abs(dc[1, 3, k] - np.sin(x) / x) < 1e-15 and dc[1, 3, k] == dc[3, 1, k]


def test_factor_is_upper_and_raises_on_the_twelve_microphone_ring():
    dc = R.coherence(R.MICS[8])
    c = R.factor(dc)                                                       # the 8-microphone ring passes ...
    assert (c[:, :, 0] == 0).all() and np.abs(np.tril(c[:, :, 5], -1)).max() == 0
    assert R.factor_residual(c, dc) < 1e-15
    piv = np.abs(c[np.arange(8), np.arange(8), 1:]).min()
    assert 1e-7 < piv < 4e-7                                               # ... with a smallest pivot of 2e-7
    with pytest.raises(np.linalg.LinAlgError, match="bin 1 "):
        R.factor(R.coherence(R.RING12))
    with pytest.raises(np.linalg.LinAlgError):
        scipy.linalg.cholesky(R.coherence(R.RING12)[:, :, 1])


def test_golden_noise_from_the_real_reference(golden):
    g = golden("g23_scene")
    for m in (2, 4):
        for length in (1000, 1087):
            key = "a_%d_%d" % (m, length)
            v, t = R.diffuse_case(m, length)
            assert np.array_equal(g[key + "_noise"], v.astype(np.float32)) and float(g[key + "_T"]) == t
            got = R.gen_diffuse_noise(g[key + "_noise"].astype(np.float64), t, R.FS, g[key + "_mic_pos"])
            want = g[key + "_out"]
            assert got.shape == want.shape == (R.out_len(length), m)
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("t60", [0, 0.2])
def test_golden_scene_from_the_real_reference(golden, t60):
    g = golden("g23_scene")
    key = "b_%g" % t60
    k = R.scene_case(t60)
    for name in ("beta", "source_signal", "traj_pts", "mic_pos", "noise_signal"):
        assert np.array_equal(g[key + "_" + name].astype(np.float64), np.asarray(k[name])), name
    out = R.simulate_case(t60)
    want = g[key + "_mic_signals"]
    assert np.abs(out["mic"] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(out["vad_sources"], g[key + "_mic_vad_sources"].astype(bool))
    assert np.array_equal(out["vad"], g[key + "_mic_vad"].astype(bool))
    assert out["vad_sources"].shape == (R.SCENE_N, 2) and 0.2 < out["vad"].mean() < 0.98
    assert np.abs(out["dp_sources"] - g[key + "_dp_mic_signals_sources"]).max() <= 1e-6 * np.abs(out["dp_sources"]).max()


def strided_acoustic_power(s):
    """acoustic_power as the reference writes it."""
    w, o = 512, 256
    s = np.ascontiguousarray(s)
    S = np.lib.stride_tricks.as_strided(s, strides=s.strides * 2, shape=(s.size - w + 1, w))[0::o]
    wp = np.mean(S ** 2, axis=-1)
    return np.mean(wp[np.nonzero(wp > 0.01 * wp.max())]), wp.size


@pytest.mark.parametrize("n", [512, 767, 768, 769, 1023, 1024, 5000])
def test_acoustic_power_equals_the_strided_window_form(n):
    x = R.power_case()[:n, 3] if n <= 5000 else None
    want, nwin = strided_acoustic_power(x)
    assert nwin == -((n - 511) // -256) == R.window_powers(x).size
    assert abs(R.acoustic_power(x) - want) <= 1e-15 * want
    with pytest.raises(ValueError):
        R.acoustic_power(x[:511])


def test_power_cases_keep_clear_of_the_threshold():
    """The condition the GPU test puts on its inputs: no window power within +-10 % of the threshold."""
    x = R.power_case()
    assert min(R.threshold_margin(x[:, i]) for i in range(x.shape[1])) > 0.1
    for n in (512, 767, 768, 5000):
        xi = R.integer_power_case(n)
        assert min(R.threshold_margin(xi[:, i]) for i in range(3)) > 0.1
        assert np.abs(xi).max() == 3 and (xi == np.round(xi)).all()


def test_gates_are_what_a_cpu_measures():
    measured = R.measure_gates()
    assert set(measured) == set(R.GATE)
    for k, v in measured.items():
        print(k, "%.3e" % v, "%.3e" % R.GATE[k])
        assert 0.8 * R.GATE[k] <= v <= 1.25 * R.GATE[k], (k, v, R.GATE[k])


@pytest.mark.parametrize("mutant", ["bin0_mixed", "nyquist_dropped", "lower_factor", "symmetric_hann"])
def test_mix_mutants_lie_beyond_the_gates(mutant):
    for m, length in ((4, 1000), (2, 1087), (8, 4097)):
        x, dc = R.mix_case(m, length).astype(np.float32).astype(np.float64), R.coherence(R.MICS[m])
        dist = np.abs(R.mix_signals(x, dc, mutant=mutant) - R.mix_signals(x, dc)).max()
        bound = R.GATE_FACTOR * R.GATE["mix/%d/%d" % (m, length)]
        print(mutant, m, length, dist, bound)
        assert dist > bound


def test_mean_mutant_lies_beyond_the_gates():
    for m in (2, 4):
        for length in (1000, 1087):
            v, t = R.diffuse_case(m, length)
            assert abs(v.mean() - 0.3) < 0.05
            dist = np.abs(R.gen_diffuse_noise(v, t, R.FS, R.MICS[m], mutant="mean_kept") - R.gen_diffuse_noise(v, t, R.FS, R.MICS[m])).max()
            assert dist > R.GATE_FACTOR * R.GATE["diffuse/%d/%d" % (m, length)]


def test_cropped_noise_power_mutant_lies_beyond_the_gates():
    """Pn over noise[0:n] instead of the whole noise: told apart on the cases whose noise is longer than n."""
    for name, (_, _, _, n, ln) in R.FINISH_CASES.items():
        mic, dp, noise, snr, n, vads = R.finish_case(name)
        dist = np.abs(R.finish(mic, dp, noise, snr, n, vads, mutant="pn_cropped")["mic"] - R.finish(mic, dp, noise, snr, n, vads)["mic"]).max()
        if ln > n:
            assert dist > R.GATE_FACTOR * R.GATE["finish/" + name], (name, dist)
        else:
            assert dist == 0


def test_vad_cases_stay_under_the_cap_in_float32():
    """The samples whose VAD float32 may decide either way are at most 1 % of a case, and outside them the float32
    restatement decides as float64 does."""
    cases = [R.finish(*R.finish_case(n_)[:5], R.finish_case(n_)[5], dt) for n_ in R.FINISH_CASES if R.FINISH_CASES[n_][2]
             for dt in (np.float64, np.float32)]
    cases += [R.simulate_case(t60, dt) for t60 in (0, 0.2) for dt in (np.float64, np.float32)]
    for f64, f32 in zip(cases[0::2], cases[1::2]):
        und = R.vad_undecided(f64["vmean"], f64["vth"], f64["vabs"])
        assert und.mean() <= 0.01
        assert np.array_equal(f64["vad_sources"][~und], f32["vad_sources"][~und])
        assert 0.05 < f64["vad_sources"].mean() < 0.95
