"""numpy restatements of the scene finish (csrc/scene.hip, fnssl/scene.py; the model is DESIGN.md §18): Habets' arbitrary
noise field generator as the reference's ``gen_diffuse_noise`` / ``mix_signals`` compute it, ``acoustic_power``, and the SNR
mix / VAD finish of ``AcousticScene.simulate``.  Written from the formulas of §18, in float64 (the reference) and float32
(the yardstick of the gates: every stage rounded to float32, the transforms by ``scipy.fft`` on float32 input, which
computes in single precision), with the shared test cases and the gate table.

Gates: the device may be at most ``GATE_FACTOR`` times as far from float64 (max abs) as the float32 restatement
is.  ``GATE`` holds the restatement's distances, measured on a CPU with ``measure_gates()``; tests/test_scene_ref_host.py
re-measures them.
"""
import numpy as np
import scipy.fft
import scipy.linalg

import rir_ref

GATE_FACTOR = 8.0
K = 256
HOP = 64
NBINS = K // 2 + 1
FS = 16000.0


def hann(dtype=np.float64, mutant=None):
    n = np.arange(K, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / ((K - 1) if mutant == "symmetric_hann" else K))).astype(dtype)


def out_len(length):
    return length + (-length) % HOP


def ring(m, radius):
    a = 2.0 * np.pi * np.arange(m) / m
    return np.stack((radius * np.cos(a), radius * np.sin(a), np.zeros(m)), axis=1)


# microphone sets of the cases, by channel count (8: the planar ring of radius 5 cm whose smallest pivot is 2e-7)
MICS = {
    1: np.array([[0.0, 0.0, 0.0]]),
    2: np.array([[-0.04, 0.0, 0.0], [0.04, 0.0, 0.0]]),
    3: np.array([[-0.04, 0.0, 0.0], [0.04, 0.0, 0.0], [0.0, 0.05, 0.01]]),
    4: np.array([[-0.04, 0.0, 0.0], [0.04, 0.0, 0.0], [0.0, 0.05, 0.01], [0.02, -0.03, 0.0]]),
    8: ring(8, 0.05),
}
RING12 = ring(12, 0.05)                        # not positive definite at bin 1 in float64
MIX_M = (1, 2, 3, 4, 8)
MIX_L = (1, 64, 1000, 1087, 4097)
FACTOR_M = (1, 2, 3, 8)


# --------------------------------------------------------------------------------------------------------------------------
# coherence and factor
# --------------------------------------------------------------------------------------------------------------------------
def coherence(mic_pos, fs=FS, nfft=K, c=343.0):
    """DC [M, M, nfft / 2 + 1] of the spherically isotropic field: sinc(w_k d_pq / (c pi)), ones on the diagonal."""
    pos = np.asarray(mic_pos, dtype=np.float64)
    m = pos.shape[0]
    ww = 2.0 * np.pi * fs * np.arange(nfft // 2 + 1) / nfft
    dc = np.ones((m, m, nfft // 2 + 1))
    for p in range(m):
        for q in range(m):
            if p != q:
                dc[p, q] = np.sinc(ww * np.linalg.norm(pos[p] - pos[q]) / (c * np.pi))
    return dc


def factor(dc, mutant=None):
    """C [M, M, bins] float64, C[:, :, k] the UPPER Cholesky factor of DC[:, :, k] for k >= 1 (slot 0 stays zero).  Raises
    numpy.linalg.LinAlgError naming the first bin that is not positive definite."""
    dc = np.asarray(dc, dtype=np.float64)
    c = np.zeros_like(dc)
    for k in range(1, dc.shape[2]):
        try:
            c[:, :, k] = scipy.linalg.cholesky(dc[:, :, k], lower=(mutant == "lower_factor"))
        except np.linalg.LinAlgError:
            raise np.linalg.LinAlgError("coherence matrix of bin %d is not positive definite" % k)
    return c


def factor_residual(c, dc):
    """max |C^T C - DC| over bins >= 1, in float64."""
    c, dc = np.asarray(c, dtype=np.float64), np.asarray(dc, dtype=np.float64)
    return float(np.abs(np.einsum("qik,qjk->ijk", c, c) - dc)[:, :, 1:].max())


# --------------------------------------------------------------------------------------------------------------------------
# mix_signals
# --------------------------------------------------------------------------------------------------------------------------
def frames_of(x, dtype, mutant=None):
    """x [L, M] -> (windowed frames [nfr, K, M], Lp): K zeros in front, zeros up to Lp = L + 2 K + pad behind."""
    length, m = x.shape
    lp = length + 2 * K + (-length) % HOP
    xp = np.zeros((lp, m), dtype=dtype)
    xp[K:K + length] = x
    nfr = 1 + (lp - K) // HOP
    w = hann(dtype, mutant)
    return np.stack([w[:, None] * xp[HOP * q:HOP * q + K] for q in range(nfr)]), lp


def mix_signals(noise, dc=None, dtype=np.float64, mutant=None, c=None):
    """noise [L, M], DC [M, M, K / 2 + 1] (or its float64 factor ``c``) -> [L + ((-L) mod 64), M]."""
    f = dtype
    cf = np.complex128 if f == np.float64 else np.complex64
    x = np.asarray(noise, dtype=f)
    length, m = x.shape
    if c is None:
        c = factor(dc, mutant)
    c = np.asarray(c).astype(f)                                            # float32: the stored factor
    fr, lp = frames_of(x, f, mutant)
    n = scipy.fft.rfft(fr, axis=1).astype(cf)                              # [nfr, bins, M]
    xs = np.zeros_like(n)
    k0 = 0 if mutant == "bin0_mixed" else 1
    k1 = NBINS - 1 if mutant == "nyquist_dropped" else NBINS
    if mutant == "bin0_mixed":
        c = c.copy()
        c[0, :, 0] = 1                                                      # DC_0 is all ones: its rank-one upper factor
    for p in range(m):
        acc = np.zeros(n.shape[:2], dtype=cf)
        for q in range(p + 1) if mutant != "lower_factor" else range(m):
            acc[:, k0:k1] = (acc[:, k0:k1] + c[q, p, k0:k1].astype(f)[None, :] * n[:, k0:k1, q]).astype(cf)
        xs[:, :, p] = acc
    o = scipy.fft.irfft(xs, n=K, axis=1).astype(f)
    w = hann(f, mutant)
    y = np.zeros((lp, m), dtype=f)
    for q in range(o.shape[0]):
        y[HOP * q:HOP * q + K] = (y[HOP * q:HOP * q + K] + (w[:, None] * o[q]).astype(f)).astype(f)
    y = (y / f(1.5)).astype(f)
    return y[K:K + out_len(length)]


def overlap_sum(length):
    """sum of Hann^2 over the frames that reach each kept sample."""
    lp = length + 2 * K + (-length) % HOP
    s = np.zeros(lp)
    w = hann()
    for q in range(1 + (lp - K) // HOP):
        s[HOP * q:HOP * q + K] += w * w
    return s[K:K + out_len(length)]


def gen_diffuse_noise(noise, T, fs, mic_pos, nfft=K, c=343.0, dtype=np.float64, mutant=None):
    """noise [M L] flat, L = int(T fs): remove the vector's mean, column m = noise[m L : (m + 1) L], mix."""
    f = dtype
    pos = np.asarray(mic_pos, dtype=np.float64)
    m, length = pos.shape[0], int(T * fs)
    v = np.asarray(noise, dtype=f).reshape(-1)[:m * length]
    if mutant != "mean_kept":
        v = (v - f(np.asarray(noise, dtype=np.float64).reshape(-1).mean())).astype(f) if f == np.float32 else v - v.mean()
    cols = v.reshape(m, length).T
    return mix_signals(cols, coherence(pos, fs, nfft, c), f, mutant)


# --------------------------------------------------------------------------------------------------------------------------
# acoustic_power and the finish
# --------------------------------------------------------------------------------------------------------------------------
def window_powers(s, dtype=np.float64):
    s = np.asarray(s, dtype=dtype).reshape(-1)
    if s.size < 512:
        raise ValueError("acoustic_power: %d samples (at least 512)" % s.size)
    nw = -((s.size - 511) // -256)
    sq = (s * s).astype(dtype)
    return np.array([sq[256 * j:256 * j + 512].sum(dtype=dtype) / dtype(512) for j in range(nw)], dtype=dtype)


def acoustic_power(s, dtype=np.float64):
    """Mean of the powers of the windows of 512 every 256 that exceed 0.01 x the largest."""
    wp = window_powers(s, dtype)
    th = dtype(0.01) * wp.max()
    return dtype(wp[wp > th].mean(dtype=dtype))


def threshold_margin(s):
    """min over windows of |power / threshold - 1| (float64): how far the nearest window power is from the threshold."""
    wp = window_powers(s)
    return float(np.abs(wp / (0.01 * wp.max()) - 1.0).min())


def finish(mic_sigs, dp_sigs, noise, snr, n, vads=None, dtype=np.float64, mutant=None, powers=None):
    """mic_sigs / dp_sigs / vads: lists over sources of [>= n, M]; noise [Ln >= n, M].  Returns a dict with P [M], Pn [M], g,
    mic [n, M] and, with vads, vmax [S], vad_sources [n, S] (bool), vad [n], vmean [n, S], vth [S], vabs [n, S] (mean_m |v|)."""
    f = dtype
    mic_sigs = [np.asarray(a, dtype=f)[:n] for a in mic_sigs]
    dp = [np.asarray(a, dtype=f)[:n] for a in dp_sigs]
    noise = np.asarray(noise, dtype=f)
    m = noise.shape[1]
    if powers is None:
        dsum = dp[0].copy()
        for a in dp[1:]:
            dsum = (dsum + a).astype(f)
        pv = np.array([acoustic_power(dsum[:, i], f) for i in range(m)], dtype=f)
        nz = noise[:n] if mutant == "pn_cropped" else noise
        pn = np.array([acoustic_power(nz[:, i], f) for i in range(m)], dtype=f)
    else:
        pv, pn = (np.asarray(a, dtype=f) for a in powers)
    g = f(np.sqrt(f(pv.mean(dtype=f)) / f(10.0 ** (snr / 10.0))) / np.sqrt(f(pn.mean(dtype=f))))
    mic = mic_sigs[0].copy()
    for a in mic_sigs[1:]:
        mic = (mic + a).astype(f)
    mic = (mic + (g * noise[:n]).astype(f)).astype(f)
    out = {"P": pv, "Pn": pn, "g": g, "mic": mic}
    if vads is not None:
        vs = [np.asarray(a, dtype=f)[:n] for a in vads]
        out["vmax"] = np.array([v.max() for v in vs], dtype=f)
        out["vth"] = (out["vmax"] * f(1e-3)).astype(f)
        out["vmean"] = np.stack([v.mean(axis=1, dtype=f) for v in vs], axis=1)
        out["vabs"] = np.stack([np.abs(v).mean(axis=1, dtype=f) for v in vs], axis=1)
        out["vad_sources"] = out["vmean"] > out["vth"][None, :]
        out["vad"] = out["vad_sources"].any(axis=1)
    return out


def vad_undecided(vmean, vth, vabs):
    """Samples whose VAD a float32 evaluation may decide either way: |mean - threshold| <= 64 x 2^-24 x mean_m sum |terms|."""
    return np.abs(np.asarray(vmean, np.float64) - np.asarray(vth, np.float64)[None, :]) <= 64.0 * 2.0 ** -24 * np.asarray(vabs, np.float64)


# --------------------------------------------------------------------------------------------------------------------------
# whole scenes on rir_ref (what the golden generator hands the reference's Dataset.py as gpuRIR)
# --------------------------------------------------------------------------------------------------------------------------
def simulate_rir(room, beta, src, rcv, nb_img, tmax, fs, tdiff=None, c=343.0, seed=0, dtype=np.float64):
    nism, ns = rir_ref.sample_counts(tdiff, tmax, fs)
    h = np.zeros((len(src), len(rcv), ns), dtype=dtype)
    h[:, :, :nism] = rir_ref.ism(room, beta, src, rcv, nb_img, nism, fs, c, dtype)
    if ns > nism:
        h[:, :, nism:] = rir_ref.tail(h[:, :, :nism], room, beta, src, rcv, ns, fs, c, seed, dtype)[0]
    return h


def simulate(room, t60, beta, src_sig, traj_pts, mic_pos, timestamps, n, noise, snr, fs=FS, c=343.0, source_vad=None, seed=0,
             dtype=np.float64):
    """AcousticScene.simulate on rir_ref: returns finish()'s dict plus "dp_sources" [n, M, S]."""
    if t60 == 0:
        tdiff = tmax = 0.1
        nb = [1, 1, 1]
    else:
        tdiff, tmax = 12.0 / 60.0 * t60, 40.0 / 60.0 * t60
        if t60 < 0.15:
            tdiff = tmax
        nb = [int(v) for v in np.ceil(2.0 * tdiff * c / np.asarray(room, dtype=np.float64))]
    full, dp, vads, vabs = [], [], ([] if source_vad is not None else None), []
    for s in range(traj_pts.shape[-1]):
        pts = traj_pts[:, :, s]
        h = simulate_rir(room, beta, pts, mic_pos, nb, tmax, fs, tdiff, c, seed + s, dtype)
        hd = simulate_rir(room, beta, pts, mic_pos, [1, 1, 1], 0.1, fs, None, c, 0, dtype)
        full.append(rir_ref.trajectory(src_sig[:, s], h, timestamps, fs, dtype))
        dp.append(rir_ref.trajectory(src_sig[:, s], hd, timestamps, fs, dtype))
        if vads is not None:
            vads.append(rir_ref.trajectory(source_vad[:, s], hd, timestamps, fs, dtype))
            vabs.append(rir_ref.trajectory(np.abs(source_vad[:, s]), np.abs(hd), timestamps, fs, dtype)[:n].mean(axis=1))
    out = finish(full, dp, noise, snr, n, vads, dtype)
    if vads is not None:
        out["vabs"] = np.stack(vabs, axis=1)                               # the terms of a VAD sample are those of its convolution
    out["dp_sources"] = np.stack([a[:n] for a in dp], axis=2)
    return out


# --------------------------------------------------------------------------------------------------------------------------
# cases and gates
# --------------------------------------------------------------------------------------------------------------------------
def mix_case(m, length):
    return np.random.RandomState(2200 + 17 * m + length).standard_normal((length, m))


def diffuse_case(m, length):
    """flat noise of mean 0.3 for gen_diffuse_noise, T such that int(T fs) = length."""
    return np.random.RandomState(2300 + m + length).standard_normal(m * length) + 0.3, (length + 0.5) / FS


def power_case():
    """[5000, 8]: loud and quiet stretches, scaled per channel; no window power near the threshold (asserted by the tests)."""
    rs = np.random.RandomState(2250)
    x = rs.standard_normal((5000, 8)) * (0.2 + 0.3 * np.arange(8))[None, :]
    x[1200:2400] *= 0.02
    x[4000:4600] *= 0.03
    return x


def integer_power_case(n):
    rs = np.random.RandomState(2260 + n)
    x = rs.randint(-3, 4, size=(n, 3)).astype(np.float64)
    if n >= 2048:
        x[1024:2048] = 0.0
        x[3100:3500] = 0.0
    x[:, 1] *= (np.arange(n) % 512 < 300)
    return x


# name -> (sources, SNR, with VAD, n, noise length)
FINISH_CASES = {
    "s1_snr30": (1, 30.0, False, 2000, 2000),
    "s2_snr-5_vad": (2, -5.0, True, 2000, 2600),
    "s2_snr30_vad": (2, 30.0, True, 1500, 1500),
    "s1_snr-5_vad": (1, -5.0, True, 1800, 2304),
}


def finish_case(name):
    """Synthetic parts of a scene, float32-exact: (mic_sigs, dp_sigs, noise, snr, n, vads or None); M = 3."""
    ns, snr, with_vad, n, ln = FINISH_CASES[name]
    rs = np.random.RandomState(2270 + len(name) + ns)
    tot = n + 300
    env = (np.sin(np.arange(tot) / 150.0) > -0.3).astype(np.float64)[:, None]
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    mic = [f32(rs.standard_normal((tot, 3)) * env * 0.1) for _ in range(ns)]
    dp = [f32(0.6 * a + 0.01 * rs.standard_normal((tot, 3)) * env) for a in mic]
    noise = f32(rs.standard_normal((ln, 3)))
    vads = None
    if with_vad:
        vads = []
        for s in range(ns):
            gate = (np.sin(np.arange(tot) / (90.0 + 40 * s)) > 0.2).astype(np.float64)
            v = np.stack([np.convolve(gate, np.r_[np.zeros(3 + i), 0.05, 0.01 * rs.standard_normal(12)])[:tot] for i in range(3)], axis=1)
            vads.append(f32(v))
    return mic, dp, noise, snr, n, vads


SCENE_ROOM = [3.2, 4.1, 2.6]
SCENE_N = 4096


def scene_case(t60):
    """The inputs of golden G23(b): 2 sources, 3 trajectory points, 2 microphones, 4096 samples.  Every array is exact in
    float32 (the device's input format) and the timestamps are binary fractions, so that int(timestamp fs) has one value."""
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)
    rs = np.random.RandomState(2280)
    env = (np.sin(np.arange(SCENE_N) / 300.0) > -0.5).astype(np.float64)
    src = rs.standard_normal((SCENE_N, 2)) * env[:, None] * 0.3
    vad = np.stack([env, (np.sin(np.arange(SCENE_N) / 210.0) > 0.0).astype(np.float64)], axis=1)
    src[:, 1] *= vad[:, 1]
    pts = np.zeros((3, 3, 2))
    pts[:, :, 0] = [[1.1, 1.3, 1.2], [1.2, 1.5, 1.2], [1.3, 1.7, 1.25]]
    pts[:, :, 1] = [[2.4, 3.0, 0.9], [2.3, 2.8, 0.95], [2.2, 2.6, 1.0]]
    mic_pos = np.array([[1.56, 2.0, 1.0], [1.64, 2.0, 1.0]])
    ts = np.array([0.0, 0.0625, 0.1875])
    noise = rs.standard_normal((SCENE_N + 448, 2))
    beta = [0.0] * 6 if t60 == 0 else rir_beta(SCENE_ROOM, t60)
    return dict(room_sz=SCENE_ROOM, T60=t60, beta=f32(beta), source_signal=f32(src), source_vad=vad, traj_pts=f32(pts),
                mic_pos=f32(mic_pos), timestamps=ts, noise_signal=f32(noise), SNR=12.0, fs=FS, t=np.arange(SCENE_N) / FS, seed=41)


def rir_beta(room, t60):
    """Sabine's reflection coefficients, equal absorption on the six walls (the closed form of fnssl.rir)."""
    room = np.asarray(room, dtype=np.float64)
    area = 2.0 * (room[0] * room[1] + room[0] * room[2] + room[1] * room[2])
    x = min(1.0, max(0.0, 0.161 * float(room.prod()) / (t60 * area)))
    return [float(np.sqrt(1.0 - x))] * 6


def simulate_case(t60, dtype=np.float64):
    k = scene_case(t60)
    return simulate(k["room_sz"], k["T60"], k["beta"], k["source_signal"], k["traj_pts"], k["mic_pos"], k["timestamps"], SCENE_N,
                    k["noise_signal"], k["SNR"], k["fs"], 343.0, k["source_vad"], k["seed"], dtype)


# max |float32 restatement - float64| per case, measured on a CPU (numpy 2.x, scipy 1.15, x86-64) by measure_gates();
# "factor/M": max |C^T C - DC| of scipy's float64 factor rounded to float32.  DESIGN.md §18
GATE = {
    "factor/1": 0.000e+00,
    "factor/2": 6.871e-08,
    "factor/3": 6.871e-08,
    "factor/8": 7.585e-08,
    "mix/1/1": 2.421e-08,
    "mix/1/64": 3.644e-07,
    "mix/1/1000": 5.322e-07,
    "mix/1/1087": 4.287e-07,
    "mix/1/4097": 5.664e-07,
    "mix/2/1": 6.965e-08,
    "mix/2/64": 3.637e-07,
    "mix/2/1000": 4.556e-07,
    "mix/2/1087": 6.730e-07,
    "mix/2/4097": 6.009e-07,
    "mix/3/1": 9.355e-08,
    "mix/3/64": 3.872e-07,
    "mix/3/1000": 5.850e-07,
    "mix/3/1087": 5.373e-07,
    "mix/3/4097": 6.520e-07,
    "mix/4/1": 1.237e-07,
    "mix/4/64": 3.216e-07,
    "mix/4/1000": 5.653e-07,
    "mix/4/1087": 6.360e-07,
    "mix/4/4097": 7.954e-07,
    "mix/8/1": 8.380e-08,
    "mix/8/64": 6.067e-07,
    "mix/8/1000": 6.192e-07,
    "mix/8/1087": 6.022e-07,
    "mix/8/4097": 7.093e-07,
    "diffuse/2/1000": 4.723e-07,
    "diffuse/2/1087": 6.033e-07,
    "diffuse/4/1000": 5.816e-07,
    "diffuse/4/1087": 7.182e-07,
    "power/random": 2.189e-07,
    "finish/s1_snr30": 1.490e-08,
    "finish/s2_snr-5_vad": 5.032e-08,
    "finish/s2_snr30_vad": 2.968e-08,
    "finish/s1_snr-5_vad": 3.519e-08,
    "simulate/0": 6.372e-07,
    "simulate_dp/0": 6.153e-07,
    "simulate/0.2": 3.039e-06,
    "simulate_dp/0.2": 6.153e-07,
}


def measure_gates(which=None):
    out = {}
    f32 = np.float32
    for m in FACTOR_M:
        dc = coherence(MICS[m])
        out["factor/%d" % m] = factor_residual(factor(dc).astype(f32), dc)
    for m in MIX_M:
        dc = coherence(MICS[m])
        for length in MIX_L:
            x = mix_case(m, length).astype(f32).astype(np.float64)
            out["mix/%d/%d" % (m, length)] = float(np.abs(mix_signals(x, dc, f32).astype(np.float64) - mix_signals(x, dc)).max())
    for m in (2, 4):
        for length in (1000, 1087):
            v, t = diffuse_case(m, length)
            v = v.astype(f32).astype(np.float64)
            out["diffuse/%d/%d" % (m, length)] = float(np.abs(
                gen_diffuse_noise(v, t, FS, MICS[m], dtype=f32).astype(np.float64) - gen_diffuse_noise(v, t, FS, MICS[m])).max())
    x = power_case().astype(f32).astype(np.float64)
    out["power/random"] = float(max(abs(float(acoustic_power(x[:, i], f32)) - acoustic_power(x[:, i])) for i in range(x.shape[1])))
    for name in FINISH_CASES:
        mic, dp, noise, snr, n, vads = finish_case(name)
        a, b = finish(mic, dp, noise, snr, n, vads, f32), finish(mic, dp, noise, snr, n, vads)
        out["finish/" + name] = float(np.abs(a["mic"].astype(np.float64) - b["mic"]).max())
    if which != "fast":
        for t60 in (0, 0.2):
            a, b = simulate_case(t60, f32), simulate_case(t60)
            out["simulate/%g" % t60] = float(np.abs(a["mic"].astype(np.float64) - b["mic"]).max())
            out["simulate_dp/%g" % t60] = float(np.abs(a["dp_sources"].astype(np.float64) - b["dp_sources"]).max())
    return out


if __name__ == "__main__":
    for k, v in measure_gates().items():
        print('    "%s": %.3e,' % (k, v))
