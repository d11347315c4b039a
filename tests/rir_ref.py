"""numpy restatements of the room simulation (csrc/rir.hip, fnssl/rir.py; the model is DESIGN.md §17) as plain loops over
images and source samples, in float64 (the reference) and float32 (the yardstick of the gates), the Philox4x32-10 generator,
the shared test cases and the gate table.

Gates (the project's convention): the device may be at most ``GATE_FACTOR`` times as far from float64 as the
float32 restatement is, max abs over the output.  ``GATE`` holds the float32 restatement's distances, measured on a CPU with
``measure_gates()``; tests/test_rir_ref_host.py re-measures them.
"""
import numpy as np

GATE_FACTOR = 8.0
FS = 16000.0
ROOM = [3.2, 4.1, 2.6]
BETA = [0.65, 0.95, 0.72, 0.88, 0.8, 0.91]
TDIFF = 0.05
TMAX = 0.125
SRC = [[1.1, 1.3, 1.2], [2.4, 3.0, 0.9], [0.6, 3.5, 1.7]]
RCV = [[1.55, 2.0, 1.0], [1.65, 2.0, 1.0], [1.6, 2.08, 1.0], [1.6, 1.92, 1.05], [2.9, 0.4, 2.2]]


def sample_counts(tdiff, tmax, fs):
    if tdiff is None or tdiff > tmax:
        tdiff = tmax
    nism, ns = int(np.ceil(tdiff * fs)), int(np.ceil(tmax * fs))
    return nism + nism % 2, ns + ns % 2


# name -> (sources, receivers, nb_img, Tdiff, c)
ISM_CASES = {
    "direct": (SRC[:1], RCV[:1], [1, 1, 1], TDIFF, 343.0),
    "even_odd": (SRC[:2], RCV[:2], [2, 3, 4], TDIFF, 343.0),
    "odd_even": (SRC[:3], RCV[:5], [5, 4, 3], TDIFF, 343.0),
    "past_nism": (SRC[:3], RCV[:5], [9, 8, 7], TDIFF, 343.0),
    "chunks": (SRC[:1], RCV[:2], [11, 9, 8], TDIFF, 343.0),
    "near": ([[1.55, 2.05, 1.0]], RCV[:2], [5, 4, 3], TDIFF, 343.0),              # 5 cm from receiver 0: window clipped at t < 0
    "singular": ([[0.5, 2.0, 1.0]], [[1.5, 2.0, 1.0]], [2, 3, 4], TDIFF, 320.0),     # 1.0 m along x at c = 320: tau = 50 exactly
    "odd_count": (SRC[:2], RCV[:2], [5, 4, 3], 0.0500625, 343.0),                 # ceil(Tdiff fs) = 801 -> 802
}
# name -> (ISM case, Tdiff, Tmax, seed, the branch every RIR of the case takes).  "short" has fewer than 3 whole segments
# after the direct path, "mean" none (48 samples against a segment of 128).
TAIL_CASES = {
    "fit": ("past_nism", TDIFF, TMAX, 7, "fit"),
    "short": ("even_odd", 0.02, TMAX, 11, "sabine_last"),
    "mean": ("even_odd", 0.003, 0.02, 5, "sabine_mean"),
}


# --------------------------------------------------------------------------------------------------------------------------
# image-source part
# --------------------------------------------------------------------------------------------------------------------------
def axis_images(n_img, length, p, b0, b1, mutant=None):
    """Per axis: image positions and reflection amplitudes for n = i - floor(N / 2), i = 0 .. N - 1."""
    lo, hi = -(n_img // 2), n_img - n_img // 2
    if mutant == "inclusive_range":
        lo, hi = -(n_img // 2), n_img // 2 + 1
    pos, amp = [], []
    for n in range(lo, hi):
        pos.append((n + 1) * length - p if n % 2 else n * length + p)
        more, less = (abs(n) + 1) // 2, abs(n) // 2
        c0, c1 = (less, more) if n > 0 else (more, less)
        if mutant == "swapped_walls":
            c0, c1 = c1, c0
        amp.append(b0 ** c0 * b1 ** c1)
    return pos, amp


def ism(room, beta, src, rcv, nb_img, nism, fs, c=343.0, dtype=np.float64, mutant=None):
    """[M_src, M_rcv, nism].  float64: the definition.  float32: the same steps in float32, the window and the sinc taken
    per tap from float32 arguments."""
    f = dtype
    src, rcv = np.asarray(src, dtype=f), np.asarray(rcv, dtype=f)
    room = [f(v) for v in room]
    beta = [f(v) for v in beta]
    tw = f(8e-3 * fs + (1.0 if mutant == "window_plus_one" else 0.0))
    half = f(0.5) * tw
    fs_c = f(fs / c)
    pi = f(np.pi)
    out = np.zeros((len(src), len(rcv), nism), dtype=f)
    for s in range(len(src)):
        ax = [axis_images(nb_img[a], room[a], src[s][a], beta[2 * a], beta[2 * a + 1], mutant) for a in range(3)]
        for r in range(len(rcv)):
            h = out[s, r]
            for px, ax_ in zip(*ax[0]):
                for py, ay in zip(*ax[1]):
                    for pz, az in zip(*ax[2]):
                        dx, dy, dz = f(px) - rcv[r][0], f(py) - rcv[r][1], f(pz) - rcv[r][2]
                        d = np.sqrt(dx * dx + dy * dy + dz * dz)
                        amp = f(ax_) * f(ay) * f(az) / (f(4) * pi * d)
                        tau = d * fs_c
                        t0, t1 = int(np.ceil(tau - half)), int(np.floor(tau + half))
                        t0, t1 = max(t0, 0), min(t1, nism - 1)
                        if t1 < t0:
                            continue
                        x = np.arange(t0, t1 + 1).astype(f) - tau
                        w = f(0.5) * (f(1) + np.cos(f(2) * pi * x / tw))
                        h[t0:t1 + 1] += (amp * w * np.sinc(x)).astype(f)
    return out


def single_windowed_sinc(d, nism, fs, c=343.0):
    """The closed form of one image at distance d, float64."""
    t = np.arange(nism, dtype=np.float64)
    tau, tw = d * fs / c, 8e-3 * fs
    x = t - tau
    return np.where(np.abs(x) <= tw / 2, 0.5 * (1 + np.cos(2 * np.pi * x / tw)) * np.sinc(x), 0.0) / (4 * np.pi * d)


# --------------------------------------------------------------------------------------------------------------------------
# Philox4x32-10 (Salmon et al. 2011), vectorised over counters
# --------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars), key: two uint32 -> [4, ...] uint32."""
    c = [np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c).astype(np.uint32)


def uniforms(seed, src, rcv, t):
    """u of samples t (int array) of RIR (src, rcv), float64 — each is exact in float32 too: ((w >> 9) + 0.5) / 2^23."""
    t = np.asarray(t, dtype=np.int64)
    w = philox4x32_10((t // 4, rcv, src, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    word = w[t % 4, np.arange(t.size)]
    return ((word >> np.uint32(9)).astype(np.float64) + 0.5) / 8388608.0


# --------------------------------------------------------------------------------------------------------------------------
# diffuse tail
# --------------------------------------------------------------------------------------------------------------------------
def sabine_slope(room, beta, fs):
    room, beta = np.asarray(room, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    area = np.array([room[1] * room[2]] * 2 + [room[0] * room[2]] * 2 + [room[0] * room[1]] * 2)
    absorb = float((area * (1 - beta ** 2)).sum())
    return -np.log(1e6) / (0.161 * room.prod() / absorb * fs) if absorb > 0 else 0.0


def tail_line(h_ism, room, beta, src, rcv, fs, c=343.0, dtype=np.float64):
    """(a, b, branch) of e = a + b t for one RIR's image-source part.  float32: the segment energies and their logarithm in
    float32, the fit in float64 from those, a and b rounded to float32 (what the kernel does)."""
    f = dtype
    nism = h_ism.size
    ls = int(round(8e-3 * fs))
    if f == np.float32:
        d = np.sqrt(((np.asarray(src, dtype=f) - np.asarray(rcv, dtype=f)) ** 2).sum(dtype=f))
        tau = d * f(fs / c)
    else:
        tau = np.sqrt(((np.asarray(src, dtype=f) - np.asarray(rcv, dtype=f)) ** 2).sum()) * fs / c
    t0 = int(np.floor(tau)) if tau < nism else nism
    nseg = (nism - t0) // ls
    h = h_ism.astype(f)
    e = np.array([np.log((h[t0 + j * ls:t0 + (j + 1) * ls] ** 2).sum(dtype=f) / f(ls) + f(1e-30)) for j in range(nseg)],
                 dtype=np.float64)
    tc = t0 + (np.arange(nseg) + 0.5) * ls
    branch = None
    if nseg >= 3:
        tm, em = tc.mean(), e.mean()
        b = ((tc - tm) * (e - em)).sum() / ((tc - tm) ** 2).sum()
        a = em - b * tm
        branch = "fit" if b < 0 else None
    if branch is None:
        b = float(f(sabine_slope(room, beta, fs)))
        if nseg >= 1:
            a, branch = e[-1] - b * tc[-1], "sabine_last"
        else:
            a, branch = float(np.log((h ** 2).sum(dtype=f) / f(nism) + f(1e-30))) - b * 0.5 * nism, "sabine_mean"
    return (float(f(a)), float(f(b)), branch) if f == np.float32 else (float(a), float(b), branch)


def tail(h_ism, room, beta, src_pos, rcv_pos, nsamples, fs, c=343.0, seed=0, dtype=np.float64):
    """h_ism [M_src, M_rcv, nism] (what the device stored) -> (tail [M_src, M_rcv, nsamples - nism], lines [M_src][M_rcv])."""
    f = dtype
    ms, mr, nism = h_ism.shape
    t = np.arange(nism, nsamples)
    out = np.zeros((ms, mr, nsamples - nism), dtype=f)
    lines = []
    for s in range(ms):
        lines.append([])
        for r in range(mr):
            a, b, branch = tail_line(h_ism[s, r], room, beta, src_pos[s], rcv_pos[r], fs, c, f)
            u = uniforms(seed, s, r, t).astype(f)
            xi = f(np.sqrt(3.0) / np.pi) * (np.log(u) - np.log(f(1) - u))
            out[s, r] = np.exp(f(0.5) * (f(a) + f(b) * t.astype(f))) * xi
            lines[-1].append((a, b, branch))
    return out, lines


# --------------------------------------------------------------------------------------------------------------------------
# moving-source mixing
# --------------------------------------------------------------------------------------------------------------------------
def w_ini(npts, nsamples, timestamps=None, fs=None):
    if timestamps is None:
        fs, timestamps = nsamples / npts, np.arange(npts)
    return np.append((np.asarray(timestamps, dtype=np.float64) * fs).astype(np.int64), nsamples)


def trajectory(x, rirs, timestamps=None, fs=None, dtype=np.float64):
    """y[t, m] = sum_k rirs[p(t - k), m, k] x[t - k], one source sample at a time in ascending order."""
    f = dtype
    x, rirs = np.asarray(x, dtype=f), np.asarray(rirs, dtype=f)
    npts, m, length = rirs.shape
    w = w_ini(npts, x.size, timestamps, fs)
    y = np.zeros((x.size + length - 1, m), dtype=f)
    for p in range(npts):
        for s in range(int(w[p]), int(w[p + 1])):
            y[s:s + length] += x[s] * rirs[p].T
    return y


def trajectory_overlap_add(x, rirs, timestamps=None, fs=None):
    """gpuRIR's description: cut the signal into per-point segments, convolve each with its RIR, overlap-add."""
    x, rirs = np.asarray(x, dtype=np.float64), np.asarray(rirs, dtype=np.float64)
    npts, m, length = rirs.shape
    w = w_ini(npts, x.size, timestamps, fs)
    y = np.zeros((x.size + length - 1, m))
    for p in range(npts):
        seg = x[w[p]:w[p + 1]]
        if seg.size == 0:
            continue
        for k in range(m):
            y[w[p]:w[p] + seg.size + length - 1, k] += np.convolve(seg, rirs[p, k])
    return y


def traj_random_case():
    rs = np.random.RandomState(2100)
    x = rs.standard_normal(1001)
    rirs = rs.standard_normal((7, 5, 300)) * np.exp(-np.arange(300) / 60.0)
    ts = np.array([0.0, 0.004, 0.0101, 0.0101, 0.027, 0.04, 0.0555])
    return x, rirs, ts


# --------------------------------------------------------------------------------------------------------------------------
# gates
# --------------------------------------------------------------------------------------------------------------------------
# max |float32 restatement - float64| per case, measured on a CPU (numpy 2.x, x86-64) by measure_gates(); DESIGN.md §17
GATE = {
    "ism/direct": 1.053e-07,
    "ism/even_odd": 7.471e-07,
    "ism/odd_even": 7.813e-07,
    "ism/past_nism": 7.808e-07,
    "ism/chunks": 6.254e-07,
    "ism/near": 4.843e-06,
    "ism/singular": 3.095e-07,
    "ism/odd_count": 7.471e-07,
    "tail/fit": 3.100e-09,
    "tail/short": 3.213e-09,
    "tail/mean": 1.075e-08,
    "traj/random": 5.113e-06,
}


def noise_bounds(n):
    """Bounds on |mean| and |variance - 1| of n unit-variance logistic samples: four standard errors (the logistic
    distribution's kurtosis is 4.2, so the sample variance has variance 3.2 / n)."""
    return 4.0 / np.sqrt(n), 4.0 * np.sqrt(3.2 / n)


def ism_case(name, dtype=np.float64):
    src, rcv, nb, tdiff, c = ISM_CASES[name]
    nism, _ = sample_counts(tdiff, TMAX, FS)
    return ism(ROOM, BETA, src, rcv, nb, nism, FS, c, dtype)


def measure_gates():
    out = {}
    for name in ISM_CASES:
        out["ism/" + name] = float(np.abs(ism_case(name, np.float32).astype(np.float64) - ism_case(name)).max())
    for name, (case, tdiff, tmax, seed, _) in TAIL_CASES.items():
        src, rcv, nb, _, c = ISM_CASES[case]
        nism, ns = sample_counts(tdiff, tmax, FS)
        h = ism(ROOM, BETA, src, rcv, nb, nism, FS, c, np.float32)
        t32, _ = tail(h, ROOM, BETA, src, rcv, ns, FS, c, seed, np.float32)
        t64, _ = tail(h, ROOM, BETA, src, rcv, ns, FS, c, seed, np.float64)
        out["tail/" + name] = float(np.abs(t32.astype(np.float64) - t64).max())
    x, rirs, ts = traj_random_case()
    y32 = trajectory(x.astype(np.float32), rirs.astype(np.float32), ts, FS, np.float32)
    y64 = trajectory(x.astype(np.float32), rirs.astype(np.float32), ts, FS, np.float64)
    out["traj/random"] = float(np.abs(y32.astype(np.float64) - y64).max())
    return out


if __name__ == "__main__":
    for k, v in measure_gates().items():
        print('    "%s": %.3e,' % (k, v))
