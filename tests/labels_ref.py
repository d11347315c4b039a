"""numpy restatement of the label stage of the reference's ``Dataset.py``: the trajectory interpolation and
``cart2sph`` of ``RandomTrajectoryDataset.getRandomScene``, the ``Segmenting_SRPDNN`` transform and the padded ``gts`` dict of
``FixTrajectoryDataset.__getitem__``.  Every function takes ``dtype``: ``np.float64`` is the reference's own arithmetic, operation
for operation (tests/golden/g24_labels.npz pins ``cart2sph`` and the transform to the real reference bit for bit; the ``gts`` padding
is a restatement without a golden record); ``np.longdouble`` is the truth the
device gates are measured from.  The cases of the GPU tests are built here from +, -, *, / and comparisons only, so every host
regenerates the same bits.

Gates.  ``D64[case]`` is the measured distance of the float64 restatement from the longdouble one, max |.| over the case's
output; the device must stay within ``GATE x D64[case]`` of the longdouble result (``GATE = 8``: room for a 2-ulp device
``atan2`` and another summation order, and far below what any mutant of the transform moves).  tests/test_labels_ref_host.py
re-measures the table.
"""
import hashlib

import numpy as np

FS = 16000.0
GATE = 8.0
LD = np.longdouble


# ------------------------------------------------------------------------------------------------------------------------
# getRandomScene: interpolation and cart2sph
# ------------------------------------------------------------------------------------------------------------------------
def interp(x, xp, fp, dtype=np.float64):
    """``np.interp(x, xp, fp)`` in ``dtype``: numpy's slope form, the first / last value outside [xp[0], xp[-1]]."""
    x, xp, fp = (np.asarray(a, dtype=dtype) for a in (x, xp, fp))
    j = np.searchsorted(xp, x, side="right") - 1                     # the last point at or before x
    out = np.empty(x.shape, dtype=dtype)
    left, right = j < 0, (x > xp[-1]) | (j >= len(xp) - 1)
    out[left] = fp[0]
    out[right] = fp[-1]
    mid = ~(left | right)
    jm = j[mid]
    slope = (fp[jm + 1] - fp[jm]) / (xp[jm + 1] - xp[jm])
    val = slope * (x[mid] - xp[jm]) + fp[jm]
    out[mid] = np.where(xp[jm] == x[mid], fp[jm], val)
    return out


def cart2sph(cart, dtype=np.float64):
    """The reference's ``cart2sph`` [n, 3] -> [n, 3]: radius, elevation from the z axis down, azimuth."""
    cart = np.asarray(cart, dtype=dtype)
    xy2 = cart[:, 0] ** 2 + cart[:, 1] ** 2
    sph = np.zeros_like(cart)
    sph[:, 0] = np.sqrt(xy2 + cart[:, 2] ** 2)
    sph[:, 1] = np.arctan2(np.sqrt(xy2), cart[:, 2])
    sph[:, 2] = np.arctan2(cart[:, 1], cart[:, 0])
    return sph


def trajectory_doa(traj_pts, timestamps, n, fs, array_pos, dtype=np.float64):
    """``getRandomScene``'s last step -> (trajectory [n, 3, S], DOA [n, 2, S])."""
    pts = np.asarray(traj_pts, dtype=dtype)
    ts = np.asarray(timestamps, dtype=dtype)
    pos = np.asarray(array_pos, dtype=dtype)
    t = np.arange(n).astype(dtype) / dtype(fs)
    nsrc = pts.shape[2]
    traj = np.zeros((n, 3, nsrc), dtype=dtype)
    doa = np.zeros((n, 2, nsrc), dtype=dtype)
    for s in range(nsrc):
        traj[:, :, s] = np.array([interp(t, ts, pts[:, i, s], dtype) for i in range(3)]).transpose()
        doa[:, :, s] = cart2sph(traj[:, :, s] - pos, dtype)[:, 1:3]
    return traj, doa


# ------------------------------------------------------------------------------------------------------------------------
# Segmenting_SRPDNN
# ------------------------------------------------------------------------------------------------------------------------
def num_windows(L, K, step):
    return int(np.floor(L / step - K / step + 1))


def window_times(L, K, step, fs, mutant=None):
    if mutant == "tw_nw":                                            # one entry per window, always
        return np.arange(num_windows(L, K, step)) * step / fs
    return np.arange(0, (L - K), step) / fs


def segment_doa(doa, L, K, step, dtype=np.float64, mutant=None):
    """The DOA half of ``Segmenting_SRPDNN.__call__``: DOA [L, 2, S] -> DOAw [N_w, 2, S].  The rows the reference appends are
    never inside a window ((N_w - 1) step + K <= L) and are not built."""
    doa = np.asarray(doa, dtype=dtype)
    nw = num_windows(L, K, step)
    pi, two_pi = dtype(np.pi), dtype(2 * np.pi)
    out = []
    for s in range(doa.shape[2]):
        w = np.ascontiguousarray(np.stack([doa[i * step:i * step + K, :, s] for i in range(nw)]))       # [N_w, K, 2]
        if mutant != "no_plus_2pi":
            for i in np.flatnonzero(np.abs(np.diff(w[..., 1], axis=1)).max(axis=1) > pi) if K > 1 else ():
                w[i, w[i, :, 1] < 0, 1] += two_pi
        w = np.mean(w, axis=1)
        if mutant == "fold_elevation":                               # the fold taken on the whole row
            w[w[:, 1] > pi] -= two_pi
        elif mutant != "no_fold":
            w[w[:, 1] > pi, 1] -= two_pi
        out.append(w)
    return np.array(out).transpose(1, 2, 0)


def segment_vad(vad, L, K, step, mutant=None):
    """A VAD [n] or [n, S] (n <= L) -> its windows [N_w, K] or [N_w, K, S] in float64, as the reference leaves them."""
    v = np.asarray(vad)
    nw = num_windows(L, K, step)
    cols = v.reshape(v.shape[0], -1)
    if mutant == "no_vad_extension":                                 # the last sample repeated instead of zeros
        ext = np.append(cols, np.tile(cols[-1:], (L - cols.shape[0], 1)), axis=0).astype(np.float64)
    else:
        ext = np.append(cols, np.zeros((L - cols.shape[0], cols.shape[1])), axis=0)
    w = np.stack([ext[i * step:i * step + K] for i in range(nw)])
    return w[..., 0] if v.ndim == 1 else w


def transform(L, scene, K, step, dtype=np.float64, mutant=None):
    """``Segmenting_SRPDNN(K, step)(x, scene)`` for x of L samples; ``scene``: dict with DOA, mic_vad_sources, mic_vad, fs ->
    dict with DOAw, mic_vad_sources, mic_vad, tw."""
    if K > L:
        raise Exception('The window size can not be larger than the signal length ({})'.format(L))
    elif step > L:
        raise Exception('The window step can not be larger than the signal length ({})'.format(L))
    return {"DOAw": segment_doa(scene["DOA"], L, K, step, dtype, mutant),
            "mic_vad": segment_vad(scene["mic_vad"], L, K, step, mutant),
            "mic_vad_sources": segment_vad(scene["mic_vad_sources"], L, K, step, mutant),
            "tw": window_times(L, K, step, scene["fs"], mutant)}


def gts(segmented, dp_signals, max_source):
    """The ``gts`` dict of ``FixTrajectoryDataset.__getitem__`` for a batch: every scene zero-padded to ``max_source`` sources
    (the reference hard-codes 2 and its training shapes) and stacked.  ``segmented``: ``transform`` outputs; ``dp_signals``: per
    scene [L, M, S_b]."""
    nb = len(segmented)
    nw, _, _ = segmented[0]["DOAw"].shape
    K = segmented[0]["mic_vad_sources"].shape[1]
    L, m, _ = dp_signals[0].shape
    out = {"doa": np.zeros((nb, nw, 2, max_source), dtype=segmented[0]["DOAw"].dtype),
           "vad_sources": np.zeros((nb, nw, K, max_source)), "dp_signal": np.zeros((nb, L, m, max_source)),
           "num_source": np.zeros(nb, dtype=np.int64)}
    for b, (sg, dp) in enumerate(zip(segmented, dp_signals)):
        ns = sg["mic_vad_sources"].shape[-1]
        out["num_source"][b] = ns
        out["doa"][b, :, :, :ns] = sg["DOAw"]
        out["vad_sources"][b, :, :, :ns] = sg["mic_vad_sources"]
        out["dp_signal"][b, :, :, :ns] = dp
    out["vad_count"] = out["vad_sources"].sum(axis=2).astype(np.int32)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# cases (arithmetic only: +, -, *, / and comparisons, so they are the same bits everywhere)
# ------------------------------------------------------------------------------------------------------------------------
ARRAY_POS = np.array([2.0, 2.5, 1.25])
TRAJ_CASES = {"p3_s1": (3, 1), "p3_s2": (3, 2), "p50_s1": (50, 1), "p50_s2": (50, 2)}
TRAJ_N = 1000


def traj_case(name):
    """(traj_pts [P, 3, S], timestamps [P], n, fs, array_pos).  The timestamps start after sample 80 and end before the last
    sample, so both clamps are hit.  Path 0 passes BEHIND the array (x < 0, y through 0: the azimuth crosses +-pi); path 1
    passes 1 mm beside the array's xy, half a metre above it (the elevation nears 0).  P = 3, S = 1 takes path 0, P = 50,
    S = 1 path 1; both move."""
    npts, nsrc = TRAJ_CASES[name]
    u = np.arange(npts) / (npts - 1)
    bump = u * (1 - u)
    behind = np.stack([-1.0 + 0.2 * bump, -0.5 + u * 1.03, 0.3 - 0.1 * u], axis=1)        # y = 0 between two samples
    over = np.stack([-0.4 + u * 0.8 + 0.05 * bump, 0.001 + 0.0 * u, 0.5 + 0.02 * bump], axis=1)
    paths = [behind, over] if nsrc == 2 else [behind if npts == 3 else over]
    pts = np.stack(paths, axis=2) + ARRAY_POS[None, :, None]
    ts = 0.005 + np.arange(npts) * 0.05 / npts
    return pts, ts, TRAJ_N, FS, ARRAY_POS


SEG_SHAPES = [(1000, 100, 37), (1000, 64, 64), (1000, 300, 350), (1000, 1000, 1000), (1087, 257, 129), (72000, 3328, 3072)]


def seg_name(shape):
    return "seg_%d_%d_%d" % shape


def seg_case(L, K, step, seed=0):
    """One scene of four sources for the shape -> dict with DOA [L, 2, 4] float64, mic_vad_sources [Lv, 4] and mic_vad [Lv]
    (bool), fs.  In window w* = N_w // 2 source 0 crosses +pi a fifth into the window (the unwrapped mean exceeds pi: the fold
    is taken), source 1 four fifths into it (the mean stays below pi); source 2 stays at negative azimuths; source 3 is
    static.  Lv < L; for N_w > 1 the last window lies wholly in the VAD's zero extension."""
    nw = num_windows(L, K, step)
    t = np.arange(L) * 1.0
    t0 = (nw // 2) * step
    rate = 1.0 / L
    doa = np.zeros((L, 2, 4))
    for s, frac in ((0, 1), (1, 4)):
        cross = t0 + (frac * K) // 5 + 0.5                           # between two samples
        az = np.pi + rate * (t - cross)
        doa[:, 1, s] = np.where(az > np.pi, az - 2 * np.pi, az)
        doa[:, 0, s] = 1.0 + 0.5 * (t / L) - 0.3 * (t / L) * (t / L) + 0.1 * s
    doa[:, 1, 2] = -2.0 + t / L
    doa[:, 0, 2] = 1.5 - 0.25 * (t / L)
    doa[:, 1, 3] = 0.7
    doa[:, 0, 3] = 1.2
    lv = (nw - 1) * step - 1 if nw > 1 else L // 2
    rs = np.random.RandomState(1000 + seed)
    vs = rs.randint(0, 2, (lv, 4)).astype(bool)
    vs[:, 3] = True
    return {"DOA": doa, "mic_vad_sources": vs, "mic_vad": vs.any(axis=1), "fs": FS}


def sub_scene(case, sources):
    """The scene restricted to some of its sources."""
    idx = list(sources)
    vs = case["mic_vad_sources"][:, idx]
    return {"DOA": np.ascontiguousarray(case["DOA"][:, :, idx]), "mic_vad_sources": vs, "mic_vad": vs.any(axis=1), "fs": case["fs"]}


# the golden cases of tests/golden/g24_labels.npz: the shapes with L <= 2000, two sources each
GOLDEN_SEG = [((1000, 100, 37), (0, 1)), ((1000, 64, 64), (2, 3)), ((1000, 300, 350), (0, 3)), ((1000, 1000, 1000), (1, 0)),
              ((1087, 257, 129), (1, 2))]


def digest(*arrays):
    """sha256 of the arrays' bytes as a uint8 vector: the golden file names its inputs by it instead of storing them."""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def dist(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)))) if np.asarray(a).size else 0.0


def measure_d64(name):
    """The distance of the float64 restatement from the longdouble one for a case of ``D64``."""
    kind, _, rest = name.partition("/")
    if kind in ("traj", "doa"):
        a = trajectory_doa(*traj_case(rest))
        b = trajectory_doa(*traj_case(rest), dtype=LD)
        return dist(a[0], b[0]) if kind == "traj" else dist(a[1], b[1])
    shape = tuple(int(v) for v in rest.split("_")[1:])
    c = seg_case(*shape)
    return dist(segment_doa(c["DOA"], *shape), segment_doa(c["DOA"], *shape, dtype=LD))


# measured (tests/test_labels_ref_host.py re-measures them): max |float64 - longdouble|
D64 = {
    "traj/p3_s1": 3.062e-16,
    "doa/p3_s1": 4.907e-16,
    "traj/p3_s2": 3.263e-16,
    "doa/p3_s2": 1.681e-13,                   # 1 mm beside the array: the trajectory's last bit is 1e-13 rad of azimuth
    "traj/p50_s1": 2.667e-16,
    "doa/p50_s1": 2.049e-14,
    "traj/p50_s2": 2.886e-16,
    "doa/p50_s2": 2.049e-14,
    "seg/seg_1000_100_37": 1.998e-15,
    "seg/seg_1000_64_64": 1.554e-15,
    "seg/seg_1000_300_350": 6.661e-15,
    "seg/seg_1000_1000_1000": 2.265e-14,
    "seg/seg_1087_257_129": 5.773e-15,
    "seg/seg_72000_3328_3072": 7.216e-14,       # numpy's mean over a middle axis adds the K rows one after another
}
