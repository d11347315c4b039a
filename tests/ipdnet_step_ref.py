"""numpy restatements of the three kernels of the IPDnet training step (csrc/ipdnet_step.hip) and the inputs of
golden G19 — test infrastructure, product code never imports it.

    pit_mse(pred, gt)          cal_loss (IPDnet/runIPDnetOn.py:196-206): float64 brute force over every permutation
    dp_vad(mix_spec, dp_spec)  cal_vad (:224-235) from given spectra
    ipdnet_targets(...)        the ground-truth half of data_preprocess (:256-283) in closed form
    g19_batch()                the waveforms / DOAs / array of tests/golden/g19_ipdnet_step.npz, from seeds
"""
import itertools

import numpy as np

SEG = 12
G19_MICS = np.array(((-0.04, 0.0, 0.0), (0.04, 0.0, 0.0), (0.0, 0.05, 0.01), (0.02, -0.03, 0.0)), dtype=np.float32)
G19_SHAPE = (2, 4, 2, 36)                                    # utterances, microphones, sources, frames


def _rs_randn(seed, shape, scale=1.0):
    """conftest.rs_randn (restated: the golden generator runs outside pytest)."""
    return (np.random.RandomState(int(seed)).standard_normal(size=tuple(int(s) for s in shape)) * scale).astype(np.float32)


def g19_batch():
    """(mic_sig [nb, ns, nch], dp_signal [nb, ns, nch, nsrc], doa [nb, nseg, 2, nsrc], mic_pos [nch, 3]), float32.
    Each source is white noise, its direct path at microphone c a delay of c samples; utterance 0's second source is
    silent throughout, utterance 1's first source stops after the first segment; the mixture is the sum of the direct
    paths plus white noise at half their level."""
    nb, nch, nsrc, nt = G19_SHAPE
    ns = 512 + (nt - 1) * 256
    src = _rs_randn(1900, (nb, ns + nch, nsrc), 0.05)
    src[0, :, 1] = 0.0
    src[1, SEG * 256 + nch:, 0] = 0.0
    dp = np.stack([src[:, nch - c:nch - c + ns, :] for c in range(nch)], axis=2)          # [nb, ns, nch, nsrc]
    mic = dp.sum(axis=3) + _rs_randn(1901, (nb, ns, nch), 0.025)
    rs = np.random.RandomState(1902)
    doa = np.stack((rs.uniform(0.2, np.pi - 0.2, (nb, nt // SEG, nsrc)), rs.uniform(-np.pi, np.pi, (nb, nt // SEG, nsrc))),
                   axis=2).astype(np.float32)
    return mic.astype(np.float32), np.ascontiguousarray(dp, dtype=np.float32), doa, G19_MICS.copy()


def perm_list(nsrc):
    return list(itertools.permutations(range(nsrc)))


def pit_mse(pred, gt):
    """pred, gt [rows, D, nsrc] (any float dtype; evaluated in float64).  Returns (loss, perm index per row, dpred):
    per row the permutation pm (``itertools.permutations`` order, strict ``<``: ties keep the earliest) minimising
    sum_j sum_d (pred[d, pm[j]] - gt[d, j])^2;  loss = mean over every element of the permuted difference squared."""
    p, g = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    rows, d, nsrc = p.shape
    perms = perm_list(nsrc)
    e = ((p[:, :, :, None] - g[:, :, None, :]) ** 2).sum(axis=1)                           # E[row, i, j]
    best = np.zeros(rows, dtype=np.int64)
    best_cost = np.full(rows, np.inf)
    for k, pm in enumerate(perms):
        cost = np.zeros(rows)
        for j in range(nsrc):
            cost = cost + e[:, pm[j], j]
        take = cost < best_cost
        best[take], best_cost[take] = k, cost[take]
    n_total = p.size
    dpred = np.zeros_like(p)
    for k, pm in enumerate(perms):
        r = np.nonzero(best == k)[0]
        for j in range(nsrc):
            dpred[r, :, pm[j]] = 2.0 * (p[r, :, pm[j]] - g[r, :, j]) / n_total
    return best_cost.sum() / n_total, best, dpred


def dp_vad(mix_spec, dp_spec, dtype=np.float64):
    """mix_spec [nb, nch, nt, 257] complex, dp_spec [nb, nsrc, nt, 257] complex (the direct paths at microphone 0)
    -> [nb, nt // 12, nsrc]: mean over the segment's frames of the mean over bins of |dp| / |mix channel 0|."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.abs(dp_spec).astype(dtype) / np.abs(mix_spec[:, :1]).astype(dtype)      # [nb, nsrc, nt, 257]
    per_frame = ratio.mean(axis=3)
    nb, nsrc, nt = per_frame.shape
    nseg = nt // SEG
    return per_frame[:, :, :nseg * SEG].reshape(nb, nsrc, nseg, SEG).mean(axis=3).transpose(0, 2, 1)


def bessel_j0(x):
    """J0 by the mid-point rule of its integral, mean over theta in (0, pi) of cos(x sin theta), 1024 points."""
    th = (np.arange(1024) + 0.5) * (np.pi / 1024)
    return np.cos(np.asarray(x, dtype=np.float64)[..., None] * np.sin(th)).mean(axis=-1)


def non_source_target(mic_pos, bins=range(1, 257)):
    """euclidean_distances_to_bessel (:209-221): [512, nmic - 1] = [J0(2 pi f_k d_m / 340) | zeros(256)]."""
    mic = np.asarray(mic_pos)
    dist = np.sqrt(np.sum((mic[1:] - mic[0]) ** 2, axis=1))
    freq = (2 * np.pi * np.linspace(0, 8000, 257) / 340)[list(bins)]
    return np.concatenate((bessel_j0(freq[:, None] * dist[None, :]), np.zeros((256, len(dist)))), axis=0).astype(np.float32)


def ipdnet_targets(doa, vad, mic_pos, non_source, bin0=1, nf_used=256, nbins=257, fre_max=8000.0, speed=340.0, th=0.001):
    """doa [nb, nseg, 2, nsrc] float32, vad [nb, nseg, nsrc] or None, mic_pos [nmic, 3] float32 ->
    [nb, nseg, 2 nf_used, nmic - 1, nsrc] float32.  The delay is formed in float32 (the reference's ``DPIPD.forward``
    is handed float32 DOAs and a float32 array: Module.py:380-388), the phase in float64 (:389-393)."""
    doa, mic = np.asarray(doa, dtype=np.float32), np.asarray(mic_pos, dtype=np.float32)
    ele, azi = doa[:, :, 0, :], doa[:, :, 1, :]
    r = np.stack((np.sin(ele) * np.cos(azi), np.sin(ele) * np.sin(azi), np.cos(ele)), axis=-1)   # [nb, nseg, nsrc, 3] float32
    diff = mic[:1] - mic[1:]                                                                # mic_0 - mic_m, float32
    tau = ((r[..., None, 0] * diff[:, 0] + r[..., None, 1] * diff[:, 1]) + r[..., None, 2] * diff[:, 2]) / np.float32(speed)
    f = np.arange(bin0, bin0 + nf_used) * (float(fre_max) / (nbins - 1))
    ph = (2 * np.pi * f)[None, None, None, :, None] * tau.astype(np.float64)[:, :, :, None, :]   # [nb, nseg, nsrc, nf, nm1]
    ipd = np.concatenate((np.cos(ph), np.sin(ph)), axis=3).astype(np.float32).transpose(0, 1, 3, 4, 2)
    if vad is None:
        return ipd
    v = np.asarray(vad, dtype=np.float32)[:, :, None, None, :]
    ns_t = np.asarray(non_source, dtype=np.float32)[None, None, :, :, None]
    out = np.where(v > np.float32(th), ipd, np.where(v <= np.float32(th), ns_t, np.float32(np.nan)))
    return out.astype(np.float32)
