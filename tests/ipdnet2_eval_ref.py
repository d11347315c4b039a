"""Float64 numpy restatement of IPDnet2's evaluation, and the seeded inputs of the G21 fixture.

    near-field targets   DPIPD2.forward(source_doa, source_distance)        IPDnet2/Module.py:443-483
    gating, Bessel fill  MyModel.data_preprocess                            IPDnet2/run_IPDnet2.py:290-322, 252-264
    MSE template search  PredDOA.pred2DOA_track                             IPDnet2/Module.py:573-666
    evaluation rules     PredDOA.evaluate, getMetric.forward 'multiple'     IPDnet2/Module.py:669-706, 144-238

Everything is float64 from the float32 inputs; the thresholds are the fp32 values torch compares against, as in
tests/doa_metric_ref.py, whose assignment (``lsap`` / ``assign`` / ``judge_assignment``) and azimuth error are used here.
"""
import numpy as np

from doa_metric_ref import assign, azi_error, judge_assignment

SPEED = 340.0
VAD_SCALE = 0.2919                      # PredDOA.evaluate: vad_est / 0.2919
VAD_TH = (0.001, 0.4)
AE_TH = 5
RATIO_EPS = 1e-6
RES_PHI = 360


def freqs(nbins=257, fre_max=8000.0):
    return np.linspace(0.0, fre_max, nbins)[1:nbins]


def nearfield_targets(doa, distance, mic, speed=SPEED):
    """doa [nb, nt, 2, nsrc] (elevation, azimuth; radians), distance [nb, nt, nsrc], mic [nmic, 3] ->
    [nb, nt, 512, nmic - 1, nsrc] float64 = [cos | sin](2 pi f tau_m), tau_m = (|src - mic_m| - |src - mic_0|) / speed,
    src = distance * r(doa).  Every operation in float64."""
    doa, distance = np.asarray(doa, dtype=np.float64), np.asarray(distance, dtype=np.float64)
    mic = np.asarray(mic, dtype=np.float64).reshape(-1, 3)
    ele, azi = doa[:, :, 0, :], doa[:, :, 1, :]
    src = np.stack((distance * np.sin(ele) * np.cos(azi), distance * np.sin(ele) * np.sin(azi), distance * np.cos(ele)), axis=-1)
    dist = np.sqrt(((src[..., None, :] - mic) ** 2).sum(axis=-1))         # [nb, nt, nsrc, nmic]
    tau = (dist[..., 1:] - dist[..., :1]) / speed                         # [nb, nt, nsrc, nmic - 1]
    ph = 2 * np.pi * freqs()[None, None, None, :, None] * tau[:, :, :, None, :]
    return np.concatenate((np.cos(ph), np.sin(ph)), axis=3).transpose(0, 1, 3, 4, 2)


def farfield_targets(doa, mic, speed=SPEED):
    """The far-field form of IPDnet's DPIPD.forward on the same layout: tau_m = r(doa) . (mic_0 - mic_m) / speed."""
    doa = np.asarray(doa, dtype=np.float64)
    mic = np.asarray(mic, dtype=np.float64).reshape(-1, 3)
    ele, azi = doa[:, :, 0, :], doa[:, :, 1, :]
    r = np.stack((np.sin(ele) * np.cos(azi), np.sin(ele) * np.sin(azi), np.cos(ele)), axis=-1)
    tau = r @ (mic[0] - mic[1:]).T / speed
    ph = 2 * np.pi * freqs()[None, None, None, :, None] * tau[:, :, :, None, :]
    return np.concatenate((np.cos(ph), np.sin(ph)), axis=3).transpose(0, 1, 3, 4, 2)


def bessel_target(mic, j0=None):
    """[512, nmic - 1] float64 = [J0(2 pi f_k d_m / 340) | zeros(256)], d_m the distance of microphone m from microphone 0.
    ``j0``: a Bessel function of order 0 (scipy.special.j0 where installed); default the mid-point rule on 1024 points."""
    mic = np.asarray(mic, dtype=np.float64).reshape(-1, 3)
    dist = np.sqrt(((mic[1:] - mic[0]) ** 2).sum(axis=1))
    x = (2 * np.pi * freqs() / SPEED)[:, None] * dist[None, :]
    if j0 is None:
        th = (np.arange(1024) + 0.5) * (np.pi / 1024)
        val = np.cos(x[..., None] * np.sin(th)).mean(axis=-1)
    else:
        val = j0(x)
    return np.concatenate((val, np.zeros_like(val)), axis=0)


def gate_targets(ipd, vad, non_source, th=0.0):
    """ipd [nb, nt, 512, nmic - 1, nsrc], vad [nb, nt, nsrc]: a (frame, source) slot keeps its target when vad > th, takes
    the non-source target when vad <= th, and is NaN when the VAD is NaN."""
    out = np.array(ipd, dtype=np.float64, copy=True)
    vad = np.asarray(vad, dtype=np.float64)
    th = float(np.float32(th))
    silent, nan = vad <= th, np.isnan(vad)
    fill = np.broadcast_to(np.asarray(non_source, dtype=np.float64)[None, None, :, :, None], out.shape)
    m = np.broadcast_to(silent[:, :, None, None, :], out.shape)
    out[m] = fill[m]
    out[np.broadcast_to(nan[:, :, None, None, :], out.shape)] = np.nan
    return out


def candidate_bank(mic, res_phi=RES_PHI, speed=SPEED):
    """([nazi, 512, nmic - 1] float64, azi [nazi]): [cos | sin] of bins 1..256 of exp(-j 2 pi f r . (mic_m - mic_0) / speed),
    elevation pi / 2, azimuth linspace(-pi, pi, res_phi) (DPIPD2.__init__ :416-441, pred2DOA_track :585)."""
    mic = np.asarray(mic, dtype=np.float64).reshape(-1, 3)
    azi = np.linspace(-np.pi, np.pi, res_phi)
    r = np.stack((np.sin(np.pi / 2) * np.cos(azi), np.sin(np.pi / 2) * np.sin(azi), np.full_like(azi, np.cos(np.pi / 2))), axis=1)
    itd = r @ (mic[1:] - mic[0]).T / speed
    ph = -2 * np.pi * freqs()[None, :, None] * itd[:, None, :]
    return np.concatenate((np.cos(ph), np.sin(ph)), axis=1), azi


def argmin_first(scores):
    """torch.argmin over the last axis: a NaN counts as the minimum and the first one wins, else the first minimum."""
    scores = np.asarray(scores)
    nan = np.isnan(scores)
    return np.where(nan.any(axis=-1), nan.argmax(axis=-1), np.where(nan, np.inf, scores).argmin(axis=-1))


def mse_search(pred, bank, nsrc=1, unk_num=True):
    """pred [nb, nt, nf2, np, ntrack], bank [ncand, nf2, np] -> (idx [ntrack, nb, nt, nsrc], vad [ntrack, nb, nt, nsrc],
    ss [ntrack, nb, nt, ncand], scores [ntrack, nb, nt, nsrc, ncand]) in float64: per source the MSE of every candidate, its
    first minimum, that MSE as the activity, then the winning template subtracted whole."""
    pred, bank = np.asarray(pred, dtype=np.float64), np.asarray(bank, dtype=np.float64)
    nb, nt, nf2, npair, ntrack = pred.shape
    flat = bank.reshape(bank.shape[0], -1)                                # index k * np + p
    res = pred.transpose(4, 0, 1, 2, 3).reshape(ntrack, nb, nt, -1).copy()
    idx = np.empty((ntrack, nb, nt, nsrc), np.int64)
    vad = np.empty((ntrack, nb, nt, nsrc))
    scores = np.empty((ntrack, nb, nt, nsrc, flat.shape[0]))
    for s in range(nsrc):
        sc = ((res[..., None, :] - flat) ** 2).mean(axis=-1)
        scores[..., s, :] = sc
        idx[..., s] = argmin_first(sc)
        vad[..., s] = np.take_along_axis(sc, idx[..., s:s + 1], axis=-1)[..., 0] if unk_num else 1.0
        res = res - flat[idx[..., s]]
    return idx, vad, scores[..., 0, :], scores


def get_metric2(doa_gt, vad_gt, doa_est, vad_est, ae_TH=AE_TH, vad_TH=VAD_TH, est_below=True, ratio_eps=RATIO_EPS, inf=10000,
                invalid=10, eps=1e-5):
    """IPDnet2's getMetric 'multiple' on the azimuth (IPDnet2/Module.py:144-238): doa_* [nb, nt, 2, ns] in DEGREES, vad_*
    [nb, nt, ns].  An estimate is active when vad_est < vad_TH[1] (``est_below``; False: >), ACC / MDR / FAR divide by
    K_gt + ratio_eps.  Returns the five metrics, the per-utterance counts and the well-posedness figures of
    tests/doa_metric_ref.get_metric."""
    doa_gt, doa_est = np.asarray(doa_gt, dtype=np.float64), np.asarray(doa_est, dtype=np.float64)
    nb, nt, _, ns_gt = doa_gt.shape
    ns_est = doa_est.shape[3]
    th = float(np.float32(ae_TH))
    t0, t1 = float(np.float32(vad_TH[0])), float(np.float32(vad_TH[1]))
    vg64, ve64 = np.asarray(vad_gt, dtype=np.float64), np.asarray(vad_est, dtype=np.float64)
    vg, ve = vg64 > t0, (ve64 < t1 if est_below else ve64 > t1)
    out = {"vad_margin": min(np.abs(vg64 - t0).min(), np.abs(ve64 - t1).min()), "gap": np.inf, "th_margin": np.inf, "tie_safe": True}
    acc, mdr, far, mae, rmse = (np.zeros(nb) for _ in range(5))
    kg, ke, kc = np.zeros(nb, np.int64), np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    for b in range(nb):
        s1 = s2 = 0.0
        for t in range(nt):
            gi = [s for s in range(ns_gt) if vg[b, t, s]]
            ei = [s for s in range(ns_est) if ve[b, t, s]] if gi else []
            kg[b] += len(gi)
            ke[b] += len(ei)
            if not gi or not ei:
                continue
            az = np.array([[azi_error(doa_est[b, t, 1, e], doa_gt[b, t, 1, g]) for e in ei] for g in gi])
            out["th_margin"] = min(out["th_margin"], np.abs(az - th).min())
            cost = np.where(az > th, float(inf), az)
            rows, cols, _tot, gap, tie_safe = assign(cost)
            out["gap"] = min(out["gap"], gap)
            out["tie_safe"] = out["tie_safe"] and tie_safe
            final = judge_assignment(cost, rows, cols, float(inf), invalid)
            for r in range(len(gi)):
                if final[r] != invalid:
                    kc[b] += 1
                    s1 += az[r, final[r]]
                    s2 += az[r, final[r]] ** 2
        with np.errstate(invalid="ignore", divide="ignore"):
            g, c, e_ = np.float64(kg[b]), np.float64(kc[b]), np.float64(ke[b])
            acc[b], mdr[b], far[b] = c / (g + ratio_eps), (g - c) / (g + ratio_eps), (e_ - c) / (g + ratio_eps)
            mae[b], rmse[b] = s1 / (c + eps), np.sqrt(s2 / (c + eps))
    out.update({"ACC": acc.mean(), "MDR": mdr.mean(), "FAR": far.mean(), "MAE": mae.mean(), "RMSE": rmse.mean(), "K_gt": kg, "K_est": ke,
                "K_corr": kc, "active_est": ve})
    return out


def evaluate(doa_est_rad, mse_act, azi_gt_deg, vad_gt, **kw):
    """PredDOA.evaluate (:669-706): doa_gt = [azi, azi] in degrees, the estimates in radians -> degrees, the activities
    divided by 0.2919."""
    azi_gt_deg = np.asarray(azi_gt_deg, dtype=np.float64)
    doa_gt = np.stack((azi_gt_deg, azi_gt_deg), axis=2)
    return get_metric2(doa_gt, vad_gt, np.asarray(doa_est_rad, dtype=np.float64) * 180 / np.pi,
                       np.asarray(mse_act, dtype=np.float64) / VAD_SCALE, **kw)


def metric_vector(ref):
    return np.array([ref[k] for k in ("ACC", "MDR", "FAR", "MAE", "RMSE")], np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs (the G21 fixture stores only results)
# ---------------------------------------------------------------------------------------------------------------------
def _circle(radius, n, phase):
    a = phase + 2 * np.pi * np.arange(n) / n
    return np.stack((radius * np.cos(a), radius * np.sin(a), np.zeros(n)), axis=1)


# float64 tables, as the reference keeps them: two microphones 8 cm apart on an axis turned by 0.3 rad (so that a
# direction and its mirror image about the axis do not both fall on the 360-point grid), and four microphones on a circle
# of 3 cm with a fifth in the centre
G21_MICS = {"mic2": np.array(((-0.04 * np.cos(0.3), -0.04 * np.sin(0.3), 0.0), (0.04 * np.cos(0.3), 0.04 * np.sin(0.3), 0.0))),
            "mic5": np.concatenate((_circle(0.03, 4, 0.2), np.zeros((1, 3))), axis=0)}
# seeds chosen so that the generator's well-posedness asserts hold on the reference's own output
# (two microphones cannot tell the directions near their own axis apart: their delay is stationary there and adjacent
# candidates score alike, so that case draws its azimuths from the two broadside sectors, 40 degrees off the axis)
_AXIS2 = 0.3 * 180 / np.pi
G21_CASES = {"mic2": dict(mic="mic2", seed=3251, silent_utt=(), sectors=((_AXIS2 + 40, _AXIS2 + 140), (_AXIS2 - 140, _AXIS2 - 40))),
             "mic5": dict(mic="mic5", seed=3672, silent_utt=(), sectors=((-170.0, 170.0),)),
             "mic5_silent": dict(mic="mic5", seed=3153, silent_utt=(1,), sectors=((-170.0, 170.0),))}
G21_NB, G21_NT, G21_NSRC = 2, 6, 2


def g21_inputs(name):
    """The seeded batch of case ``name``: a dict of float32 arrays (mic: float64)
        azi_deg  [nb, nt, nsrc]   the dataset's azimuth labels in degrees
        doa      [nb, nt, 2, nsrc] (pi / 2, azimuth) in radians, formed in fp32 as run_IPDnet2.py:290-292 does
        distance [nb, nt, nsrc]   0.3 .. 3 m
        vad      [nb, nt, nsrc]   the per-frame label: 1 / 0, some frames with one active source
        pred     [nb, nt, 512, nmic - 1, 2]: per track the near-field DP-IPD of one source (tracks in swapped order on odd
                 frames) plus white noise of a small or a large variance, so that the MSE activities fall on both sides
                 of 0.4 * 0.2919
    """
    c = G21_CASES[name]
    mic = G21_MICS[c["mic"]]
    rng = np.random.RandomState(c["seed"])
    nb, nt, nsrc = G21_NB, G21_NT, G21_NSRC
    sectors = np.asarray(c["sectors"], dtype=np.float64)
    azi_deg = rng.uniform(0.0, 1.0, (nb, nt, nsrc))
    if len(sectors) > 1:
        pick = sectors[rng.randint(0, len(sectors), (nb, nt, nsrc))]
        azi_deg = pick[..., 0] + azi_deg * (pick[..., 1] - pick[..., 0])
    else:                                                                  # (one sector: the draw order of the first version)
        azi_deg = sectors[0, 0] + azi_deg * (sectors[0, 1] - sectors[0, 0])
    azi_deg = azi_deg.astype(np.float32)
    ele_deg = np.full_like(azi_deg, 90.0)
    doa = (np.stack((ele_deg, azi_deg), axis=2) / np.float32(180) * np.float32(np.pi)).astype(np.float32)
    distance = rng.uniform(0.3, 3.0, (nb, nt, nsrc)).astype(np.float32)
    distance[0, 0, 0], distance[0, 1, 1] = 0.3, 3.0
    vad = (rng.rand(nb, nt, nsrc) < 0.75).astype(np.float32)
    vad[0, 0], vad[0, 1], vad[0, 2] = (1, 1), (1, 0), (0, 1)
    for b in c["silent_utt"]:
        vad[b] = 0
    clean = nearfield_targets(doa, distance, mic)                          # [nb, nt, 512, nmic - 1, nsrc]
    clean[:, 1::2] = clean[:, 1::2, :, :, ::-1]
    sigma = np.where(rng.rand(nb, nt, 1, 1, nsrc) < 0.65, 0.2, 0.5)
    pred = clean + sigma * rng.standard_normal(clean.shape)
    return {"mic": mic, "azi_deg": azi_deg, "doa": doa, "distance": distance, "vad": vad, "pred": pred.astype(np.float32)}
