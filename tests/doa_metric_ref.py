"""Float64 numpy restatement of the reference's DOA evaluation, and the seeded inputs of the G20 fixture.

    getMetric.forward 'single'    FN-SSL/Lightning/Module.py:140-180
    getMetric.forward 'multiple'  FN-SSL/Lightning/Module.py:182-276, IPDnet/Module.py:143-237
    judge_assignment              as written (:278-285 / :239-246)
    PredDOA.pred2DOA              IPDnet/Module.py:463-579

The assignment needs no scipy: ``lsap`` restates the algorithm behind ``scipy.optimize.linear_sum_assignment`` (so that
exactly tied optima fall as they do there — with more ground truths than estimates a 10000-cost pair ties whichever row
takes it, and ``judge_assignment`` as written then gives different counts for the tied choices), and every call is checked
against an exhaustive search, which also yields the tie figures.  Sums are float64; the THRESHOLDS are the fp32 values torch compares
against (``tensor_fp32 > 0.001`` rounds the scalar to fp32 first), so that an input exactly at a threshold is decided as
the reference decides it.  Besides the metrics every function returns the integer per-utterance counts, the smallest
distance of an azimuth error from ``ae_TH`` / of a VAD from its threshold, and the smallest gap between the best and
the nearest different assignment total — the well-posedness figures the fixture generator and the GPU tests assert on.
"""
import itertools

import numpy as np

AE_ORDER = ("azi", "ele", "aziele")


def degrees(x):
    return np.asarray(x, dtype=np.float64) * 180 / np.pi


def azi_error(est, gt):
    return np.abs(np.mod(est - gt + 180, 360) - 180)                    # np.mod is floored, like torch's %


def ele_error(est, gt):
    return np.abs(est - gt)


def aziele_error(ele_est, azi_est, ele_gt, azi_gt):
    eg, ag, ee, ae = (np.asarray(v, dtype=np.float64) / 180 * np.pi for v in (ele_gt, azi_gt, ele_est, azi_est))
    aux = np.cos(eg) * np.cos(ee) + np.sin(eg) * np.sin(ee) * np.cos(ag - ae)
    aux = np.clip(aux, -0.99999, 0.99999)
    return np.abs(np.arccos(aux)) * 180 / np.pi


def assign_exhaustive(cost):
    """Minimum-total-cost assignment of a (<= 4 x 4) matrix by exhaustive search.  Returns (total, optimal, gap): the best
    total, the list of ALL assignments that reach it (to 1e-9 relative: the same terms summed in another order; each a
    sorted list of (row, col)), and the distance to the best total beyond that (inf when there is none)."""
    n, m = cost.shape
    small, big = (n, m) if n <= m else (m, n)
    every = []
    for p in itertools.permutations(range(big), small):
        pairs = sorted((i, p[i]) if n <= m else (p[i], i) for i in range(small))
        every.append((sum(float(cost[r, c]) for r, c in pairs), pairs))
    tot = min(t for t, _ in every)
    same = 1e-9 * max(1.0, abs(tot))
    worse = [t for t, _ in every if t - tot > same]
    return tot, [p for t, p in every if t - tot <= same], (min(worse) - tot) if worse else np.inf


def lsap(cost):
    """The shortest-augmenting-path algorithm scipy.optimize.linear_sum_assignment runs (Crouse's rectangular LSAP), step for
    step in float64, so that exact ties fall as they do there: rows in order; the unassigned columns are scanned from the
    highest index down, a column replaces the current minimum when it is strictly lower, or equal and still free; a matrix
    with more rows than columns is solved transposed and the pairs sorted by row.  Returns (rows, cols)."""
    cost = np.asarray(cost, dtype=np.float64)
    tr = cost.shape[1] < cost.shape[0]
    c = cost.T if tr else cost
    nr, nc = c.shape
    u, v = np.zeros(nr), np.zeros(nc)
    path, col4row, row4col = [-1] * nc, [-1] * nr, [-1] * nc
    for cur in range(nr):
        min_val, i, sink = 0.0, cur, -1
        remaining = [nc - it - 1 for it in range(nc)]
        SR, SC, spc = [False] * nr, [False] * nc, [np.inf] * nc
        while sink == -1:
            index, lowest = -1, np.inf
            SR[i] = True
            for it, j in enumerate(remaining):
                r = min_val + c[i, j] - u[i] - v[j]
                if r < spc[j]:
                    path[j], spc[j] = i, r
                if spc[j] < lowest or (spc[j] == lowest and row4col[j] == -1):
                    lowest, index = spc[j], it
            min_val = lowest
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            remaining[index] = remaining[-1]
            remaining.pop()
        u[cur] += min_val
        for k in range(nr):
            if SR[k] and k != cur:
                u[k] += min_val - spc[col4row[k]]
        for j in range(nc):
            if SC[j]:
                v[j] -= min_val - spc[j]
        j = sink
        while True:
            k = path[j]
            row4col[j] = k
            col4row[k], j = j, col4row[k]
            if k == cur:
                break
    if not tr:
        return list(range(nr)), list(col4row)
    pairs = sorted((col4row[k], k) for k in range(nr))
    return [r for r, _ in pairs], [k for _, k in pairs]


def assign(cost):
    """(rows, cols, total, gap, tie_safe): the pair list ``lsap`` gives, checked against the exhaustive optimum; ``gap`` is the
    distance from the optimum to the nearest different total, ``tie_safe`` says that all exactly tied optima agree on their
    VALID pairs (they differ only in which row takes a 10000-cost estimate — the one tie that is decided by the algorithm's
    steps, not by rounding)."""
    rows, cols = lsap(cost)
    tot, optimal, gap = assign_exhaustive(cost)
    assert sorted(zip(rows, cols)) in optimal, (cost, rows, cols, tot)
    big = cost.max()
    valid = {tuple(p for p in pairs if cost[p] != big or big <= 360) for pairs in optimal}
    return rows, cols, tot, gap, len(valid) == 1


def judge_assignment(cost, rows, cols, inf, invalid):
    final = [invalid] * cost.shape[0]
    for i in range(min(cost.shape)):
        if cost[rows[i], cols[i]] != inf:
            final[rows[i]] = cols[i]
        else:
            final[i] = invalid                                            # as written: position i, not rows[i]
    return final


def get_metric(doa_gt, vad_gt, doa_est, vad_est, source_mode, ae_mode=("azi",), ae_TH=30, useVAD=True, vad_TH=(0.5, 0.5),
               inf=10000, invalid=10, eps=1e-5):
    """doa_* [nb, nt, 2, ns] in DEGREES, vad_* [nb, nt, ns].  Returns a dict: 'ACC', ('MDR', 'FAR'), 'MAE' / 'RMSE' as
    {mode: value} for the modes of ``ae_mode``, 'K_gt', 'K_est', 'K_corr' int64 [nb], 'th_margin', 'vad_margin', 'gap'."""
    doa_gt, doa_est = np.asarray(doa_gt, dtype=np.float64), np.asarray(doa_est, dtype=np.float64)
    nb, nt, _, ns_gt = doa_gt.shape
    ns_est = doa_est.shape[3]
    th = float(np.float32(ae_TH))
    vad_margin = np.inf
    if useVAD:
        t0, t1 = float(np.float32(vad_TH[0])), float(np.float32(vad_TH[1]))
        vg64, ve64 = np.asarray(vad_gt, dtype=np.float64), np.asarray(vad_est, dtype=np.float64)
        vad_margin = min(np.abs(vg64 - t0).min(), np.abs(ve64 - t1).min())
        vg, ve = vg64 > t0, ve64 > t1
    else:
        vg, ve = np.ones((nb, nt, ns_gt), bool), np.ones((nb, nt, ns_est), bool)
    modes = [m for m in AE_ORDER if m in ae_mode]
    out = {"vad_margin": vad_margin, "gap": np.inf, "th_margin": np.inf, "tie_safe": True}

    def errs(b, t, e, g):
        return {"azi": azi_error(doa_est[b, t, 1, e], doa_gt[b, t, 1, g]), "ele": ele_error(doa_est[b, t, 0, e], doa_gt[b, t, 0, g]),
                "aziele": aziele_error(doa_est[b, t, 0, e], doa_est[b, t, 1, e], doa_gt[b, t, 0, g], doa_gt[b, t, 1, g])}

    if source_mode == "single":
        ve = ve & vg
        az = azi_error(doa_est[:, :, 1, :], doa_gt[:, :, 1, :])
        if vg.any():
            out["th_margin"] = np.abs(az[vg] - th).min()
        corr = (az < th) & ve
        el = ele_error(doa_est[:, :, 0, :], doa_gt[:, :, 0, :])
        azel = aziele_error(doa_est[:, :, 0, :], doa_est[:, :, 1, :], doa_gt[:, :, 0, :], doa_gt[:, :, 1, :])
        e = {"azi": az, "ele": el, "aziele": azel}
        with np.errstate(invalid="ignore", divide="ignore"):
            out["ACC"] = np.float64(corr.sum()) / np.float64(vg.sum())
            out["MAE"] = {m: np.float64((vg * e[m]).sum()) / np.float64(vg.sum()) for m in modes}
        out["K_gt"], out["K_est"], out["K_corr"] = vg.sum(axis=(1, 2)), ve.sum(axis=(1, 2)), corr.sum(axis=(1, 2))
        return out

    acc, mdr, far = np.zeros(nb), np.zeros(nb), np.zeros(nb)
    mae, rmse = {m: np.zeros(nb) for m in modes}, {m: np.zeros(nb) for m in modes}
    kg, ke, kc = np.zeros(nb, np.int64), np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    for b in range(nb):
        s1, s2 = {m: 0.0 for m in modes}, {m: 0.0 for m in modes}
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
                    e = errs(b, t, ei[final[r]], gi[r])
                    for m in modes:
                        s1[m] += e[m]
                        s2[m] += e[m] * e[m]
        with np.errstate(invalid="ignore", divide="ignore"):
            g, c, e_ = np.float64(kg[b]), np.float64(kc[b]), np.float64(ke[b])
            acc[b], mdr[b], far[b] = c / g, (g - c) / g, (e_ - c) / g
            for m in modes:
                mae[m][b] = s1[m] / (c + eps)
                rmse[m][b] = np.sqrt(s2[m] / (c + eps))
    out.update({"ACC": acc.mean(), "MDR": mdr.mean(), "FAR": far.mean(), "MAE": {m: mae[m].mean() for m in modes},
                "RMSE": {m: rmse[m].mean() for m in modes}, "K_gt": kg, "K_est": ke, "K_corr": kc,
                "per_utt": {"ACC": acc, "MDR": mdr, "FAR": far}})
    return out


# ---------------------------------------------------------------------------------------------------------------------
# PredDOA.pred2DOA (IPDnet/Module.py:463-579), max_num_sources = 1
# ---------------------------------------------------------------------------------------------------------------------
def template_bank(mic, res_phi=180, nf=257, fre_max=8000.0, speed=340.0):
    """[nazi, 2 * 256, nmic - 1] float64: [cos | sin] of bins 1..256 of exp(-j 2 pi f r . (mic_m - mic_0) / speed), elevation
    pi / 2, azimuth linspace(0, pi, res_phi) (DPIPD.__init__ :334-361, pred2DOA_track :499)."""
    mic = np.asarray(mic, dtype=np.float64).reshape(-1, 3)
    azi = np.linspace(0, np.pi, res_phi)
    r = np.stack([np.cos(azi), np.sin(azi), np.full_like(azi, np.cos(np.pi / 2))], axis=1) * np.array([np.sin(np.pi / 2)] * 2 + [1.0])
    fre = np.linspace(0.0, fre_max, nf)[1:257]
    itd = r @ (mic[1:] - mic[0]).T / speed                                # [nazi, nmic - 1]
    ph = -2 * np.pi * fre[None, :, None] * itd[:, None, :]                # [nazi, 256, nmic - 1]
    return np.concatenate((np.cos(ph), np.sin(ph)), axis=1), azi


def pred2doa(pred, mic, res_phi=180, unk_num=True):
    """pred [nb, nt, 512, nmic - 1, ntrack] -> (idx int [nb, nt, ntrack], doa [nb, nt, 2, ntrack] radians,
    vad [nb, nt, ntrack], scores [nb, nt, ntrack, nazi]) in float64."""
    pred = np.asarray(pred, dtype=np.float64)
    bank, azi = template_bank(mic, res_phi)
    nb, nt, nf2, npair, ntrack = pred.shape
    flat = bank.reshape(res_phi, -1)                                      # index k * npair + p, like pred.view(nb, nt, -1)
    x = pred.transpose(0, 1, 4, 2, 3).reshape(nb, nt, ntrack, -1)
    scores = x @ flat.T / (npair * nf2 / 2)
    idx = scores.argmax(axis=-1)
    win = flat[idx]                                                       # [nb, nt, ntrack, X]
    ratio = (win * x).sum(-1) / (win * win).sum(-1)
    doa = np.stack((np.full(idx.shape, np.pi / 2), azi[idx]), axis=2)     # [nb, nt, 2, ntrack]
    return idx, doa, (ratio if unk_num else np.ones_like(ratio)), scores


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs (the G20 fixture stores only results)
# ---------------------------------------------------------------------------------------------------------------------
def _subsets(n):
    return [[i for i in range(n) if m >> i & 1] for m in range(1, 1 << n)]


def draw_metric_inputs(nb, nt, ns_gt, ns_est, seed, ae_TH, vad_TH, radians=False, match=0.7, silent_utt=(), no_est_seg=(),
                       th_margin=1e-3, vad_margin=1e-6, azi_range=(0.0, 180.0)):
    """Random float32 DOAs / VADs with a useful mix of hits, misses, false alarms and silence.  Estimates are ground truths
    plus a small or a large azimuth offset (probability ``match`` of small), in shuffled source order.  Entries whose
    float64 azimuth error (every ground truth against every estimate of the segment) lies within ``th_margin`` degrees of
    ``ae_TH``, and VADs within ``vad_margin`` of a threshold, are REDRAWN until none is left; so are segments in which, for
    some subset of active sources, two assignments are closer than ``th_margin`` degrees in total cost."""
    rng = np.random.RandomState(seed)
    unit = np.pi / 180 if radians else 1.0
    lo, hi = azi_range

    def draw_seg():
        g = np.stack((rng.uniform(30, 150, ns_gt), rng.uniform(lo, hi, ns_gt)))                  # (ele, azi) degrees
        e = np.empty((2, ns_est))
        order = rng.permutation(max(ns_gt, ns_est))
        for j in range(ns_est):
            src = order[j] % ns_gt
            off = rng.uniform(-0.6, 0.6) * ae_TH if rng.rand() < match else rng.uniform(1.5, 4.0) * ae_TH * rng.choice([-1, 1])
            e[0, j] = g[0, src] + rng.uniform(-8, 8)
            e[1, j] = np.clip(g[1, src] + off, lo, hi)
        return (g * unit).astype(np.float32), (e * unit).astype(np.float32)

    def ok_seg(g, e):
        gd, ed = (degrees(g), degrees(e)) if radians else (g.astype(np.float64), e.astype(np.float64))
        az = azi_error(ed[1][None, :], gd[1][:, None])
        th = float(np.float32(ae_TH))
        if np.abs(az - th).min() <= th_margin:
            return False
        # whatever subset of the sources the VADs leave active, the assignment must not hang on rounding: on a line two
        # ground truths on the same side of two estimates give EQUAL totals for both pairings (only RMSE tells them apart)
        cost = np.where(az > th, 10000.0, az)
        for rows in _subsets(ns_gt):
            for cols in _subsets(ns_est):
                _r, _c, _tot, gap, tie_safe = assign(cost[np.ix_(rows, cols)])
                if gap <= th_margin or not tie_safe:
                    return False
        return True

    def draw_vad(n, thr):
        v = np.where(rng.rand(n) < 0.75, rng.uniform(thr, 1.0, n) + 0.01, rng.uniform(0.0, thr, n) * 0.9).astype(np.float32)
        while (np.abs(v.astype(np.float64) - float(np.float32(thr))) <= vad_margin).any():
            v = np.where(rng.rand(n) < 0.75, rng.uniform(thr, 1.0, n) + 0.01, rng.uniform(0.0, thr, n) * 0.9).astype(np.float32)
        return v

    doa_gt, doa_est = np.empty((nb, nt, 2, ns_gt), np.float32), np.empty((nb, nt, 2, ns_est), np.float32)
    vad_gt, vad_est = np.empty((nb, nt, ns_gt), np.float32), np.empty((nb, nt, ns_est), np.float32)
    for b in range(nb):
        for t in range(nt):
            g, e = draw_seg()
            while not ok_seg(g, e):
                g, e = draw_seg()
            doa_gt[b, t], doa_est[b, t] = g, e
            vad_gt[b, t], vad_est[b, t] = draw_vad(ns_gt, vad_TH[0]), draw_vad(ns_est, vad_TH[1])
    for b in silent_utt:
        vad_gt[b] = 0.0
    for b, t in no_est_seg:
        vad_est[b, t] = 0.0
    return doa_gt, vad_gt, doa_est, vad_est


def threshold_case(ae_TH, vad_TH):
    """One utterance, six segments, one source a side, built so that every fp32 operation of the reference is EXACT:
    ground-truth azimuth 0, estimates ae_TH - 2^-16, ae_TH, ae_TH + 2^-16 degrees (2^-16 is the fp32 step at 180 + ae_TH,
    where the reference's ``est - gt + 180`` lives), then VADs exactly at the two thresholds (fp32) and one step above."""
    step = 2.0 ** -16
    az = np.array([ae_TH - step, ae_TH, ae_TH + step, ae_TH / 2, ae_TH / 2, ae_TH / 2], np.float32)
    t0, t1 = np.float32(vad_TH[0]), np.float32(vad_TH[1])
    vg = np.array([1, 1, 1, t0, np.nextafter(t0, np.float32(2)), 1], np.float32)
    ve = np.array([1, 1, 1, 1, 1, t1], np.float32)
    doa_gt = np.zeros((1, 6, 2, 1), np.float32)
    doa_gt[:, :, 0] = 90
    doa_est = doa_gt.copy()
    doa_est[0, :, 1, 0] = az
    return doa_gt, vg.reshape(1, 6, 1), doa_est, ve.reshape(1, 6, 1)


def judge_case(ae_TH):
    """3 ground truths, 2 estimates, all active, degrees.  Segment 0: one estimate is valid for row 1, the other invalid for
    every row — the optimal assignments tie exactly (10000 whichever row takes it) and linear_sum_assignment gives the
    invalid estimate row 0, the FIRST pair.  Segment 1: the first assigned pair (row 0) invalid, the second (row 1) valid.
    With scipy's tie rule ``final_assignment[i]`` clears the pair's own row in both (i = rows[i]); the slip bites from
    4 x 3 on (``erase_case``)."""
    doa_gt = np.zeros((1, 2, 2, 3), np.float32)
    doa_est = np.zeros((1, 2, 2, 2), np.float32)
    doa_gt[:, :, 0], doa_est[:, :, 0] = 90, 90
    th = float(ae_TH)
    doa_gt[0, 0, 1] = [150.0, 20.0, 100.0]
    doa_est[0, 0, 1] = [20.0 + 0.25 * th, 100.0 + 1.75 * th]
    doa_gt[0, 1, 1] = [60.0, 120.0, 175.0]
    doa_est[0, 1, 1] = [60.0 + 1.5 * th, 120.0 + 0.5 * th]
    return doa_gt, np.ones((1, 2, 3), np.float32), doa_est, np.ones((1, 2, 2), np.float32)


def erase_case():
    """4 ground truths, 3 estimates, ae_TH = 10, degrees, all active: linear_sum_assignment returns rows (1, 2, 3) with the
    pairs (1, est 1) valid (1 degree), (2, est 2) INVALID, (3, est 0) valid (7 degrees).  judge_assignment as written
    clears final_assignment[1] — the position of the invalid pair — and so erases row 1's valid assignment: one correct
    source where two pairs are valid."""
    doa_gt = np.zeros((1, 1, 2, 4), np.float32)
    doa_est = np.zeros((1, 1, 2, 3), np.float32)
    doa_gt[:, :, 0], doa_est[:, :, 0] = 90, 90
    doa_gt[0, 0, 1] = [146.75, 70.75, 74.25, 94.75]
    doa_est[0, 0, 1] = [101.75, 69.75, 103.75]
    return doa_gt, np.ones((1, 1, 4), np.float32), doa_est, np.ones((1, 1, 3), np.float32)


def g20_pred(mic, nb, nt, seed, ntrack=2, noise=0.35):
    """Seeded noisy DP-IPDs [nb, nt, 512, nmic - 1, ntrack] (float32) with their ground truth: per (utterance, segment,
    track) a true azimuth, the true DP-IPD exp(+j 2 pi f r . (mic_0 - mic_m) / 340) scaled by an activity in {~1, ~0.15}
    plus white noise.  Returns (pred, doa_gt [nb, nt, 2, ntrack] radians float32, vad_gt [nb, nt, ntrack] float32)."""
    rng = np.random.RandomState(seed)
    mic = np.asarray(mic, dtype=np.float64).reshape(-1, 3)
    fre = np.linspace(0.0, 8000.0, 257)[1:257]
    azi = rng.uniform(0.6, np.pi - 0.6, (nb, nt, ntrack))
    act = np.where(rng.rand(nb, nt, ntrack) < 0.7, rng.uniform(0.8, 1.1, (nb, nt, ntrack)), rng.uniform(0.05, 0.25, (nb, nt, ntrack)))
    r = np.stack((np.cos(azi), np.sin(azi), np.zeros_like(azi)), axis=-1)                 # elevation pi / 2
    tau = r @ (mic[0] - mic[1:]).T / 340.0                                                # [nb, nt, ntrack, nmic - 1]
    ph = 2 * np.pi * fre[None, None, None, :, None] * tau[:, :, :, None, :]               # [nb, nt, ntrack, 256, nmic - 1]
    ipd = np.concatenate((np.cos(ph), np.sin(ph)), axis=3) * act[..., None, None]
    pred = ipd.transpose(0, 1, 3, 4, 2) + noise * rng.standard_normal((nb, nt, 512, mic.shape[0] - 1, ntrack))
    # ground truth: the true azimuth, sometimes moved away (a miss), in swapped track order for odd segments
    gt_azi = azi + np.where(rng.rand(nb, nt, ntrack) < 0.8, rng.uniform(-0.05, 0.05, azi.shape), rng.uniform(0.3, 0.6, azi.shape))
    gt_azi = np.clip(gt_azi, 0.0, np.pi)
    gt_azi[:, 1::2] = gt_azi[:, 1::2, ::-1]
    vad_gt = np.where(rng.rand(nb, nt, ntrack) < 0.8, rng.uniform(0.01, 0.5, azi.shape), 0.0)
    doa_gt = np.stack((np.full_like(gt_azi, np.pi / 2), gt_azi), axis=2)
    return pred.astype(np.float32), doa_gt.astype(np.float32), vad_gt.astype(np.float32)


# the arrays of group (c): a 2-microphone and a 4-microphone array
G20_MICS = {"mic2": np.array(((-0.04, 0.0, 0.0), (0.04, 0.0, 0.0)), np.float32),
            "mic4": np.array(((-0.06, 0.0, 0.0), (-0.02, 0.0, 0.0), (0.02, 0.0, 0.0), (0.06, 0.0, 0.0)), np.float32)}
# seeds chosen so that the generator's well-posedness asserts hold on the reference's own output (argmax margins, ties)
G20_PRED = {"mic2": dict(nb=3, nt=6, seed=2621), "mic4": dict(nb=3, nt=6, seed=2049)}

# group (a): FN-SSL 'single' through PredDOA.evaluate (radians in, ae_TH 5, vad_TH 2/3)
G20_SINGLE = {"single_1src": dict(nb=4, nt=8, ns=1, seed=1101), "single_2src": dict(nb=4, nt=8, ns=2, seed=1102)}
# group (b): IPDnet 'multiple', direct calls in degrees (ae_TH 10, vad_TH [0.001, 0.5])
G20_MULTI = {
    "multi_2x2": dict(nb=4, nt=8, ns_gt=2, ns_est=2, seed=1201, silent_utt=(2,), no_est_seg=((0, 1), (1, 3), (3, 0))),
    "multi_1x2": dict(nb=3, nt=6, ns_gt=1, ns_est=2, seed=1202),
    "multi_2x1": dict(nb=3, nt=6, ns_gt=2, ns_est=1, seed=1203),
    "multi_3x2": dict(nb=3, nt=6, ns_gt=3, ns_est=2, seed=1204, no_est_seg=((1, 2),)),
    "multi_2x3": dict(nb=3, nt=6, ns_gt=2, ns_est=3, seed=1205, silent_utt=(1,)),
}
G20_AE_TH, G20_VAD_TH = 10, (0.001, 0.5)


def g20_single_inputs(name):
    c = G20_SINGLE[name]
    return draw_metric_inputs(c["nb"], c["nt"], c["ns"], c["ns"], c["seed"], 5, (2 / 3, 2 / 3), radians=True)


def g20_multi_inputs(name):
    if name == "multi_threshold":
        return threshold_case(G20_AE_TH, G20_VAD_TH)
    if name == "multi_judge":
        return judge_case(G20_AE_TH)
    if name == "multi_erase":
        return erase_case()
    c = dict(G20_MULTI[name])
    return draw_metric_inputs(c.pop("nb"), c.pop("nt"), c.pop("ns_gt"), c.pop("ns_est"), c.pop("seed"), G20_AE_TH, G20_VAD_TH, **c)


G20_MULTI_NAMES = tuple(G20_MULTI) + ("multi_threshold", "multi_judge", "multi_erase")
