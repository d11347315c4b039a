"""Float64 references for the two ends of the pipeline (tests/test_gpu_frontend.py, tests/test_gpu_doa.py): the STFT
with its framing, the recursive magnitude mean, the pair and array features, and the iterative IPD -> DOA search.

Plain numpy in float64; nothing here calls the library under test.  The float32 coefficient tables of the recursion
(``oracle.fnssl_oracle.forgetting_coefs``) are part of the specification and are passed in as they are."""
import numpy as np

WIN = 512
NBIN = 257


def hann64():
    """torch.hann_window(512) (periodic), in float64."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WIN, dtype=np.float64) / WIN)


def num_frames(ns, hop, center):
    """Frames of torch.stft(n_fft=512, hop_length=hop, center=center) on ns samples (0: no frame / not allowed)."""
    if center:
        return ns // hop + 1 if ns > WIN // 2 else 0
    return (ns - WIN) // hop + 1 if ns >= WIN else 0


def frames64(sig, hop, center):
    """sig [nb, ns, nch] -> windowed frames float64 [nb, nch, nt, 512]: frame t = samples t*hop .. t*hop + 511 of the
    signal (extended by 256 reflected samples at both ends when ``center``), by index arithmetic."""
    x = np.asarray(sig, dtype=np.float64).transpose(0, 2, 1)                     # [nb, nch, ns]
    nt = num_frames(x.shape[2], hop, center)
    assert nt > 0, "signal too short"
    if center:
        x = np.pad(x, ((0, 0), (0, 0), (WIN // 2, WIN // 2)), mode="reflect")
    idx = np.arange(nt)[:, None] * hop + np.arange(WIN)[None, :]               # [nt, 512]
    return x[:, :, idx] * hann64()


def stft64(sig, hop=256, center=False):
    """sig [nb, ns, nch] -> complex128 [nb, nch, nt, 257]; never rounded to complex64."""
    return np.fft.rfft(frames64(sig, hop, center), n=WIN, axis=-1)


def magsum64(spec):
    """sum_k |X[k]| over the 257 bins: [nb, nch, nt]."""
    return np.abs(spec).sum(axis=-1)


def mu64(magsum, a, b, count):
    """mu_t = a_t mu_{t-1} + b_t mean_t, mu_{-1} = 0, mean_t = magsum[..., t] / count, in float64.
    magsum [..., nt]: the magnitudes of one normalisation group summed per frame; a, b: float32 tables [nt]."""
    mean = np.asarray(magsum, dtype=np.float64) / float(count)
    a = np.asarray(a).astype(np.float64)
    b = np.asarray(b).astype(np.float64)
    mu = np.zeros(mean.shape[:-1], dtype=np.float64)
    out = np.empty_like(mean)
    for t in range(mean.shape[-1]):
        mu = a[t] * mu + b[t] * mean[..., t]
        out[..., t] = mu
    return out


def pair_list(nch, ch_mode):
    if ch_mode == "M":
        return [(0, j) for j in range(1, nch)]
    assert ch_mode == "MM"
    return [(i, j) for i in range(nch - 1) for j in range(i + 1, nch)]


def pair_features64(spec, ch_mode, a, b, eps=1e-6, layout=1):
    """spec complex128 [nb, nch, nt, 257] -> (x, mu [nb * np, nt]); x [nb * np, 4, 256, nt] (layout 1) or
    [nb * np, nt, 256, 4] (layout 0), channels [Re i, Re j, Im i, Im j] of bins 1..256 divided by (mu + eps)."""
    nb, nch, nt, _ = spec.shape
    pairs = pair_list(nch, ch_mode)
    ms = magsum64(spec)
    pi = [p[0] for p in pairs]
    pj = [p[1] for p in pairs]
    mu = mu64(ms[:, pi] + ms[:, pj], a, b, 2 * NBIN).reshape(nb * len(pairs), nt)
    den = (mu + float(np.float32(eps)))[:, :, None]                               # [nb', nt, 1]
    si = spec[:, pi, :, 1:].reshape(nb * len(pairs), nt, NBIN - 1)
    sj = spec[:, pj, :, 1:].reshape(nb * len(pairs), nt, NBIN - 1)
    x0 = np.stack([si.real / den, sj.real / den, si.imag / den, sj.imag / den], axis=-1)   # [nb', nt, 256, 4]
    return (x0 if layout == 0 else x0.transpose(0, 3, 2, 1)), mu


def array_features64(spec, a, b, eps=1e-6, layout=1):
    """spec complex128 [nb, nch, nt, 257] -> (x, mu [nb, nt]); x [nb, 2 nch, 256, nt] (layout 1) or
    [nb, nt, 256, 2 nch] (layout 0), channels [Re ch 0.. | Im ch 0..] of bins 1..256 divided by (mu + eps)."""
    nb, nch, nt, _ = spec.shape
    mu = mu64(magsum64(spec).sum(axis=1), a, b, nch * NBIN)
    den = (mu + float(np.float32(eps)))[:, None, :, None]
    s = spec[..., 1:] / den                                                       # [nb, nch, nt, 256]
    x1 = np.concatenate([s.real, s.imag], axis=1).transpose(0, 1, 3, 2)           # [nb, 2 nch, 256, nt]
    return (x1 if layout == 1 else x1.transpose(0, 3, 2, 1)), mu


def ipd2doa_ref(pred, bank, nsrc, unk_num, follow=None, dtype=np.float64):
    """SourceDetectLocalize 'IDL' in ``dtype``: pred [nb, nt, nf2, np], bank [..., nf2, np] (any leading candidate
    axes).  Per source: scores = residual . template / (nf2 * np / 2), first argmax, ratio = <t, res> / <t, t>,
    residual -= ratio * t.  With ``follow`` [nb, nt, nsrc] the candidate sequence is taken from it instead of the
    argmax (the scores and ratios are then those along that sequence).
    Returns (idx [nb, nt, nsrc], vad [nb, nt, nsrc], ss [nb, nt, ncand], scores [nsrc, nb, nt, ncand],
    ratio [nb, nt, nsrc])."""
    pred = np.asarray(pred)
    nb, nt, nf2, npair = pred.shape
    X = nf2 * npair
    flat = np.asarray(bank).reshape(-1, X).astype(dtype)
    res = pred.reshape(nb * nt, X).astype(dtype)
    norm = dtype(X / 2.0)
    idx = np.empty((nb * nt, nsrc), dtype=np.int64)
    ratio = np.empty((nb * nt, nsrc), dtype=dtype)
    scores = np.empty((nsrc, nb * nt, flat.shape[0]), dtype=dtype)
    for s in range(nsrc):
        scores[s] = res @ flat.T / norm
        idx[:, s] = scores[s].argmax(axis=1) if follow is None else np.asarray(follow).reshape(nb * nt, nsrc)[:, s]
        tm = flat[idx[:, s]]
        ratio[:, s] = (tm * res).sum(axis=1) / (tm * tm).sum(axis=1)
        res = res - ratio[:, s, None] * tm
    ratio = ratio.reshape(nb, nt, nsrc)
    vad = ratio.copy() if unk_num else np.ones_like(ratio)
    return (idx.reshape(nb, nt, nsrc), vad, scores[0].reshape(nb, nt, -1), scores.reshape(nsrc, nb, nt, -1), ratio)


def ipd2doa64(pred, bank, nsrc, unk_num, follow=None):
    return ipd2doa_ref(pred, bank, nsrc, unk_num, follow, np.float64)


def peaks_ref(ss, nsrc):
    """The peak rule of SourceDetectLocalize 'PD' per frame: ss [nframes, nele, nazi]; the last azimuth column is
    dropped, a cell is a peak when strictly larger than its 8 neighbours (azimuth circular over nazi - 1 columns,
    elevation clamped), the nsrc largest are kept, equal values in ascending flat-index order.
    Returns (idx [nframes, nsrc] flat e * nazi + a or -1, val [nframes, nsrc] (0 where none), count [nframes])."""
    ss = np.asarray(ss)
    nfr, nele, nazi = ss.shape
    g = ss[:, :, :nazi - 1]
    ok = np.ones(g.shape, dtype=bool)
    for de in (-1, 0, 1):
        ge = g[:, np.clip(np.arange(nele) + de, 0, nele - 1), :]
        for da in (-1, 0, 1):
            if de or da:
                ok &= g > np.roll(ge, -da, axis=2)
    idx = np.full((nfr, nsrc), -1, dtype=np.int64)
    val = np.zeros((nfr, nsrc), dtype=ss.dtype)
    cnt = np.zeros((nfr,), dtype=np.int64)
    for f in range(nfr):
        e, a = np.nonzero(ok[f])
        flat = e * nazi + a                                                       # ascending
        order = np.argsort(-g[f, e, a], kind="stable")[:nsrc]
        cnt[f] = len(order)
        idx[f, :len(order)] = flat[order]
        val[f, :len(order)] = g[f, e, a][order]
    return idx, val, cnt


def wave_argmax(score):
    """Host restatement of the candidate choice of ipd2doa_kernel (csrc/doa.hip): 64 lanes each scan candidates
    lane, lane + 64, ... in ascending order starting from candidate 0, then a six-level xor butterfly; a NaN beats any
    number, among NaNs and among equal numbers the lower index wins.  Returns lane 0's index."""
    score = np.asarray(score, dtype=np.float32)
    n = score.shape[0]

    def nan(v):
        return v != v

    bv = np.full(64, score[0], dtype=np.float32)
    bi = np.zeros(64, dtype=np.int64)
    for lane in range(64):
        for c in range(lane, n, 64):
            v = score[c]
            if v > bv[lane] or (nan(v) and not nan(bv[lane])):
                bv[lane], bi[lane] = v, c
    d = 32
    while d >= 1:
        ov, oi = bv[np.arange(64) ^ d].copy(), bi[np.arange(64) ^ d].copy()
        for lane in range(64):
            on, bn = nan(ov[lane]), nan(bv[lane])
            take = (not bn or oi[lane] < bi[lane]) if on else \
                (not bn and (ov[lane] > bv[lane] or (ov[lane] == bv[lane] and oi[lane] < bi[lane])))
            if take:
                bv[lane], bi[lane] = ov[lane], oi[lane]
        d >>= 1
    return int(bi[0])
