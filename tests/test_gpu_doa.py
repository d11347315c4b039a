"""GPU tests of csrc/doa.hip beyond the goldens, against float64 (tests/frontend_doa_ref.py): ipd2doa_kernel at config
size, on the full 37 x 73 grid (2701 candidates, 105 of them bit-identical to an earlier one), on candidate counts and
vector lengths that are not multiples of 4 or 64, through every pred layout; exact ties, constructed; non-finite
predictions (torch.argmax's rule: a NaN is the maximum, the first wins); and doa_peaks_kernel on a grid that needs the
dynamic-LDS attribute, plateaus, equal peaks and 600 frames.  Run with -m gpu on an MI355X.

Bounds.  A score: rtol 1e-5, atol 1e-6 (the project's spectrum tolerance).  A chosen candidate must be a maximum of the
float64 scores within twice that: s64[idx] >= max - 2 (1e-6 + 1e-5 |max|), for every segment and source; the float64
scores of source 1.. are taken along the DEVICE's own earlier choices (``follow``), so two precisions never have to
break a near-tie the same way.  Projection ratio: rtol 1e-4, atol 1e-6 for source 0; for later sources
max(1e-4 |r| + 1e-6, 4 d_r), d_r being what the same followed chain in float32 numpy deviates from float64."""
import ctypes as C

import numpy as np
import pytest

import frontend_doa_ref as R
from conftest import assert_close, rs_randn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MICS4 = np.array([[0.04, 0.0, 0.0], [0.0, 0.04, 0.0], [-0.04, 0.0, 0.0], [0.0, -0.04, 0.02]])
MICS8 = np.stack([0.05 * np.cos(np.arange(8) * np.pi / 4), 0.05 * np.sin(np.arange(8) * np.pi / 4),
                  0.01 * (np.arange(8) % 2)], axis=1)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()                      # fail loudly if the extension is missing
    return torch.device("cuda:0")


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def score_tol(s):
    return 1e-6 + 1e-5 * np.abs(s)


def grid_bank(mics, ch_mode, nele=37, nazi=73):
    """[nele, nazi, 512, np] float32: [cos | sin] of bins 1..256 of every direction of the grid."""
    from oracle import fnssl_oracle as O
    t, _ = O.dpipd_templates(mics, nele, nazi, 257, 8000.0, ch_mode, 340.0)
    return np.ascontiguousarray(np.concatenate((t.real[:, :, 1:257, :], t.imag[:, :, 1:257, :]), axis=2).astype(np.float32))


def default_bank(mics, ch_mode):
    """The 37-candidate bank PredDOA searches: middle elevation row, upper azimuth half."""
    from oracle import fnssl_oracle as O
    t, cand = O.dpipd_templates(mics, 37, 73, 257, 8000.0, ch_mode, 340.0)
    return O.template_bank(t, cand)[0]


def synthetic_bank(ncand, seed):
    """[1, ncand, 500, 3]: X = 1500 is not a multiple of 64."""
    return rs_randn(seed, (1, ncand, 500, 3))


def make_pred(bank, nb, nt, seed, mix):
    """tanh(randn) alone, or 0.3 x tanh(randn) + 0.6 x a random template of the bank per segment."""
    nf2, npair = bank.shape[2:]
    pred = np.tanh(rs_randn(seed, (nb, nt, nf2, npair)))
    if mix:
        flat = bank.reshape(-1, nf2, npair)
        pick = np.random.RandomState(seed + 1).randint(0, flat.shape[0], size=(nb, nt))
        pred = (0.3 * pred + 0.6 * flat[pick]).astype(np.float32)
    return pred


def first_of_identical(bank):
    """For every candidate, the lowest index among the candidates whose template rows are bit-identical to its own."""
    flat = np.ascontiguousarray(bank.reshape(-1, bank.shape[2] * bank.shape[3]))
    _, first, inv = np.unique(flat.view(np.uint32), axis=0, return_index=True, return_inverse=True)
    return first[inv.reshape(-1)]


def check_localize(dev, bank, pred, nsrc, mode, what):
    """Run fnssl.doa.localize and hold it to the float64 chain.  Returns (idx, vad, ss) as numpy and the measured d_r."""
    from fnssl import doa as fdoa
    nb, nt = pred.shape[:2]
    ncand = bank.shape[0] * bank.shape[1]
    unk = mode == "unkNum"
    idx, vad, ss = fdoa.localize(to_dev(pred, dev), to_dev(bank, dev), nb, nsrc, mode)
    torch.cuda.synchronize(dev)
    idx, vad, ss = idx.cpu().numpy().astype(np.int64), vad.cpu().numpy(), ss.cpu().numpy().reshape(nb, nt, ncand)
    assert idx.shape == vad.shape == (nb, nt, nsrc)
    assert (idx >= 0).all() and (idx < ncand).all(), "%s: candidate out of range" % what
    # the device's spectrum against float64, every element
    _, _, ss64, scores, ratio = R.ipd2doa64(pred, bank, nsrc, unk, follow=idx)
    assert_close(ss, ss64, 1e-5, 1e-6, what + ": ss")
    # every choice is a maximum of the float64 scores along the device's own earlier choices, within rounding
    first = first_of_identical(bank)
    for s in range(nsrc):
        sc = scores[s]
        top = sc.max(axis=2)
        chosen = np.take_along_axis(sc, idx[:, :, s, None], axis=2)[..., 0]
        short = top - chosen
        print("%s: source %d: chosen candidate at most %.3g below the float64 maximum (allowed %.3g .. %.3g), %d of %d segments "
              "differ from the float64 argmax" % (what, s, short.max(), 2 * score_tol(top).min(), 2 * score_tol(top).max(),
                                                  int((sc.argmax(axis=2) != idx[:, :, s]).sum()), nb * nt))
        bad = np.argwhere(short > 2 * score_tol(top))
        assert bad.size == 0, "%s: source %d of segments %s is not a maximum: %g below" % (what, s, bad[:4].tolist(), short.max())
        lower = np.argwhere(first[idx[:, :, s]] != idx[:, :, s])
        assert lower.size == 0, "%s: source %d of segments %s: a lower candidate has the same template" % (what, s, lower[:4].tolist())
    # the projection ratio
    d_r = np.zeros(nsrc)
    if unk:
        _, _, _, _, r32 = R.ipd2doa_ref(pred, bank, nsrc, True, follow=idx, dtype=np.float32)
        for s in range(nsrc):
            d_r[s] = np.abs(r32[..., s].astype(np.float64) - ratio[..., s]).max()
            allow = 1e-4 * np.abs(ratio[..., s]) + 1e-6
            if s > 0:
                allow = np.maximum(allow, 4 * d_r[s])
            err = np.abs(vad[..., s] - ratio[..., s])
            print("%s: source %d ratio: host float32 d_r %.3g, device %.3g" % (what, s, d_r[s], err.max()))
            bad = np.argwhere(err > allow)
            assert bad.size == 0, "%s: ratio of source %d off by %g at %s (d_r %g)" % (what, s, err.max(), bad[:4].tolist(), d_r[s])
    else:
        assert (vad == 1).all(), "%s: kNum reports 1" % what
    return idx, vad, ss, d_r


# --------------------------------------------------------------------------- a. sizes and layouts
@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("nsrc,mode", [(1, "kNum"), (2, "unkNum"), (3, "unkNum"), (3, "kNum")])
def test_config2_shape_against_float64(dev, nsrc, mode, mix):
    """Config 2: 32 utterances x 25 segments, 6 pairs, the default 37-candidate bank; pred in the network's own layout
    [nb * np, nt, 512] (read in place) and as the re-batched 4-D tensor: same bits.

    Measured on an MI355X over this file's cases: the float32 host chain's d_r is <= 1.1e-7 for source 0 and <= 7.2e-8
    for later sources, the device's own deviation from float64 <= 8.9e-8 and <= 5.9e-8 (so 1e-4 |r| + 1e-6 decided
    every allowance); all 16 940 choices (segment, source) were the float64 argmax itself, shortfall 0."""
    from fnssl import doa as fdoa
    nb, nt = 32, 25
    bank = default_bank(MICS4, "MM")
    assert bank.shape == (1, 37, 512, 6)
    pred = make_pred(bank, nb, nt, 5100 + nsrc, mix)
    idx, vad, ss, _ = check_localize(dev, bank, pred, nsrc, mode, "config 2, %d sources %s mix %d" % (nsrc, mode, mix))
    net = to_dev(pred.transpose(0, 3, 1, 2).reshape(nb * 6, nt, 512), dev)                  # [nb * np, nt, 2 nf]
    i2, v2, s2 = fdoa.localize(net, to_dev(bank, dev), nb, nsrc, mode)
    np.testing.assert_array_equal(i2.cpu().numpy(), idx)
    np.testing.assert_array_equal(v2.cpu().numpy(), vad)
    np.testing.assert_array_equal(s2.cpu().numpy().reshape(ss.shape), ss)


@pytest.mark.parametrize("mix", [False, True])
def test_full_grid_against_float64(dev, mix):
    """The full 37 x 73 grid, 4 microphones 'MM': X = 3072, 2701 candidates, 105 of them bit-identical to an earlier
    one (the elevation-0 row and most azimuth -pi / +pi pairs), so the first-index rule decides real answers."""
    bank = grid_bank(MICS4, "MM")
    assert bank.shape == (37, 73, 512, 6)
    first = first_of_identical(bank)
    assert (first != np.arange(2701)).sum() >= 72, "the grid no longer holds duplicate templates"
    pred = make_pred(bank, 2, 25, 5200, mix)
    for nsrc, mode in ((2, "unkNum"), (3, "kNum")):
        check_localize(dev, bank, pred, nsrc, mode, "full grid, %d sources %s mix %d" % (nsrc, mode, mix))


@pytest.mark.parametrize("mix", [False, True])
def test_eight_microphones_m_mode_against_float64(dev, mix):
    bank = default_bank(MICS8, "M")
    assert bank.shape == (1, 37, 512, 7)
    pred = make_pred(bank, 4, 25, 5300, mix)
    check_localize(dev, bank, pred, 2, "unkNum", "8 microphones 'M' mix %d" % mix)
    check_localize(dev, bank, pred, 1, "kNum", "8 microphones 'M', one source, mix %d" % mix)


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("ncand", [1, 3, 37, 65, 130])
def test_candidate_counts_and_odd_vector_length(dev, ncand, mix):
    """A synthetic bank [1, ncand, 500, 3]: X = 1500 (23 full lane sweeps and a ragged one), candidate counts below,
    at and past one wave's 64 lanes and not multiples of the four waves."""
    bank = synthetic_bank(ncand, 5400 + ncand)
    pred = make_pred(bank, 3, 7, 5500 + ncand, mix)
    for nsrc, mode in ((1, "unkNum"), (2, "kNum"), (3, "unkNum")):
        check_localize(dev, bank, pred, nsrc, mode, "%d candidates, %d sources %s mix %d" % (ncand, nsrc, mode, mix))


def test_pred_layouts_give_identical_results(dev):
    """pred is read through four strides: the contiguous [nb, nt, 2nf, np] tensor, the network's [nb, np, nt, 2nf]
    memory, a fully reversed memory order, and a slice of a larger buffer all give the same bits."""
    from fnssl import doa as fdoa
    bank = default_bank(MICS4, "MM")
    nb, nt = 5, 9
    pred = make_pred(bank, nb, nt, 5600, True)
    idx, vad, ss, _ = check_localize(dev, bank, pred, 3, "unkNum", "contiguous pred")
    p = to_dev(pred, dev)
    big = torch.full((nb, nt + 3, 512 + 5, 6 * 2), 3.0, dtype=torch.float32, device=dev)
    big[:, 2:2 + nt, 5:, ::2] = p
    views = {"network": p.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1),
             "reversed": p.permute(2, 3, 1, 0).contiguous().permute(3, 2, 0, 1),
             "slice": big[:, 2:2 + nt, 5:, ::2]}
    for name, v in views.items():
        assert v.shape == p.shape and v.stride() != p.stride()
        i2, v2, s2 = fdoa.localize(v, to_dev(bank, dev), nb, 3, "unkNum")
        i3, v3, s3 = fdoa.localize(v.contiguous(), to_dev(bank, dev), nb, 3, "unkNum")
        for a, b, c in ((i2, i3, idx), (v2, v3, vad), (s2, s3, ss)):
            assert torch.equal(a, b), "%s view differs from its contiguous copy" % name
            np.testing.assert_array_equal(a.cpu().numpy().reshape(c.shape), c)


# --------------------------------------------------------------------------- b. exact ties
@pytest.mark.parametrize("nsrc", [1, 2])
def test_constructed_ties_take_the_lowest_index(dev, nsrc):
    """Candidate 5 copied into candidates 70 and 900 (lanes 5, 6 and 4 of three different sweeps; waves 1, 2 and 0 of
    the scoring loop): pred = 0.9 x that template + noise must answer 5; the second source is none of the three unless
    float64 says their residual score is still the maximum."""
    bank = synthetic_bank(1000, 5700)
    bank[0, 70] = bank[0, 5]
    bank[0, 900] = bank[0, 5]
    nb, nt = 2, 6
    pred = (0.9 * bank[0, 70][None, None] + 0.05 * rs_randn(5701, (nb, nt, 500, 3))).astype(np.float32)
    idx, _, _, _ = check_localize(dev, bank, pred, nsrc, "unkNum", "constructed ties, %d sources" % nsrc)
    assert (idx[:, :, 0] == 5).all(), idx[:, :, 0]
    if nsrc == 2:
        assert not np.isin(idx[:, :, 1], (70, 900)).any(), idx[:, :, 1]           # 5 itself is held to float64 above


def test_real_grid_duplicates_take_the_first_column(dev):
    """The elevation-0 row of the real grid is one template 73 times; most azimuth -pi / +pi columns are the same
    template too: the template of (row 0, column 40) must return column 0, that of (row r, column 72) column 0."""
    bank = grid_bank(MICS4, "MM")
    assert all(np.array_equal(bank[0, a], bank[0, 0]) for a in range(73))
    rows = [r for r in range(1, 36) if np.array_equal(bank[r, 72], bank[r, 0])]
    assert len(rows) >= 8, "the grid no longer holds identical -pi / +pi templates"
    rows = rows[:: max(1, len(rows) // 8)][:8]
    pred = np.stack([bank[0, 40]] + [bank[r, 72] for r in rows])[None]            # [1, 1 + len(rows), 512, 6]
    idx, vad, _, _ = check_localize(dev, bank, pred, 1, "unkNum", "real-grid duplicates")
    assert idx[0, :, 0].tolist() == [0] + [r * 73 for r in rows]
    assert_close(vad[0, :, 0], np.ones(1 + len(rows)), 1e-4, 1e-6, "a template projects onto itself with ratio 1")


# --------------------------------------------------------------------------- c. non-finite input
@pytest.mark.parametrize("mode", ["unkNum", "kNum"])
def test_non_finite_predictions_follow_torch_argmax(dev, mode):
    """A segment that holds a NaN has only NaN scores: candidate 0 for every source (torch.argmax: the first NaN),
    NaN ratio ('unkNum') or 1 ('kNum').  A segment with one +inf has scores of +inf, -inf and NaN: source 0 is what
    torch.argmax gives on the float32 scores the device returned, later sources stay in range.  Every other segment
    has the bits of a run without the bad segments, and the device still works afterwards."""
    from fnssl import doa as fdoa
    bank = default_bank(MICS4, "MM")
    bdev = to_dev(bank, dev)
    nb, nt, nsrc = 2, 6, 3
    clean = make_pred(bank, nb, nt, 5800, True)
    bad = clean.copy()
    bad[0, 1] = np.nan
    bad[0, 3, 100, 2] = np.nan
    bad[1, 2, 300, 4] = np.inf
    ci, cv, cs = [t.cpu().numpy() for t in fdoa.localize(to_dev(clean, dev), bdev, nb, nsrc, mode)]
    bi, bv, bs = [t.cpu().numpy() for t in fdoa.localize(to_dev(bad, dev), bdev, nb, nsrc, mode)]
    torch.cuda.synchronize(dev)
    assert (bi >= 0).all() and (bi < 37).all()
    for seg in ((0, 1), (0, 3)):
        assert np.isnan(bs[seg]).all(), "a NaN element makes every score NaN"
        assert (bi[seg] == 0).all(), "NaN scores: the first one is the maximum, got %s" % bi[seg]
        assert np.isnan(bv[seg]).all() if mode == "unkNum" else (bv[seg] == 1).all()
    s = bs[1, 2].reshape(-1)
    assert not np.isfinite(s).any()
    assert bi[1, 2, 0] == int(torch.argmax(torch.from_numpy(s)))
    good = np.ones((nb, nt), dtype=bool)
    good[0, 1] = good[0, 3] = good[1, 2] = False
    np.testing.assert_array_equal(bi[good], ci[good])
    np.testing.assert_array_equal(bv[good], cv[good])
    np.testing.assert_array_equal(bs[good], cs[good])
    again = [t.cpu().numpy() for t in fdoa.localize(to_dev(clean, dev), bdev, nb, nsrc, mode)]   # a following launch succeeds
    for a, b in zip(again, (ci, cv, cs)):
        np.testing.assert_array_equal(a, b)


def test_non_finite_predictions_through_peak_detection(dev):
    """localize_pd on the same kind of batch: a NaN spectrum has no peak (every v > neighbour is false, in the
    reference too): count 0 and idx -1; the other frames as without the bad segments."""
    from fnssl import doa as fdoa
    bank = grid_bank(MICS4, "MM", 9, 13)
    bdev = to_dev(bank, dev)
    nb, nt = 2, 6
    clean = make_pred(bank, nb, nt, 5900, True)
    bad = clean.copy()
    bad[0, 1] = np.nan
    bad[1, 4, 7, 0] = np.nan
    ci, cv, cc, cs = [t.cpu().numpy() for t in fdoa.localize_pd(to_dev(clean, dev), bdev, nb, 2)]
    bi, bv, bc, bs = [t.cpu().numpy() for t in fdoa.localize_pd(to_dev(bad, dev), bdev, nb, 2)]
    want_i, want_v, want_c = R.peaks_ref(cs.reshape(nb * nt, 9, 13), 2)
    np.testing.assert_array_equal(ci.reshape(nb * nt, 2), want_i)
    np.testing.assert_array_equal(cc.reshape(-1), want_c)
    np.testing.assert_array_equal(cv.reshape(nb * nt, 2), want_v)
    for seg in ((0, 1), (1, 4)):
        assert bc[seg] == 0 and (bi[seg] == -1).all() and (bv[seg] == 0).all()
    good = np.ones((nb, nt), dtype=bool)
    good[0, 1] = good[1, 4] = False
    np.testing.assert_array_equal(bi[good], ci[good])
    np.testing.assert_array_equal(bc[good], cc[good])
    np.testing.assert_array_equal(bv[good], cv[good])
    np.testing.assert_array_equal(bs[good], cs[good])


# --------------------------------------------------------------------------- d. peak detection
def run_peaks(dev, ss, nsrc):
    from fnssl import doa as fdoa
    nfr, nele, nazi = ss.shape
    d = to_dev(ss, dev)
    idx = torch.full((nfr, nsrc), -7, dtype=torch.int32, device=dev)
    val = torch.full((nfr, nsrc), -7.0, dtype=torch.float32, device=dev)
    cnt = torch.full((nfr,), -7, dtype=torch.int32, device=dev)
    fdoa._lib.check(fdoa._lib.load().fnssl_doa_peaks(C.c_void_p(d.data_ptr()), nfr, nele, nazi, nsrc, C.c_void_p(idx.data_ptr()),
                                                     C.c_void_p(val.data_ptr()), C.c_void_p(cnt.data_ptr()), None), "doa_peaks")
    torch.cuda.synchronize(dev)
    return idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()


def check_peaks(dev, ss, nsrc, what):
    idx, val, cnt = run_peaks(dev, ss, nsrc)
    wi, wv, wc = R.peaks_ref(ss, nsrc)
    np.testing.assert_array_equal(cnt, wc, err_msg=what + ": count")
    np.testing.assert_array_equal(idx, wi, err_msg=what + ": idx")
    np.testing.assert_array_equal(val, wv, err_msg=what + ": val")
    return idx, val, cnt


def test_peaks_on_a_grid_that_needs_the_dynamic_lds_attribute(dev):
    """181 x 37 cells x 2 arrays x 4 bytes = 53.6 KB of dynamic LDS: past the 48 KB a kernel gets without
    hipFuncSetAttribute."""
    ss = rs_randn(6000, (5, 181, 37))
    _, _, cnt = check_peaks(dev, ss, 2, "181 x 37")
    assert (cnt == 2).all()
    check_peaks(dev, np.round(ss * 2).astype(np.float32), 8, "181 x 37, coarse values")


def test_peaks_plateau_and_equal_peaks_over_all_waves(dev):
    """Two equal neighbours: neither is a peak (the comparison is strict).  More peaks than nsrc with equal values
    whose flat indices fall into all four waves' shares (thread i % 256, wave = thread / 64): ascending flat index
    wins, whichever wave holds it."""
    nele, nazi = 20, 40
    ss = np.zeros((3, nele, nazi), dtype=np.float32)
    ss[0, 5, 7] = ss[0, 5, 8] = 3.0                                               # plateau: no peak
    ss[0, 9, 20] = 1.0                                                            # the frame's only peak
    cells = [(17, 30), (2, 3), (8, 13), (11, 25), (5, 35), (14, 2), (3, 21), (12, 9)]
    flat = sorted(e * nazi + a for e, a in cells)
    assert {(i % 256) // 64 for i in flat} == {0, 1, 2, 3} and {(i % 256) // 64 for i in flat[:4]} != {0}
    for e, a in cells:
        ss[1, e, a] = 2.0                                                         # eight equal peaks
        ss[2, e, a] = 2.0
    ss[2, 16, 16] = 5.0                                                           # and one larger, in frame 2
    for nsrc in (1, 3, 8):
        idx, val, cnt = check_peaks(dev, ss, nsrc, "plateau and ties, nsrc %d" % nsrc)
        assert cnt.tolist() == [1, min(8, nsrc), min(9, nsrc)]
        assert idx[0, 0] == 9 * nazi + 20
        assert idx[1].tolist() == flat[:nsrc]
        assert idx[2].tolist() == ([16 * nazi + 16] + flat)[:nsrc]


def test_peaks_eight_sources_600_frames(dev):
    """600 frames in one launch, nsrc = 8, coarse values (plateaus, equal peaks, frames with fewer than 8 peaks)."""
    ss = np.round(rs_randn(6100, (600, 9, 13)) * 1.5).astype(np.float32)
    _, _, cnt = check_peaks(dev, ss, 8, "600 frames")
    assert cnt.min() < 8 and cnt.max() >= 2
    check_peaks(dev, rs_randn(6101, (600, 37, 73)), 8, "600 frames of the 37 x 73 grid")
