"""CPU tests of tests/frontend_doa_ref.py: the float64 references of the front end and the DOA back end against the
float32 oracle (itself pinned to the real reference through tests/golden) on golden inputs, and the host restatement of
ipd2doa_kernel's candidate scan against torch.argmax on scores with ties, NaN and infinities.  No GPU."""
import numpy as np
import pytest

import frontend_doa_ref as R
from conftest import assert_close, load_golden, rs_randn
from oracle import fnssl_oracle as O

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("hop,center", [(256, False), (320, True)])
def test_stft64_matches_oracle_on_g1_input(hop, center):
    """O.stft multiplies by a float32 window in float32 and rounds the result to complex64, so it differs from stft64
    by at most 2 x 2^-24 of sum |x w| over the frame (window and product rounding) plus one complex64 rounding of the
    value (2^-24 per component)."""
    g = load_golden("g1_stft")
    sig = rs_randn(g["seed"], g["shape"])
    want = O.stft(sig, hop, center).transpose(0, 3, 2, 1)                         # [nb, nch, nt, 257]
    got = R.stft64(sig, hop, center)
    assert got.dtype == np.complex128 and got.shape == want.shape
    assert got.shape[2] == R.num_frames(sig.shape[1], hop, center)
    bound = 2.0 ** -23 * np.abs(R.frames64(sig, hop, center)).sum(axis=-1).max() + 2.0 ** -23 * np.abs(want).max()
    err = np.abs(got - want).max()
    assert err <= bound, "stft64 vs oracle: %g > %g" % (err, bound)
    if not center and hop == 256:
        assert np.abs(got - g["out"].transpose(0, 3, 2, 1)).max() <= 5e-6 * np.abs(g["out"]).max(), "vs reference golden"


def test_stft64_framing_edges():
    assert R.num_frames(512, 256, False) == 1 and R.num_frames(511, 256, False) == 0
    assert R.num_frames(257, 256, True) == 2 and R.num_frames(256, 256, True) == 0
    assert R.num_frames(1000, 1, False) == 489 and R.num_frames(1000, 512, True) == 2
    sig = rs_randn(5, (1, 257, 1))
    fr = R.frames64(sig, 256, True)[0, 0]
    x, w = sig[0, :, 0].astype(np.float64), R.hann64()
    i0 = np.abs(np.arange(-256, 256))                                            # left reflection: x[-n] = x[n]
    i1 = np.arange(0, 512)
    i1 = np.where(i1 > 256, 2 * 256 - i1, i1)                                    # right reflection: x[2 (ns - 1) - i]
    np.testing.assert_array_equal(fr[0], x[i0] * w)
    np.testing.assert_array_equal(fr[1], x[i1] * w)


@pytest.mark.parametrize("sl", [8, 298])
def test_mu64_matches_oracle_forgetting_norm_at_24_frames(sl):
    """G3's input (24 frames): the float32 recursion rounds each product and each sum once (three roundings a frame
    on values that decay geometrically), and the float32 mean over 514 values a few more: 3e-6 relative is the
    project's own bound for mu against the float32 oracle."""
    g = load_golden("g3_fnorm")
    mag = np.abs(rs_randn(g["seed"], g["shape"])) + np.float32(0.1)
    want = O.forgetting_norm(mag, sl)[:, 0, 0, :]
    assert_close(want, g["out_sl%d" % sl][:, 0, 0, :], 2e-6, 0, "oracle vs reference golden")
    a, b = O.forgetting_coefs(mag.shape[3], sl)
    got = R.mu64(mag.astype(np.float64).sum(axis=(1, 2)), a, b, mag.shape[1] * mag.shape[2])
    assert got.dtype == np.float64
    assert_close(got, want, 3e-6, 0, "mu64 vs forgetting_norm")


@pytest.mark.parametrize("ch_mode", ["MM", "M"])
def test_features64_match_oracle_preprocess(ch_mode):
    sig = rs_randn(21, (2, 512 + 23 * 256, 3), 0.05)
    spec = R.stft64(sig)
    a, b = O.forgetting_coefs(spec.shape[2], 298)
    x1, mu = R.pair_features64(spec, ch_mode, a, b, layout=1)
    assert_close(x1, O.data_preprocess(sig, ch_mode), 2e-5, 2e-5, "pair features")
    x0, _ = R.pair_features64(spec, ch_mode, a, b, layout=0)
    np.testing.assert_array_equal(x0, x1.transpose(0, 3, 2, 1))
    a, b = O.forgetting_coefs(spec.shape[2], 280)
    y1, _ = R.array_features64(spec, a, b, layout=1)
    assert_close(y1, O.array_preprocess(sig), 2e-5, 2e-5, "array features")
    y0, _ = R.array_features64(spec, a, b, layout=0)
    np.testing.assert_array_equal(y0, y1.transpose(0, 3, 2, 1))


def _g12_case():
    g = load_golden("g12_doa")
    tmpl, cand = O.dpipd_templates(g["tmpl_mics"], 37, 73, 257, 8000.0, "MM", 340.0)
    bank, cand = O.template_bank(tmpl, cand)
    pred = np.tanh(rs_randn(int(g["m4_seed"][0]), (2, 4, 512, 6)))
    return g, bank, cand, pred


def test_ipd2doa64_matches_oracle_on_g12_input():
    g, bank, cand, pred = _g12_case()
    doa, vad, ss = O.source_detect_localize(pred, bank, cand, 2, "unkNum")
    np.testing.assert_array_equal(doa, g["m4_doa"])
    idx, vad64, ss64, scores, ratio = R.ipd2doa64(pred, bank, 2, True)
    np.testing.assert_array_equal(cand[1][idx].astype(np.float32), doa[:, :, 1, :])
    assert_close(ss64.reshape(ss.shape), ss, 1e-5, 1e-6, "ss")
    assert_close(vad64, vad, 1e-4, 1e-6, "ratio")
    assert_close(vad64, g["m4_vad"], 1e-4, 1e-6, "ratio vs golden")
    # follow: the same chain along a given candidate sequence; kNum reports 1
    idx2, vad2, _, scores2, ratio2 = R.ipd2doa64(pred, bank, 2, False, follow=idx)
    np.testing.assert_array_equal(idx2, idx)
    np.testing.assert_array_equal(ratio2, ratio)
    np.testing.assert_array_equal(scores2, scores)
    assert (vad2 == 1).all()
    other = (idx + 3) % 37
    idx3, _, _, scores3, _ = R.ipd2doa64(pred, bank, 2, True, follow=other)
    np.testing.assert_array_equal(idx3, other)
    np.testing.assert_array_equal(scores3[0], scores[0])
    assert not np.array_equal(scores3[1], scores[1])
    # the float32 restatement of the same chain stays within the project's bounds of the float64 one
    _, _, ss32, _, r32 = R.ipd2doa_ref(pred, bank, 2, True, follow=idx, dtype=np.float32)
    assert ss32.dtype == np.float32
    assert_close(ss32, ss64, 1e-5, 1e-6, "float32 chain ss")
    assert_close(r32[..., 0], ratio[..., 0], 1e-4, 1e-6, "float32 chain ratio")


def test_peaks_ref_matches_oracle_rule():
    """peaks_ref against the per-cell loop of O.source_detect_localize_pd on a small grid (two sources, every frame
    with at least two peaks), ties included."""
    rs = np.random.RandomState(3)
    ss = np.round(rs.standard_normal((6, 7, 9)) * 2).astype(np.float32)          # coarse values: plateaus and ties
    idx, val, cnt = R.peaks_ref(ss, 2)
    w = 8
    for f in range(6):
        found = []
        for e in range(7):
            for a in range(w):
                v = ss[f, e, a]
                if all(v > ss[f, min(max(e + de, 0), 6), (a + da) % w] for de in (-1, 0, 1) for da in (-1, 0, 1) if de or da):
                    found.append((e * 9 + a, v))
        found.sort(key=lambda kv: -kv[1])
        assert cnt[f] == min(len(found), 2)
        assert [k for k, _ in found[:2]] == [k for k in idx[f] if k >= 0]
        assert [v for _, v in found[:2]] == list(val[f, :cnt[f]])


def test_wave_argmax_is_torch_argmax():
    """The candidate scan of ipd2doa_kernel, restated lane by lane, returns torch.argmax's index on float32 scores with
    exact ties, NaN (counts as the maximum, the first wins), +inf / -inf, for candidate counts around the wave size."""
    rs = np.random.RandomState(11)
    for n in (1, 2, 3, 37, 63, 64, 65, 130, 2701):
        base = np.round(rs.standard_normal(n) * 3).astype(np.float32)             # many exact ties
        cases = [base, np.full(n, -np.inf, np.float32), np.full(n, np.nan, np.float32), np.full(n, np.inf, np.float32)]
        for k in range(6):
            s = base.copy()
            pos = rs.randint(0, n, size=min(n, 4))
            s[pos[0]] = np.nan if k % 2 == 0 else np.inf
            if k >= 2:
                s[pos[1:]] = (np.nan, -np.inf, np.inf)[:len(pos) - 1]
            if k >= 4:
                s[rs.randint(0, n, size=n // 2 + 1)] = -np.inf
            cases.append(s)
        for s in cases:
            want = int(torch.argmax(torch.from_numpy(s)))
            assert R.wave_argmax(s) == want, (n, s[:8], want)
            assert 0 <= R.wave_argmax(s) < n
