"""GPU tests of csrc/frontend.hip at real sizes against float64 (tests/frontend_doa_ref.py): the persistent frame walk
of stft_rows_kernel with every frame checked, every hop / centring / short length, structured signals with a
per-channel bound, recordings that cross the 1024-frame tile of the recursion, and arrays too wide for the frame-row
kernels.  Run with -m gpu on an MI355X; nothing here reads the reference checkout.

Bounds.  Spectrum: 5e-6 of the largest magnitude of the SAME (utterance, channel) (the project's STFT constant, on the
channel's own scale).  Magnitude sums: rtol 2e-6 on Gaussian input; on structured input max(2e-6, 4 d) of the
channel's largest sum, d being what a float32 torch.stft -> abs -> sum on the host deviates by.  mu on long signals:
max(3e-6, 3 d_mu) relative, d_mu being the float32 oracle's own deviation from float64.  Features: rtol 2e-5, atol
2e-5.  Every test prints the figures it measured before it asserts (pytest -s shows them)."""
import numpy as np
import pytest

import frontend_doa_ref as R
from conftest import assert_close, rs_randn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SPEC_TOL = 5e-6
MAGSUM_RTOL = 2e-6
FS = 16000


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()                      # fail loudly if the extension is missing
    return torch.device("cuda:0")


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def layouts(sig, dev):
    """The three waveform layouts of one logical [nb, ns, nch] batch: contiguous (sc == 1), [nb, nch, ns] memory
    (sn == 1), and every second channel of a 2 nch-channel buffer (neither stride is 1)."""
    a = to_dev(sig, dev)
    b = a.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    wide = torch.full((sig.shape[0], sig.shape[1], 2 * sig.shape[2]), 7.0, dtype=torch.float32, device=dev)
    wide[:, :, ::2] = a
    c = wide[:, :, ::2]
    assert a.stride(2) == 1 and b.stride(1) == 1 and c.stride(1) != 1 and c.stride(2) != 1
    return {"nsc": a, "ncs": b, "strided": c}


def spec_errors(spec, magsum, want, dev):
    """Per (utterance, channel): max |got - want| and max |want| of the spectrum; the magnitude sums' relative error
    per frame.  Compared on the device in float64 (the references are a hundred megabytes at walk size)."""
    w = to_dev(want, dev)                                                        # complex128 [nb, nch, nt, 257]
    got = torch.view_as_complex(spec).to(torch.complex128)
    assert got.shape == w.shape, "spectrum shape %s vs %s" % (tuple(got.shape), tuple(w.shape))
    err = (got - w).abs().amax(dim=(2, 3)).cpu().numpy()
    scale = w.abs().amax(dim=(2, 3)).cpu().numpy()
    ws = w.abs().sum(dim=3)
    serr = (magsum.to(torch.float64) - ws).abs().cpu().numpy()
    return err, scale, serr, ws.cpu().numpy()


def check_gaussian(spec, magsum, want, dev, what):
    """Every frame of the spectrum within SPEC_TOL of its channel's peak, every magnitude sum within MAGSUM_RTOL."""
    err, scale, serr, ws = spec_errors(spec, magsum, want, dev)
    rel = err / scale
    srel = serr / ws
    print("%s: spectrum %.3g of the channel peak, magsum %.3g relative" % (what, rel.max(), srel.max()))
    bad = np.argwhere(err > SPEC_TOL * scale)
    assert bad.size == 0, "%s: spectrum of (utterance, channel) %s off by %g of the channel's peak" % (
        what, bad[:4].tolist(), rel.max())
    badf = np.argwhere(serr > MAGSUM_RTOL * ws)
    assert badf.size == 0, "%s: magsum of %d frames off, first (b, c, t) %s, worst %g relative" % (
        what, len(badf), badf[:4].tolist(), srel.max())


def per_frame_kernel(monkeypatch, on):
    if on:
        monkeypatch.setenv("FNSSL_STFT_PER_FRAME", "1")
    else:
        monkeypatch.delenv("FNSSL_STFT_PER_FRAME", raising=False)


# --------------------------------------------------------------------------- a. the frame walk
def rows_waves(nch):
    return 4 if nch <= 4 else (8 if nch <= 8 else 16)


def walk_shape(dev, nch, extra=(0, 2)):
    """(nb, nt, CUs): at least 3 frames for every workgroup of the largest grid stft_rows_kernel can get (CUs * 32 / NW
    workgroups) and a ragged last sweep (the grid is a multiple of CUs), for nt and for nt + each of ``extra`` (the
    centred framing of the same signal has two more frames); nt odd, so neither a multiple of 4 nor of 64."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    nw = rows_waves(nch)
    nb = 32 // nw                                                                # 8 / 4 / 2 utterances
    need = 3 * cus * (32 // nw)
    nt = -(-need // nb) | 1
    while any((nb * (nt + e)) % cus == 0 for e in extra):
        nt += 2
    return nb, nt, cus


def assert_walk(nb, nt, nch, cus):
    """The test's own guard: a device with more CUs must not turn this back into a one-frame-per-workgroup test."""
    assert nb * nt >= 3 * cus * 32 // rows_waves(nch), "walk: %d frames do not give every workgroup three" % (nb * nt)
    assert (nb * nt) % cus != 0, "walk: %d frames leave no ragged last sweep on %d CUs" % (nb * nt, cus)
    assert nt % 4 != 0 and nt % 64 != 0


@pytest.mark.parametrize("nch", [2, 4, 5, 8, 9, 16])
def test_frame_walk_every_frame_against_float64(dev, monkeypatch, nch):
    """stft_rows_kernel<0, NW> as a persistent kernel: every workgroup walks at least three frames (prefetch of the
    next frame, commit, ragged last sweep), and EVERY frame of the spectrum and of magsum is compared with stft64.
    The three waveform layouts give the same bits; an utterance run alone (a smaller grid, another walk) gives the same
    bits; the one-wave-per-frame kernel (another algorithm) meets the same float64 bound, uncentred and centred.

    Measured on an MI355X (256 CUs: 8 / 4 / 2 utterances x 769 and 771 frames): spectrum <= 2.1e-7 of the channel's
    peak, magsum <= 1.7e-7 relative, both kernels."""
    from fnssl import ops
    nb, nt, cus = walk_shape(dev, nch)
    hop = 256
    ns = 512 + (nt - 1) * hop + 37
    sig = rs_randn(4100 + nch, (nb, ns, nch))
    views = layouts(sig, dev)
    for center in (False, True):
        want = R.stft64(sig, hop, center)
        ntc = want.shape[2]
        assert ntc == (nt + 2 if center else nt) == ops.num_frames(ns, hop, center)
        assert_walk(nb, ntc, nch, cus)
        per_frame_kernel(monkeypatch, False)
        spec, magsum = ops.stft(views["nsc"], hop, center)
        check_gaussian(spec, magsum, want, dev, "rows kernel, %d ch, center %d, %d x %d frames" % (nch, center, nb, ntc))
        for name in ("ncs", "strided"):
            s2, m2 = ops.stft(views[name], hop, center)
            assert torch.equal(s2, spec) and torch.equal(m2, magsum), "layout %s differs (center %d)" % (name, center)
        for u in (0, nb // 2, nb - 1):
            s1, m1 = ops.stft(views["nsc"][u:u + 1], hop, center)
            assert torch.equal(s1[0], spec[u]) and torch.equal(m1[0], magsum[u]), "utterance %d alone differs" % u
        del s1, m1, s2, m2
        per_frame_kernel(monkeypatch, True)
        spec, magsum = ops.stft(views["strided" if center else "ncs"], hop, center)
        check_gaussian(spec, magsum, want, dev, "per-frame kernel, %d ch, center %d" % (nch, center))
        del spec, magsum, want


@pytest.mark.parametrize("hop,center", [(256, False), (320, True)])
@pytest.mark.parametrize("nch", [4, 8, 15, 16])
def test_array_frontend_equals_two_step_path_at_walk_size(dev, nch, hop, center):
    """MODE 1 -> recursion -> MODE 2 (ops.array_frontend, which never writes the spectrum) against MODE 0 -> recursion ->
    pack (ops.preprocess_array, layout 0): same bits, with every workgroup of both transform passes walking at least
    three frames."""
    from fnssl import ops
    nb, nt, cus = walk_shape(dev, nch, extra=(0,))
    ns = (nt - 1) * hop + 11 if center else 512 + (nt - 1) * hop + 11
    assert ops.num_frames(ns, hop, center) == nt == R.num_frames(ns, hop, center)
    assert_walk(nb, nt, nch, cus)
    sig = to_dev(rs_randn(4200 + nch, (nb, ns, nch), 0.05), dev)
    one = ops.array_frontend(sig, hop=hop, center=center)
    two = ops.preprocess_array(sig, layout=0, hop=hop, center=center)
    assert one.shape == two.shape == (nb, nt, 256, 2 * nch)
    assert torch.isfinite(one).all()
    assert torch.equal(one, two), "array_frontend differs from stft + array_features in %d of %d rows" % (
        int((one != two).any(dim=3).any(dim=2).sum()), nb * nt)


# --------------------------------------------------------------------------- b. hops, centring, short and odd lengths
@pytest.mark.parametrize("per_frame", [False, True])
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("hop", [1, 100, 160, 256, 320, 512])
def test_hops_and_centring(dev, monkeypatch, hop, center, per_frame):
    """Every hop class of the ABI (1..512) with samples left over after the last frame, both framings, both kernels:
    the frame count is stft64's own, then the values."""
    from fnssl import ops
    left = {1: 0, 100: 63, 160: 159, 256: 255, 320: 1, 512: 300}[hop]
    ns = 512 + 9 * hop + left if hop > 1 else 512 + 40
    sig = rs_randn(4300 + hop, (2, ns, 3))
    want = R.stft64(sig, hop, center)
    per_frame_kernel(monkeypatch, per_frame)
    spec, magsum = ops.stft(to_dev(sig, dev), hop, center)
    assert spec.shape[2] == magsum.shape[2] == want.shape[2] == R.num_frames(ns, hop, center)
    check_gaussian(spec, magsum, want, dev, "hop %d center %d per-frame %d, %d frames" % (hop, center, per_frame, want.shape[2]))


@pytest.mark.parametrize("per_frame", [False, True])
def test_smallest_legal_signals(dev, monkeypatch, per_frame):
    """ns = 512 uncentred: one frame.  ns = 257 centred: two frames whose reflections on BOTH sides fall into the
    same frame's 512 samples.  ns = 256 centred: reflect padding is not defined (torch.stft's own check)."""
    from fnssl import ops
    per_frame_kernel(monkeypatch, per_frame)
    for ns, center, hop, nt in ((512, False, 256, 1), (257, True, 256, 2), (257, True, 1, 258), (300, True, 320, 1)):
        sig = rs_randn(4400 + ns + hop, (2, ns, 5))
        want = R.stft64(sig, hop, center)
        spec, magsum = ops.stft(to_dev(sig, dev), hop, center)
        assert spec.shape[2] == want.shape[2] == nt
        check_gaussian(spec, magsum, want, dev, "ns %d center %d hop %d per-frame %d" % (ns, center, hop, per_frame))
    with pytest.raises(RuntimeError, match="too short for reflect padding"):
        ops.stft(torch.zeros(1, 256, 2, device=dev), 256, True)
    with pytest.raises(RuntimeError, match="shorter than one"):
        ops.stft(torch.zeros(1, 511, 2, device=dev), 256, False)


# --------------------------------------------------------------------------- c. signal classes
CLASSES = ["gaussian", "quiet", "dc", "sine40", "cos100.37", "impulses", "zero", "zero2"]
STRUCTURED = ("dc", "sine40", "cos100.37", "impulses")


def class_batch(ns, seed):
    """[2, ns, 8]: Gaussian; Gaussian at 1e-4 of its neighbour's level; 1 + 1e-3 x Gaussian (DC); a sine exactly on bin
    40; a cosine at bin 100.37; two impulses; two all-zero channels (so that one microphone pair is silent)."""
    rs = np.random.RandomState(seed)
    n = np.arange(ns, dtype=np.float64)
    sig = np.zeros((2, ns, len(CLASSES)), dtype=np.float64)
    for u in range(2):
        g = rs.standard_normal(ns)
        sig[u, :, 0] = g
        sig[u, :, 1] = 1e-4 * rs.standard_normal(ns)
        sig[u, :, 2] = 1.0 + 1e-3 * rs.standard_normal(ns)
        sig[u, :, 3] = np.sin(2 * np.pi * 40.0 * n / 512 + 0.3 * u)
        sig[u, :, 4] = np.cos(2 * np.pi * 100.37 * n / 512 + 0.7 * u)
        sig[u, [ns // 3 + 5 * u, ns // 3 + 700 + u], 5] = (1.0, -0.5)
    return sig.astype(np.float32)


def host_float32_magsum(sig, hop, center):
    """An independent float32 chain on the host: torch.stft, abs, sum over the bins: [nb, nch, nt]."""
    nb, ns, nch = sig.shape
    x = torch.from_numpy(np.ascontiguousarray(sig.transpose(0, 2, 1))).reshape(nb * nch, ns)
    s = torch.stft(x, 512, hop_length=hop, win_length=512, window=torch.hann_window(512), center=center,
                   pad_mode="reflect", return_complex=True)                      # [nb * nch, 257, nt]
    return s.abs().sum(dim=1).reshape(nb, nch, -1).numpy()


@pytest.mark.parametrize("per_frame", [False, True])
@pytest.mark.parametrize("hop,center", [(160, False), (256, False), (320, False), (160, True), (256, True), (320, True)])
def test_signal_classes_per_channel_bound(dev, monkeypatch, hop, center, per_frame):
    """Spectrum: max |got - want| <= 5e-6 x max |want| over each (utterance, channel)'s OWN spectrum, so the channel
    80 dB below its neighbour is held to its own scale.  An all-zero channel gives exactly zero spectrum and magsum.
    magsum: rtol 2e-6 on the Gaussian channels; on the structured ones (DC, tones, impulses) the allowance is
    max(2e-6, 4 d) of the channel's largest sum, d = the host float32 torch.stft chain's deviation from float64 on the
    same input (a frame that catches an impulse at the window's edge has a tiny sum no float32 chain gets to 2e-6).

    Measured on an MI355X (range over the six framings and both kernels; d and the device's own deviation relative to
    the channel's largest sum):
        DC         d 2.5e-7 .. 3.7e-7   device <= 3.3e-7
        sine 40    d 2.0e-7 .. 6.6e-7   device <= 6.6e-7
        cos 100.37 d 7.4e-8 .. 2.1e-7   device <= 2.7e-7
        impulses   d 7.7e-8 .. 1.7e-7   device <= 1.1e-7 (3.2e-6 of the frame's OWN sum where the impulse sits at the
                                        window's edge: why the scale is the channel's)
    so the allowance was 2e-6 .. 2.7e-6.  Gaussian channels: <= 1.5e-7 of each frame's own sum.  Spectrum: <= 2.5e-7
    of the channel's peak on every class, the channel 80 dB down included."""
    from fnssl import ops
    ns = 512 + 40 * hop + 77
    sig = class_batch(ns, 4500 + hop)
    want = R.stft64(sig, hop, center)
    host32 = host_float32_magsum(sig, hop, center)
    per_frame_kernel(monkeypatch, per_frame)
    spec, magsum = ops.stft(to_dev(sig, dev), hop, center)
    err, scale, serr, ws = spec_errors(spec, magsum, want, dev)
    assert host32.shape == ws.shape
    top = ws.max(axis=2)                                                         # the channel's largest sum
    fails = []
    for c, name in enumerate(CLASSES):
        rel = err[:, c] / np.where(scale[:, c] > 0, scale[:, c], 1)
        if name.startswith("zero"):
            assert (scale[:, c] == 0).all()
            assert not spec[:, c].any() and not magsum[:, c].any(), "all-zero channel: spectrum or magsum not exactly zero"
            continue
        d = (np.abs(host32[:, c] - ws[:, c]).max(axis=1) / top[:, c]).max()
        dev_d = (serr[:, c].max(axis=1) / top[:, c]).max()
        with np.errstate(invalid="ignore", divide="ignore"):
            elementwise = np.nanmax(serr[:, c] / ws[:, c])                       # frames without an impulse are 0 / 0
        print("hop %d center %d per-frame %d %-9s: spectrum %.3g of the channel peak; magsum of the channel's largest sum: "
              "host float32 d %.3g, device %.3g; device elementwise %.3g" % (hop, center, per_frame, name, rel.max(), d, dev_d, elementwise))
        if (err[:, c] > SPEC_TOL * scale[:, c]).any():
            fails.append("%s: spectrum off by %g of the channel's peak" % (name, rel.max()))
        if name in STRUCTURED:
            allow = max(MAGSUM_RTOL, 4 * d)
            if (serr[:, c] > allow * top[:, c, None]).any():
                fails.append("%s: magsum off by %g of the channel's largest sum, allowed %g (host float32 d %g)" % (name, dev_d, allow, d))
        elif (serr[:, c] > MAGSUM_RTOL * ws[:, c]).any():
            fails.append("%s: magsum off by %g relative" % (name, elementwise))
    assert not fails, "; ".join(fails)
    if per_frame or hop != 256 or center:
        return
    # features of the same batch: finite everywhere, and the silent pair (6, 7) is 0 / eps = 0
    x, mu = ops.pair_features(spec, magsum, "MM", layout=0)
    assert torch.isfinite(x).all() and torch.isfinite(mu).all()
    last = ops.num_pairs(len(CLASSES), "MM") - 1                                 # pair (6, 7) of each utterance
    for u in range(2):
        p = u * (last + 1) + last
        assert not mu[p].any() and not x[p].any(), "silent pair: mu or features not exactly zero"
    xa, mua = ops.array_features(spec[:, 6:8].contiguous(), magsum[:, 6:8].contiguous(), layout=0)
    assert not xa.any() and not mua.any()


# --------------------------------------------------------------------------- d. long recordings
def drifting_signal(nt, nch, seed, hop=256, nb=2):
    """A level that drifts slowly, so that a lost carry of mu is far larger than rounding."""
    ns = 512 + (nt - 1) * hop
    t = np.arange(ns, dtype=np.float64) / FS
    env = 0.2 + np.abs(np.sin(2 * np.pi * 0.3 * t))
    g = np.random.RandomState(seed).standard_normal((nb, ns, nch))
    return (0.05 * g * env[None, :, None]).astype(np.float32)


def split_report(err, tol, what):
    """Fail with the frames below 1024 and from 1024 on reported separately (frames on the LAST axis)."""
    bad = err > tol
    if not bad.any():
        return
    ratio = err / np.where(tol > 0, tol, 1)
    lo, hi = ratio[..., :1024], ratio[..., 1024:]
    first = int(np.argwhere(bad.reshape(-1, bad.shape[-1]).any(axis=0))[0, 0])
    raise AssertionError("%s: frames < 1024: %d bad, worst %.3g x the bound; frames >= 1024: %d bad, worst %s x the bound; "
                         "first bad frame %d" % (what, int(bad[..., :1024].sum()), lo.max(), int(bad[..., 1024:].sum()),
                                                 "%.3g" % hi.max() if hi.size else "n/a", first))


def oracle_mu_deviation(mag32, sample_length, mu64):
    """d_mu: the float32 oracle's (O.forgetting_norm) largest relative deviation from mu64 on the same input."""
    from oracle import fnssl_oracle as O
    mu32 = O.forgetting_norm(mag32, sample_length)[:, 0, 0, :]
    return float((np.abs(mu32 - mu64) / np.abs(mu64)).max())


@pytest.mark.parametrize("ch_mode", ["MM", "M"])
@pytest.mark.parametrize("nt", [1024, 1025, 1300, 2100])
def test_long_recordings_pair_path(dev, nt, ch_mode):
    """ema_kernel carries mu across its 1024-frame tiles: exactly one tile, one frame past it, one carry, two carries.
    mu against mu64 within max(3e-6, 3 d_mu) relative, features in both layouts against the float64 chain.

    Measured on an MI355X (relative deviation of mu from mu64): sample_length 298: float32 oracle d_mu 7.8e-7 .. 1.5e-6,
    device 5.7e-7 .. 9.2e-7 (allowed 3e-6 .. 4.5e-6); sample_length 8: d_mu 2.0e-7 .. 2.3e-7, device 1.7e-7 .. 2.0e-7.
    Features: worst absolute error 3.4e-6.  With m reset at every tile, mu of frame 1024 is 2e5 times the bound off."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    sig = drifting_signal(nt, 3, 4600 + nt)
    want = R.stft64(sig)
    assert want.shape[2] == nt
    spec, magsum = ops.stft(to_dev(sig, dev))
    mag32 = np.abs(O.add_ch_to_batch(np.transpose(O.stft(sig), (0, 3, 1, 2)), ch_mode))
    for sl in (298, 8):
        a, b = ops.forgetting_coefs_host(nt, sl)
        np.testing.assert_array_equal(a, O.forgetting_coefs(nt, sl)[0])
        x64, mu64 = R.pair_features64(want, ch_mode, a, b, layout=1)
        d_mu = oracle_mu_deviation(mag32, sl, mu64)
        x1, mu = ops.pair_features(spec, magsum, ch_mode, sample_length=sl, layout=1)
        x0, mu0 = ops.pair_features(spec, magsum, ch_mode, sample_length=sl, layout=0)
        assert torch.equal(mu, mu0)
        mu = mu.cpu().numpy()
        allow = max(3e-6, 3 * d_mu)
        print("pair %s nt %d sample_length %d: float32 oracle d_mu %.3g, device %.3g (allowed %.3g)" % (
            ch_mode, nt, sl, d_mu, (np.abs(mu - mu64) / mu64).max(), allow))
        split_report(np.abs(mu - mu64), allow * np.abs(mu64), "mu, %s, sample_length %d" % (ch_mode, sl))
        x1 = x1.cpu().numpy()
        print("    features: worst |err| %.3g" % np.abs(x1 - x64).max())
        split_report(np.abs(x1 - x64), 2e-5 + 2e-5 * np.abs(x64), "features layout 1, %s, sample_length %d" % (ch_mode, sl))
        x0 = x0.cpu().numpy().transpose(0, 3, 2, 1)
        split_report(np.abs(x0 - x64), 2e-5 + 2e-5 * np.abs(x64), "features layout 0, %s, sample_length %d" % (ch_mode, sl))


@pytest.mark.parametrize("nt", [1024, 1025, 1300, 2100])
def test_long_recordings_array_path(dev, nt):
    """ema_array_kernel across its tiles, pack_array_kernel<0> and pack_array_planes_kernel (64-frame tiles: 1300 and
    2100 are not multiples of 64), and the spectrum-free ops.array_frontend, five channels, against float64.

    Measured on an MI355X: float32 oracle d_mu 8.1e-7 .. 1.1e-6, device 4.8e-7 .. 9.8e-7 (allowed 3e-6 .. 3.2e-6)."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    sl = 280
    sig = drifting_signal(nt, 5, 4700 + nt)
    want = R.stft64(sig)
    d = to_dev(sig, dev)
    spec, magsum = ops.stft(d)
    a, b = ops.forgetting_coefs_host(nt, sl)
    x64, mu64 = R.array_features64(want, a, b, layout=1)
    d_mu = oracle_mu_deviation(np.abs(np.transpose(O.stft(sig), (0, 3, 1, 2))), sl, mu64)
    allow = max(3e-6, 3 * d_mu)
    x1, mu1 = ops.array_features(spec, magsum, sample_length=sl, layout=1)
    x0, mu0 = ops.array_features(spec, magsum, sample_length=sl, layout=0)
    assert torch.equal(mu0, mu1)
    mu = mu1.cpu().numpy()
    print("array nt %d: float32 oracle d_mu %.3g, device %.3g (allowed %.3g)" % (nt, d_mu, (np.abs(mu - mu64) / mu64).max(), allow))
    split_report(np.abs(mu - mu64), allow * np.abs(mu64), "array mu")
    tol = 2e-5 + 2e-5 * np.abs(x64)
    split_report(np.abs(x1.cpu().numpy() - x64), tol, "array features layout 1")
    split_report(np.abs(x0.cpu().numpy().transpose(0, 3, 2, 1) - x64), tol, "array features layout 0")
    xf = ops.array_frontend(d, sample_length=sl)
    assert torch.equal(xf, x0), "array_frontend differs from stft + array_features"
    split_report(np.abs(xf.cpu().numpy().transpose(0, 3, 2, 1) - x64), tol, "array_frontend")


# --------------------------------------------------------------------------- e. wide arrays
def test_wide_array_features(dev):
    """33 channels: the one-wave-per-frame STFT, pack_array_kernel<0> with 66 KB of dynamic LDS (the
    hipFuncSetAttribute branch) and the planes kernel at nt = 70 (one full and one ragged 64-frame tile)."""
    from fnssl import ops
    nch, nt, sl = 33, 70, 280
    sig = rs_randn(4800, (2, 512 + (nt - 1) * 256 + 9, nch), 0.05)
    want = R.stft64(sig)
    spec, magsum = ops.stft(to_dev(sig, dev))
    check_gaussian(spec, magsum, want, dev, "33 channels")
    a, b = ops.forgetting_coefs_host(nt, sl)
    x64, mu64 = R.array_features64(want, a, b, layout=1)
    for layout in (0, 1):
        x, mu = ops.array_features(spec, magsum, sample_length=sl, layout=layout)
        assert_close(mu.cpu().numpy(), mu64, 3e-6, 0, "33-channel mu")
        x = x.cpu().numpy()
        assert_close(x if layout == 1 else x.transpose(0, 3, 2, 1), x64, 2e-5, 2e-5, "33-channel features, layout %d" % layout)


def test_too_wide_array_is_rejected(dev):
    """81 channels: the staging row of pack_array_kernel<0> would need 162 KB of LDS: an error, not a launch."""
    from fnssl import ops
    spec = torch.zeros((1, 81, 2, 257, 2), dtype=torch.float32, device=dev)
    magsum = torch.zeros((1, 81, 2), dtype=torch.float32, device=dev)
    for layout in (0, 1):
        with pytest.raises(RuntimeError, match="do not fit the staging row"):
            ops.array_features(spec, magsum, layout=layout)
    torch.cuda.synchronize(dev)
    x, _ = ops.array_features(spec[:, :5].contiguous(), magsum[:, :5].contiguous(), layout=0)   # the next launch is fine
    assert not x.any()
