"""GPU parity tests (run with -m gpu on an MI355X): every HIP kernel and the whole
DP-IPD path against the numpy oracle on seeded inputs and against the committed
golden vectors that were generated from the real reference.

Tolerance (north_star): fp32, rtol 1e-4 (+ atol 1e-5 because the outputs are tanh
of small numbers, SURVEY.md §7 "hard parts").  Integer/index work (pair order,
shapes) is exact.  Nothing here reads /root/reference.
"""
import os

import numpy as np
import pytest

from conftest import assert_close, load_golden, rs_randn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()                      # fail loudly if the extension is missing
    return torch.device("cuda:0")


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def lstm_state(I, H, bidir, seed):
    from fnssl import weights as W
    return W.make_state([("L." + n, s) for n, s in W.lstm_param_shapes(I, H, bidir)], seed=seed)


def packed_dirs(sd, c0, c2, bidir, dev):
    from fnssl import ops
    out = []
    for sfx in [""] + (["_reverse"] if bidir else []):
        out.append(ops.pack_lstm(sd["L.weight_ih_l0" + sfx], sd["L.weight_hh_l0" + sfx], sd["L.bias_ih_l0" + sfx],
                                 sd["L.bias_hh_l0" + sfx], c0, c2, dev))
    return out


# --------------------------------------------------------------------------- front end
def test_stft_matches_oracle_and_golden(dev):
    from fnssl import ops
    from oracle import fnssl_oracle as O
    g = load_golden("g1_stft")
    sig = rs_randn(g["seed"], g["shape"])
    spec, magsum = ops.stft(to_dev(sig, dev))
    got = torch.view_as_complex(spec).permute(0, 3, 2, 1).cpu().numpy()      # [nb, 257, nt, nch]
    scale = np.abs(g["out"]).max()
    assert got.shape == g["out"].shape
    assert np.abs(got - g["out"]).max() <= 5e-6 * scale, "vs reference golden"
    assert np.abs(got - O.stft(sig)).max() <= 5e-6 * scale, "vs oracle"
    want_sum = np.abs(O.stft(sig)).sum(axis=1).transpose(0, 2, 1)             # [nb, nch, nt]
    assert_close(magsum.cpu().numpy(), want_sum, 2e-6, 0, "magsum")


def test_stft_reads_permuted_batch_in_place(dev):
    from fnssl import ops
    batch = to_dev(rs_randn(7, (3, 2, 512 + 5 * 256)), dev)                  # [nb, nch, ns] like the dataloader
    a, _ = ops.stft(batch.permute(0, 2, 1))
    b, _ = ops.stft(batch.permute(0, 2, 1).contiguous())
    assert torch.equal(a, b)


@pytest.mark.parametrize("nch,layout", [(16, "nsc"), (17, "nsc"), (17, "ncs"), (33, "nsc")])
def test_stft_many_channels_matches_oracle(dev, nch, layout):
    """More channels than the frame-row kernel's fetch covers (16 waves x 64 lanes x 8 samples = 16 x 512): from 17
    channels on fnssl_stft_ex must take the one-wave-per-frame kernel — round 3's gate was the LDS size only, and the
    samples beyond 8192 per frame were never fetched (silently wrong spectra).  Both waveform layouts, magsum included."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    sig = rs_randn(900 + nch, (2, 512 + 4 * 256, nch))
    d = to_dev(sig, dev)
    if layout == "ncs":
        d = d.permute(0, 2, 1).contiguous().permute(0, 2, 1)             # [nb, nch, ns] memory, logical [nb, ns, nch]
    spec, magsum = ops.stft(d)
    got = torch.view_as_complex(spec).permute(0, 3, 2, 1).cpu().numpy()      # [nb, 257, nt, nch]
    want = O.stft(sig)
    scale = np.abs(want).max()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 5e-6 * scale, "vs oracle: %g" % (np.abs(got - want).max() / scale)
    assert_close(magsum.cpu().numpy(), np.abs(want).sum(axis=1).transpose(0, 2, 1), 2e-6, 0, "magsum")


def test_array_frontend_rejects_more_channels_than_it_fetches(dev):
    from fnssl import ops
    with pytest.raises(RuntimeError, match="at most 16 channels"):
        ops.array_frontend(torch.zeros(1, 512 + 5 * 256, 17, device=dev))


def test_stft_rejects_short_signal(dev):
    from fnssl import ops
    with pytest.raises(RuntimeError, match="shorter than one"):
        ops.stft(torch.zeros(1, 100, 2, device=dev))


@pytest.mark.parametrize("ch_mode", ["MM", "M"])
def test_features_match_oracle(dev, ch_mode):
    from fnssl import ops
    from oracle import fnssl_oracle as O
    sig = rs_randn(21, (2, 512 + 30 * 256, 4), 0.05)
    want = O.data_preprocess(sig, ch_mode)                                   # [nb', 4, 256, nt]
    x1 = ops.preprocess(to_dev(sig, dev), ch_mode, layout=1).cpu().numpy()
    x0 = ops.preprocess(to_dev(sig, dev), ch_mode, layout=0).cpu().numpy()
    assert_close(x1, want, 2e-5, 2e-5, "layout 1")
    np.testing.assert_array_equal(x0, np.transpose(x1, (0, 3, 2, 1)))


def test_features_golden_and_both_norm_branches(dev):
    from fnssl import ops
    from oracle import fnssl_oracle as O
    g = load_golden("g4_features")
    sig4 = rs_randn(g["seed4"], g["shape4"], float(g["scale4"]))
    x = ops.preprocess(to_dev(sig4, dev), "MM", layout=1).cpu().numpy()
    assert_close(x[:, :, ::16, :], g["x4_sub"], 2e-5, 2e-5, "golden x4 MM")
    # nt > sample_length exercises the second branch of forgetting_norm (utils.py:39-44)
    sig = rs_randn(22, (1, 512 + 19 * 256, 2))
    spec, magsum = ops.stft(to_dev(sig, dev))
    _, mu = ops.pair_features(spec, magsum, "MM", sample_length=8)
    mag = np.abs(O.add_ch_to_batch(np.transpose(O.stft(sig), (0, 3, 1, 2)), "MM"))
    assert_close(mu.cpu().numpy(), O.forgetting_norm(mag, 8)[:, 0, 0, :], 3e-6, 0, "mu, sample_length=8")


def test_nchw_to_seq_is_the_reference_permute(dev):
    from fnssl import ops
    x = to_dev(rs_randn(31, (3, 4, 37, 45)), dev)
    assert torch.equal(ops.nchw_to_seq(x), x.permute(0, 3, 2, 1).contiguous())


def test_module_dropins(dev):
    import Module as at_module
    g = load_golden("g2_pairs")
    d = to_dev(g["inp"], dev)
    np.testing.assert_array_equal(at_module.AddChToBatch("MM")(d).cpu().numpy(), g["out_mm"])
    np.testing.assert_array_equal(at_module.AddChToBatch("M")(d).cpu().numpy(), g["out_m"])
    g1 = load_golden("g1_stft")
    sig = rs_randn(g1["seed"], g1["shape"])
    st = at_module.STFT(512, 0.5, 512)(to_dev(sig, dev))
    assert st.dtype == torch.complex64 and tuple(st.shape) == g1["out"].shape
    assert np.abs(st.cpu().numpy() - g1["out"]).max() <= 5e-6 * np.abs(g1["out"]).max()


# --------------------------------------------------------------------------- LSTM kernel
LSTM_CASES = [
    # c0, c2, H, bidir, mode, nb, nt, nf
    (4, 0, 16, True, "full", 2, 5, 7),
    (32, 4, 32, False, "narrow", 2, 6, 9),
    (4, 0, 128, True, "full", 1, 19, 6),
    (256, 0, 128, True, "full", 2, 9, 5),
    (256, 4, 256, False, "narrow", 1, 7, 21),
    (256, 0, 256, False, "narrow", 2, 5, 17),
    (256, 4, 128, True, "narrow", 1, 6, 18),
    (48, 20, 64, False, "full", 1, 17, 4),
]


def run_layer(dev, c0, c2, H, bidir, mode, nb, nt, nf, variant=0, seed=0, with_skip=None):
    from fnssl import ops
    from oracle import fnssl_oracle as O
    sd = lstm_state(c0 + c2, H, bidir, 1000 + seed)
    x0 = rs_randn(1100 + seed, (nb, nt, nf, c0)) if c0 else None
    x1 = rs_randn(1200 + seed, (nb, nt, nf, c0)) if (c0 and with_skip) else None
    x2 = rs_randn(1300 + seed, (nb, nt, nf, c2)) if c2 else None
    ndir = 2 if bidir else 1
    out = torch.full((nb, nt, nf, ndir * H), float("nan"), device=dev)
    ops.lstm_layer(mode, None if x0 is None else to_dev(x0, dev), None if x1 is None else to_dev(x1, dev),
                   None if x2 is None else to_dev(x2, dev), packed_dirs(sd, c0, c2, bidir, dev), H, out, variant)
    parts = []
    if x0 is not None:
        parts.append(x0 + x1 if x1 is not None else x0)
    if x2 is not None:
        parts.append(x2)
    xin = np.concatenate(parts, axis=-1)
    if mode == "full":
        seqs = xin.reshape(nb * nt, nf, -1)
        want = O.lstm(seqs, sd, "L.", bidir).reshape(nb, nt, nf, -1)
    else:
        seqs = np.transpose(xin, (0, 2, 1, 3)).reshape(nb * nf, nt, -1)
        want = np.transpose(O.lstm(seqs, sd, "L.", bidir).reshape(nb, nf, nt, -1), (0, 2, 1, 3))
    return out.cpu().numpy(), want


@pytest.mark.parametrize("case", LSTM_CASES)
def test_lstm_layer_matches_oracle(dev, case):
    c0, c2, H, bidir, mode, nb, nt, nf = case
    got, want = run_layer(dev, *case, seed=c0 + H)
    assert not np.isnan(got).any(), "some outputs were never written"
    assert_close(got, want, RTOL, ATOL, "lstm %s" % (case,))
    got, want = run_layer(dev, *case, seed=c0 + H + 1, with_skip=True)
    assert_close(got, want, RTOL, ATOL, "lstm + residual input %s" % (case,))


@pytest.mark.parametrize("H,c0", [(256, 256), (128, 256), (128, 4)])
def test_lstm_kernel_variants_are_bit_identical(dev, H, c0):
    """All launch geometries (waves per workgroup, LDS ring or direct weight reads) run the same
    k-ordered fp32 MFMA chain per sequence, so they must agree bit for bit."""
    base, want = run_layer(dev, c0, 0, H, True if H == 128 else False, "narrow", 2, 6, 23, variant=1, seed=5,
                           with_skip=c0 > 4)
    assert_close(base, want, RTOL, ATOL, "variant 1")
    for v in range(2, 9):
        got, _ = run_layer(dev, c0, 0, H, True if H == 128 else False, "narrow", 2, 6, 23, variant=v, seed=5,
                           with_skip=c0 > 4)
        np.testing.assert_array_equal(got, base, err_msg="variant %d differs from variant 1" % v)


def test_lstm_strided_views_and_ragged_tail(dev):
    """Sequence count not a multiple of 16, outputs written into a permuted (narrow-layout) buffer."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    nb, nt, nf, H = 3, 7, 11, 32
    sd = lstm_state(16, H, False, 77)
    x = rs_randn(78, (nb, nt, nf, 16))
    buf = torch.full((nb, nf, nt, H), float("nan"), device=dev)
    ops.lstm_layer("narrow", to_dev(x, dev), None, None, packed_dirs(sd, 16, 0, False, dev), H,
                   buf.permute(0, 2, 1, 3))
    seqs = np.transpose(x, (0, 2, 1, 3)).reshape(nb * nf, nt, -1)
    want = O.lstm(seqs, sd, "L.", False).reshape(nb, nf, nt, H)
    assert_close(buf.cpu().numpy(), want, RTOL, ATOL, "narrow layout output")


def test_lstm_fused_residual_output(dev):
    """out_sum = h + skip (the next layer's residual input) is exactly the separate add."""
    from fnssl import ops
    for mode, H, bidir in (("narrow", 256, False), ("full", 128, True), ("narrow", 32, True)):
        nb, nt, nf = 2, 7, 19
        c0 = 256 if H > 32 else 32
        sd = lstm_state(c0, H, bidir, 91)
        w = packed_dirs(sd, c0, 0, bidir, dev)
        x = to_dev(rs_randn(92, (nb, nt, nf, c0)), dev)
        ndir = 2 if bidir else 1
        skip = to_dev(rs_randn(93, (nb, nt, nf, ndir * H)), dev)
        plain = torch.empty((nb, nt, nf, ndir * H), device=dev)
        ops.lstm_layer(mode, x, None, None, w, H, plain)
        out = torch.full_like(plain, float("nan"))
        osum = torch.full_like(plain, float("nan"))
        ops.lstm_layer(mode, x, None, None, w, H, out, skip=skip, out_sum=osum)
        assert torch.equal(out, plain), "raw output changed: max diff %g" % float((out - plain).abs().max())
        assert torch.equal(osum, plain + skip), "sum output: max diff %g" % float((osum - plain - skip).abs().max())


def test_launch_planner_and_static_kernels_match_generic(dev):
    """variant 0 = launch planner (uneven multi-round wave counts) + shape-specialised kernels;
    it must be bit-identical to an explicit generic variant."""
    from fnssl import ops
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    # (mode, H, bidir, c0, c2, nb, nt, nf, with residual output)
    cases = [("full", 128, True, 256, 0, 1, 33000, 3, True),     # 2063 groups x 2 dirs -> 17 waves/CU -> rounds 9(12) + ...
             ("full", 128, True, 4, 0, 1, 40000, 3, False),
             ("narrow", 256, False, 256, 0, 3, 5, 1000, True),
             ("narrow", 256, False, 256, 4, 3, 5, 1000, True),
             ("narrow", 128, True, 256, 4, 1, 4, 700, True),
             # IPDnet shapes (16-channel concat skip): 4 / 8 / 12 waves per CU, full-band block 2
             ("narrow", 256, False, 256, 16, 1, 4, 16000, False),
             ("narrow", 256, False, 256, 16, 2, 3, 16000, False),
             ("narrow", 256, False, 256, 16, 3, 3, 16000, False),
             ("full", 128, True, 256, 16, 1, 19200, 3, False)]
    for mode, H, bidir, c0, c2, nb, nt, nf, with_sum in cases:
        sd = lstm_state(c0 + c2, H, bidir, 300 + c0 + c2 + H)
        w = packed_dirs(sd, c0, c2, bidir, dev)
        ndir = 2 if bidir else 1
        x0 = torch.randn((nb, nt, nf, c0), generator=g, device=dev)
        x2 = torch.randn((nb, nt, nf, c2), generator=g, device=dev) if c2 else None
        skip = torch.randn((nb, nt, nf, ndir * H), generator=g, device=dev) if with_sum else None
        outs = []
        for variant in (0, 5 if H == 128 else 4):
            out = torch.full((nb, nt, nf, ndir * H), float("nan"), device=dev)
            osum = torch.full_like(out, float("nan")) if with_sum else None
            ops.lstm_layer(mode, x0, None, x2, w, H, out, variant, skip=skip, out_sum=osum)
            outs.append((out, osum))
        assert not torch.isnan(outs[0][0]).any(), (mode, H, c0, c2)
        assert torch.equal(outs[0][0], outs[1][0]), (mode, H, c0, c2)
        if with_sum:
            assert torch.equal(outs[0][1], outs[1][1]), (mode, H, c0, c2)


def test_lstm_rejects_bad_descriptors(dev):
    from fnssl import ops
    sd = lstm_state(16, 32, False, 5)
    w = packed_dirs(sd, 16, 0, False, dev)
    x = torch.zeros(1, 4, 4, 16, device=dev)
    with pytest.raises(RuntimeError, match="out shape"):
        ops.lstm_layer("full", x, None, None, w, 32, torch.zeros(1, 4, 4, 64, device=dev))
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        ops.lstm_layer("full", x.cpu(), None, None, w, 32, torch.zeros(1, 4, 4, 32, device=dev))


# --------------------------------------------------------------------------- blocks / network
@pytest.mark.parametrize("online", [True, False])
def test_fnblock_golden(dev, online):
    import Model as at_model
    from fnssl import weights as W
    g = load_golden("g6_fnblock")
    t = "on" if online else "off"
    s1, sx, s2 = [int(v) for v in g[t + "_seeds"]]
    b1 = at_model.FNblock(4, hidden_size=32, is_online=online, is_first=True)
    b1.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_fnblock_state(s1, 4, 32, online, True).items()})
    b2 = at_model.FNblock(32, hidden_size=32, is_online=online, is_first=False)
    b2.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_fnblock_state(s2, 32, 32, online, False).items()})
    b1, b2 = b1.to(dev).eval(), b2.to(dev).eval()
    x = to_dev(rs_randn(sx, (2, 6, 8, 4)), dev)
    y1, fb1, nb1 = b1(x)
    y2, fb2, nb2 = b2(y1, fb_skip=fb1, nb_skip=nb1)
    for name, got in [("y1", y1), ("fb1", fb1), ("nb1", nb1), ("y2", y2), ("fb2", fb2), ("nb2", nb2)]:
        assert tuple(got.shape) == g[t + "_" + name].shape, name
        assert_close(got.contiguous().cpu().numpy(), g[t + "_" + name], RTOL, ATOL, t + " " + name)


def build_net(dev, seed, online=True, doa=False):
    import Model as at_model
    from fnssl import weights as W
    sd = W.make_fnssl_state(seed, is_online=online, is_doa=doa)
    net = at_model.FN_SSL(is_online=online, is_doa=doa)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(dev).eval(), sd


@pytest.mark.parametrize("online", [True, False])
def test_fnssl_golden(dev, online):
    g = load_golden("g7_fnssl")
    t = "on" if online else "off"
    sw, sa, sb, sc = [int(v) for v in g[t + "_seeds"]]
    net, _ = build_net(dev, sw, online)
    for key, seed, shape in (("_a", sa, (2, 4, 16, 24)), ("_b", sb, (1, 4, 256, 36)), ("_c", sc, (3, 4, 16, 29))):
        got = net(to_dev(rs_randn(seed, shape), dev)).cpu().numpy()
        assert_close(got, g[t + key], RTOL, ATOL, "FN_SSL %s%s" % (t, key))


def test_fnssl_doa_golden(dev):
    g = load_golden("g7_fnssl")
    sw, sx = [int(v) for v in g["doa_seeds"]]
    net, _ = build_net(dev, sw, True, True)
    got = net(to_dev(rs_randn(sx, (1, 4, 256, 12)), dev)).cpu().numpy()
    assert got.shape == (1, 1, 180)
    assert_close(got, g["doa_out"], RTOL, ATOL, "DOA head")


def test_fnssl_block_by_block_equals_fused(dev):
    """FNblock.forward x3 + head (the reference's call sequence) == the fused library forward."""
    from fnssl import ops
    net, _ = build_net(dev, 55)
    x = to_dev(rs_randn(56, (2, 4, 32, 26)), dev)
    fused = net(x)
    xs = x.permute(0, 3, 2, 1)
    y, fb, nbs = net.block_1(xs)
    y, fb, nbs = net.block_2(y, fb_skip=fb, nb_skip=nbs)
    y, fb, nbs = net.block_3(y, fb_skip=fb, nb_skip=nbs)
    out = ops.head(y.permute(0, 2, 1, 3), net.emb2ipd.weight.detach(), net.emb2ipd.bias.detach())
    assert torch.equal(out, fused), "max diff %g" % float((out - fused).abs().max())


def test_fnssl_requires_eval_and_device(dev):
    import Model as at_model
    net = at_model.FN_SSL().to(dev)
    # train mode (a fresh nn.Module's default) = the autograd route (tests/test_gpu_autograd.py); the streaming entry is
    # inference only
    assert net(torch.zeros(1, 4, 16, 12, device=dev)).grad_fn is not None
    with pytest.raises(RuntimeError, match="eval"):
        net.forward_stream(torch.zeros(1, 4, 16, 12, device=dev))
    net.eval()
    assert net(torch.zeros(1, 4, 16, 12, device=dev)).grad_fn is None
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        net(torch.zeros(1, 4, 16, 12))
    with pytest.raises(RuntimeError, match="expected"):
        net(torch.zeros(1, 3, 16, 12, device=dev))
    assert tuple(net(torch.zeros(2, 4, 16, 11, device=dev)).shape) == (2, 0, 32)   # < 12 frames: empty, like AvgPool


def test_predict_step_config1_golden(dev):
    """BASELINE config 1: one 4 s 2-mic utterance, waveform -> DP-IPD, against the reference's output."""
    import predict_step as ps
    from fnssl import weights as W
    g = load_golden("g9_config1")
    sw, sx = [int(v) for v in g["seeds"]]
    model = ps.MyModel(device=str(dev))
    model.arch.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_fnssl_state(sw).items()})
    model = model.to(dev).eval()
    batch = to_dev(rs_randn(sx, g["shape"], float(g["scale"])), dev)
    out = model.predict_step(batch, 0)
    assert tuple(out.shape) == (1, 20, 512)
    assert_close(out.cpu().numpy(), g["out"], RTOL, ATOL, "config 1 end to end")
    feats = model.data_preprocess(batch.permute(0, 2, 1))[0]
    assert tuple(feats.shape) == (1, 4, 256, 249)
    assert_close(feats.cpu().numpy()[:, :, ::32, ::8], g["x_sub"], 2e-5, 2e-5, "config 1 features")


# --------------------------------------------------------------------------- size-independent properties
def test_pairs_are_independent_and_chunking_is_exact(dev):
    """Every mic pair is an independent unit: a pair's output must not depend on
    its batch mates, on the pass it is processed in, or on the launch geometry."""
    net, _ = build_net(dev, 61)
    x = to_dev(rs_randn(62, (7, 4, 48, 40)), dev)
    whole = net(x)
    net.chunk_pairs = 3
    chunked = net(x)
    net.chunk_pairs = 0
    assert torch.equal(whole, chunked)
    for p in (0, 3, 6):
        assert torch.equal(net(x[p:p + 1]), whole[p:p + 1])


def test_full_size_frame_slice_against_oracle(dev):
    """BASELINE config-2 geometry (257 bins x 300 frames) on one 2-mic utterance vs the oracle."""
    from oracle import fnssl_oracle as O
    import predict_step as ps
    net, sd = build_net(dev, 71)
    batch = rs_randn(72, (1, 2, 77056), 0.05)
    model = ps.MyModel(device=str(dev))
    model.arch = net
    out = model.predict_step(to_dev(batch, dev), 0).cpu().numpy()
    want = O.predict_step(sd, batch, "MM", True)
    assert out.shape == want.shape == (1, 25, 512)
    assert_close(out, want, RTOL, ATOL, "257 x 300 utterance")


# --------------------------------------------------------------------------- IPD -> DOA back end (next row)
def test_doa_backend_golden(dev):
    """PredDOA / SourceDetectLocalize / DPIPD drop-ins against the reference's outputs: candidate
    choices exact, spectra and ratios within fp32 tolerance."""
    import Module as at_module
    g = load_golden("g12_doa")
    for ci in range(2):
        seed, nbp, nt, ns, knum = [int(v) for v in g["c%d_cfg" % ci]]
        pd = at_module.PredDOA(method_mode="IDL", source_num_mode="kNum" if knum else "unkNum",
                               max_num_sources=ns, ch_mode="MM", device=str(dev)).to(dev)
        pred = to_dev(np.tanh(rs_randn(seed, (nbp, nt, 512))), dev)
        out, _ = pd.predgt2DOA(pred_batch=pred, gt_batch=None)
        np.testing.assert_array_equal(out["doa"].cpu().numpy(), g["c%d_doa" % ci])
        assert_close(out["vad_sources"].cpu().numpy(), g["c%d_vad" % ci], 1e-4, 1e-6, "vad")
        assert_close(out["spatial_spectrum"].cpu().numpy(), g["c%d_ss" % ci], 1e-5, 1e-6, "spatial spectrum")
    # time_pool_size (Module.py:723-730): localisation on the mean of every 2 consecutive segments == localisation of the
    # pooled prediction
    pd = at_module.PredDOA(max_num_sources=1, ch_mode="MM", device=str(dev)).to(dev)
    pred = to_dev(np.tanh(rs_randn(1230, (3, 5, 512))), dev)
    pooled = torch.stack((pred[:, 0:2].mean(dim=1), pred[:, 2:4].mean(dim=1)), dim=1)
    a_, _ = pd.predgt2DOA(pred_batch=pred, time_pool_size=2)
    b_, _ = pd.predgt2DOA(pred_batch=pooled)
    assert a_["doa"].shape == (3, 2, 2, 1)
    np.testing.assert_array_equal(a_["doa"].cpu().numpy(), b_["doa"].cpu().numpy())
    assert_close(a_["spatial_spectrum"].cpu().numpy(), b_["spatial_spectrum"].cpu().numpy(), 1e-5, 1e-6, "pooled spectrum")
    mics4 = g["tmpl_mics"]
    for mode in ("MM", "M"):
        t, _, cand = at_module.DPIPD([5, 9], mics4, nf=257, fre_max=8000, ch_mode=mode, speed=340)()
        assert_close(t[:, :, ::16, :], g["tmpl_" + mode], 1e-5, 1e-5, "template " + mode)
    from fnssl import doa as fdoa
    t, cand = fdoa.dpipd_templates(mics4, 37, 73, 257, 8000, "MM", 340)
    bank, cand = fdoa.template_bank(t)
    sdl = at_module.SourceDetectLocalize(max_num_sources=2, source_num_mode="unkNum", meth_mode="IDL")
    pred4 = to_dev(np.tanh(rs_randn(int(g["m4_seed"][0]), (2, 4, 512, 6))), dev)
    doa, vad, ss = sdl(pred_ipd=pred4, dpipd_template=to_dev(bank, dev), doa_candidate=cand)
    np.testing.assert_array_equal(doa.cpu().numpy(), g["m4_doa"])
    assert_close(vad.cpu().numpy(), g["m4_vad"], 1e-4, 1e-6, "4-mic vad")
    assert_close(ss.cpu().numpy(), g["m4_ss"], 1e-5, 1e-6, "4-mic spatial spectrum")


def test_doa_peak_detection_golden(dev):
    """SourceDetectLocalize(meth_mode='PD') (fnssl_ipd2doa + fnssl_doa_peaks) against the REAL reference's outputs (G17) and
    against the oracle on a frame with a single peak (broadcast) and with none (RuntimeError, like Module.py:615)."""
    import Module as at_module
    from fnssl import doa as fdoa
    from oracle import fnssl_oracle as O
    g = load_golden("g17_doa_pd")
    mics = g["mics"]
    for ci in range(int(g["ncases"][0])):
        seed, nb, nt, nele, nazi, mm, ns, knum = [int(v) for v in g["c%d_cfg" % ci]]
        gen = at_module.DPIPD([nele, nazi], mics, nf=257, fre_max=8000, ch_mode="MM" if mm else "M", speed=340)
        t, _, cand = gen()
        bank = np.concatenate((t.real[:, :, 1:257, :], t.imag[:, :, 1:257, :]), axis=2).astype(np.float32)
        pred = np.tanh(rs_randn(seed, (nb, nt, 512, bank.shape[-1])))
        mix = float(g["c%d_mix" % ci][0])
        if mix:
            pred = (pred * 0.3 + mix * bank[nele // 2 + 1, 4][None, None]).astype(np.float32)
        sdl = at_module.SourceDetectLocalize(max_num_sources=ns, source_num_mode="kNum" if knum else "unkNum", meth_mode="PD")
        doa, vad, ss = sdl(pred_ipd=to_dev(pred, dev), dpipd_template=to_dev(bank, dev), doa_candidate=cand)
        assert_close(ss.cpu().numpy(), g["c%d_ss" % ci], 1e-5, 1e-6, "pd spectrum %d" % ci)
        np.testing.assert_array_equal(doa.cpu().numpy(), g["c%d_doa" % ci])
        assert_close(vad.cpu().numpy(), g["c%d_vad" % ci], 1e-4, 1e-6, "pd vad %d" % ci)
    for ns in (1, 3):
        with pytest.raises(RuntimeError):
            at_module.SourceDetectLocalize(max_num_sources=ns, meth_mode="PD")(to_dev(pred, dev), to_dev(bank, dev), cand)
    # the kernel alone on hand-made spectra: ties keep index order, a frame with one peak, a frame with none
    ss = np.zeros((3, 5, 7), dtype=np.float32)
    ss[0, 2, 1] = ss[0, 3, 4] = 2.0                       # two equal peaks: the lower flat index first
    ss[0, 1, 6] = 9.0                                     # last azimuth column: never a peak (:581)
    ss[0, 0, 3] = 9.0                                     # elevation row 0: never a peak (clamped neighbour = itself)
    ss[1, 2, 0] = 1.0                                     # one peak; its circular neighbour is column 5, not 6
    ss[1, 2, 6] = 5.0
    idx = torch.empty((3, 2), dtype=torch.int32, device=dev)
    val = torch.empty((3, 2), dtype=torch.float32, device=dev)
    cnt = torch.empty((3,), dtype=torch.int32, device=dev)
    import ctypes as C
    lib = fdoa._lib.load()
    fdoa._lib.check(lib.fnssl_doa_peaks(C.c_void_p(to_dev(ss, dev).data_ptr()), 3, 5, 7, 2, C.c_void_p(idx.data_ptr()),
                                        C.c_void_p(val.data_ptr()), C.c_void_p(cnt.data_ptr()), None), "doa_peaks")
    torch.cuda.synchronize(dev)
    assert cnt.tolist() == [2, 1, 0]
    assert idx.tolist() == [[2 * 7 + 1, 3 * 7 + 4], [2 * 7 + 0, -1], [-1, -1]] and val.tolist() == [[2.0, 2.0], [1.0, 0.0], [0.0, 0.0]]


def test_data_preprocess_nor_flag_false_is_the_raw_real_imag_pairs(dev):
    """main.py:219-221: with nor_flag=False the features are the pairs' real / imaginary STFT parts as they are."""
    import predict_step as ps
    from fnssl import ops
    m = ps.MyModel(device=str(dev))
    sig = to_dev(rs_randn(61, (2, 512 + 23 * 256, 3), 0.1), dev)                       # [nb, ns, nch]
    x, = m.data_preprocess(sig, nor_flag=False)
    spec, _ = ops.stft(sig)                                                          # [nb, nch, nt, 257] (re, im) interleaved
    spec = spec.reshape(2, 3, 24, 257, 2)
    pairs = [(0, 1), (0, 2), (1, 2)]
    assert tuple(x.shape) == (6, 4, 256, 24)
    for b in range(2):
        for p, (i, j) in enumerate(pairs):
            want = torch.stack((spec[b, i, :, 1:, 0], spec[b, j, :, 1:, 0], spec[b, i, :, 1:, 1], spec[b, j, :, 1:, 1]), 0)   # [4, nt, 256]
            assert torch.equal(x[b * 3 + p], want.permute(0, 2, 1)), (b, p)
    xn, = m.data_preprocess(sig)                                                      # and the default still normalises
    assert not torch.equal(xn, x)


def test_dpipd_targets_kernel_golden_and_reference_training_step_literal(dev):
    """The training TARGETS on device (fnssl_dpipd_targets) against the real reference's (G16: DPIPD.forward(source_doa) +
    main.py:227-262) and the oracle; then the reference's training_step as written — batch = (mic_sig, {'doa', 'vad_sources'}),
    `in_batch, gt_batch = self.data_preprocess(mic_sig_batch, gt_batch)`, forward with a graph, cal_loss, backward, Adam —
    through predict_step.MyModel(fused_engine=False)."""
    import predict_step as ps
    from fnssl import doa as fdoa
    from fnssl import weights as W
    from oracle import fnssl_oracle as O
    g = load_golden("g16_dpipd_targets")
    for name in ("c0", "c1", "c2", "c3"):
        mode = "MM" if int(g[name + "_cfg"][0]) else "M"
        use_vad = bool(int(g[name + "_cfg"][1]))
        mics, doa, vad = g[name + "_mics"], g[name + "_doa"], g[name + "_vad"]
        ipd, vmean = fdoa.dpipd_targets(to_dev(doa, dev), to_dev(vad, dev), mics, mode, 1, 256, 257, 8000.0, 340.0, use_vad)
        assert_close(ipd.cpu().numpy(), g[name + "_ipd"], 0, 2e-6, name + " targets vs the reference")
        assert_close(vmean.cpu().numpy(), g[name + "_vmean"], 0, 1e-7, name + " vad mean")
        want, _ = O.dpipd_targets(doa, vad, mics, mode, use_vad)
        assert_close(ipd.cpu().numpy(), want, 0, 2e-6, name + " targets vs the oracle")
    # no VAD tensor: every source active
    ipd_nv, _ = fdoa.dpipd_targets(to_dev(g["c1_doa"], dev), None, g["c1_mics"], "MM", use_vad=True)
    want_nv, _ = O.dpipd_targets(g["c1_doa"], np.ones_like(g["c1_vad"]), g["c1_mics"], "MM", True)
    assert_close(ipd_nv.cpu().numpy(), want_nv, 0, 2e-6, "targets without a VAD tensor")
    # ---- the reference's training_step, literally (two-microphone array of main.py:121-123)
    m = ps.MyModel(device=str(dev), fused_engine=False)
    m.arch.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in W.make_fnssl_state(9).items()})
    m.to(dev).train()
    nb, nseg = 2, 2
    sig = to_dev(rs_randn(51, (nb, 512 + (12 * nseg - 1) * 256, 2), 0.1), dev)           # [nb, ns, nch]
    rs = np.random.RandomState(52)
    doa = np.stack((np.full((nb, nseg, 1), np.pi / 2), rs.uniform(0.0, np.pi, (nb, nseg, 1))), axis=2).astype(np.float32)
    vad = np.ones((nb, nseg, 12, 1), dtype=np.float32)
    opt = m.configure_optimizers()["optimizer"]
    losses = []
    for _ in range(4):
        gt = {"doa": torch.from_numpy(doa), "vad_sources": torch.from_numpy(vad)}       # host tensors, as a dataloader yields
        out = m.training_step((sig, gt), 0)
        assert gt["ipd"].shape == (nb, nseg, 512, 1) and gt["ipd"].is_cuda and gt["vad_sources"].shape == (nb, nseg, 1)
        opt.zero_grad()
        out["loss"].backward()
        opt.step()
        losses.append(float(out["loss"].detach()))
    want_ipd, _ = O.dpipd_targets(doa, vad, np.array(((-0.04, 0.0, 0.0), (0.04, 0.0, 0.0))), "MM", True)
    assert_close(gt["ipd"].cpu().numpy(), want_ipd, 0, 2e-6, "targets built inside training_step")
    assert losses[-1] < losses[0], losses


def test_waveform_to_doa_end_to_end(dev):
    """waveform -> DP-IPD -> DOA entirely on device equals oracle forward + oracle back end."""
    import Module as at_module
    import predict_step as ps
    from oracle import fnssl_oracle as O
    net, sd = build_net(dev, 81)
    model = ps.MyModel(device=str(dev))
    model.arch = net
    batch = rs_randn(82, (2, 2, 512 + 35 * 256), 0.05)
    pred = model.predict_step(to_dev(batch, dev), 0)
    pd = at_module.PredDOA(max_num_sources=1, device=str(dev)).to(dev)
    out, _ = pd.predgt2DOA(pred_batch=pred)
    want = O.pred_to_doa(O.predict_step(sd, batch, "MM", True), 2, np.array(((-0.04, 0, 0), (0.04, 0, 0))))
    np.testing.assert_array_equal(out["doa"].cpu().numpy(), want["doa"])
    assert_close(out["spatial_spectrum"].cpu().numpy(), want["spatial_spectrum"], 1e-4, 1e-5, "spectrum")


# --------------------------------------------------------------------------- IPDnet row
def _ipdnet_module():
    import importlib.util
    import os
    import sys
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(here, "fn-ssl_amd", "IPDnet", "FixedAarryIPDnet.py")
    if "fnssl_ipdnet_dropin" in sys.modules:
        return sys.modules["fnssl_ipdnet_dropin"]
    spec = importlib.util.spec_from_file_location("fnssl_ipdnet_dropin", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["fnssl_ipdnet_dropin"] = mod
    spec.loader.exec_module(mod)
    return mod


def _oracle_conv(xa, xb, w, act):
    """[nb, nf, nt, C] channels-last operands -> causal conv, channels-last."""
    from oracle import fnssl_oracle as O
    x = xa if xb is None else np.concatenate([xa, xb], axis=-1)
    y = O.conv3x3_pad12(np.transpose(x, (0, 3, 1, 2)), w)[:, :, :, :-2]
    if act == "relu":
        y = np.maximum(y, 0)
    elif act == "tanh":
        y = np.tanh(y)
    return np.transpose(y, (0, 2, 3, 1))


@pytest.mark.parametrize("cout,ca,cb,nb,nf,nt,act", [
    (128, 16, 4, 2, 5, 23, "relu"),      # conv1 of the 2-mic network, ragged time tile
    (128, 32, 16, 1, 3, 40, "none"),     # segment B with a full 16-channel block
    (128, 128, 0, 1, 4, 16, "relu"),     # conv2
    (6, 128, 0, 2, 3, 5, "tanh"),        # conv3, cout not a multiple of 4, nt < 3 taps + tile
    (28, 128, 0, 1, 1, 33, "tanh"),      # 8-mic head, a single frequency row
    (64, 16, 12, 1, 2, 17, "none"),      # 4-tile kernel with a 3-block remainder
])
def test_conv3x3_causal_matches_oracle(dev, cout, ca, cb, nb, nf, nt, act):
    from fnssl import ops
    w = rs_randn(2100 + cout + ca, (cout, ca + cb, 3, 3), 0.1)
    xa = rs_randn(2200, (nb, nf, nt, ca))
    xb = rs_randn(2201, (nb, nf, nt, cb)) if cb else None
    packed = ops.pack_conv3x3(w, ca, cb, dev)
    got = ops.conv3x3_causal(to_dev(xa, dev), to_dev(xb, dev) if cb else None, packed, cout, act)
    assert got.shape == (nb, nf, nt, (cout + 3) // 4 * 4)
    got = got.cpu().numpy()
    assert_close(got[..., :cout], _oracle_conv(xa, xb, w, act), RTOL, ATOL, "conv3x3")
    assert not got[..., cout:].any(), "padding channels must be zero"


def test_conv3x3_reads_strided_operands_in_place(dev):
    """The head reads the narrow-band output ([nb, nf, nt, C]) and the network input (stored
    [nb, nt, nf, C]) through strides; results equal the contiguous call bit for bit."""
    from fnssl import ops
    nb, nf, nt, ca, cb, cout = 2, 4, 19, 32, 4, 128
    w = rs_randn(2300, (cout, ca + cb, 3, 3), 0.1)
    packed = ops.pack_conv3x3(w, ca, cb, dev)
    xa = to_dev(rs_randn(2301, (nb, nf, nt, ca)), dev)
    xb_store = to_dev(rs_randn(2302, (nb, nt, nf, cb)), dev)
    xb = xb_store.permute(0, 2, 1, 3)
    wide = to_dev(rs_randn(2303, (nb, nf, nt, ca + 16)), dev)
    wide[..., :ca] = xa
    a = ops.conv3x3_causal(xa, xb.contiguous(), packed, cout, "relu")
    b = ops.conv3x3_causal(wide[..., :ca], xb, packed, cout, "relu")
    assert torch.equal(a, b)


def test_conv3x3_and_pool_reject_bad_arguments(dev):
    from fnssl import _lib, ops
    with pytest.raises(RuntimeError, match="unsupported sizes"):
        ops.pack_conv3x3(np.zeros((129, 16, 3, 3), np.float32), 16, 0, dev)
    with pytest.raises(RuntimeError, match="unsupported sizes"):
        ops.pack_conv3x3(np.zeros((8, 20, 3, 3), np.float32), 20, 0, dev)        # ca must be a multiple of 16
    with pytest.raises(RuntimeError, match="does not match"):
        ops.pack_conv3x3(np.zeros((8, 20, 3, 3), np.float32), 16, 8, dev)
    x = torch.zeros((1, 2, 8, 16), device=dev)
    with pytest.raises(RuntimeError):
        ops.conv3x3_causal(x.cpu(), None, x, 8)
    lib = _lib.load()
    assert lib.fnssl_avgpool_time(None, 1, 1, 4, 1, None, None) != 0
    assert b"avgpool_time" in lib.fnssl_last_error()


def test_avgpool_time_matches_oracle(dev):
    from fnssl import ops
    from oracle import fnssl_oracle as O
    x = rs_randn(2400, (2, 3, 26, 8))
    for k in (3, 4):
        got = ops.avgpool_time(to_dev(x, dev), k).cpu().numpy()
        want = np.transpose(O.avgpool_t(np.transpose(x, (0, 3, 1, 2)), k), (0, 2, 3, 1))
        assert_close(got, want, 1e-6, 1e-7, "avgpool k=%d" % k)
    assert ops.avgpool_time(to_dev(x[:, :, :2], dev), 3).shape == (2, 3, 0, 8)


def test_causcnnblock_golden(dev):
    M = _ipdnet_module()
    g = load_golden("g10_ipdnet")
    blk = M.CausCnnBlock(inp_dim=20, out_dim=6).eval()
    sdc = {"conv%d.weight" % (i + 1): torch.from_numpy(rs_randn(1700 + i, s, 0.1)) for i, s in
           enumerate([(128, 20, 3, 3), (128, 128, 3, 3), (6, 128, 3, 3)])}
    blk.load_state_dict(sdc)
    blk.to(dev)
    got = blk(to_dev(rs_randn(1710, (2, 20, 7, 26)), dev))
    assert_close(got.cpu().numpy(), g["cnn_out"], RTOL, ATOL, "CausCnnBlock vs reference golden")


def test_ipdnet_golden(dev):
    """IPDnet.forward against outputs of the real reference (2-mic online/offline, 8-mic hidden 256,
    257-like wide band) and against the oracle."""
    from fnssl import weights as W
    from oracle import fnssl_oracle as O
    M = _ipdnet_module()
    g = load_golden("g10_ipdnet")
    ci = 0
    while "c%d_cfg" % ci in g:
        cfg = [int(v) for v in g["c%d_cfg" % ci]]
        isz, hid, mt, online, wseed, xseed = cfg[:6]
        shape = tuple(cfg[6:])
        sd = W.make_ipdnet_state(wseed, isz, hid, mt, bool(online))
        net = M.IPDnet(input_size=isz, hidden_size=hid, max_track=mt, is_online=bool(online)).eval()
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
        net.to(dev)
        x = rs_randn(xseed, shape)
        got = net(to_dev(x, dev)).cpu().numpy()
        assert_close(got, g["c%d_out" % ci], RTOL, ATOL, "IPDnet case %d vs reference golden" % ci)
        assert_close(got, O.ipdnet_forward(sd, x, bool(online)), RTOL, ATOL, "IPDnet case %d vs oracle" % ci)
        ci += 1
    assert ci == 4


def test_ipdnet_chunkwise_offline_inference_golden(dev):
    from fnssl import weights as W
    M = _ipdnet_module()
    g = load_golden("g10_ipdnet")
    sd = W.make_ipdnet_state(1520, 4, 128, 2, False)
    net = M.IPDnet(input_size=4, hidden_size=128, max_track=2, is_online=False, n_seg=24).eval()
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    net.to(dev)
    got = net(to_dev(rs_randn(1620, (2, 4, 16, 40)), dev), offline_inference=True)
    assert_close(got.cpu().numpy(), g["seg_out"], RTOL, ATOL, "chunk-wise offline inference")


def test_ipdnet_fnblock_reference_signature(dev):
    """FNblock.forward(x, fb_skip, nb_skip) of the IPDnet tree returns the concatenated tensor."""
    from fnssl import weights as W
    from oracle import fnssl_oracle as O
    M = _ipdnet_module()
    sd = W.make_ipdnet_state(2500, 4, 128, 2, True)
    nb, nt, nf = 2, 12, 9
    x = rs_randn(2501, (nb, nt, nf, 4))
    b1 = M.FNblock(input_size=4, hidden_size=128, add_skip_dim=4, is_online=True, is_first=True).eval()
    b2 = M.FNblock(input_size=128, hidden_size=128, add_skip_dim=4, is_online=True, is_first=False).eval()
    for blk, pre in ((b1, "block_1."), (b2, "block_2.")):
        blk.load_state_dict({k[len(pre):]: torch.from_numpy(v.copy()) for k, v in sd.items() if k.startswith(pre)})
        blk.to(dev)
    xd = to_dev(x, dev)
    fb = xd.reshape(nb * nt, nf, 4)
    nbs = xd.permute(0, 2, 1, 3).reshape(nb * nf, nt, 4)
    y1 = b1(xd, fb, nbs)
    y2 = b2(y1, fb, nbs)
    w1 = O.ipdnet_block(sd, "block_1.", x, x, True)
    w2 = O.ipdnet_block(sd, "block_2.", w1, x, True)
    assert_close(y1.cpu().numpy(), w1, RTOL, ATOL, "block_1")
    assert_close(y2.cpu().numpy(), w2, RTOL, ATOL, "block_2")


def test_ipdnet_config3_shape_smoke(dev):
    """BASELINE.json config 3 geometry at a reduced batch: 8 mics, hidden 256, 257 bins, 48 frames."""
    from fnssl import weights as W
    M = _ipdnet_module()
    sd = W.make_ipdnet_state(2600, 16, 256, 2, True)
    net = M.IPDnet(input_size=16, hidden_size=256, max_track=2, is_online=True).eval()
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    net.to(dev)
    x = to_dev(rs_randn(2601, (2, 16, 257, 48)), dev)
    y = net(x)
    assert y.shape == (2, 4, 514, 7, 2)
    assert torch.isfinite(y).all() and float(y.abs().max()) <= 1.0
    # utterances are independent: a batch of one gives the same rows bit for bit
    assert torch.equal(net(x[1:2]), y[1:2])


def test_ipdnet_array_features_golden(dev):
    """STFT + all-channel recursive normalisation (runIPDnetOn.py:240-254) in both layouts."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    g = load_golden("g10_ipdnet")
    sig = rs_randn(1630, (2, 256 * 14, 4), 0.1)
    x1 = ops.preprocess_array(to_dev(sig, dev), layout=1)
    x0 = ops.preprocess_array(to_dev(sig, dev), layout=0)
    scale = np.abs(g["feat_out"]).max()
    assert x1.shape == g["feat_out"].shape
    assert np.abs(x1.cpu().numpy() - g["feat_out"]).max() <= 5e-6 * scale, "vs reference golden"
    assert np.abs(x1.cpu().numpy() - O.array_preprocess(sig)).max() <= 5e-6 * scale, "vs oracle"
    assert torch.equal(x0, x1.permute(0, 3, 2, 1).contiguous()), "layout 0 is the same numbers, channels-last"


def test_ipdnet_waveform_to_ipd(dev):
    """Waveforms -> features -> IPDnet, against the oracle chain (8 microphones, 16 input channels)."""
    from fnssl import ops
    from fnssl import weights as W
    from oracle import fnssl_oracle as O
    M = _ipdnet_module()
    sd = W.make_ipdnet_state(2700, 16, 128, 2, True)
    net = M.IPDnet(input_size=16, hidden_size=128, max_track=2, is_online=True).eval()
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    net.to(dev)
    sig = rs_randn(2701, (1, 256 * 25, 8), 0.1)
    got = net(ops.preprocess_array(to_dev(sig, dev)))
    want = O.ipdnet_forward(sd, O.array_preprocess(sig), True)
    assert got.shape == want.shape == (1, 2, 512, 7, 2)
    assert_close(got.cpu().numpy(), want, RTOL, ATOL, "waveform -> IPD")


# --------------------------------------------------------------------------- streaming
def test_lstm_carry_state_continues_a_sequence(dev):
    """Two calls with carry == one call over the concatenated steps, bit for bit (generic and static kernels)."""
    from fnssl import ops
    for c0, c2 in ((256, 0), (256, 4)):
        H, nb, nf, T1, T2 = 256, 1, 40, 5, 7
        sd = lstm_state(c0 + c2, H, False, 3100 + c2)
        w = packed_dirs(sd, c0, c2, False, dev)
        x0 = to_dev(rs_randn(3101, (nb, T1 + T2, nf, c0)), dev)
        x2 = to_dev(rs_randn(3102, (nb, T1 + T2, nf, c2)), dev) if c2 else None
        whole = torch.empty((nb, nf, T1 + T2, H), device=dev).permute(0, 2, 1, 3)
        ops.lstm_layer("narrow", x0, None, x2, w, H, whole)
        buf = torch.full((nb, nf, T1 + T2 + 1, H), float("nan"), device=dev)
        ws = ops.lstm_state_workspace(nb * nf, H, dev)
        a = buf[:, :, 1:T1 + 1].permute(0, 2, 1, 3)
        ops.lstm_layer("narrow", x0[:, :T1], None, x2[:, :T1] if c2 else None, w, H, a, carry_workspace=ws)
        b = buf[:, :, T1 + 1:].permute(0, 2, 1, 3)                  # the row before it is chunk 1's last h
        ops.lstm_layer("narrow", x0[:, T1:], None, x2[:, T1:] if c2 else None, w, H, b, carry_workspace=ws, carry=True)
        assert torch.equal(buf[:, :, 1:].permute(0, 2, 1, 3), whole), (c0, c2)
    with pytest.raises(RuntimeError, match="carry"):
        ops.lstm_layer("narrow", x0, None, x2, w, H, whole, carry=True)


@pytest.mark.parametrize("doa", [False, True])
def test_fnssl_forward_stream_equals_whole_signal(dev, doa):
    import Model
    from fnssl import weights as W
    nf = 256 if doa else 24
    net = Model.FN_SSL(is_doa=doa).eval()
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in W.make_fnssl_state(3200, is_doa=doa).items()})
    net.to(dev)
    x = to_dev(rs_randn(3201, (2, 4, nf, 48)), dev)
    whole = net(x)
    outs, state = [], None
    for lo, hi in ((0, 12), (12, 36), (36, 48)):
        y, state = net.forward_stream(x[..., lo:hi].contiguous(), state)
        outs.append(y)
    assert state["frames"] == 48
    assert torch.equal(torch.cat(outs, dim=1), whole)
    with pytest.raises(RuntimeError, match="multiple of 12"):
        net.forward_stream(x[..., :13].contiguous())
    off = Model.FN_SSL(is_online=False).eval().to(dev)
    with pytest.raises(RuntimeError, match="online"):
        off.forward_stream(x)


# --------------------------------------------------------------------------- bf16 MFMA path (BASELINE config 3)
# Tolerances.  Against the bf16-emulating oracle (same operand rounding, fp32 accumulation in another order;
# an operand that sits on a rounding boundary can flip one bf16 ulp = 2^-8 relative) the LSTM outputs agree to
# 4e-3 absolute (|h| <= 1; typically 1e-6).  Against the fp32 oracle the network output (tanh, |y| <= 1) is within 2e-2
# relative + 2e-3 absolute — the tolerance SURVEY.md §8d suggests for config 3.
BF_ATOL = 4e-3


@pytest.mark.parametrize("mode,H,bidir,c0,c2,nb,nt,nf", [
    ("narrow", 256, False, 256, 16, 1, 9, 40),      # IPDnet hidden 256: narrow-band, ragged last group
    ("full", 128, True, 256, 16, 1, 20, 7),         # full-band of block 2, both directions
    ("full", 128, True, 16, 0, 2, 9, 6),            # full-band of block 1: the 16 input channels alone
    ("narrow", 128, False, 128, 16, 2, 7, 16),      # hidden 128 (two microphones, padded skip)
    ("full", 64, True, 128, 16, 1, 18, 5),
    ("full", 64, True, 16, 0, 1, 17, 4),
    ("narrow", 128, True, 256, 16, 1, 6, 24),       # offline narrow-band (bi-directional H=128 on 256 + 16)
])
def test_lstm_bf16_layer_matches_bf16_oracle(dev, mode, H, bidir, c0, c2, nb, nt, nf):
    from fnssl import ops
    from oracle import fnssl_oracle as O
    I = c0 + c2
    sd = lstm_state(I, H, bidir, 4100 + H + I)
    x = rs_randn(4101, (nb, nt, nf, I), 0.7)
    seq = x.reshape(nb * nt, nf, I) if mode == "full" else np.transpose(x, (0, 2, 1, 3)).reshape(nb * nf, nt, I)
    want = O.lstm(seq, sd, "L.", bidir, bf16=True)
    want32 = O.lstm(seq, sd, "L.", bidir)
    ndir = 2 if bidir else 1
    want, want32 = [w.reshape(nb, nt, nf, -1) if mode == "full" else np.transpose(w.reshape(nb, nf, nt, -1), (0, 2, 1, 3))
                    for w in (want, want32)]
    w = [ops.pack_lstm_bf16(sd["L.weight_ih_l0" + s], sd["L.weight_hh_l0" + s], sd["L.bias_ih_l0" + s],
                            sd["L.bias_hh_l0" + s], c0, c2, dev) for s in ([""] + (["_reverse"] if bidir else []))]
    xd = to_dev(x, dev)
    out = torch.full((nb, nt, nf, ndir * H), float("nan"), device=dev)
    ops.lstm_layer(mode, xd[..., :c0].contiguous(), None, xd[..., c0:].contiguous() if c2 else None, w, H, out, bf16=True)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= BF_ATOL, "vs bf16 oracle: %g" % np.abs(got - want).max()
    assert np.abs(got - want32).max() <= 3e-2, "vs fp32 oracle: %g" % np.abs(got - want32).max()


def test_lstm_bf16_rejects_unbuilt_shapes(dev):
    from fnssl import ops
    sd = lstm_state(128, 256, False, 4200)
    w = [ops.pack_lstm_bf16(sd["L.weight_ih_l0"], sd["L.weight_hh_l0"], sd["L.bias_ih_l0"], sd["L.bias_hh_l0"], 128, 0, dev)]
    x = torch.zeros((1, 4, 16, 128), device=dev)
    out = torch.zeros((1, 4, 16, 256), device=dev)
    with pytest.raises(RuntimeError, match="bf16 path is not built"):
        ops.lstm_layer("narrow", x, None, None, w, 256, out, bf16=True)
    with pytest.raises(RuntimeError, match="unsupported sizes"):
        ops.pack_lstm_bf16(np.zeros((1024, 132), np.float32), sd["L.weight_hh_l0"], sd["L.bias_ih_l0"], sd["L.bias_hh_l0"],
                           128, 4, dev)


@pytest.mark.parametrize("isz,hid,online,shape", [(16, 256, True, (1, 16, 32, 24)), (4, 128, True, (2, 4, 16, 24)),
                                                  (16, 256, False, (1, 16, 16, 36))])
def test_ipdnet_bf16_config3(dev, isz, hid, online, shape):
    """IPDnet after .bfloat16() (bf16 weights, bf16 MFMA operands, fp32 accumulate) against the bf16-emulating
    oracle and, at the config-3 tolerance, against the fp32 oracle."""
    from fnssl import weights as W
    from oracle import fnssl_oracle as O
    M = _ipdnet_module()
    sd = W.make_ipdnet_state(4300 + isz, isz, hid, 2, online)
    net = M.IPDnet(input_size=isz, hidden_size=hid, max_track=2, is_online=online).eval()
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    net.to(dev).bfloat16()
    x = rs_randn(4301, shape)
    y = net(to_dev(x, dev).bfloat16())
    assert y.dtype == torch.bfloat16
    want_bf = O.ipdnet_forward(sd, x, online, bf16=True)
    want_32 = O.ipdnet_forward(sd, x, online)
    got = y.float().cpu().numpy()
    assert got.shape == want_32.shape
    # the returned tensor is itself rounded to bf16 (relative 2^-9)
    assert np.abs(got - want_bf).max() <= BF_ATOL + 4e-3 * np.abs(want_bf).max(), np.abs(got - want_bf).max()
    assert_close(got, want_32, 2e-2, 2e-3, "bf16 IPDnet vs fp32 oracle")
    # fp32 input works too and returns fp32
    y32 = net(to_dev(O.bf16_round(x), dev))
    assert y32.dtype == torch.float32 and np.abs(y32.cpu().numpy() - want_bf).max() <= BF_ATOL


@pytest.mark.parametrize("nb,nf,nt", [(8, 32, 24), (64, 256, 300)])
def test_ipdnet_bf16_two_stream_branch_vs_oracle_and_one_stream(dev, monkeypatch, nb, nf, nt):
    """The branch BASELINE config 3's benchmark runs (IPDnet.forward: bf16 wide path, batch >= 8 -> the two halves of
    the batch on two side streams with per-stream workspaces, record_stream, torch.cat) — at the smallest batch that
    takes it and at config 3's real 64 x 16 x 256 x 300 batch (600 full-band workgroups, multi-pass conv tiles):
      * one utterance of the batch against the bf16-restating oracle and, at SURVEY 8d's config-3 tolerance, the fp32 one;
      * the whole output bit-identical to the one-stream path (FNSSL_IPDNET_ONE_STREAM=1);
      * three repetitions bit-identical (a race between the side streams would show)."""
    from fnssl import weights as W
    from oracle import fnssl_oracle as O
    M = _ipdnet_module()
    monkeypatch.delenv("FNSSL_IPDNET_ONE_STREAM", raising=False)
    monkeypatch.setenv("FNSSL_IPDNET_STREAMS", "2")          # (opt-in since the cluster kernels: one stream is the default)
    sd = W.make_ipdnet_state(4500, 16, 256, 2, True)
    net = M.IPDnet(input_size=16, hidden_size=256, max_track=2, is_online=True).eval()
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    net.to(dev).bfloat16()
    assert net._two_streams(nb), "this batch must take the two-stream branch"
    x = O.bf16_round(rs_randn(4501, (nb, 16, nf, nt)))
    xd = to_dev(x, dev)
    outs = [net(xd) for _ in range(3)]
    torch.cuda.synchronize()
    assert outs[0].dtype == torch.float32 and tuple(outs[0].shape) == (nb, nt // 12, 2 * nf, 7, 2)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "two-stream runs differ: a race"
    monkeypatch.setenv("FNSSL_IPDNET_ONE_STREAM", "1")
    assert not net._two_streams(nb)
    one = net(xd)
    assert torch.equal(one, outs[0]), "two streams vs one stream"
    monkeypatch.delenv("FNSSL_IPDNET_ONE_STREAM")
    for b in sorted({0, nb // 2, nb - 1}) if nb <= 8 else (nb // 2 + 3,):       # a row of each half / one of the big batch
        want_bf = O.ipdnet_forward(sd, x[b:b + 1], True, bf16=True)
        got = outs[0][b:b + 1].cpu().numpy()
        assert np.abs(got - want_bf).max() <= BF_ATOL, (b, np.abs(got - want_bf).max())
        assert_close(got, O.ipdnet_forward(sd, x[b:b + 1], True), 2e-2, 2e-3, "bf16 IPDnet (two streams) vs fp32 oracle")


@pytest.mark.parametrize("cout,ca,cb,nb,nf,nt,act", [(128, 256, 16, 1, 4, 21, "relu"), (128, 128, 0, 2, 3, 16, "relu"),
                                                      (28, 128, 0, 1, 2, 9, "tanh"), (4, 128, 0, 1, 5, 5, "tanh"),
                                                      (128, 16, 16, 1, 3, 17, "none")])
def test_conv3x3_bf16_matches_bf16_oracle(dev, cout, ca, cb, nb, nf, nt, act):
    from fnssl import ops
    from oracle import fnssl_oracle as O
    w = rs_randn(4400 + cout + ca, (cout, ca + cb, 3, 3), 0.1)
    xa = rs_randn(4401, (nb, nf, nt, ca))
    xb = rs_randn(4402, (nb, nf, nt, cb)) if cb else None
    packed = ops.pack_conv3x3(w, ca, cb, dev, bf16=True)
    got = ops.conv3x3_causal(to_dev(xa, dev), to_dev(xb, dev) if cb else None, packed, cout, act, bf16=True).cpu().numpy()
    want = _oracle_conv(O.bf16_round(xa), O.bf16_round(xb) if cb else None, O.bf16_round(w), act)
    scale = max(1.0, np.abs(want).max())
    assert np.abs(got[..., :cout] - want).max() <= 2e-5 * scale, np.abs(got[..., :cout] - want).max()
    assert not got[..., cout:].any()
    with pytest.raises(RuntimeError, match="unsupported sizes"):
        ops.pack_conv3x3(np.zeros((8, 20, 3, 3), np.float32), 16, 4, dev, bf16=True)


# --------------------------------------------------------------------------- randomized shape sweep
def test_lstm_random_shapes_all_launch_paths(dev):
    """40 seeded random layer shapes (hidden size, input segments, batch, frames, bins, direction, layout) through
    whatever launch path the planner picks (generic / shape-specialised / several-waves-per-group / multi-round),
    each against the oracle; plus the explicit single-geometry variant, which must agree bit for bit."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    rng = np.random.RandomState(20260927)
    for it in range(40):
        H = int(rng.choice([16, 32, 64, 128, 256]))
        bidir = bool(rng.randint(2))
        mode = "full" if rng.randint(2) else "narrow"
        c0 = int(rng.choice([0, 4, 16, 64, 128, 256])) if H >= 64 else int(rng.choice([4, 16, 32]))
        c2 = int(rng.choice([0, 4, 16])) if c0 else int(rng.choice([4, 16]))
        nb, nt, nf = int(rng.randint(1, 4)), int(rng.randint(1, 10)), int(rng.randint(1, 45))
        I = c0 + c2
        sd = lstm_state(I, H, bidir, 5000 + it)
        x = rs_randn(5100 + it, (nb, nt, nf, I), 0.8)
        seq = x.reshape(nb * nt, nf, I) if mode == "full" else np.transpose(x, (0, 2, 1, 3)).reshape(nb * nf, nt, I)
        want = O.lstm(seq, sd, "L.", bidir)
        want = want.reshape(nb, nt, nf, -1) if mode == "full" else np.transpose(want.reshape(nb, nf, nt, -1), (0, 2, 1, 3))
        w = packed_dirs(sd, c0, c2, bidir, dev)
        xd = to_dev(x, dev)
        x0 = xd[..., :c0].contiguous() if c0 else None
        x2 = xd[..., c0:].contiguous() if c2 else None
        ndir = 2 if bidir else 1
        outs = []
        for variant in (0, 2):
            if mode == "narrow":       # natural narrow-band storage
                out = torch.full((nb, nf, nt, ndir * H), float("nan"), device=dev).permute(0, 2, 1, 3)
            else:
                out = torch.full((nb, nt, nf, ndir * H), float("nan"), device=dev)
            ops.lstm_layer(mode, x0, None, x2, w, H, out, variant)
            outs.append(out)
        tag = (it, mode, H, bidir, c0, c2, nb, nt, nf)
        assert_close(outs[0].cpu().numpy(), want, RTOL, ATOL, "random shape %s" % (tag,))
        assert torch.equal(outs[0], outs[1]), tag


@pytest.mark.parametrize("online", [True, False])
def test_fnssl_bf16_fast_mode(dev, online):
    """FN_SSL after .bfloat16(): bf16 MFMA operands in the six LSTMs, everything else fp32 — against the
    bf16-emulating oracle (tight) and the fp32 oracle (the deviation a user of the fast mode gets)."""
    import Model
    from fnssl import weights as W
    from oracle import fnssl_oracle as O
    sd = W.make_fnssl_state(4500, is_online=online)
    net = Model.FN_SSL(is_online=online).eval()
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    net.to(dev).bfloat16()
    x = rs_randn(4501, (2, 4, 24, 36))
    y = net(to_dev(x, dev).bfloat16())
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (2, 3, 48)
    want_bf = O.fnssl_forward(sd, x, online, bf16=True)
    want_32 = O.fnssl_forward(sd, x, online)
    got = y.float().cpu().numpy()
    assert np.abs(got - want_bf).max() <= BF_ATOL + 4e-3 * np.abs(want_bf).max()
    assert_close(got, want_32, 2e-2, 4e-3, "bf16 fast mode vs fp32 oracle")
    y32 = net(to_dev(O.bf16_round(x), dev))                      # fp32 in, fp32 out
    assert y32.dtype == torch.float32 and np.abs(y32.cpu().numpy() - want_bf).max() <= BF_ATOL
    with pytest.raises(RuntimeError, match="FN_SSL.forward"):
        net.block_1(to_dev(rs_randn(1, (1, 2, 3, 4)), dev))


# --------------------------------------------------------------------------- size-independent properties
def test_online_models_are_causal_bit_for_bit(dev):
    """The online FN-SSL and IPDnet must not look ahead: the output for the first 36 frames is the same whether
    or not 12 more frames follow (full-band layers only mix frequencies, narrow-band LSTMs and the conv head are
    causal).  Checked bit for bit at the full 256-bin width, in fp32 and in the bf16 mode."""
    import Model
    from fnssl import weights as W
    M = _ipdnet_module()
    fn = Model.FN_SSL().eval()
    fn.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in W.make_fnssl_state(5300).items()})
    ipd = M.IPDnet(input_size=16, hidden_size=256, max_track=2, is_online=True).eval()
    ipd.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in W.make_ipdnet_state(5301, 16, 256, 2, True).items()})
    xf = to_dev(rs_randn(5302, (3, 4, 256, 48)), dev)
    xi = to_dev(rs_randn(5303, (2, 16, 256, 48)), dev)
    for net, x in ((fn, xf), (ipd, xi)):
        net.to(dev)
        for bf in (False, True):
            if bf:
                net.bfloat16()
            whole = net(x)
            prefix = net(x[..., :36].contiguous())
            assert torch.equal(whole[:, :3], prefix), (type(net).__name__, bf)
    # the offline FN-SSL is NOT causal (bi-directional narrow-band LSTM): the same check must fail there
    off = Model.FN_SSL(is_online=False).eval()
    off.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in W.make_fnssl_state(5304, is_online=False).items()})
    off.to(dev)
    assert not torch.equal(off(xf)[:, :3], off(xf[..., :36].contiguous()))


@pytest.mark.parametrize("isz,hid", [(16, 256), (4, 128)])
def test_ipdnet_forward_stream_equals_whole_signal(dev, isz, hid):
    from fnssl import weights as W
    M = _ipdnet_module()
    sd = W.make_ipdnet_state(5400 + isz, isz, hid, 2, True)
    net = M.IPDnet(input_size=isz, hidden_size=hid, max_track=2, is_online=True).eval()
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    net.to(dev)
    x = to_dev(rs_randn(5401, (2, isz, 20, 72)), dev)
    whole = net(x)
    outs, state = [], None
    for lo, hi in ((0, 12), (12, 48), (48, 60), (60, 72)):
        y, state = net.forward_stream(x[..., lo:hi].contiguous(), state)
        outs.append(y)
    assert state["frames"] == 72
    assert torch.equal(torch.cat(outs, dim=1), whole)
    with pytest.raises(RuntimeError, match="multiple of 12"):
        net.forward_stream(x[..., :10].contiguous())
    off = M.IPDnet(input_size=isz, hidden_size=hid, is_online=False).eval().to(dev)
    with pytest.raises(RuntimeError, match="online"):
        off.forward_stream(x[..., :12].contiguous())


# --------------------------------------------------------------------------- config 2 at its real batch
def test_config2_full_batch_independence_and_oracle(dev):
    """BASELINE config 2 as benchmarked: 32 utterances x 4 mics x 77 056 samples -> 192 pairs x 300 frames through
    the full-chip launch geometry (lstm_static_kernel<256,12,..>, the 15 + 14 wave H = 128 rounds) that the small
    cases never reach.  (i) pairs are independent: three utterances of the batch run alone (different launch
    geometry: the several-waves-per-group kernels) give bit-identical rows; (ii) one 4-mic utterance's 6 pairs match
    the PyTorch-CPU restatement of Lightning/main.py:184-189 at rtol 1e-4 / atol 1e-5."""
    import predict_step as ps
    from fnssl import weights as W
    from oracle import torch_ref as R
    free, _ = torch.cuda.mem_get_info(dev)
    # (a failure, not a skip: on a shared box the headline configuration must not drop out of the parity set silently)
    assert free >= 100 * 2 ** 30, "config 2 needs ~90 GB of free HBM for the 192-pair activation plan, %.0f GB free" % (free / 2 ** 30)
    sd = W.make_fnssl_state(0)
    model = ps.MyModel(ch_mode="MM", device=str(dev))
    model.arch.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(dev).eval()
    gen = torch.Generator(device=dev)
    gen.manual_seed(77)
    batch = torch.randn((32, 4, 77056), generator=gen, device=dev)
    # the kernels this test is about: at this size the library must pick the operand-ring kernel for the narrow-band layers
    # and the cluster-resident kernel for the full-band ones (descriptors only: nothing is launched, nothing dereferenced)
    from fnssl import ops as _ops
    big = torch.empty((192, 300, 256, 256), device=dev)                  # (never touched: one buffer stands in for every operand)
    bign = torch.empty((192, 256, 300, 256), device=dev).permute(0, 2, 1, 3)
    wf = [torch.empty(int(_ops._lib.load().fnssl_lstm_packed_floats(256, 0, 128)), device=dev)] * 2
    wn = [torch.empty(int(_ops._lib.load().fnssl_lstm_packed_floats(256, 0, 256)), device=dev)]
    assert _ops.lstm_plan("full", big, None, None, wf, 128, big, skip=big, out_sum=big) == ("f32_cluster", 1)
    assert _ops.lstm_plan("narrow", big, None, None, wn, 256, bign, skip=big, out_sum=bign) == ("static4", 1)
    del big, bign
    torch.cuda.empty_cache()
    out = model.predict_step(batch, 0)
    assert tuple(out.shape) == (192, 25, 512) and bool(torch.isfinite(out).all())
    for u in (0, 13, 31):
        alone = model.predict_step(batch[u:u + 1], 0)
        assert torch.equal(alone, out[6 * u:6 * u + 6]), "utterance %d differs when run alone" % u
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    want = R.predict_step(R.build(sd, True), batch[13:14].cpu(), "MM")
    assert_close(out[78:84].cpu().numpy(), want.numpy(), RTOL, ATOL, "config-2 utterance vs CPU reference")
    from fnssl import ops
    ops.release_workspaces()
    torch.cuda.empty_cache()


def test_streamed_row_cluster_kernel_vs_cpu_reference(dev):
    """The H = 256 STREAMED-ROW form of lstm_f32c_kernel (16 waves per member, h_{t-1} through the operand ring: what the
    narrow-band layers run between 9 groups per cluster and the full-chip launch) against the CPU restatement of the
    reference — 6 utterances x 4 mics ('MM': 36 pairs = 36 groups per cluster of 16 CUs) x 36 frames from the waveform.
    The small goldens stop at 8 groups per cluster (the held-row form), so this is the streamed form's oracle contact."""
    import predict_step as ps
    from fnssl import ops, weights as W
    from oracle import torch_ref as R
    sd = W.make_fnssl_state(5)
    model = ps.MyModel(ch_mode="MM", device=str(dev))
    model.arch.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(dev).eval()
    nb, nch, nt = 6, 4, 36
    npair = nb * nch * (nch - 1) // 2
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    groups_per_cluster = -(-(npair * 256 // 16) // (ncu // 16))
    assert 8 < groups_per_cluster and npair * 16 < 12 * ncu, "not the streamed-row regime on this device (%d CUs)" % ncu
    a = torch.empty((npair, nt, 256, 256), device=dev)
    an = torch.empty((npair, 256, nt, 256), device=dev).permute(0, 2, 1, 3)
    x4 = torch.empty((npair, nt, 256, 4), device=dev)
    lib = ops._lib.load()
    w_plain = [torch.empty(int(lib.fnssl_lstm_packed_floats(256, 0, 256)), device=dev)]
    w_cat = [torch.empty(int(lib.fnssl_lstm_packed_floats(256, 4, 256)), device=dev)]
    assert ops.lstm_plan("narrow", a, None, None, w_plain, 256, an, skip=a, out_sum=an)[0] == "f32_cluster"      # blocks 2-3
    assert ops.lstm_plan("narrow", a, None, x4, w_cat, 256, an, skip=a, out_sum=an)[0] == "f32_cluster"          # block 1 (cat)
    del a, an, x4
    batch = torch.randn((nb, nch, 512 + (nt - 1) * 256), generator=torch.Generator(device="cpu").manual_seed(909)) * 0.1
    ops.cluster_fallbacks(dev, reset=True)
    got = model.predict_step(batch.to(dev), 0)
    torch.cuda.synchronize(dev)
    assert ops.cluster_fallbacks(dev) == 0, "a cluster kernel gave up: the comparison would be of the fallback kernels"
    want = R.predict_step(R.build(sd, True), batch, "MM")
    assert tuple(got.shape) == tuple(want.shape) == (npair, nt // 12, 512)
    assert_close(got.cpu().numpy(), want.numpy(), RTOL, ATOL, "streamed-row cluster kernel vs CPU reference")


def test_streaming_carry_survives_a_cluster_member_that_never_shows_up(dev, monkeypatch):
    """FN_SSL.forward_stream's narrow-band layers (H = 256, carry_state) run the cluster-resident kernel, which advances the
    carried cell state in place.  With a member missing in the SECOND chunk (FNSSL_CLUSTER_TEST_STALL) the guarded fallback
    must restart from c_{-1} as it was before the aborted launch (snapshot + restore_cell_kernel): outputs of that chunk and
    of the one after it (which depends on the carried state) bit-equal to the undisturbed run."""
    import Model
    from fnssl import ops, weights as W
    sd = W.make_fnssl_state(2)
    net = Model.FN_SSL(is_online=True)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(dev).eval()
    x = (torch.randn((3, 4, 256, 36), generator=torch.Generator(device="cpu").manual_seed(31)) * 0.5).to(dev)
    for k in ("FNSSL_CLUSTER_TEST_STALL", "FNSSL_CLUSTER_SPIN_LIMIT", "FNSSL_NO_F32_CLUSTER", "FNSSL_NO_F32_SMALL"):
        monkeypatch.delenv(k, raising=False)
    ops._lib.refresh_tuning()

    def run(stall_chunk):
        st, outs = None, []
        for i, t0 in enumerate(range(0, 36, 12)):
            if i == stall_chunk:
                monkeypatch.setenv("FNSSL_CLUSTER_TEST_STALL", "3")
                monkeypatch.setenv("FNSSL_CLUSTER_SPIN_LIMIT", "20000")
            ops._lib.refresh_tuning()
            y, st = net.forward_stream(x[..., t0:t0 + 12], st)
            torch.cuda.synchronize(dev)
            monkeypatch.delenv("FNSSL_CLUSTER_TEST_STALL", raising=False)
            monkeypatch.delenv("FNSSL_CLUSTER_SPIN_LIMIT", raising=False)
            ops._lib.refresh_tuning()
            outs.append(y)
        return torch.cat(outs, dim=1)

    ops.cluster_fallbacks(dev, reset=True)
    want = run(-1)
    assert ops.cluster_fallbacks(dev) == 0
    whole = net(x)
    assert torch.equal(want, whole), "streaming differs from the whole-signal forward"
    got = run(1)
    assert ops.cluster_fallbacks(dev) > 0, "no cluster kernel gave up: the fault injection did not reach the streaming layers"
    assert torch.equal(got, want), "a cluster kernel that gave up in a streaming call corrupted the carried state"
    ops.cluster_fallbacks(dev, reset=True)


# --------------------------------------------------------------------------- wide bf16 kernels (32 sequences per wave)
@pytest.mark.parametrize("mode,H,bidir,c0,c2,nb,nt,nf,x0_bf", [
    ("narrow", 256, False, 256, 16, 1, 9, 40, True),     # ragged: 40 sequences = one full + one partial 32-group
    ("narrow", 256, False, 256, 16, 3, 5, 64, True),     # 192 sequences: several workgroups
    ("full", 128, True, 256, 16, 1, 20, 7, True),        # block-2 full-band, both directions, 20 sequences
    ("full", 128, True, 16, 0, 2, 33, 6, False),         # block-1 full-band: 16 fp32 feature channels, 66 sequences
])
def test_lstm_bf16_wide_matches_oracle_and_narrow_kernel(dev, mode, H, bidir, c0, c2, nb, nt, nf, x0_bf):
    """lstm_bf16w.h (v_mfma_f32_32x32x16_bf16, LDS-DMA tile ring, bf16 activations, bias as three bf16 terms) against
    the bf16-emulating oracle, and against the 16-sequence bf16 kernel on the same bf16-representable input."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    I = c0 + c2
    sd = lstm_state(I, H, bidir, 5100 + H + I)
    x = O.bf16_round(rs_randn(5101, (nb, nt, nf, I), 0.7))            # bf16-representable: both kernels see the same x
    seq = x.reshape(nb * nt, nf, I) if mode == "full" else np.transpose(x, (0, 2, 1, 3)).reshape(nb * nf, nt, I)
    want = O.lstm(seq, sd, "L.", bidir, bf16=True)
    ndir = 2 if bidir else 1
    want = want.reshape(nb, nt, nf, -1) if mode == "full" else np.transpose(want.reshape(nb, nf, nt, -1), (0, 2, 1, 3))
    sfx = [""] + (["_reverse"] if bidir else [])
    args = lambda s: (sd["L.weight_ih_l0" + s], sd["L.weight_hh_l0" + s], sd["L.bias_ih_l0" + s], sd["L.bias_hh_l0" + s])  # noqa: E731
    ww = [ops.pack_lstm_bf16w(*args(s), c0, c2, dev) for s in sfx]
    wn = [ops.pack_lstm_bf16(*args(s), c0, c2, dev) for s in sfx]
    xd = to_dev(x, dev)
    x0 = xd[..., :c0].contiguous()
    x2 = xd[..., c0:].contiguous() if c2 else None
    out_w = torch.full((nb, nt, nf, ndir * H), float("nan"), device=dev, dtype=torch.bfloat16)
    ops.lstm_layer(mode, x0.bfloat16() if x0_bf else x0, None, x2, ww, H, out_w, bf16=True, wide=True)
    out_n = torch.full((nb, nt, nf, ndir * H), float("nan"), device=dev)
    ops.lstm_layer(mode, x0, None, x2, wn, H, out_n, bf16=True)
    got = out_w.float().cpu().numpy()
    assert np.isfinite(got).all()
    # the wide kernel's output is itself rounded to bf16 (2^-9 relative, |h| <= 1)
    assert np.abs(got - want).max() <= BF_ATOL + 2e-3, "vs bf16 oracle: %g" % np.abs(got - want).max()
    assert np.abs(got - out_n.cpu().numpy()).max() <= BF_ATOL + 2e-3
    # typical agreement is at rounding level, not at the worst-case bound
    assert np.abs(got - O.bf16_round(want)).mean() < 2e-4


def test_lstm_cluster_status_reads_only_an_existing_lstm_workspace(dev):
    """The status read allocates nothing: on a stream no LSTM call has run on there is no status word to read."""
    from fnssl import ops
    with torch.cuda.device(dev), torch.cuda.stream(torch.cuda.Stream(dev)):
        ops._ws_cache.pop(ops._ws_key(dev, "lstm"), None)   # (torch pools its streams: an earlier test may have used this one)
        with pytest.raises(RuntimeError, match="no LSTM call has run"):
            ops.lstm_cluster_status(512, 256, 1, dev)


@pytest.mark.parametrize("nb,nt,nf", [
    (2, 7, 256),      # 512 sequences: exactly one cluster
    (3, 5, 200),      # 600 sequences: a second cluster with 88 live sequences (ragged tile, idle waves)
    (9, 4, 257),      # 2313 sequences: five clusters, q_inner not a multiple of 32
    (65, 3, 256),     # 16640 sequences: 33 clusters = two launches (32 clusters fill the 256 CUs)
])
def test_lstm_bf16_cluster_kernel_matches_oracle_and_pair_split(dev, monkeypatch, nb, nt, nf):
    """lstm_bf16c.h (weights resident in the LDS of an 8-CU cluster, h_t exchanged through L2 with tagged hand-offs)
    against the bf16-emulating oracle, and bit-for-bit against the pair-split kernels (FNSSL_NO_CLUSTER=1) it replaces
    for IPDnet's narrow-band shape; twice, to catch a hand-off race."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    H, c0, c2 = 256, 256, 16
    sd = lstm_state(c0 + c2, H, False, 5400 + nb)
    x = O.bf16_round(rs_randn(5401 + nf, (nb, nt, nf, c0 + c2), 0.7))
    seq = np.transpose(x, (0, 2, 1, 3)).reshape(nb * nf, nt, c0 + c2)
    want = np.transpose(O.lstm(seq, sd, "L.", False, bf16=True).reshape(nb, nf, nt, -1), (0, 2, 1, 3))
    w = [ops.pack_lstm_bf16w(sd["L.weight_ih_l0"], sd["L.weight_hh_l0"], sd["L.bias_ih_l0"], sd["L.bias_hh_l0"], c0, c2, dev)]
    xd = to_dev(x, dev)
    x0, x2 = xd[..., :c0].contiguous().bfloat16(), xd[..., c0:].contiguous()

    def run():
        out = torch.full((nb, nt, nf, H), float("nan"), device=dev, dtype=torch.bfloat16)
        ops.lstm_layer("narrow", x0, None, x2, w, H, out, bf16=True, wide=True)
        return out

    def plan():
        return ops.lstm_plan("narrow", x0, None, x2, w, H, torch.empty((nb, nt, nf, H), device=dev, dtype=torch.bfloat16), bf16=True, wide=True)

    monkeypatch.delenv("FNSSL_NO_CLUSTER", raising=False)
    monkeypatch.delenv("FNSSL_CLUSTER_SPREAD", raising=False)
    assert plan()[0] == "bf16_cluster", "the comparison below would be pair-split against pair-split: %r" % (plan(),)
    a, a2 = run(), run()
    monkeypatch.setenv("FNSSL_CLUSTER_SPREAD", "1")        # members of a cluster on different XCDs: placement must not matter
    s1, s2 = run(), run()
    monkeypatch.delenv("FNSSL_CLUSTER_SPREAD")
    assert torch.equal(a, s1) and torch.equal(a, s2), "the hand-off depends on which XCD a member runs on"
    with torch.cuda.device(dev):
        ws = ops._ws_cache[ops._ws_key(dev, "lstm")]
        assert ops.lstm_cluster_status(nb * nf, H, 1, dev) == 0        # no bounded wait ran out
        assert ops._ws_cache[ops._ws_key(dev, "lstm")].data_ptr() == ws.data_ptr()   # read from the buffer the kernel wrote
    monkeypatch.setenv("FNSSL_NO_CLUSTER", "1")
    assert plan()[0] == "bf16_pair"
    b = run()
    got = a.float().cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= BF_ATOL + 2e-3, "vs bf16 oracle: %g" % np.abs(got - want).max()
    assert torch.equal(a, b), "cluster kernel differs from the pair-split kernels"
    assert torch.equal(a, a2), "cluster kernel is not repeatable"


@pytest.mark.parametrize("c0,c2,nb,nt,nf", [
    (256, 16, 64, 300, 24),      # config 3's full-band batch (blocks 2-3): 1200 tiles -> 30 clusters x 20 tiles per direction (3 + 2 parts per SIMD)
    (16, 0, 64, 300, 24),        # block 1's layer (the fp32 feature block only: the recurrent operands are the whole window)
    (256, 16, 37, 300, 9),       # 11100 sequences = 347 tiles (the last one 28 sequences) -> 18 clusters x 20 per direction; the last
                                 # cluster holds 7 tiles: waves 0-6 one live part + a phantom, wave 7 leaves after the weight load
    (256, 16, 30, 300, 7),       # 9000 sequences = 282 tiles -> 15 clusters x 19 per direction (waves 0-2 three parts, 3-7 two)
])
def test_lstm_bf16_full_band_cluster_split_equals_full_clusters_and_pair_split(dev, monkeypatch, c0, c2, nb, nt, nf):
    """Round 6: the bf16 cluster kernel's tiles per cluster are a launch parameter and forward_bf16c cuts the H = 128 full-band
    layers into MORE clusters of 17 - 20 tiles (waves with three and with two parts, waves with none leave) instead of full
    clusters of 24.  Bit-for-bit against the full clusters (FNSSL_CLUSTER_FULL_TILES=1) and against the pair-split kernels
    (FNSSL_NO_CLUSTER_H128=1, what both replace), twice, no bounded wait ran out; a few sequences against the bf16 oracle."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    H, ndir = 128, 2
    sd = lstm_state(c0 + c2, H, True, 7100 + c0)
    sfx = ["", "_reverse"]
    w = [ops.pack_lstm_bf16w(sd["L.weight_ih_l0" + s_], sd["L.weight_hh_l0" + s_], sd["L.bias_ih_l0" + s_], sd["L.bias_hh_l0" + s_],
                             c0, c2, dev) for s_ in sfx]
    g = torch.Generator(device="cpu").manual_seed(7101 + nb)
    x = (torch.randn((nb, nt, nf, c0 + c2), generator=g) * 0.7).bfloat16().float()          # bf16-representable
    xd = x.to(dev)
    x0 = xd[..., :c0].contiguous()
    x0 = x0.bfloat16() if c2 else x0                                                       # block 1: the fp32 feature channels
    x2 = xd[..., c0:].contiguous() if c2 else None

    def run():
        out = torch.full((nb, nt, nf, ndir * H), float("nan"), device=dev, dtype=torch.bfloat16)
        ops.lstm_layer("full", x0, None, x2, w, H, out, bf16=True, wide=True)
        return out

    def plan():
        return ops.lstm_plan("full", x0, None, x2, w, H, torch.empty((nb, nt, nf, ndir * H), device=dev, dtype=torch.bfloat16),
                             bf16=True, wide=True)[0]

    for k in ("FNSSL_NO_CLUSTER", "FNSSL_NO_CLUSTER_H128", "FNSSL_NO_CLUSTER_B1", "FNSSL_CLUSTER_FULL_TILES", "FNSSL_CLUSTER_SPREAD"):
        monkeypatch.delenv(k, raising=False)
    assert plan() == "bf16_cluster", plan()
    a, a2 = run(), run()
    with torch.cuda.device(dev):
        assert ops.lstm_cluster_status(nb * nt, H, ndir, dev) == 0
    assert not torch.isnan(a.float()).any()
    assert torch.equal(a, a2), "not repeatable"
    monkeypatch.setenv("FNSSL_CLUSTER_FULL_TILES", "1")
    assert plan() == "bf16_cluster"
    b = run()
    assert torch.equal(a, b), "clusters of 17 - 20 tiles differ from full clusters"
    monkeypatch.delenv("FNSSL_CLUSTER_FULL_TILES")
    monkeypatch.setenv("FNSSL_NO_CLUSTER_H128", "1")
    monkeypatch.setenv("FNSSL_NO_CLUSTER_B1", "1")
    assert plan() == "bf16_pair", plan()
    c = run()
    assert torch.equal(a, c), "cluster kernel differs from the pair-split kernels"
    rows = [(0, 0), (nb // 2, nt // 2), (nb - 1, nt - 1)]
    seq = np.stack([x[b_, t_].numpy() for b_, t_ in rows])
    want = O.lstm(seq, sd, "L.", True, bf16=True)
    got = np.stack([a[b_, t_].float().cpu().numpy() for b_, t_ in rows])
    assert np.abs(got - want).max() <= BF_ATOL + 2e-3, np.abs(got - want).max()


@pytest.mark.parametrize("mode,H,bidir,c0,c2,nb,nt,nf", [
    ("narrow", 256, False, 256, 16, 64, 60, 256),  # config 3's narrow-band batch: 16384 sequences x 60 steps
    ("full", 128, True, 256, 16, 64, 300, 48),     # config 3's full-band batch (blocks 2, 3): 19200 sequences x 2 directions x 48 steps
    ("full", 128, True, 16, 0, 64, 300, 48),       # block 1 (the 144-column stream: several workgroups per CU, drained barriers)
])
def test_pair_split_kernels_are_bit_stable_over_many_launches(dev, monkeypatch, mode, H, bidir, c0, c2, nb, nt, nf):
    """Round-3 finding (lstm_bf16p.h, launch_bf16p_k): with counted waits at the ring barriers one shape read a stale weight
    record a few times per launch whenever several workgroups shared a CU; it runs drained barriers since.  The soak the
    advisor asked for, on EVERY pair-split shape at config 3's batch: 100 launches (5 - 6 k steps) bit-identical to the first, and identical
    to the same kernels with drained barriers everywhere (FNSSL_BF16P_DRAIN=1) — a ring-accounting race would show as a
    difference between the two or between launches."""
    from fnssl import ops
    sd = lstm_state(c0 + c2, H, bidir, 6100 + H + c0)
    sfx = [""] + (["_reverse"] if bidir else [])
    w = [ops.pack_lstm_bf16w(sd["L.weight_ih_l0" + s_], sd["L.weight_hh_l0" + s_], sd["L.bias_ih_l0" + s_], sd["L.bias_hh_l0" + s_], c0, c2, dev)
         for s_ in sfx]
    g = torch.Generator(device=dev)
    g.manual_seed(6101)
    x0 = torch.randn((nb, nt, nf, c0), generator=g, device=dev) * 0.7
    x2 = torch.randn((nb, nt, nf, c2), generator=g, device=dev) * 0.7 if c2 else None
    x0 = x0.bfloat16() if c2 else x0                     # (block 1: the fp32 feature block is the only input)
    ndir = len(sfx)
    monkeypatch.setenv("FNSSL_NO_CLUSTER", "1")          # the pair-split kernels themselves, not as a fallback
    monkeypatch.setenv("FNSSL_NO_CLUSTER_H128", "1")
    monkeypatch.delenv("FNSSL_BF16P_DRAIN", raising=False)

    def run():
        out = torch.full((nb, nt, nf, ndir * H), float("nan"), device=dev, dtype=torch.bfloat16)
        ops.lstm_layer(mode, x0, None, x2, w, H, out, bf16=True, wide=True)
        return out

    fam = ops.lstm_plan(mode, x0, None, x2, w, H, torch.empty((nb, nt, nf, ndir * H), device=dev, dtype=torch.bfloat16), bf16=True, wide=True)[0]
    assert fam == "bf16_pair", fam
    first = run()
    assert not torch.isnan(first.float()).any()
    bad = 0
    for _ in range(100):
        bad += int(not torch.equal(run(), first))
    assert bad == 0, "%d of 100 launches differ from the first" % bad
    monkeypatch.setenv("FNSSL_BF16P_DRAIN", "1")
    assert torch.equal(run(), first), "drained barriers give different bits"


@pytest.mark.parametrize("nb,nt,nf,summed,c0", [
    (96, 256, 5, True, 256),     # 24576 sequences x 2 directions = 3072 groups: exactly one 12-wave round, 96 groups per cluster
    (97, 300, 4, True, 256),     # 29100 sequences: ragged last group (12 live sequences), groups that cross an utterance boundary
    (96, 256, 3, False, 256),    # without the fused residual output
    (97, 300, 4, False, 4),      # block 1's layer: 4 input channels (one remainder quad)
])
def test_lstm_f32_cluster_kernel_equals_rounds_and_oracle(dev, monkeypatch, nb, nt, nf, summed, c0):
    """lstm_f32c.h (H = 128 full-band layers at full-chip size: hidden slices over clusters of 8 CUs, 16-sequence groups as
    work items, h_t handed over through the output tensor) bit-for-bit against the per-wave rounds of lstm_static_kernel
    (FNSSL_NO_F32_CLUSTER=1), twice, and a few sequences against the oracle."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    H = 128
    sd = lstm_state(c0, H, True, 5600 + nb)
    w = [ops.pack_lstm(sd["L.weight_ih_l0" + s_], sd["L.weight_hh_l0" + s_], sd["L.bias_ih_l0" + s_], sd["L.bias_hh_l0" + s_], c0, 0, dev)
         for s_ in ("", "_reverse")]
    g = torch.Generator(device="cpu").manual_seed(5601 + nf)
    x = (torch.randn((nb, nt, nf, c0), generator=g) * 0.5).to(dev)
    skip = (torch.randn((nb, nt, nf, 2 * H), generator=g) * 0.5).to(dev) if summed else None

    def run():
        out = torch.full((nb, nt, nf, 2 * H), float("nan"), device=dev)
        osum = torch.full_like(out, float("nan")) if summed else None
        ops.lstm_layer("full", x, None, None, w, H, out, skip=skip, out_sum=osum)
        return out, osum

    def plan():
        o = torch.empty((nb, nt, nf, 2 * H), device=dev)
        return ops.lstm_plan("full", x, None, None, w, H, o, skip=skip, out_sum=torch.empty_like(o) if summed else None)

    monkeypatch.delenv("FNSSL_NO_F32_CLUSTER", raising=False)
    monkeypatch.delenv("FNSSL_NO_F32C_B1", raising=False)
    assert plan() == ("f32_cluster", 1), "the comparison below would be rounds against rounds: %r" % (plan(),)
    a, asum = run()
    a2, _ = run()
    monkeypatch.setenv("FNSSL_NO_F32_CLUSTER", "1")
    fam, rounds = plan()
    assert fam in ("static", "generic") and rounds >= 1, (fam, rounds)
    b, bsum = run()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, a2), "cluster kernel differs from the rounds / is not repeatable"
    if summed:
        assert torch.equal(asum, bsum)
        assert torch.equal(asum, a + skip)
    with torch.cuda.device(dev):
        assert ops.lstm_cluster_status(nb * nt, H, 2, dev) == 0
    rows = [(0, 0), (nb // 2, nt - 1), (nb - 1, nt - 1)]                       # first / boundary-crossing / ragged group
    seq = np.stack([x[b_, t_].cpu().numpy() for b_, t_ in rows])             # [3, nf, c0]
    want = O.lstm(seq, sd, "L.", True)
    got = np.stack([a[b_, t_].cpu().numpy() for b_, t_ in rows])
    assert_close(got, want, RTOL, ATOL, "fp32 cluster kernel vs oracle")


@pytest.mark.parametrize("mode,H,nb,nt,nf,c2,summed", [
    ("narrow", 256, 6, 20, 256, 0, True),      # one 4-mic utterance: 96 groups = 6 per cluster of 16 CUs (blocks 2-3, fused residual)
    ("narrow", 256, 6, 20, 256, 4, True),      # block 1: [256 | 4] = the concatenated data channels as a remainder quad of src2
    ("narrow", 256, 1, 37, 256, 4, False),     # one 2-mic utterance: ONE group per cluster, last block's shape (no residual)
    ("narrow", 256, 3, 13, 250, 0, False),     # ragged: 750 sequences = 46 groups + 14 sequences, groups cross pairs
    ("narrow", 256, 11, 9, 250, 4, True),      # 172 groups = 11 per cluster (ragged): h_{t-1} streamed through the operand ring, 16 waves
    ("narrow", 256, 40, 5, 256, 0, False),     # 40 per cluster = 2 per wave + 8 leftover groups that change hands every step (streamed-row form)
    ("narrow", 256, 288, 3, 256, 0, True),     # ABOVE the full-chip launch, 18 groups per CU (48 utterances): 1.5 rounds of 12 waves per CU
                                               # would idle a quarter of the second round — the cluster kernel takes it
    ("full", 128, 1, 249, 256, 0, True),       # one 2-mic utterance, full-band: 16 groups per direction = one per cluster
    ("full", 128, 6, 40, 256, 0, False),       # 240 sequences: 15 groups per direction, fewer than clusters
])
def test_few_sequence_launches_take_the_slice_resident_cluster_kernel_and_equal_the_split_kernels(dev, monkeypatch, mode, H, nb, nt, nf, c2, summed):
    """Round 5: the reference's real predict shapes (one recording, Learner.py:219-272) are a handful of 16-sequence groups.
    They now run on the cluster-resident kernel (lstm_f32c.h, generalised to H = 256 / clusters of 16 and to the
    concatenated 4-channel segment) instead of the several-waves-per-group kernels that stream the whole weight matrix
    from L2 per group and step: bit-identical h (and fused residual output), twice, status word 0, no fallback; a few
    sequences against the oracle."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    bidir = mode == "full"
    ndir = 2 if bidir else 1
    c0 = 256
    sd = lstm_state(c0 + c2, H, bidir, 5900 + nb + c2)
    sfx = ("", "_reverse") if bidir else ("",)
    w = [ops.pack_lstm(sd["L.weight_ih_l0" + s_], sd["L.weight_hh_l0" + s_], sd["L.bias_ih_l0" + s_], sd["L.bias_hh_l0" + s_], c0, c2, dev)
         for s_ in sfx]
    g = torch.Generator(device="cpu").manual_seed(5901 + nf + nt)
    x0 = (torch.randn((nb, nt, nf, c0), generator=g) * 0.5).to(dev)
    x2 = (torch.randn((nb, nt, nf, c2), generator=g) * 0.5).to(dev) if c2 else None
    skip = (torch.randn((nb, nt, nf, ndir * H), generator=g) * 0.5).to(dev) if summed else None

    def buf():
        if mode == "full":
            return torch.full((nb, nt, nf, ndir * H), float("nan"), device=dev)
        return torch.full((nb, nf, nt, ndir * H), float("nan"), device=dev).permute(0, 2, 1, 3)      # narrow-band storage

    def run(plan=False):
        out = buf()
        osum = buf() if summed else None
        r = ops.lstm_layer(mode, x0, None, x2, w, H, out, skip=skip, out_sum=osum, plan_only=plan)
        return r if plan else (out, osum)

    for k in ("FNSSL_NO_F32_SMALL", "FNSSL_NO_F32_CLUSTER", "FNSSL_F32C_GATE_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    ops.cluster_fallbacks(dev, reset=True)
    assert run(plan=True) == ("f32_cluster", 1), run(plan=True)
    a, asum = run()
    a2, _ = run()
    with torch.cuda.device(dev):
        assert ops.lstm_cluster_status(nb * (nt if mode == "full" else nf), H, ndir, dev) == 0
    # both work distributions of the cluster kernel: every wave owns a group / the four waves of a slot share one (one gate
    # each, activated gates exchanged through LDS) — the default picks by groups per cluster
    for gs in ("1", "4"):
        monkeypatch.setenv("FNSSL_F32C_GATE_SPLIT", gs)
        assert run(plan=True) == ("f32_cluster", 1)
        g_out, g_sum = run()
        assert torch.equal(g_out, a), "gate split %s differs from the default" % gs
        if summed:
            assert torch.equal(g_sum, asum)
        with torch.cuda.device(dev):
            assert ops.lstm_cluster_status(nb * (nt if mode == "full" else nf), H, ndir, dev) == 0
    monkeypatch.delenv("FNSSL_F32C_GATE_SPLIT")
    assert ops.cluster_fallbacks(dev) == 0
    monkeypatch.setenv("FNSSL_NO_F32_SMALL", "1")
    fam, _ = run(plan=True)
    assert fam in ("split", "split_static", "static", "static3", "static4", "generic"), fam
    b, bsum = run()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, a2), "cluster kernel differs from the split kernels / is not repeatable"
    if summed:
        assert torch.equal(asum, bsum) and torch.equal(asum, a + skip)
    xin = torch.cat((x0, x2), dim=-1) if c2 else x0
    if mode == "full":
        rows = [(0, 0), (nb - 1, nt - 1)]
        seq = np.stack([xin[b_, t_].cpu().numpy() for b_, t_ in rows])
        got = np.stack([a[b_, t_].cpu().numpy() for b_, t_ in rows])
    else:
        rows = [(0, 0), (nb - 1, nf - 1), (nb // 2, 17)]
        seq = np.stack([xin[b_, :, f_].cpu().numpy() for b_, f_ in rows])
        got = np.stack([a[b_, :, f_].cpu().numpy() for b_, f_ in rows])
    assert_close(got, O.lstm(seq, sd, "L.", bidir), RTOL, ATOL, "few-sequence cluster kernel vs oracle")


@pytest.mark.parametrize("kind", ["f32", "bf16", "f32_h256", "f32_gate_split", "f32_h256_gate_split", "f32_h256_streamed_row"])
def test_cluster_kernel_gives_up_cleanly_and_the_same_call_recomputes_the_layer(dev, monkeypatch, kind):
    """A member workgroup that never shows up (FNSSL_CLUSTER_TEST_STALL: what a CU-masked, shared or busy device does to
    a kernel that needs all its members resident) must cost time, not the process and not the result: the waiting waves
    give up after the spin limit, record a code, every workgroup drains, and the guarded per-wave / pair-split launch of
    the SAME fnssl_lstm_forward call recomputes the layer — output equal to the fallback kernels', the caller's counter
    incremented, no exception, the device still usable."""
    from fnssl import ops
    if kind == "f32":
        H, c0, nb, nt, nf, ndir = 128, 256, 96, 256, 3, 2
        sd = lstm_state(c0, H, True, 5700)
        w = [ops.pack_lstm(sd["L.weight_ih_l0" + s_], sd["L.weight_hh_l0" + s_], sd["L.bias_ih_l0" + s_], sd["L.bias_hh_l0" + s_], c0, 0, dev)
             for s_ in ("", "_reverse")]
        x = (torch.randn((nb, nt, nf, c0), generator=torch.Generator(device="cpu").manual_seed(5701)) * 0.5).to(dev)
        skip = (torch.randn((nb, nt, nf, 2 * H), generator=torch.Generator(device="cpu").manual_seed(5702)) * 0.5).to(dev)
        off_env, fam, nseq = "FNSSL_NO_F32_CLUSTER", "f32_cluster", nb * nt

        def run(counter=None, plan=False):
            out = torch.full((nb, nt, nf, 2 * H), float("nan"), device=dev)
            osum = torch.full_like(out, float("nan"))
            r = ops.lstm_layer("full", x, None, None, w, H, out, skip=skip, out_sum=osum, fallback_count=counter, plan_only=plan)
            return r if plan else torch.cat([out, osum], -1)
    elif kind.startswith("f32_"):
        # round 5's forms of the fp32 cluster kernel: H = 256 (clusters of 16, the concatenated data channels), and the gate
        # split of a one-group-per-cluster launch (four waves per group: a sibling that gave up must not leave the other
        # three spinning on the slot's LDS counter)
        if kind == "f32_gate_split":
            mode_, H, c0, c2, nb, nt, nf, ndir = "full", 128, 256, 0, 1, 249, 64, 2      # 16 groups per direction = 1 per cluster
        elif kind == "f32_h256_gate_split":
            mode_, H, c0, c2, nb, nt, nf, ndir = "narrow", 256, 256, 4, 1, 40, 256, 1     # 16 groups = 1 per cluster of 16
        elif kind == "f32_h256_streamed_row":
            mode_, H, c0, c2, nb, nt, nf, ndir = "narrow", 256, 256, 4, 10, 24, 256, 1    # 160 groups = 10 per cluster: 16 waves per
                                                                                            # member, h_{t-1} through the operand ring
        else:
            mode_, H, c0, c2, nb, nt, nf, ndir = "narrow", 256, 256, 4, 6, 40, 256, 1     # 96 groups = 6 per cluster (row held)
        sd = lstm_state(c0 + c2, H, ndir == 2, 5720 + nb)
        w = [ops.pack_lstm(sd["L.weight_ih_l0" + s_], sd["L.weight_hh_l0" + s_], sd["L.bias_ih_l0" + s_], sd["L.bias_hh_l0" + s_], c0, c2, dev)
             for s_ in (("", "_reverse") if ndir == 2 else ("",))]
        gcpu = torch.Generator(device="cpu").manual_seed(5721)
        x = (torch.randn((nb, nt, nf, c0), generator=gcpu) * 0.5).to(dev)
        x2 = (torch.randn((nb, nt, nf, c2), generator=gcpu) * 0.5).to(dev) if c2 else None
        skip = (torch.randn((nb, nt, nf, ndir * H), generator=gcpu) * 0.5).to(dev)
        off_env, fam, nseq = "FNSSL_NO_F32_SMALL", "f32_cluster", nb * (nt if mode_ == "full" else nf)

        def run(counter=None, plan=False):
            shape = (nb, nt, nf, ndir * H)
            mk = (lambda: torch.full(shape, float("nan"), device=dev)) if mode_ == "full" else \
                (lambda: torch.full((nb, nf, nt, ndir * H), float("nan"), device=dev).permute(0, 2, 1, 3))
            out, osum = mk(), mk()
            r = ops.lstm_layer(mode_, x, None, x2, w, H, out, skip=skip, out_sum=osum, fallback_count=counter, plan_only=plan)
            return r if plan else torch.cat([out, osum], -1)
    else:
        H, c0, c2, nb, nt, nf, ndir = 256, 256, 16, 9, 4, 257, 1
        sd = lstm_state(c0 + c2, H, False, 5710)
        w = [ops.pack_lstm_bf16w(sd["L.weight_ih_l0"], sd["L.weight_hh_l0"], sd["L.bias_ih_l0"], sd["L.bias_hh_l0"], c0, c2, dev)]
        xd = (torch.randn((nb, nt, nf, c0 + c2), generator=torch.Generator(device="cpu").manual_seed(5711)) * 0.7).to(dev)
        x0, x2 = xd[..., :c0].contiguous().bfloat16(), xd[..., c0:].contiguous()
        off_env, fam, nseq = "FNSSL_NO_CLUSTER", "bf16_cluster", nb * nf

        def run(counter=None, plan=False):
            out = torch.full((nb, nt, nf, H), float("nan"), device=dev, dtype=torch.bfloat16)
            r = ops.lstm_layer("narrow", x0, None, x2, w, H, out, bf16=True, wide=True, fallback_count=counter, plan_only=plan)
            return r if plan else out

    for k in (off_env, "FNSSL_CLUSTER_TEST_STALL", "FNSSL_CLUSTER_SPIN_LIMIT", "FNSSL_NO_F32C_B1", "FNSSL_CLUSTER_SPREAD",
              "FNSSL_F32C_GATE_SPLIT", "FNSSL_NO_F32_CLUSTER", "FNSSL_NO_F32_SMALL"):
        monkeypatch.delenv(k, raising=False)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    assert run(plan=True)[0] == fam
    good = run(counter)
    with torch.cuda.device(dev):
        assert ops.lstm_cluster_status(nseq, H, ndir, dev) == 0 and int(counter.item()) == 0
    monkeypatch.setenv(off_env, "1")
    want = run()
    assert torch.equal(good, want)
    monkeypatch.delenv(off_env)
    monkeypatch.setenv("FNSSL_CLUSTER_TEST_STALL", "3")         # member 3 of cluster 0 exits at once
    monkeypatch.setenv("FNSSL_CLUSTER_SPIN_LIMIT", "20000")     # ~30 ms instead of ~1.5 s
    got = run(counter)                                           # must not raise, must not kill the process
    torch.cuda.synchronize(dev)
    with torch.cuda.device(dev):
        st = ops.lstm_cluster_status(nseq, H, ndir, dev)
    assert st != 0 and (st >> 16) in (1, 3, 4), "the stalled cluster did not record a code: %#x" % st
    assert int(counter.item()) == 1, "the guarded fallback did not run exactly once: %d" % int(counter.item())
    assert torch.equal(got, want), "after a failed hand-off the layer was not recomputed by the fallback kernels"
    monkeypatch.delenv("FNSSL_CLUSTER_TEST_STALL")
    monkeypatch.delenv("FNSSL_CLUSTER_SPIN_LIMIT")
    again = run(counter)                                         # and the next call is a normal cluster launch again
    with torch.cuda.device(dev):
        assert ops.lstm_cluster_status(nseq, H, ndir, dev) == 0 and int(counter.item()) == 1
    assert torch.equal(again, want)


@pytest.mark.parametrize("c2,summed", [(0, True), (0, False), (4, True)])
def test_lstm_operand_ring_kernel_equals_one_slice_kernel(dev, monkeypatch, c2, summed):
    """lstm_static3.h (round 4: h_{t-1} streamed through the operand ring like x_t, no register spills) bit-for-bit against the
    one-slice lstm_static_kernel at the full-chip narrow-band size — for the three layer variants of the
    network, with a reversed-direction-free, ragged-free shape and steps 0..6 (step 0 reads h_{-1} = 0 through a
    zero-record descriptor); a few sequences against the oracle."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    H, c0, nb, nt, nf = 256, 256, 192, 7, 256            # 49152 sequences = 256 CUs x 12 waves x 16: config 2's launch geometry
    sd = lstm_state(c0 + c2, H, False, 5800 + c2)
    w = [ops.pack_lstm(sd["L.weight_ih_l0"], sd["L.weight_hh_l0"], sd["L.bias_ih_l0"], sd["L.bias_hh_l0"], c0, c2, dev)]
    g = torch.Generator(device="cpu").manual_seed(5801 + c2)
    x0 = (torch.randn((nb, nt, nf, c0), generator=g) * 0.5).to(dev)
    x2 = (torch.randn((nb, nt, nf, c2), generator=g) * 0.5).to(dev) if c2 else None
    skip = (torch.randn((nb, nt, nf, H), generator=g) * 0.5).to(dev) if summed else None

    def run(plan=False):
        out = torch.full((nb, nf, nt, H), float("nan"), device=dev).permute(0, 2, 1, 3)
        osum = torch.full((nb, nf, nt, H), float("nan"), device=dev).permute(0, 2, 1, 3) if summed else None
        r = ops.lstm_layer("narrow", x0, None, x2, w, H, out, skip=skip, out_sum=osum, plan_only=plan)
        return r if plan else (out, osum)

    for k in ("FNSSL_NO_STATIC3", "FNSSL_NO_STATIC2", "FNSSL_NO_STATIC4"):
        monkeypatch.delenv(k, raising=False)
    assert run(plan=True) == ("static4", 1), run(plan=True)
    a, asum = run()                                      # round 6: four slices per pass, LDS-DMA weight ring (lstm_static4.h)
    a6, a6sum = run()                                    # (and again: repeatable)
    for _ in range(3):                                   # the DMA ring's counted waits: a race would show between launches
        r_, rs_ = run()
        assert torch.equal(r_, a) and (not summed or torch.equal(rs_, asum)), "four-slice kernel is not repeatable"
    monkeypatch.setenv("FNSSL_NO_STATIC4", "1")          # two slices per pass (lstm_static3.h)
    assert run(plan=True) == ("static3", 1)
    p2, p2sum = run()
    assert torch.equal(a, p2) and (not summed or torch.equal(asum, p2sum)), "four slices per pass differ from two"
    monkeypatch.delenv("FNSSL_NO_STATIC4")
    monkeypatch.setenv("FNSSL_NO_STATIC3", "1")
    assert run(plan=True)[0] == "static"
    b, bsum = run()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, a6), "operand-ring kernel differs from the kernels it replaces"
    if summed:
        assert torch.equal(asum, bsum) and torch.equal(asum, a6sum) and torch.equal(asum, a + skip)
    rows = [(0, 0), (77, 131), (nb - 1, nf - 1)]
    xin = torch.cat([x0, x2], -1) if c2 else x0
    seq = np.stack([xin[b_, :, f_].cpu().numpy() for b_, f_ in rows])           # [3, nt, c0 + c2]
    want = O.lstm(seq, sd, "L.", False)
    got = np.stack([a[b_, :, f_].cpu().numpy() for b_, f_ in rows])
    assert_close(got, want, RTOL, ATOL, "operand-ring kernel vs oracle")


@pytest.mark.parametrize("summed", [False, True])
def test_lstm_operand_ring_kernels_ragged_tail(dev, summed):
    """The tail handling of the full-chip narrow-band rounds (one prologue for lstm_static.h, lstm_static3.h and
    lstm_static4.h: clamped sequence index, `valid`, the spare cell slot of an idle wave) at the smallest ragged size that
    still selects them on 256 CUs: 49125 sequences = 3071 groups, so the last workgroup's last wave has no group and the
    last group has 5 sequences.  Three steps; the three families bit for bit, plain and with the fused residual; the last
    sequence against the oracle; the rows behind the last sequence untouched."""
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    if ncu != 256:
        pytest.skip("49125 sequences select the full-chip rounds on 256 CUs, this device has %d" % ncu)
    from fnssl import _lib, ops
    from oracle import fnssl_oracle as O
    H, c0, nt, nf, spare = 256, 256, 3, 49125, 27
    sd = lstm_state(c0, H, False, 5830)
    w = [ops.pack_lstm(sd["L.weight_ih_l0"], sd["L.weight_hh_l0"], sd["L.bias_ih_l0"], sd["L.bias_hh_l0"], c0, 0, dev)]
    g = torch.Generator(device="cpu").manual_seed(5831)
    x0 = (torch.randn((1, nt, nf, c0), generator=g) * 0.5).to(dev)
    skip = (torch.randn((1, nt, nf, H), generator=g) * 0.5).to(dev) if summed else None

    def run(plan=False, **knobs):
        # the row's knobs and no others, whatever the environment says; without the small-shape cluster kernel, which
        # would take 3071 groups
        tuning = _lib.make_tuning(base=_lib.Tuning(), no_f32_small=1, **knobs)
        buf = torch.full((1, nf + spare, nt, H), float("nan"), device=dev)
        bsum = torch.full((1, nf + spare, nt, H), float("nan"), device=dev) if summed else None
        out = buf[:, :nf].permute(0, 2, 1, 3)
        osum = bsum[:, :nf].permute(0, 2, 1, 3) if summed else None
        r = ops.lstm_layer("narrow", x0, None, None, w, H, out, skip=skip, out_sum=osum, plan_only=plan, tuning=tuning)
        return r if plan else (buf, bsum)

    assert run(plan=True) == ("static4", 1), run(plan=True)
    assert run(plan=True, no_static4=1) == ("static3", 1), run(plan=True, no_static4=1)
    assert run(plan=True, no_static3=1)[0] == "static", run(plan=True, no_static3=1)
    a, asum = run()
    b, bsum = run(no_static4=1)
    c, csum = run(no_static3=1)
    assert torch.isfinite(a[:, :nf]).all()
    for name, o, osum in (("static4", a, asum), ("static3", b, bsum), ("static", c, csum)):
        assert torch.isnan(o[:, nf:]).all(), "%s wrote behind the last sequence" % name
        assert not summed or torch.isnan(osum[:, nf:]).all(), "%s wrote the residual output behind the last sequence" % name
    assert torch.equal(a[:, :nf], b[:, :nf]), "four slices per pass differ from two at the ragged tail"
    assert torch.equal(a[:, :nf], c[:, :nf]), "four slices per pass differ from the one-slice kernel at the ragged tail"
    if summed:
        assert torch.equal(asum[:, :nf], bsum[:, :nf]) and torch.equal(asum[:, :nf], csum[:, :nf])
        assert torch.equal(asum[:, :nf], a[:, :nf] + skip.permute(0, 2, 1, 3))
    want = O.lstm(x0[0, :, nf - 1].cpu().numpy()[None], sd, "L.", False)            # [1, nt, H]
    assert_close(a[0, nf - 1].cpu().numpy()[None], want, RTOL, ATOL, "last valid sequence vs oracle")


def test_lstm_forward_rejects_an_input_that_aliases_an_output(dev):
    """The recurrence re-reads h_{t-1} from `out`, and the guarded fallback kernels behind a cluster kernel that gave up
    recompute the layer from the inputs: an in-place call would corrupt either (round-4 advisor note) — it is an error."""
    from fnssl import ops
    sd = lstm_state(256, 256, False, 5250)
    w = [ops.pack_lstm(sd["L.weight_ih_l0"], sd["L.weight_hh_l0"], sd["L.bias_ih_l0"], sd["L.bias_hh_l0"], 256, 0, dev)]
    x = torch.zeros((1, 4, 16, 256), device=dev)
    with pytest.raises(RuntimeError, match="aliases"):
        ops.lstm_layer("narrow", x, None, None, w, 256, x)
    out = torch.empty_like(x)
    with pytest.raises(RuntimeError, match="aliases"):
        ops.lstm_layer("narrow", x, None, None, w, 256, out, skip=x, out_sum=x)
    ops.lstm_layer("narrow", x, None, None, w, 256, out)              # (and the legitimate call goes through)


def test_lstm_bf16_wide_rejects_unbuilt_shapes(dev):
    from fnssl import ops
    sd = lstm_state(128, 256, False, 5200)
    w = [ops.pack_lstm_bf16w(sd["L.weight_ih_l0"], sd["L.weight_hh_l0"], sd["L.bias_ih_l0"], sd["L.bias_hh_l0"], 128, 0, dev)]
    x = torch.zeros((1, 4, 16, 128), device=dev, dtype=torch.bfloat16)
    out = torch.zeros((1, 4, 16, 256), device=dev, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="wide bf16 path is not built"):
        ops.lstm_layer("narrow", x, None, None, w, 256, out, bf16=True, wide=True)


def test_conv3x3_bf16_input_matches_fp32_input(dev):
    """fnssl_conv3x3_causal_bf16a (segment A arrives as bf16) == the bf16 kernel fed the same values as fp32."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    w = rs_randn(5300, (128, 272, 3, 3), 0.05)
    xa = O.bf16_round(rs_randn(5301, (2, 5, 19, 256)))
    xb = rs_randn(5302, (2, 5, 19, 16))
    packed = ops.pack_conv3x3(w, 256, 16, dev, bf16=True)
    a = ops.conv3x3_causal(to_dev(xa, dev), to_dev(xb, dev), packed, 128, "relu", bf16=True)
    b = ops.conv3x3_causal(to_dev(xa, dev).bfloat16(), to_dev(xb, dev), packed, 128, "relu", bf16=True)
    assert torch.equal(a, b)


# --------------------------------------------------------------------------- LDS-staged bf16 conv (conv_bf16x.hip)
@pytest.mark.parametrize("cout,ca,cb,nb,nf,nt,act", [(128, 256, 16, 1, 4, 21, "relu"),      # IPDnet conv1, one tile
                                                      (128, 128, 0, 2, 3, 100, "relu"),      # conv2: 2 time tiles, ragged
                                                      (128, 256, 16, 2, 5, 130, "none"),     # 3 time tiles, halo across tiles
                                                      (96, 32, 32, 1, 2, 64, "tanh"),        # partial cout tile, 2 skip groups
                                                      (128, 64, 0, 3, 70, 70, "relu")])      # > 256 workgroup tiles? no: passes
def test_conv3x3_bf16x_matches_bf16_oracle(dev, cout, ca, cb, nb, nf, nt, act):
    from fnssl import ops
    from oracle import fnssl_oracle as O
    w = rs_randn(5400 + cout + ca, (cout, ca + cb, 3, 3), 0.1)
    xa = O.bf16_round(rs_randn(5401, (nb, nf, nt, ca)))
    xb = rs_randn(5402, (nb, nf, nt, cb)) if cb else None
    assert ops.conv3x3_bf16x_supported(cout, ca, cb)
    packed = ops.pack_conv3x3_bf16x(w, ca, cb, dev)
    got = ops.conv3x3_causal_bf16x(to_dev(xa, dev).bfloat16(), to_dev(xb, dev) if cb else None, packed, cout, act)
    got = got.cpu().numpy()
    want = _oracle_conv(xa, O.bf16_round(xb) if cb else None, O.bf16_round(w), act)
    scale = max(1.0, np.abs(want).max())
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 2e-5 * scale, np.abs(got - want).max()


def test_conv3x3_bf16x_many_passes_and_strided_views(dev):
    """More workgroup tiles than workgroups (several passes per workgroup, ring and tile buffers wrapping across
    tiles) and inputs that are strided views (the [b, t, f, c] tensors IPDnet hands over, permuted)."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    nb, nf, nt, ca, cb, cout = 5, 257, 67, 32, 16, 128            # 5 * 257 * 2 = 2570 wave tiles -> 643 workgroup tiles
    w = rs_randn(5410, (cout, ca + cb, 3, 3), 0.1)
    xa = O.bf16_round(rs_randn(5411, (nb, nt, nf, ca)))           # stored [b, t, f, c]
    xb = rs_randn(5412, (nb, nt, nf, cb))
    packed = ops.pack_conv3x3_bf16x(w, ca, cb, dev)
    got = ops.conv3x3_causal_bf16x(to_dev(xa, dev).bfloat16().permute(0, 2, 1, 3), to_dev(xb, dev).permute(0, 2, 1, 3),
                                   packed, cout, "relu").cpu().numpy()
    want = _oracle_conv(xa.transpose(0, 2, 1, 3), O.bf16_round(xb).transpose(0, 2, 1, 3), O.bf16_round(w), "relu")
    assert np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), np.abs(got - want).max()
    # and bit-identical to the first bf16 kernel on the same operands? no: different accumulation order; close
    p1 = ops.pack_conv3x3(w, ca, cb, dev, bf16=True)
    ref = ops.conv3x3_causal(to_dev(xa, dev).bfloat16().permute(0, 2, 1, 3), to_dev(xb, dev).permute(0, 2, 1, 3), p1, cout,
                             "relu", bf16=True).cpu().numpy()
    assert np.abs(got - ref).max() <= 2e-5 * max(1.0, np.abs(want).max())
    with pytest.raises(RuntimeError, match="unsupported sizes"):
        ops.pack_conv3x3_bf16x(np.zeros((28, 128, 3, 3), np.float32), 128, 0, dev)
    assert not ops.conv3x3_bf16x_supported(128, 48, 0) and not ops.conv3x3_bf16x_supported(128, 64, 8)


def test_avgpool_time_bf16_is_the_rounded_fp32_pool(dev):
    from fnssl import ops
    x = to_dev(rs_randn(5420, (2, 3, 25, 128)), dev)
    for k in (3, 4):
        assert torch.equal(ops.avgpool_time(x, k, bf16_out=True), ops.avgpool_time(x, k).bfloat16())


@pytest.mark.parametrize("pool,nt", [(3, 300), (3, 64), (3, 5), (4, 100), (4, 67), (3, 2)])
def test_conv3x3_bf16x_fused_pool_equals_conv_then_pool(dev, pool, nt):
    """The pooling fused into the conv epilogue reproduces conv -> avgpool_time bit for bit (fp32 and bf16 output),
    including ragged lengths (frames past the last whole window dropped) and tiles of 63 frames (pool 3)."""
    from fnssl import ops
    from oracle import fnssl_oracle as O
    nb, nf, ca, cb, cout = 2, 5, 64, 16, 128
    w = rs_randn(5500 + pool + nt, (cout, ca + cb, 3, 3), 0.1)
    xa = to_dev(O.bf16_round(rs_randn(5501, (nb, nf, nt, ca))), dev).bfloat16()
    xb = to_dev(rs_randn(5502, (nb, nf, nt, cb)), dev)
    packed = ops.pack_conv3x3_bf16x(w, ca, cb, dev)
    plain = ops.conv3x3_causal_bf16x(xa, xb, packed, cout, "relu")
    for bf in (False, True):
        fused = ops.conv3x3_causal_bf16x(xa, xb, packed, cout, "relu", pool=pool, bf16_out=bf)
        want = ops.avgpool_time(plain, pool, bf16_out=bf)
        assert fused.shape == want.shape == (nb, nf, nt // pool, cout) and fused.dtype == want.dtype
        assert torch.equal(fused, want), (fused.float() - want.float()).abs().max()


def test_conv3x3_bf16x_random_shapes_against_first_bf16_kernel(dev):
    """30 seeded random problems (channel groups, skip segment or not, partial cout tiles, ragged frames / bins, all
    three poolings, strided inputs) through the LDS-staged kernel against the first bf16 kernel + avgpool_time, which
    the tests above pin to the bf16 oracle: same operand rounding, different summation order."""
    from fnssl import ops
    rng = np.random.RandomState(20260928)
    for it in range(30):
        ca = 32 * int(rng.randint(1, 5))
        cb = 16 * int(rng.randint(0, 3))
        cout = int(rng.choice([68, 96, 100, 128]))
        nb, nf, nt = int(rng.randint(1, 4)), int(rng.randint(1, 9)), int(rng.randint(1, 150))
        pool = int(rng.choice([1, 3, 4]))
        act = str(rng.choice(["none", "relu", "tanh"]))
        w = rs_randn(5600 + it, (cout, ca + cb, 3, 3), 0.1)
        xa = to_dev(rs_randn(5700 + it, (nb, nt, nf, ca)), dev).bfloat16().permute(0, 2, 1, 3)   # stored [b, t, f, c]
        xb = to_dev(rs_randn(5800 + it, (nb, nf, nt, cb)), dev) if cb else None
        px = ops.pack_conv3x3_bf16x(w, ca, cb, dev)
        p1 = ops.pack_conv3x3(w, ca, cb, dev, bf16=True)
        got = ops.conv3x3_causal_bf16x(xa, xb, px, cout, act, pool=pool)
        ref = ops.conv3x3_causal(xa, xb, p1, cout, act, bf16=True)[..., :cout]
        if pool > 1:
            ref = ops.avgpool_time(ref.contiguous(), pool) if nt // pool else ref[:, :, :0]
        assert got.shape == ref.shape, (it, got.shape, ref.shape)
        if got.numel():
            err = (got - ref).abs().max().item()
            assert err <= 3e-5 * max(1.0, ref.abs().max().item()), (it, ca, cb, cout, nb, nf, nt, pool, act, err)


def test_timing_select_brackets_one_kernel_name(dev):
    """fnssl_timing_select: with a name selected only launches of that kernel are bracketed (what bench.py does inside
    its timed region); None restores all."""
    from fnssl import ops
    x = to_dev(rs_randn(5900, (2, 3, 24, 128)), dev)
    ops.timing_collect()
    ops.timing_select("avgpool_time")
    ops.timing_enable(True)
    ops.avgpool_time(x, 3)
    ops.nchw_to_seq(to_dev(rs_randn(5901, (1, 4, 8, 6)), dev))
    ops.timing_enable(False)
    got = ops.timing_collect()
    assert set(got) == {"avgpool_time"} and got["avgpool_time"]["count"] == 1
    ops.timing_select(None)
    ops.timing_enable(True)
    ops.avgpool_time(x, 3)
    ops.nchw_to_seq(to_dev(rs_randn(5901, (1, 4, 8, 6)), dev))
    ops.timing_enable(False)
    assert set(ops.timing_collect()) == {"avgpool_time", "nchw_to_seq"}


def test_forward_survives_a_cluster_member_that_never_shows_up(dev, monkeypatch):
    """Product path (DeviceNet.forward -> fnssl_forward): with one member workgroup of the cluster-resident kernels
    missing (FNSSL_CLUSTER_TEST_STALL), the forward neither raises nor dies, returns the SAME output, counts the
    recomputed layers in the device counter handed down through fnssl_net.fallback_count, and reports them — one forward
    later, from the 4-byte asynchronous read-back — as a RuntimeWarning."""
    import warnings
    from fnssl import ops, weights as W
    nb, nt, nf = 96, 256, 256                        # 96 pairs x 256 frames x 2 directions = 3072 groups: the cluster kernel's size
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 60 * 2 ** 30:
        pytest.skip("needs ~45 GB of free HBM, %.0f GB free" % (free / 2 ** 30))
    net = ops.DeviceNet(W.make_fnssl_state(0), dev)
    x0 = (torch.randn((nb, nt, nf, 4), generator=torch.Generator(device="cpu").manual_seed(6000)) * 0.5).to(dev)
    for k in ("FNSSL_CLUSTER_TEST_STALL", "FNSSL_CLUSTER_SPIN_LIMIT", "FNSSL_NO_F32_CLUSTER"):
        monkeypatch.delenv(k, raising=False)
    want = net.forward(x0)
    torch.cuda.synchronize(dev)
    assert int(net.fallbacks.item()) == 0
    monkeypatch.setenv("FNSSL_CLUSTER_TEST_STALL", "5")
    monkeypatch.setenv("FNSSL_CLUSTER_SPIN_LIMIT", "20000")
    got = net.forward(x0)
    torch.cuda.synchronize(dev)
    assert torch.equal(got, want), "the forward's result changed when a cluster member went missing"
    # all six layers take the cluster-resident kernel at this size since round 5 (96 x 256 narrow-band sequences = 1536
    # groups = 6 per CU: clusters of 16), and member 5 of cluster 0 is missing in each of them
    assert int(net.fallbacks.item()) == 6, "six layers should have been recomputed, counted %d" % int(net.fallbacks.item())
    monkeypatch.delenv("FNSSL_CLUSTER_TEST_STALL")
    monkeypatch.delenv("FNSSL_CLUSTER_SPIN_LIMIT")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        again = net.forward(x0)
        torch.cuda.synchronize(dev)
    assert any(issubclass(r.category, RuntimeWarning) and "recomputed" in str(r.message) for r in rec), [str(r.message) for r in rec]
    assert torch.equal(again, want) and int(net.fallbacks.item()) == 6
    ops.release_workspaces()
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------- every exit of the LSTM routers
# One descriptor per exit of the forward router (lstm.hip) and of the backward's (lstm_train.hip), "narrow" layout: nf
# sequences x 2 steps, the fewest sequences that still select the exit on 256 CUs.  Columns: hidden, directions, sequences,
# c0, c2, what else the call carries, tuning knobs -> expected (family, rounds) — a family name alone for a backward call.
# The expected values are what the library answered BEFORE its host dispatch was restructured (same device): literals, so
# that a routing change shows up here as a diff of this table.
_ROUTER_EXITS = [
    # H, ndir, nseq, c0, c2, extras, knobs, expected
    (64, 1, 16, 4, 0, (), {}, ("generic", 1)),
    # H = 128 rounds: [256 | 4] channels are no cluster shape; 513 groups x 2 directions = 5 waves per CU: past the split kernels
    (128, 2, 8193, 256, 4, ("sum",), {}, ("static", 1)),
    # H = 256: exactly one full-chip round of 12 waves per CU (3072 groups; one fewer and the cluster kernel takes it)
    (256, 1, 49137, 256, 0, (), {}, ("static4", 1)),
    (256, 1, 49137, 256, 0, (), {"no_static4": 1}, ("static3", 1)),
    (256, 2, 16, 256, 0, (), {}, ("split_static", 1)),
    (128, 1, 16, 256, 0, ("src1",), {}, ("split", 1)),
    (128, 2, 16, 256, 0, (), {}, ("f32_cluster", 1)),
    (128, 2, 16, 256, 0, ("sum",), {}, ("f32_cluster", 1)),
    (256, 1, 16, 256, 0, ("carry",), {}, ("f32_cluster", 1)),
    (128, 2, 16, 256, 4, ("reserve",), {}, ("train", 1)),
    (128, 1, 32, 16, 0, ("wide",), {}, ("bf16_pair", 1)),
    (256, 1, 32, 256, 16, ("wide",), {}, ("bf16_cluster", 1)),
    (256, 2, 16, 0, 0, ("backward",), {}, "bwd"),
    (128, 2, 16, 0, 0, ("backward",), {}, "bwd_cluster"),
]


def _router_exit(dev, H, ndir, nseq, c0, c2, extras, knobs):
    """What fnssl_lstm_plan / fnssl_lstm_backward_plan answer for one row of _ROUTER_EXITS (nothing is launched, no
    operand is dereferenced: the tensors are never initialised)."""
    from fnssl import _lib, ops
    lib = _lib.load()
    tuning = _lib.make_tuning(base=_lib.Tuning(), **knobs)     # the row's knobs and no others, whatever the environment says
    nt = 2

    def act(c, dtype=torch.float32, rows=nt):
        return torch.empty((1, rows, nseq, c), device=dev, dtype=dtype)

    if "backward" in extras:
        res = torch.empty(ops.lstm_reserve_floats(nseq, H, ndir, nt), device=dev)
        bw = [torch.empty(int(lib.fnssl_lstm_bwd_packed_floats(0, H)), device=dev)] * ndir
        return ops.lstm_backward("narrow", res, act(ndir * H), act(ndir * 4 * H), None, bw, H, 0, plan_only=True, tuning=tuning)
    wide = "wide" in extras
    kw = dict(tuning=tuning)
    if wide:
        w = [torch.empty(int(lib.fnssl_lstm_packed_floats_bf16w(c0, c2, H)), device=dev)] * ndir
        x0, x2 = act(c0, torch.bfloat16 if c2 else torch.float32), act(c2) if c2 else None     # IPDnet: bf16 activations, fp32 features
        out = act(ndir * H, torch.bfloat16)
        kw.update(bf16=True, wide=True)
    else:
        w = [torch.empty(int(lib.fnssl_lstm_packed_floats(c0, c2, H)), device=dev)] * ndir
        x0, x2 = act(c0), act(c2) if c2 else None
        out = act(ndir * H, rows=nt + 1)[:, 1:]                 # (a streaming call reads h_{-1} from the row before `out`)
    if "sum" in extras:
        kw.update(skip=act(ndir * H), out_sum=act(ndir * H, rows=nt + 1)[:, 1:])
    if "reserve" in extras:
        kw.update(reserve=torch.empty(ops.lstm_reserve_floats(nseq, H, ndir, nt), device=dev))
    if "carry" in extras:
        kw.update(carry_workspace=ops.lstm_state_workspace(nseq, H, dev), carry=True)
    return ops.lstm_plan("narrow", x0, act(c0) if "src1" in extras else None, x2, w, H, out, **kw)


def test_every_router_exit_reports_its_family_and_rounds(dev):
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    assert ncu == 256, "the table's sequence counts select these exits on 256 CUs, this device has %d" % ncu
    from fnssl import ops
    got = [_router_exit(dev, *row[:-1]) for row in _ROUTER_EXITS]
    ops.release_workspaces()
    torch.cuda.empty_cache()
    assert got == [row[-1] for row in _ROUTER_EXITS], "\n".join(
        "%s: got %s, expected %s" % (row[:-1], g, row[-1]) for row, g in zip(_ROUTER_EXITS, got) if g != row[-1])
