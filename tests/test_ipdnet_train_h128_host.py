"""Host-side checks of IPDnet training at the reference's default width, hidden_size = 128 (no GPU): which modules are
trainable and which ``IPDnet.forward`` routes by itself, the train graph's layer shapes (full-band BiLSTM H = 64), the
dropout sites' seeds and keep-scale tensors, the H = 64 sizes the LSTM training entry points accept, ``forward_train``'s
refusals, and the G22 golden step of the real reference against the CPU restatement the GPU tests compare with."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from fnssl import _lib, ipdnet_train, train

import ipdnet_train_ref as R

H128_SHAPES = [("block_1.fullLstm", "full", 64, 2, 4, 0, 0), ("block_1.narrLstm", "narrow", 128, 1, 128, 4, 128),
               ("block_2.fullLstm", "full", 64, 2, 128, 4, 128), ("block_2.narrLstm", "narrow", 128, 1, 128, 4, 128)]


def _ipdnet(*args):
    from IPDnet.FixedAarryIPDnet import IPDnet
    return IPDnet(*args)


def test_trainable_and_supported():
    for net in (_ipdnet(), _ipdnet(4, 128, 2, False), _ipdnet(8, 128, 2, True), _ipdnet(16, 256, 2, True)):
        assert ipdnet_train.trainable(net)
        assert not ipdnet_train.trainable(net, offline_inference=True)
    assert not ipdnet_train.supported(_ipdnet())                     # forward does not route the default model
    assert not ipdnet_train.supported(_ipdnet(4, 128, 2, False))
    assert ipdnet_train.supported(_ipdnet(16, 256, 2, True))
    assert not ipdnet_train.trainable(_ipdnet(4, 64, 2, True))       # full-band H = 32: no training kernels
    assert not ipdnet_train.trainable(_ipdnet(4, 128, 1, True))      # cout = 2
    assert not ipdnet_train.trainable(_ipdnet(4, 128, 2, True).bfloat16())


def test_hidden128_graph_layer_shapes():
    g = ipdnet_train.IPDnetTrainGraph(_ipdnet())
    assert [(L.name, L.mode, L.hidden, L.ndir, L.c0, L.c2, L.c0g) for L in g.lstms] == H128_SHAPES
    off = ipdnet_train.IPDnetTrainGraph(_ipdnet(4, 128, 2, False))
    assert [(L.mode, L.hidden, L.ndir, L.c0, L.c2, L.c0g) for L in off.lstms] == [
        ("full", 64, 2, 4, 0, 0), ("narrow", 64, 2, 128, 4, 128), ("full", 64, 2, 128, 4, 128),
        ("narrow", 64, 2, 128, 4, 128)]
    assert g.ch == off.ch == 128 and ipdnet_train.IPDnetTrainGraph(_ipdnet(16, 256, 2, True)).ch == 256
    # every site's activation is hidden_size channels wide in both modes
    for m in (g.model, off.model):
        for blk in (m.block_1, m.block_2):
            assert 2 * blk.fullLstm.hidden_size == 128
            assert blk.narrLstm.hidden_size * (2 if blk.narrLstm.bidirectional else 1) == 128


def test_site_seeds_unchanged_and_keep_scale_keyed_by_global_utterance():
    assert ipdnet_train.site_seeds(77) == [train.layer_seed(77, s) for s in range(4)]
    assert len(set(ipdnet_train.site_seeds(77))) == 4
    from oracle import train_ref
    seed = ipdnet_train.site_seeds(5)[2]
    a = train_ref.dropout_scale(seed, (4, 3, 2, 128))
    b = train_ref.dropout_scale(seed, (2, 3, 2, 128), b0=2)
    np.testing.assert_array_equal(a[2:], b)                               # keyed by the global utterance index
    assert set(np.unique(a)) <= {0.0, 1.25}
    # the hash runs over the logical [nb, nt, nf, 128] activation: element ((u nt + t) nf + f) 128 + c, i.e. the flat
    # stream of the 256-wide tensor with half as many rows
    wide = train_ref.dropout_scale(seed, (4, 3, 1, 256))
    np.testing.assert_array_equal(a.reshape(-1), wide.reshape(-1))
    np.testing.assert_array_equal(R.site_masks(5, 4, 3, 2, 0, c=128)[2].numpy(), a)


def test_h64_sizes_of_the_lstm_training_entry_points():
    lib = _lib.load()
    assert lib.fnssl_abi_version() == 19                                   # no new entry points
    assert lib.fnssl_lstm_reserve_bytes(72, 64, 2, 24) == 5 * 2 * 24 * 4 * 5 * 1024
    # [W_ih[:, :c0g] | W_hh]^T in 64-channel output slices: one (block 1) and three (c0g = 128), 17 quads each
    assert lib.fnssl_lstm_bwd_packed_floats(0, 64) == 1 * 17 * 4 * 256
    assert lib.fnssl_lstm_bwd_packed_floats(128, 64) == 3 * 17 * 4 * 256
    assert lib.fnssl_lstm_bwd_workspace_bytes(72, 64, 2) > 0
    d = _lib.LstmBwdDesc()
    d.hidden, d.ndir, d.nseq, d.nsteps, d.q_inner, d.c0g = 64, 2, 72, 24, 36, 128
    assert lib.fnssl_lstm_backward(C.byref(d), None) != 0
    err = lib.fnssl_last_error()
    assert b"null pointer" in err and b"hidden size" not in err, err       # fails on the pointers, not on H = 64
    d.hidden = 32
    assert lib.fnssl_lstm_backward(C.byref(d), None) != 0
    assert b"hidden size 32 unsupported" in lib.fnssl_last_error()


def test_pack_bwd_h64_places_every_weight_once():
    """The packed BPTT stream at both co_pad values of H = 64 (64: block 1; 192: c0g = 128): output block ``qq`` of
    output slice ``so`` covers channels qq * co_pad / 4 + 16 so .. + 15 of [dx | dh] — the index the kernel's phase B
    stores by — and holds [W_ih[:, :c0g] | W_hh]^T exactly once."""
    from fnssl import ops
    rs = np.random.RandomState(7)
    H = 64
    for c_in, c0g in ((4, 0), (132, 128)):
        w_ih = rs.standard_normal((4 * H, c_in)).astype(np.float32)
        w_hh = rs.standard_normal((4 * H, H)).astype(np.float32)
        packed = ops.pack_lstm_bwd_host(w_ih, w_hh, c0g)
        co = (c0g + H + 63) // 64 * 64
        nso, hq = co // 64, co // 4
        assert co == (64 if c0g == 0 else 192)
        recs = packed.reshape(nso, 17, 4, 64, 4)                           # [slice][quad][record j][lane][qq]
        assert not recs[:, 0].any()                                        # the accumulator-init quad
        wt = np.concatenate((w_ih[:, :c0g], w_hh), axis=1).T               # [c0g + H, 4H]
        got = np.zeros_like(wt)
        for so in range(nso):
            for qq in range(4):
                for l in range(64):
                    o = qq * hq + 16 * so + (l & 15)
                    ku = 16 * np.arange(16)[:, None] + 4 * (l >> 4) + np.arange(4)[None, :]     # [v][j]
                    vals = recs[so, 1:, :, l, qq]                          # [v][j]
                    if o < c0g + H:
                        got[o, ku] += vals
                    else:
                        assert not vals.any()
        np.testing.assert_array_equal(got, wt)
        # the carried-dh record of a dh block, (ob - c0g) >> 4, runs over the H / 16 = 4 hidden slices exactly once
        dh_recs = sorted((qq * hq + 16 * so - c0g) >> 4 for so in range(nso) for qq in range(4)
                         if c0g <= qq * hq + 16 * so < c0g + H)
        assert dh_recs == [0, 1, 2, 3]


def test_forward_train_refusals():
    net = _ipdnet().eval()
    with pytest.raises(RuntimeError, match="eval\\(\\) mode"):
        net.forward_train(torch.zeros(1, 4, 16, 24))
    net.train()
    with pytest.raises(RuntimeError, match="no training kernels"):
        net.forward_train(torch.zeros(1, 4, 16, 24), offline_inference=True)
    with pytest.raises(RuntimeError, match="no training kernels"):
        _ipdnet().bfloat16().train().forward_train(torch.zeros(1, 4, 16, 24))
    with pytest.raises(RuntimeError, match="ROCm"):                      # trainable: the HIP route (no CPU path)
        net.forward_train(torch.zeros(1, 4, 16, 24))
    with pytest.raises(RuntimeError, match="call .eval\\(\\) first"):   # forward keeps its routing
        net(torch.zeros(1, 4, 16, 24))


def test_train_step_module_opt_in_is_a_trailing_keyword():
    import inspect
    from IPDnet.train_step import MyModel
    params = list(inspect.signature(MyModel.__init__).parameters.values())
    assert [p.name for p in params[-2:]] == ["arch", "train_on_device"] and params[-1].default is False


def test_golden_g22_matches_cpu_restatement():
    """G22 (the real reference at hidden 128, tests/golden/make_golden_ipdnet_train_h128.py) against RefIPDnet with the
    same masks, on the CPU: the restatement the GPU tests compare with computes what the reference computes."""
    from fnssl import weights as W
    g = load_golden("g22_ipdnet_train_h128")
    want_cfg = {"a": (4, 1, 2, 24, 36), "b": (4, 0, 2, 20, 24), "c": (8, 1, 2, 16, 36)}
    for case in ("a", "b", "c"):
        nc, online, nb, nf, nt = (int(v) for v in g[case + "_cfg"])
        assert (nc, online, nb, nf, nt) == want_cfg[case]
        sd = W.make_ipdnet_state(int(g[case + "_wseed"]), nc, 128, 2, bool(online))
        ref = R.RefIPDnet(nc, 128, 2, bool(online))
        ref.load_state_dict(R.state_tensors(sd))
        ref.train()
        pred = ref(torch.from_numpy(g[case + "_x"]), R.site_masks(int(g[case + "_base"]), nb, nt, nf, 0, c=128))
        np.testing.assert_allclose(pred.detach().numpy(), g[case + "_pred"], rtol=1e-5, atol=1e-6)
        loss = R.pit_mse(pred, torch.from_numpy(g[case + "_gt"]))
        assert abs(loss.item() - float(g[case + "_loss"])) <= 1e-6 * abs(float(g[case + "_loss"]))
        loss.backward()
        for i, (k, p) in enumerate(ref.named_parameters()):
            gd = p.grad.double().numpy()
            norm = float(g[case + "_gnorm"][i])
            assert abs(np.sqrt((gd * gd).sum()) - norm) <= 1e-5 * norm + 1e-12, k
            n = min(16, gd.size)
            np.testing.assert_allclose(gd.reshape(-1)[:n], g[case + "_ghead"][i][:n], rtol=0,
                                       atol=1e-5 * np.abs(gd).max() + 1e-12, err_msg=k)
