"""Host-side checks of IPDnet training (no GPU): the conv-backward entry points are declared, exported and validate
their arguments before touching the device; unsupported configurations keep the forward-only error; the dropout sites'
seeds and shapes."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from fnssl import _lib, ipdnet_train, ops, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fnssl_conv3x3_packed_floats_backward_data", "fnssl_conv3x3_pack_backward_data",
       "fnssl_conv3x3_act_pool_backward", "fnssl_conv3x3_causal_backward_data",
       "fnssl_conv3x3_weight_grads_workspace_bytes", "fnssl_conv3x3_weight_grads")


def test_conv_backward_symbols_declared_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fnssl.h")).read()
    declared = set(re.findall(r"\b(fnssl_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.fnssl_abi_version() == 19


def test_conv_backward_entries_validate_before_launch():
    lib = _lib.load()
    p = C.c_void_p(64)                       # never dereferenced: every call below must fail validation first
    assert lib.fnssl_conv3x3_packed_floats_backward_data(28, 128, 128) > 0
    assert lib.fnssl_conv3x3_packed_floats_backward_data(128, 272, 256) == (
        2 * lib.fnssl_conv3x3_packed_floats(128, 128, 0))
    assert lib.fnssl_conv3x3_packed_floats_backward_data(30, 128, 128) == 0     # cout % 4
    assert lib.fnssl_conv3x3_packed_floats_backward_data(128, 128, 130) == 0    # cin_g > cin
    assert lib.fnssl_conv3x3_act_pool_backward(p, p, 1, 2, 12, 6, 3, 1, p, None) != 0          # c % 4
    assert lib.fnssl_conv3x3_act_pool_backward(p, p, 1, 2, 12, 8, 3, 3, p, None) != 0          # act
    assert lib.fnssl_conv3x3_causal_backward_data(p, 0, 0, 0, 30, p, 128, 1, 2, 12, p, 128, None) != 0
    assert lib.fnssl_conv3x3_causal_backward_data(p, 0, 0, 0, 128, p, 128, 1, 2, 12, p, 64, None) != 0   # dx stride
    assert lib.fnssl_conv3x3_causal_backward_data(p, 6, 0, 0, 128, p, 128, 1, 2, 12, p, 128, None) != 0  # stride % 4
    assert lib.fnssl_conv3x3_weight_grads_workspace_bytes(2, 3, 12, 128, 256, 16) > 0
    assert lib.fnssl_conv3x3_weight_grads(p, 0, 0, 0, 128, p, 0, 0, 0, 256, p, 0, 0, 0, 6, 2, 3, 12, p, p, 1 << 30,
                                          None) != 0                                          # cb % 4
    assert lib.fnssl_conv3x3_weight_grads(p, 0, 0, 0, 128, p, 0, 0, 0, 256, None, 0, 0, 0, 0, 2, 3, 12, p, p, 16,
                                          None) != 0                                          # workspace too small
    assert b"workspace" in lib.fnssl_last_error()


def test_unsupported_configurations_keep_the_forward_only_error():
    from IPDnet.FixedAarryIPDnet import IPDnet
    with pytest.raises(RuntimeError, match="call .eval\\(\\) first"):
        IPDnet().train()(torch.zeros(1, 4, 256, 24))                     # hidden 128: full-band H = 64
    bf = IPDnet(16, 256, 2, True).bfloat16().train()
    assert not ipdnet_train.supported(bf)
    with pytest.raises(RuntimeError, match="call .eval\\(\\) first"):
        bf(torch.zeros(1, 16, 8, 24))
    off = IPDnet(16, 256, 2, False).train()
    assert ipdnet_train.supported(off) and not ipdnet_train.supported(off, offline_inference=True)
    with pytest.raises(RuntimeError, match="call .eval\\(\\) first"):
        off(torch.zeros(1, 16, 8, 24), offline_inference=True)
    net = IPDnet(16, 256, 2, True).train()
    assert ipdnet_train.supported(net)
    for call in (lambda: net.block_1.run(None, torch.zeros(1, 24, 8, 16)),
                 lambda: net.conv.run(torch.zeros(1, 8, 24, 256), torch.zeros(1, 8, 24, 16)),
                 lambda: net.forward_stream(torch.zeros(1, 16, 8, 24))):
        with pytest.raises(RuntimeError, match="call .eval\\(\\) first"):
            call()
    with pytest.raises(RuntimeError, match="ROCm"):                     # supported: the HIP route (no CPU path)
        net(torch.zeros(1, 16, 8, 24))


def test_dropout_sites_seeds_and_shapes():
    from IPDnet.FixedAarryIPDnet import IPDnet
    net = IPDnet(16, 256, 2, True)
    assert ipdnet_train.dropout_sites(net) == [net.block_1.dropout_full, net.block_1.dropout_narr,
                                               net.block_2.dropout_full, net.block_2.dropout_narr]
    assert ipdnet_train.site_seeds(77) == [train.layer_seed(77, s) for s in range(4)]
    assert len(set(ipdnet_train.site_seeds(77))) == 4
    g = ipdnet_train.IPDnetTrainGraph(net)
    assert [(L.name, L.mode, L.hidden, L.ndir, L.c0, L.c2, L.c0g) for L in g.lstms] == [
        ("block_1.fullLstm", "full", 128, 2, 16, 0, 0), ("block_1.narrLstm", "narrow", 256, 1, 256, 16, 256),
        ("block_2.fullLstm", "full", 128, 2, 256, 16, 256), ("block_2.narrLstm", "narrow", 256, 1, 256, 16, 256)]
    # every site's activation is 256 channels wide in both modes (keep-scale tensors are logical [nb, nt, nf, 256])
    off = IPDnet(16, 256, 2, False)
    for m in (net, off):
        for blk in (m.block_1, m.block_2):
            assert 2 * blk.fullLstm.hidden_size == 256
            assert blk.narrLstm.hidden_size * (2 if blk.narrLstm.bidirectional else 1) == 256
    from oracle import train_ref
    a = train_ref.dropout_scale(ipdnet_train.site_seeds(5)[2], (4, 3, 2, 256))
    b = train_ref.dropout_scale(ipdnet_train.site_seeds(5)[2], (2, 3, 2, 256), b0=2)
    np.testing.assert_array_equal(a[2:], b)                               # keyed by the global utterance index
    assert set(np.unique(a)) <= {0.0, 1.25}
