"""GPU tests of IPDnet training on the HIP path (fnssl/ipdnet_train.py, csrc/conv_train.hip): ``IPDnet.forward`` in
``train()`` mode at hidden_size 256 returns a tensor with a ``grad_fn``; ``loss.backward()`` runs the conv-head backward
(act / pool backward, anti-causal fp32-MFMA dgrad, split-K wgrad), the BPTT and weight-gradient kernels.  Checked
against a PyTorch CPU autograd restatement (tests/ipdnet_train_ref.py) with the same dropout masks, and against the
real reference's golden step (tests/golden/g18_ipdnet_train.npz)."""
import numpy as np
import pytest

from conftest import load_golden, rs_randn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ipdnet_train_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


def rel_close(got, want, tol, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = np.abs(want).max() + 1e-30
    err = np.abs(got - want).max() / scale
    assert err <= tol, "%s: max err %.3g of the largest entry (tol %g)" % (what, err, tol)


def _nets(dev, sd, nc, online, mt=2):
    from IPDnet.FixedAarryIPDnet import IPDnet
    net = IPDnet(nc, 256, mt, online)
    net.load_state_dict(R.state_tensors(sd))
    net = net.to(dev).train()
    ref = R.RefIPDnet(nc, 256, mt, online)
    ref.load_state_dict(R.state_tensors(sd))
    return net, ref


def _run_case(dev, nc, online, nb, nf, nt, wseed, base=1234, b0=0):
    from fnssl import weights as W
    sd = W.make_ipdnet_state(wseed, nc, 256, 2, online)
    net, ref = _nets(dev, sd, nc, online)
    net.force_dropout_base = base
    net.utt_offset = b0
    x = rs_randn(wseed + 1, (nb, nc, nf, nt))
    gt = rs_randn(wseed + 2, (nb, nt // 12, 2 * nf, nc // 2 - 1, 2), 0.5)
    pred = net(torch.from_numpy(x).to(dev))
    assert pred.grad_fn is not None
    loss = R.pit_mse(pred, torch.from_numpy(gt).to(dev))
    loss.backward()
    xr = torch.from_numpy(x)
    pref = ref(xr, R.site_masks(base, nb, nt, nf, b0))
    lref = R.pit_mse(pref, torch.from_numpy(gt))
    lref.backward()
    return net, ref, pred, loss, pref, lref, sd, x, gt


# ----------------------------------------------------------------------------------------------------------------
# conv head backward, unit level
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf,nt", [(2, 36), (17, 41), (1, 24)])
def test_conv_head_backward_matches_cpu_autograd(dev, nf, nt):
    """Config-3 channel counts 272 -> 128 -> 128 -> 28: dgrad into the 256 FN-block channels only, wgrad of all three
    convs (+= across two calls), nt = 41 leaves frames past the last whole pooling window, nf 1 / 2 / 17 the bin edges."""
    from fnssl import ops
    nb = 2
    rs = np.random.RandomState(nf * 100 + nt)
    ws = [(rs.uniform(-1, 1, s) / np.sqrt(s[1] * 9)).astype(np.float32)
          for s in ((128, 272, 3, 3), (128, 128, 3, 3), (28, 128, 3, 3))]
    xa = rs.standard_normal((nb, nf, nt, 256)).astype(np.float32)
    xb = rs.standard_normal((nb, nf, nt, 16)).astype(np.float32)
    dout = rs.standard_normal((nb, nf, nt // 12, 28)).astype(np.float32)
    # CPU autograd
    conv = R.RefConv(272, 28)
    for m, w in zip((conv.conv1, conv.conv2, conv.conv3), ws):
        m.weight.data = torch.from_numpy(w)
    xc = torch.from_numpy(np.concatenate((xa, xb), axis=3)).permute(0, 3, 1, 2).requires_grad_()
    yc = conv(xc)
    (yc * torch.from_numpy(dout).permute(0, 3, 1, 2)).sum().backward()
    # HIP
    d = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    xa_d, xb_d = d(xa), d(xb)
    f1 = ops.pack_conv3x3(ws[0], 256, 16, dev)
    f2 = ops.pack_conv3x3(ws[1], 128, 0, dev)
    f3 = ops.pack_conv3x3(ws[2], 128, 0, dev)
    y1 = ops.conv3x3_causal(xa_d, xb_d, f1, 128, "relu")
    p1 = ops.avgpool_time(y1, 3)
    y2 = ops.conv3x3_causal(p1, None, f2, 128, "relu")
    p2 = ops.avgpool_time(y2, 4)
    y3 = ops.conv3x3_causal(p2, None, f3, 28, "tanh")
    np.testing.assert_allclose(y3.cpu().numpy(), yc.detach().permute(0, 2, 3, 1).numpy(), rtol=1e-4, atol=1e-5)
    g = [torch.zeros(w.shape, device=dev) for w in ws]
    for _ in range(2):                                       # += accumulation: two calls give twice the gradient
        dz3 = ops.conv3x3_act_pool_backward(d(dout), y3, 1, "tanh")
        ops.conv3x3_weight_grads(dz3, p2, None, g[2])
        dp2 = ops.conv3x3_causal_backward_data(dz3, ops.pack_conv3x3_backward_data(ws[2], 128, dev), 128)
        dz2 = ops.conv3x3_act_pool_backward(dp2, y2, 4, "relu")
        ops.conv3x3_weight_grads(dz2, p1, None, g[1])
        dp1 = ops.conv3x3_causal_backward_data(dz2, ops.pack_conv3x3_backward_data(ws[1], 128, dev), 128)
        dz1 = ops.conv3x3_act_pool_backward(dp1, y1, 3, "relu")
        ops.conv3x3_weight_grads(dz1, xa_d, xb_d, g[0])
        dx = ops.conv3x3_causal_backward_data(dz1, ops.pack_conv3x3_backward_data(ws[0], 256, dev), 256)
    want_dx = xc.grad.permute(0, 2, 3, 1).numpy()
    assert dx.shape == (nb, nf, nt, 256)
    rel_close(dx.cpu().numpy(), want_dx[..., :256], 5e-5, "dgrad conv1 (256 channels)")
    for k, m in enumerate((conv.conv1, conv.conv2, conv.conv3)):
        rel_close(g[k].cpu().numpy(), 2 * m.weight.grad.numpy(), 5e-5, "wgrad conv%d (two calls)" % (k + 1))


# ----------------------------------------------------------------------------------------------------------------
# whole network against the CPU restatement
# ----------------------------------------------------------------------------------------------------------------
CASES = {"a": (16, True, 2, 16, 36, 1800), "b": (16, False, 2, 20, 24, 1810), "c": (4, True, 2, 24, 36, 1820)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_train_step_matches_cpu_restatement(dev, case):
    nc, online, nb, nf, nt, wseed = CASES[case]
    net, ref, pred, loss, pref, lref, sd, x, gt = _run_case(dev, nc, online, nb, nf, nt, wseed)
    np.testing.assert_allclose(pred.detach().cpu().numpy(), pref.detach().numpy(), rtol=1e-4, atol=1e-5)
    assert abs(loss.item() - lref.item()) <= 1e-5 * abs(lref.item())
    rp = dict(ref.named_parameters())
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        rel_close(p.grad.cpu().numpy(), rp[k].grad.numpy(), 5e-4, "grad " + k)
    # one Adam step on both; eval() then sees the stepped weights
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    opt_r = torch.optim.Adam(ref.parameters(), lr=5e-4)
    opt.step()
    opt_r.step()
    for k, p in net.named_parameters():
        g = rp[k].grad.abs().numpy()
        sel = g > 1e-3 * g.max()
        np.testing.assert_allclose(p.detach().cpu().numpy()[sel], rp[k].detach().numpy()[sel], rtol=0, atol=2e-5)
    net.eval()
    with torch.no_grad():
        ye = net(torch.from_numpy(x).to(dev)).cpu().numpy()
        ref.eval()
        yr = ref(torch.from_numpy(x), [None] * 4).numpy()
    np.testing.assert_allclose(ye, yr, rtol=1e-4, atol=1e-5)


def test_train_step_matches_reference_golden(dev):
    """G18: the real reference (FixedAarryIPDnet.IPDnet in train() mode, dropout as the keep-scale masks, PIT-MSE,
    autograd, torch.optim.Adam(lr=5e-4)) on cases (a)-(c)."""
    g = load_golden("g18_ipdnet_train")
    for case in ("a", "b", "c"):
        nc, online, nb, nf, nt = (int(v) for v in g[case + "_cfg"])
        from fnssl import weights as W
        sd = W.make_ipdnet_state(int(g[case + "_wseed"]), nc, 256, 2, bool(online))
        net, _ = _nets(dev, sd, nc, bool(online))
        net.force_dropout_base = int(g[case + "_base"])
        net.utt_offset = 0
        pred = net(torch.from_numpy(g[case + "_x"]).to(dev))
        np.testing.assert_allclose(pred.detach().cpu().numpy(), g[case + "_pred"], rtol=1e-4, atol=1e-5)
        loss = R.pit_mse(pred, torch.from_numpy(g[case + "_gt"]).to(dev))
        assert abs(loss.item() - float(g[case + "_loss"])) <= 1e-5 * abs(float(g[case + "_loss"]))
        loss.backward()
        names = [k for k, _ in net.named_parameters()]
        for i, (k, p) in enumerate(net.named_parameters()):
            gd = p.grad.cpu().numpy().astype(np.float64)
            norm = float(g[case + "_gnorm"][i])
            assert abs(np.sqrt((gd * gd).sum()) - norm) <= 5e-4 * norm + 1e-12, k
            head = g[case + "_ghead"][i]
            np.testing.assert_allclose(gd.reshape(-1)[:16], head, rtol=0, atol=5e-4 * np.abs(gd).max() + 1e-12,
                                       err_msg=k)
        torch.optim.Adam(net.parameters(), lr=5e-4).step()
        for i, k in enumerate(names):
            p = dict(net.named_parameters())[k].detach().cpu().numpy().reshape(-1)[:16]
            np.testing.assert_allclose(p, g[case + "_phead"][i], rtol=0, atol=2e-5, err_msg=k)


def test_batch_sharding_equals_one_batch(dev):
    """Utterances [0:4) with utt_offset 0 plus [4:8) with utt_offset 4 give the gradients of one 8-utterance call: the
    dropout masks follow the global utterance index."""
    from fnssl import weights as W
    from IPDnet.FixedAarryIPDnet import IPDnet
    sd = W.make_ipdnet_state(1900, 16, 256, 2, True)
    nb, nf, nt = 8, 16, 24
    x = torch.from_numpy(rs_randn(1901, (nb, 16, nf, nt))).to(dev)
    gt = torch.from_numpy(rs_randn(1902, (nb, nt // 12, 2 * nf, 7, 2), 0.5)).to(dev)

    def grads(parts):
        net = IPDnet(16, 256, 2, True)
        net.load_state_dict(R.state_tensors(sd))
        net = net.to(dev).train()
        net.force_dropout_base = 99
        for lo, hi in parts:
            net.utt_offset = lo
            # the sum of per-row MSE means: the shards' losses add up to the whole batch's (times nb)
            (R.pit_mse(net(x[lo:hi]), gt[lo:hi]) * (hi - lo)).backward()
        return {k: p.grad.clone() for k, p in net.named_parameters()}

    one = grads([(0, nb)])
    two = grads([(0, 4), (4, nb)])
    for k in one:
        rel_close(two[k].cpu().numpy(), one[k].cpu().numpy(), 1e-5, "sharded grad " + k)


def test_config3_geometry(dev):
    """16 utterances x 8 microphones x 256 bins x 300 frames: finite gradients, per-utterance batch independence, the
    LSTM calls' kernel families, no cluster fallback."""
    from fnssl import ops
    from fnssl import weights as W
    from IPDnet.FixedAarryIPDnet import IPDnet
    sd = W.make_ipdnet_state(2000, 16, 256, 2, True)
    net = IPDnet(16, 256, 2, True)
    net.load_state_dict(R.state_tensors(sd))
    net = net.to(dev).train()
    net.force_dropout_base = 5
    nb, nf, nt = 16, 256, 300
    x = torch.from_numpy(rs_randn(2001, (nb, 16, nf, nt), 0.5)).to(dev)
    ops.cluster_fallbacks(dev, reset=True)
    pred = net(x)
    loss = (pred * pred).mean()
    loss.backward()
    torch.cuda.synchronize()
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all().item(), k
    assert ops.cluster_fallbacks(dev) == 0
    # batch independence: utterances 3 and 11 alone (same global index -> same masks) give the same prediction
    net.zero_grad()
    for u in (3, 11):
        net.utt_offset = u
        pu = net(x[u:u + 1])
        np.testing.assert_allclose(pu.detach().cpu().numpy(), pred[u:u + 1].detach().cpu().numpy(), rtol=1e-4,
                                   atol=1e-5)
    net.utt_offset = None
    # the families the LSTM calls take at this geometry (plan functions launch nothing)
    g = net._train_graph
    XF = torch.empty((nb, nt, nf, 16), device=dev)
    A = torch.empty((nb, nt, nf, 256), device=dev)
    fw, bw, _, _ = g.streams(dev)
    fams = []
    for L, s0, s2 in ((g.lf1, XF, None), (g.ln1, A, XF), (g.lf2, A, XF), (g.ln2, A, XF)):
        nseq, nsteps = (nb * nt, nf) if L.mode == "full" else (nb * nf, nt)
        res = torch.empty(ops.lstm_reserve_floats(nseq, L.hidden, L.ndir, nsteps), device=dev)
        out = torch.empty((nb, nt, nf, L.ndir * L.hidden), device=dev)
        fams.append(ops.lstm_plan(L.mode, s0, None, s2, fw[L.name], L.hidden, out, reserve=res)[0])
        dx = torch.empty((nb, nt, nf, L.ndir * L.c0g), device=dev) if L.c0g else None
        fams.append(ops.lstm_backward(L.mode, res, out, torch.empty((nb, nt, nf, L.ndir * 4 * L.hidden), device=dev), dx,
                                      bw[L.name], L.hidden, L.c0g, plan_only=True))
        del res
    assert all(isinstance(f, str) and not f.startswith("unknown") for f in fams), fams
    print("config-3 LSTM families (fwd, bwd per layer):", fams)


def test_no_vendor_kernels_on_the_path(dev, monkeypatch):
    """conv2d / matmul / bmm / mm raise during the train-mode forward and backward: nothing on the route uses them."""
    from fnssl import weights as W
    sd = W.make_ipdnet_state(2100, 16, 256, 2, True)
    net, _ = _nets(dev, sd, 16, True)
    x = torch.from_numpy(rs_randn(2101, (2, 16, 16, 24))).to(dev)

    def boom(*a, **k):
        raise AssertionError("vendor kernel called on the IPDnet training path")

    monkeypatch.setattr(torch.nn.functional, "conv2d", boom)
    for name in ("matmul", "bmm", "mm"):
        monkeypatch.setattr(torch, name, boom)
    pred = net(x)
    (pred * pred).sum().backward()
    assert all(p.grad is not None for p in net.parameters())
