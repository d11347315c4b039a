"""GPU tests of IPDnet training on the HIP path (fnssl/ipdnet_train.py, csrc/conv_train.hip): ``IPDnet.forward`` in
``train()`` mode at hidden_size 256 returns a tensor with a ``grad_fn``; ``loss.backward()`` runs the conv-head backward
(act / pool backward, anti-causal fp32-MFMA dgrad, split-K wgrad), the BPTT and weight-gradient kernels.  Checked
against a PyTorch CPU autograd restatement (tests/ipdnet_train_ref.py) with the same dropout masks, and against the
real reference's golden step (tests/golden/g18_ipdnet_train.npz).  At config-3 size (and a ragged twin): layer by
layer and the whole network against float64 references (tests/fp64_ref.py)."""
import numpy as np
import pytest

from conftest import assert_close, load_golden, rs_randn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import fp64_ref as F64  # noqa: E402
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


def rel_err(got, want, tol, what):
    """rel_close for tensors of any device / dtype (compared in float64); prints the measured error."""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    err = float((got - want).abs().max() / (want.abs().max() + 1e-30))
    print("CHECK %-58s %.3g of the largest entry (tol %g)" % (what, err, tol))
    assert err <= tol, "%s: max err %.3g of the largest entry (tol %g)" % (what, err, tol)


def fails_without(want, parts, tol, what):
    """``want`` is a sum over all rows, checked at ``tol`` of its largest entry: leaving out any of ``parts`` (the
    contribution of one 16-row stage, of one whole slab) must move some entry by more than that."""
    scale = float(want.abs().max())
    for name, p in parts.items():
        moved = float(p.abs().max())
        assert moved > tol * scale, "%s: without %s the result moves by %.3g of the largest entry only (tol %g)" % (
            what, name, moved / scale, tol)


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


# ----------------------------------------------------------------------------------------------------------------
# config-3 size (16 utterances x 256 bins x 300 frames) and its ragged twin against float64
# ----------------------------------------------------------------------------------------------------------------
# the twin: the last 16-sequence group is partial in both band modes (15 * 301 and 15 * 250 sequences), full-band groups
# straddle utterance boundaries (301 frames per utterance), 301 frames are not a whole number of pooling windows
GEOMS = {"config3": (16, 256, 300), "twin": (15, 250, 301)}
# (mode, hidden, ndir, c0, c2, c0g) of a train-graph LSTM -> (forward family with a reserve, BPTT family), at both
# geometries
LSTM_FAMILIES = {
    ("full", 128, 2, 16, 0, 0): ("train", "bwd_cluster"),           # block 1 full band
    ("narrow", 256, 1, 256, 16, 256): ("train", "bwd"),              # online narrow band (blocks 1 and 2)
    ("full", 128, 2, 256, 16, 256): ("train", "bwd_cluster"),        # block 2 full band
    ("narrow", 128, 2, 256, 16, 256): ("train", "bwd_cluster"),      # offline narrow band (blocks 1 and 2)
}
# layer -> (online model?, index in IPDnetTrainGraph.lstms): one of each distinct shape above
LAYERS = {"full1": (True, 0), "narrow_online": (True, 1), "full2": (True, 2), "narrow_offline": (False, 1)}


def _shape(L):
    return (L.mode, L.hidden, L.ndir, L.c0, L.c2, L.c0g)


def _train_graph(dev, online, wseed):
    from fnssl import ipdnet_train
    from fnssl import weights as W
    sd = W.make_ipdnet_state(wseed, 16, 256, 2, online)
    net, _ = _nets(dev, sd, 16, online)
    return ipdnet_train.IPDnetTrainGraph(net)


def _free():
    import gc
    from fnssl import ops
    gc.collect()
    ops.release_workspaces()
    torch.cuda.empty_cache()


def assert_lstm_families(g, nb, nf, nt, dev):
    """Every LSTM call of the train graph takes the family LSTM_FAMILIES names, with the operands in the graph's
    natural layouts (plan queries: nothing is launched)."""
    from fnssl import ops
    fw, bw, _, _ = g.streams(dev)
    got, want = [], []
    for L in g.lstms:
        nseq, nsteps = (nb * nt, nf) if L.mode == "full" else (nb * nf, nt)
        x0 = L.natural(nb, nt, nf, L.c0, dev)
        x2 = L.natural(nb, nt, nf, L.c2, dev) if L.c2 else None
        res = torch.empty(ops.lstm_reserve_floats(nseq, L.hidden, L.ndir, nsteps), device=dev)
        out = L.natural(nb, nt, nf, L.ndir * L.hidden, dev)
        da = L.natural(nb, nt, nf, L.ndir * 4 * L.hidden, dev)
        dx = L.natural(nb, nt, nf, L.ndir * L.c0g, dev) if L.c0g else None
        got.append((L.name, ops.lstm_plan(L.mode, x0, None, x2, fw[L.name], L.hidden, out, reserve=res)[0],
                    ops.lstm_backward(L.mode, res, out, da, dx, bw[L.name], L.hidden, L.c0g, plan_only=True)))
        want.append((L.name,) + LSTM_FAMILIES[_shape(L)])
        del x0, x2, res, out, da, dx
    _free()
    assert got == want, got


def _sampled_sequences(mode, nb, nf, nt):
    """The first, a middle and the last 16-sequence group, and the group holding the first utterance boundary."""
    q = nt if mode == "full" else nf                  # sequences per utterance
    nseq = nb * q
    ng = (nseq + 15) // 16
    groups = sorted({0, ng // 2, q // 16, ng - 1})
    return [s for g in groups for s in range(16 * g, min(16 * g + 16, nseq))]


@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_lstm_layer_at_config3_vs_float64(dev, layer, geom):
    """One IPDnet LSTM layer at full size, operands in the train graph's natural layouts ([D | x] with the 16 skip
    channels concatenated): exact kernel families; the reserve-saving forward equals the plain one bit for bit; h, dA
    (gate order i, f, g, o) and dx of sampled sequences against a float64 step loop (sequences are independent, so a
    sample is an exact check); the weight gradients over ALL rows against float64 products of the kernel's own dA,
    inputs and shifted h, with a tolerance that one missing 16-row stage or slab of the split-K sum would exceed."""
    from fnssl import _lib, ops
    online, idx = LAYERS[layer]
    nb, nf, nt = GEOMS[geom]
    g = _train_graph(dev, online, 2200)
    L = g.lstms[idx]
    mode, H, ndir, c0, c2, c0g = _shape(L)
    nseq, nsteps = (nb * nt, nf) if mode == "full" else (nb * nf, nt)
    if geom == "twin":
        assert nseq % 16 and (nt if mode == "full" else nf) % 16 and nt % 3 and nt % 12
    fw, bw, _, _ = g.streams(dev)
    gen = torch.Generator(device=dev).manual_seed(2201 + idx)
    x0 = L.natural(nb, nt, nf, c0, dev).normal_(0, 0.5, generator=gen)
    x2 = L.natural(nb, nt, nf, c2, dev).normal_(0, 0.5, generator=gen) if c2 else None
    res = torch.empty(ops.lstm_reserve_floats(nseq, H, ndir, nsteps), device=dev)
    out = L.natural(nb, nt, nf, ndir * H, dev)
    dh = L.natural(nb, nt, nf, ndir * H, dev).normal_(0, 1, generator=gen)
    da = L.natural(nb, nt, nf, ndir * 4 * H, dev)
    dx = L.natural(nb, nt, nf, ndir * c0g, dev) if c0g else None
    fams = (ops.lstm_plan(mode, x0, None, x2, fw[L.name], H, out, reserve=res)[0],
            ops.lstm_backward(mode, res, dh, da, dx, bw[L.name], H, c0g, plan_only=True))
    assert fams == LSTM_FAMILIES[_shape(L)], fams
    ops.lstm_layer(mode, x0, None, x2, fw[L.name], H, out, reserve=res)
    plain = L.natural(nb, nt, nf, ndir * H, dev)
    ops.lstm_layer(mode, x0, None, x2, fw[L.name], H, plain)
    assert torch.equal(out, plain), "the reserve-saving forward computes the same h"
    del plain
    ops.lstm_backward(mode, res, dh, da, dx, bw[L.name], H, c0g)
    del res
    # ---- sampled sequences against a float64 step loop (CPU)
    seqs = torch.tensor(_sampled_sequences(mode, nb, nf, nt), device=dev)
    q = nt if mode == "full" else nf
    bi, qi = seqs // q, seqs % q

    def sample(t):                  # logical [nb, nt, nf, C] -> [S, nsteps, C] of the sampled sequences
        return (t if mode == "full" else t.permute(0, 2, 1, 3))[bi, qi].double().cpu()

    params = [[p.detach().double().cpu() for p in L.params(n)]
              for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    h64, da64, dx64 = F64.lstm_bptt(torch.cat([sample(x0)] + ([sample(x2)] if c2 else []), -1), list(zip(*params)),
                                    sample(dh))
    got_h = sample(out)
    assert_close(got_h.numpy(), h64.numpy(), 1e-4, 1e-5, "%s %s: h of the sampled sequences" % (layer, geom))
    print("CHECK %-58s %.3g of the tolerance (rtol 1e-4, atol 1e-5)" % (
        "%s %s h" % (layer, geom), float(((got_h - h64).abs() / (1e-5 + 1e-4 * h64.abs())).max())))
    rel_err(sample(da), da64, 2e-4, "%s %s dA (sampled)" % (layer, geom))
    if c0g:
        assert dx.shape[-1] == ndir * c0g                # the 16 concatenated skip channels get no gradient
        rel_err(sample(dx), dx64[..., :c0g].reshape(dx64.shape[0], nsteps, ndir * c0g), 2e-4,
                "%s %s dx (sampled)" % (layer, geom))
    # ---- weight gradients over all rows against float64 products (on the device)
    init = 0.5
    gw = {k: [torch.full(s, init, device=dev) for _ in range(ndir)]
          for k, s in (("wih", (4 * H, c0 + c2)), ("whh", (4 * H, H)), ("bih", (4 * H,)), ("bhh", (4 * H,)))}
    ops.lstm_weight_grads(L.rows(da), L.rows(x0), L.rows(x2) if c2 else None, L.rows(out), H, ndir, nsteps,
                          gw["wih"], gw["whh"], gw["bih"], gw["bhh"])
    rows = nseq * nsteps
    xs = [L.rows(x0)] + ([L.rows(x2)] if c2 else [])
    part = lambda r0, r1: F64.lstm_weight_grads(L.rows(da), xs, L.rows(out), H, ndir, nsteps, r0, r1)  # noqa: E731
    want = part(0, rows)
    # the split-K plan of this launch (csrc/wgrad.hip): slab count from the workspace size, rows per slab restated
    M, ncat = ndir * 4 * H, c0 + c2 + H
    slabs = (_lib.load().fnssl_lstm_weight_grads_workspace_bytes(rows, H, ndir, c0, c2) - 256) // (4 * M * (ncat + 1))
    ntiles = ((0 if c0 == 4 else (c0 + 127) // 128) + (0 if c2 == 4 and c0 != 4 else (c2 + 127) // 128)
              + (H + 127) // 128)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    plan, rps = F64.slab_plan(rows, M // 256 * ntiles, cus, 4, 512)
    assert plan == slabs >= 64, (plan, slabs)
    stage, last = part(rps - 16, rps), part((slabs - 1) * rps, rows)
    for d in range(ndir):
        for k, name in (("wih", "dW_ih"), ("whh", "dW_hh"), ("bih", "db_ih"), ("bhh", "db_hh")):
            w = want["b" if k[0] == "b" else k][d]
            what = "%s %s %s[%d] (%d slabs)" % (layer, geom, name, d, slabs)
            rel_err(gw[k][d].double() - init, w, 2e-5, what)
            fails_without(w, {"one 16-row stage": stage["b" if k[0] == "b" else k][d],
                              "the last slab": last["b" if k[0] == "b" else k][d]}, 2e-5, what)
    del x0, x2, out, dh, da, dx, gw, want, stage, last
    _free()


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
    assert_lstm_families(net._train_graph, nb, nf, nt, dev)


@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_conv_head_backward_at_config3_vs_float64(dev, geom):
    """The conv head's backward at full size, channels 272 -> 128 -> 128 -> 28, pools 3 / 4 / none, conv 1's X read in
    place from [D3 | x] as the train graph passes them: act / pool backward and dgrad (conv 1: two 128-channel chunks)
    of one whole utterance against float64 autograd of the same op (both are local in f and t: exact); the weight
    gradients of all three convs over ALL rows (+= over two calls) against float64 tap-shifted products, from a launch
    of at least 64 slabs, with a tolerance that one missing 16-row stage or slab would exceed."""
    from fnssl import _lib, ops
    nb, nf, nt = GEOMS[geom]
    u = nb - 1
    rs = np.random.RandomState(2400 + nt)
    ws = [(rs.uniform(-1, 1, s) / np.sqrt(s[1] * 9)).astype(np.float32)
          for s in ((128, 272, 3, 3), (128, 128, 3, 3), (28, 128, 3, 3))]
    gen = torch.Generator(device=dev).manual_seed(2401)
    D3 = torch.empty((nb, nf, nt, 256), device=dev).normal_(0, 1, generator=gen).permute(0, 2, 1, 3)
    XN = torch.empty((nb, nf, nt, 16), device=dev).normal_(0, 1, generator=gen).permute(0, 2, 1, 3)
    xa, xb = D3.permute(0, 2, 1, 3), XN.permute(0, 2, 1, 3)          # conv 1's operands, as ipdnet_train.py passes them
    Y1 = ops.conv3x3_causal(xa, xb, ops.pack_conv3x3(ws[0], 256, 16, dev), 128, "relu")
    P1 = ops.avgpool_time(Y1, 3)
    Y2 = ops.conv3x3_causal(P1, None, ops.pack_conv3x3(ws[1], 128, 0, dev), 128, "relu")
    P2 = ops.avgpool_time(Y2, 4)
    Y3 = ops.conv3x3_causal(P2, None, ops.pack_conv3x3(ws[2], 128, 0, dev), 28, "tanh")
    assert tuple(Y3.shape) == (nb, nf, nt // 12, 28) and float(Y3.abs().max()) < 1
    dY3 = torch.empty(Y3.shape, device=dev).normal_(0, 1, generator=gen)
    bwd = [ops.pack_conv3x3_backward_data(w, c, dev) for w, c in zip(ws, (256, 128, 128))]
    dZ3 = ops.conv3x3_act_pool_backward(dY3, Y3, 1, "tanh")
    dP2 = ops.conv3x3_causal_backward_data(dZ3, bwd[2], 128)
    dZ2 = ops.conv3x3_act_pool_backward(dP2, Y2, 4, "relu")
    dP1 = ops.conv3x3_causal_backward_data(dZ2, bwd[1], 128)
    dZ1 = ops.conv3x3_act_pool_backward(dP1, Y1, 3, "relu")
    dX = ops.conv3x3_causal_backward_data(dZ1, bwd[0], 256)
    # ---- act / pool backward and dgrad of utterance u against float64 autograd (CPU)
    c = lambda t: t[u].cpu()   # noqa: E731
    for what, y, dp, k, act, dz in (("3 (tanh)", Y3, dY3, 1, "tanh", dZ3),
                                    ("2 (relu, pool 4)", Y2, dP2, 4, "relu", dZ2),
                                    ("1 (relu, pool 3)", Y1, dP1, 3, "relu", dZ1)):
        rel_err(c(dz), F64.act_pool_backward(c(y), c(dp), k, act), 1e-6, "%s act/pool backward %s" % (geom, what))
    for what, dz, w, cin_g, got in (("conv 3", dZ3, ws[2], 128, dP2), ("conv 2", dZ2, ws[1], 128, dP1),
                                    ("conv 1 (256 of 272 channels)", dZ1, ws[0], 256, dX)):
        rel_err(c(got), F64.conv_backward_data(c(dz), torch.from_numpy(w), cin_g), 5e-5, "%s dgrad %s" % (geom, what))
    del dP2, dP1, dX
    # ---- weight gradients over all rows against float64 products (on the device)
    lib = _lib.load()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for what, dz, xs in (("conv 3", dZ3, [P2]), ("conv 2", dZ2, [P1]), ("conv 1", dZ1, [xa, xb])):
        nbb, nff, ntt, cout = dz.shape
        cin = sum(x.shape[3] for x in xs)
        grad = torch.zeros((cout, cin, 3, 3), device=dev)
        for _ in range(2):                                             # += accumulation
            ops.conv3x3_weight_grads(dz, xs[0], xs[1] if len(xs) > 1 else None, grad)
        rows = nbb * nff * ntt
        part = lambda r0, r1: F64.conv_weight_grads(dz, xs, r0, r1)   # noqa: E731
        want = 2 * part(0, rows)
        # the split-K plan of this launch (csrc/conv_train.hip): slab count from the workspace size, rows per slab
        # restated
        wsb = lib.fnssl_conv3x3_weight_grads_workspace_bytes(nbb, nff, ntt, cout, xs[0].shape[3], cin - xs[0].shape[3])
        slabs = (wsb - 256) // (cout * 9 * cin * 4)
        plan, rps = F64.slab_plan(rows, (cout + 127) // 128 * ((9 * cin + 127) // 128), cus, 8, 256)
        assert plan == slabs >= 64, (what, plan, slabs)
        name = "%s wgrad %s (%d slabs, 2 calls)" % (geom, what, slabs)
        rel_err(grad, want, 2e-5, name)
        fails_without(want, {"one 16-row stage": 2 * part(rps - 16, rps),
                             "the last slab": 2 * part((slabs - 1) * rps, rows)}, 2e-5, name)
    del D3, XN, xa, xb, Y1, P1, Y2, P2, Y3, dY3, dZ3, dZ2, dZ1
    _free()


def _config3_net(dev, online, wseed, base):
    from fnssl import weights as W
    sd = W.make_ipdnet_state(wseed, 16, 256, 2, online)
    net, _ = _nets(dev, sd, 16, online)
    net.force_dropout_base = base
    return sd, net


@pytest.mark.parametrize("online", [True, False], ids=["online", "offline"])
def test_config3_sampled_utterance_grads_vs_float64(dev, online):
    """The full 16-utterance config-3 batch, online and offline models, with a loss that reads only utterance 11:
    exact LSTM families per layer; its prediction and every parameter gradient against the float64 CPU restatement
    (tests/ipdnet_train_ref.py) of that utterance alone, with the dropout masks of its place in the batch.  The
    kernels run at full size; the other utterances get zero upstream gradient.

    The float64 run takes the conv-head ReLUs' branches from the kernels' forward: among the ~13 M ReLU inputs of one
    utterance a few lie within fp32 rounding of zero, and one such flip moves the gradients by up to 1.4e-3 of their
    largest entry (PyTorch's own fp32 CPU autograd against float64 shows the same on this utterance).  The test asserts
    that every differing branch sits at an input within 1e-5 of the largest |input|, i.e. at a tie."""
    from fnssl import ipdnet_train
    nb, nf, nt, u, base = 16, 256, 300, 11, 31
    sd, net = _config3_net(dev, online, 2500 + online, base)
    net.utt_offset = 0
    x = rs_randn(2501, (nb, 16, nf, nt), 0.5)
    G = rs_randn(2502, (nt // 12, 2 * nf, 7, 2))
    xd = torch.from_numpy(x).to(dev)
    pred = net(xd)
    (pred[u] * torch.from_numpy(G).to(dev)).sum().backward()
    got = {k: p.grad.cpu() for k, p in net.named_parameters()}
    pu = pred[u].detach().cpu().numpy()
    assert_lstm_families(net._train_graph, nb, nf, nt, dev)
    del pred
    _free()
    # the branches the kernels' backward takes: the same forward again, its saved post-ReLU outputs of utterance u
    _, saved = net._train_graph.forward(xd, ipdnet_train.site_seeds(base), 0)
    relu = [(saved[k][u:u + 1] > 0).permute(0, 3, 1, 2).cpu() for k in ("Y1", "Y2")]
    del saved, net, xd
    _free()
    ref = R.RefIPDnet(16, 256, 2, online)
    ref.load_state_dict(R.state_tensors(sd))
    ref = ref.double().train()
    masks = [m.double() for m in R.site_masks(base, 1, nt, nf, b0=u)]
    pr = ref(torch.from_numpy(x[u:u + 1]).double(), masks, relu)
    (pr[0] * torch.from_numpy(G).double()).sum().backward()
    model = "online" if online else "offline"
    print("CHECK %s ReLU branches that differ from float64's (count, largest |input| there / largest |input|): %s"
          % (model, ref.conv.mask_flips))
    assert all(n <= 64 and r <= 1e-5 for n, r in ref.conv.mask_flips), ref.conv.mask_flips
    assert_close(pu, pr[0].detach().numpy(), 1e-4, 1e-5, "prediction of utterance %d" % u)
    for k, p in ref.named_parameters():
        rel_err(got[k], p.grad, 5e-4, "%s grad %s" % (model, k))


@pytest.mark.parametrize("online", [True, False], ids=["online", "offline"])
def test_config3_whole_batch_equals_sum_of_single_utterances(dev, online):
    """The gradient of a whole-batch loss sum_u <pred[u], G[u]> at config 3 equals the sum of the 16 single-utterance
    runs (utt_offset = u: same dropout masks): ties the full-size kernels to the small-batch path, and catches any leak
    between utterances (which the sampled-utterance check cannot see)."""
    nb, nf, nt = 16, 256, 300
    x = torch.from_numpy(rs_randn(2601, (nb, 16, nf, nt), 0.5)).to(dev)
    G = torch.from_numpy(rs_randn(2602, (nb, nt // 12, 2 * nf, 7, 2))).to(dev)

    def grads(parts):
        _, net = _config3_net(dev, online, 2600 + online, 57)
        for lo, hi in parts:
            net.utt_offset = lo
            (net(x[lo:hi]) * G[lo:hi]).sum().backward()
        g = {k: p.grad.clone() for k, p in net.named_parameters()}
        del net
        _free()
        return g

    one = grads([(0, nb)])
    parts = grads([(u, u + 1) for u in range(nb)])
    model = "online" if online else "offline"
    for k in one:
        rel_err(parts[k], one[k], 2e-5, "%s sum of 16 utterances, grad %s" % (model, k))


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
