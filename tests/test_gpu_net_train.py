"""Training of the IPDnet2 encoder, head, whole network and training step on the device (csrc/spatialnet_net_train.hip with
the layer's backwards, through fnssl.spatialnet_train, IPDnet2.IPDnet2.OnlineSpatialNet.forward_train and
IPDnet2.run_step.MyModel(train_on_device=True)) against the float64 autograd restatement of tests/net_train_ref.py.

Every leg of R.legs(group) compares every gradient of its group (encoder: dW, db and, where x requires it, dx; head: dx + 4;
net: all 2 + 40 L + 4 parameters) with float64: max|got - f64| / max|f64| <= 8 x the float32 restatement's own figure
(R.GATE_F32: per tensor the largest over the legs of the group, measured on the host, re-measured by
test_net_train_ref_host.py — none is chosen from what the kernels give).  Figures are printed before they are asserted.
Net inputs: R.net_input (drawn frame by frame, no PReLU input within 1e-4 of zero)."""
import ctypes as C
import functools

import numpy as np
import pytest

import net_train_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _state(cfg):
    from fnssl import weights as W
    return W.make_ipdnet2_state(0, **dict(cfg))


def state(key):
    return _state(tuple(sorted(R.net_cfg(LEGS[key]).items()))) if key[0] == "net" else None


LEGS = {(g, l[0]): l for g in R.GROUPS for l in R.legs(g)}
IDS = ["%s-%s" % k for k in LEGS]


def inputs(key):
    """(parameters, x, dout) of a leg — computed once per leg (R.leg_inputs caches), shared, never modified."""
    return R.leg_inputs(key[0], LEGS[key], state(key))


@functools.lru_cache(maxsize=None)
def reference(key):
    """(out, gradients) of a leg in float64 — computed once per leg, shared, never modified."""
    p, x, dout = inputs(key)
    return R.gradients(key[0], LEGS[key], p, x, dout)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def place_bfth(a, layout, dev):
    """a logical [B, F, T, H] on the device, stored frame-major ([B, T, F, H]) or plainly contiguous."""
    t = T(a, dev)
    return t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) if layout == "frame" else t


def make_net(dev, sd, leg):
    import IPDnet2.IPDnet2 as M
    net = M.OnlineSpatialNet(dim_input=leg[3], dim_output=16, num_layers=leg[1], dim_hidden=96, num_heads=4, kernel_size=(5, 3),
                             conv_groups=(8, 8), norms=["LN", "LN", "GN", "LN", "LN", "LN"], dim_squeeze=8, num_freqs=leg[2],
                             attention='mamba(16,4)', rope=False, time_compression_layer=0, fre_compression_ratio=16,
                             time_compression_ratio=5)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return net.to(dev)


def device_gradients(key, dev, x_grad=None):
    """(out, {tensor: gradient or None}) of a leg on the device; step leg: out = (prediction, loss)."""
    import IPDnet2.IPDnet2 as M
    from fnssl import ipdnet_step, spatialnet_train as ST
    group, leg = key[0], LEGS[key]
    p, x, dout = inputs(key)
    if group == "encoder":
        conv = M.CausalConv1d(leg[2], 96, 5)
        conv.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
        conv = conv.to(dev)
        xd = T(x, dev)
        if leg[5] == "tstride":                              # stored [B, C, T, F]: the time stride is nf
            xd = xd.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
            assert xd.stride(3) == leg[3] != 1
        xd.requires_grad_(leg[8])
        out = ST.encoder_train(xd, conv)
        named = {"weight": conv.weight, "bias": conv.bias}
        cot = place_bfth(dout, leg[6], dev)
    elif group == "head":
        fi = M.FreqInverse(nfreq=16 * leg[2], compression_ratio=16, hidden_dim=96, out_dim=16)
        dec = torch.nn.Linear(16, 16)
        fi.trans2.load_state_dict({"weight": torch.from_numpy(p[R.HEAD_PARAMS[0]]), "bias": torch.from_numpy(p[R.HEAD_PARAMS[1]])})
        dec.load_state_dict({"weight": torch.from_numpy(p[R.HEAD_PARAMS[2]]), "bias": torch.from_numpy(p[R.HEAD_PARAMS[3]])})
        fi, dec = fi.to(dev), dec.to(dev)
        xd = place_bfth(x, leg[4], dev).requires_grad_(True)
        out = ST.head_train(xd, fi, dec)
        named = dict(zip(R.HEAD_PARAMS, (fi.trans2.weight, fi.trans2.bias, dec.weight, dec.bias)))
        cot = T(dout, dev)
    else:
        net = make_net(dev, state(key), leg).train()
        xd = T(x, dev).requires_grad_(bool(x_grad))
        out = net.forward_train(xd)
        named = {k: net.get_parameter(k) for k in R.net_param_names(leg[1])}
        cot = T(dout, dev)
    assert out.grad_fn is not None
    if group == "net" and leg[6] == "step":
        cut = out[:, :cot.shape[1]]                          # a view: dpred is strided, the cut frame gets zero gradient
        loss = ipdnet_step.PitMSE.apply(cut, cot)
        loss.backward()
        out = out.detach()
    else:
        out.backward(cot)
    torch.cuda.synchronize()
    g = {"x": xd.grad}
    g.update({k: v.grad for k, v in named.items()})
    return out.detach(), g


def check_leg(key, got_out, got):
    want_out, want = reference(key)
    ok = True
    name = "%s/%s" % key
    e = R.rel_err(got_out.cpu().numpy(), want_out)
    print("%-26s %-40s err %.3e" % (name, "out (forward)", e))
    for k in R.tensors(key[0], LEGS[key]):
        assert got[k] is not None, k
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape, (k, g.shape, want[k].shape)
        assert np.isfinite(g).all(), k
        e, gate = R.rel_err(g, want[k]), R.gate(key[0], k)
        print("%-26s %-40s err %.3e  gate %.3e  (max|f64| %.3e)%s" % (name, k, e, gate, np.abs(want[k]).max(),
                                                                     "" if e <= gate else "   <-- FAIL"))
        ok &= e <= gate
    return ok


@pytest.mark.parametrize("key", list(LEGS), ids=IDS)
def test_gradients_vs_float64(dev, key):
    out, g = device_gradients(key, dev)
    if key[0] == "encoder" and not LEGS[key][8]:
        assert g["x"] is None, "dx is formed only where x requires a gradient"
    assert check_leg(key, out, g), "%s/%s: a gradient misses its gate (figures above)" % key


@pytest.mark.parametrize("key", [("encoder", "many_tiles"), ("head", "many"), ("net", "l2_f128_nt10")], ids=lambda k: "%s-%s" % k)
def test_twice_is_bitwise_equal(dev, key):
    _, a = device_gradients(key, dev)
    _, b = device_gradients(key, dev)
    for k in R.tensors(key[0], LEGS[key]):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("key", [k for k in LEGS if k[0] == "net"], ids=lambda k: "%s-%s" % k)
def test_train_forward_is_the_eval_forward_bitwise(dev, key):
    leg = LEGS[key]
    _, x, _ = inputs(key)
    net = make_net(dev, state(key), leg)
    xd = T(x, dev)
    out = net.train().forward_train(xd)
    assert out.grad_fn is not None and out.shape == (leg[4], leg[5] // 5, 2 * leg[2], 4, 2)
    with torch.no_grad():
        assert net.forward_train(xd).grad_fn is None
        want = net.eval()(xd)
    assert torch.equal(out.detach(), want)


def test_single_points_reach_exactly_their_taps(dev):
    """dout is one (b, f) point.  At t = 0 every tap but the last reads padding: dW[:, :, :4] is exactly 0.  At t = nt - 1
    dx is non-zero exactly in the last 5 frames of that (b, f) row."""
    _, g = device_gradients(("encoder", "point_t0"), dev)
    dw = g["weight"].cpu().numpy()
    assert (dw[:, :, :4] == 0).all() and (dw[:, :, 4] != 0).all()
    assert (reference(("encoder", "point_t0"))[1]["weight"][:, :, :4] == 0).all()
    key = ("encoder", "point_tlast")
    _, g = device_gradients(key, dev)
    nz = g["x"].cpu().numpy() != 0                             # [B, C, F, T]
    want = np.zeros_like(nz)
    want[0, :, 3, LEGS[key][4] - 5:] = True
    assert np.array_equal(nz, want) and np.array_equal(reference(key)[1]["x"] != 0, want)


def test_single_output_element_lands_on_its_decoder_row(dev):
    """(2f + gg, m, a) = (last, 3, 1) is decoder output j = a*8 + gg*4 + m = 15 of the last fine bin of the last frame."""
    key = ("head", "element_last")
    _, g = device_gradients(key, dev)
    db = g["decoder.bias"].cpu().numpy()
    assert db[15] != 0 and (db[:15] == 0).all()
    dwd = g["decoder.weight"].cpu().numpy()
    assert (dwd[:15] == 0).all() and (dwd[15] != 0).all()
    dx = g["x"].cpu().numpy()                                  # [B, Fc, T', H]: only the last compressed bin of the last frame
    nz = np.abs(dx).max(-1) != 0
    want = np.zeros_like(nz)
    want[0, -1, -1] = True
    assert np.array_equal(nz, want)
    dbfi = g["freq_inverse.trans2.bias"].cpu().numpy().reshape(16, 16)      # [o, r]: fine bin r = 15 alone
    assert (dbfi[:, :15] == 0).all() and (dbfi[:, 15] != 0).all()


def test_saturated_head_is_finite_and_exactly_zero_where_tanh_is_one(dev):
    key = ("head", "saturated")
    _, g = device_gradients(key, dev)
    for k, v in g.items():
        assert torch.isfinite(v).all(), k
    dx = g["x"].cpu().numpy().reshape(-1, R.H)                 # points in (b, fc, t2) order, as R.leg_inputs scaled them
    assert (dx[2::3] == 0).all(), "min|u| = 20: every tanh of the point is +-1, dx is exactly 0"
    assert (dx[0::3] != 0).any() and (dx[1::3] != 0).any()


def test_tail_frames_get_exactly_zero(dev):
    """nt = 12: frames 10 and 11 reach no pooled frame; with x requiring a gradient, dx of the tail is exactly zero."""
    key = ("net", "l2_f128_nt12")
    _, g = device_gradients(key, dev, x_grad=True)
    dx = g["x"]
    assert dx is not None and (dx[:, :, :, 10:] == 0).all() and (dx[:, :, :, :10] != 0).any()
    want = reference(key)[1]["x"]
    print("net/l2_f128_nt12 x err %.3e (printed, not gated: the features carry no gradient in training)" % R.rel_err(dx.cpu().numpy(), want))
    assert (want[:, :, :, 10:] == 0).all()


def test_step_cut_frame_gets_zero_gradient(dev):
    key = ("net", "step")
    from fnssl import ipdnet_step
    leg = LEGS[key]
    p, x, gt = inputs(key)
    net = make_net(dev, state(key), leg).train()
    pred = net.forward_train(T(x, dev))
    pred.retain_grad()
    loss = ipdnet_step.PitMSE.apply(pred[:, :gt.shape[1]], T(gt, dev))
    assert loss.grad_fn is not None
    loss.backward()
    assert (pred.grad[:, gt.shape[1]:] == 0).all() and (pred.grad[:, :gt.shape[1]] != 0).any()
    want_pred, _ = reference(key)
    want_loss = float(R.pit_mse(torch.tensor(want_pred[:, :gt.shape[1]]), torch.tensor(gt.astype(np.float64)))[0])
    print("step loss %.9e  float64 %.9e" % (float(loss.detach()), want_loss))
    assert torch.isfinite(loss)


# ------------------------------------------------------------------------------------------------------------------ #
# through the modules
# ------------------------------------------------------------------------------------------------------------------ #
def test_module_modes(dev):
    key = ("net", "l2_f128_nt10")
    leg = LEGS[key]
    x = T(inputs(key)[1], dev)
    net = make_net(dev, state(key), leg)
    with pytest.raises(RuntimeError, match="eval"):
        net.eval().forward_train(x)
    with pytest.raises(RuntimeError, match="forward-only"):
        net.train()(x)
    with pytest.raises(RuntimeError, match="expected"):
        net.forward_train(x[:, :3])
    with pytest.raises(RuntimeError, match="expected"):
        net.forward_train(x[:, :, :64])
    with pytest.raises(RuntimeError, match="fp32"):
        net.forward_train(x.bfloat16())
    with torch.no_grad():
        assert net.forward_train(x).grad_fn is None
    net = net.bfloat16().train()
    with pytest.raises(RuntimeError, match="fp32"):
        net.forward_train(x)


def test_my_model_trains_on_device(dev):
    from fnssl import weights as W
    from test_gpu_ipdnet2_eval import _batch, run_step
    RS = run_step()
    leg = ("arch", 2, 256, 10)
    sd = W.make_ipdnet2_state(4601, num_layers=2)
    model = RS.MyModel(device="cuda:0", arch=make_net(dev, sd, leg), train_on_device=True).to(dev)
    batch = [x.to(dev) for x in _batch(10)]
    model.eval()
    with torch.no_grad():
        want = model.validation_step(batch, 0)
    model.train()
    loss = model.training_step(batch, 0)["loss"]
    assert loss.grad_fn is not None and loss.shape == () and torch.equal(loss.detach(), want)
    loss.backward()
    params = list(model.arch.parameters())
    assert len(params) == 2 + 40 * 2 + 4
    for name, q in model.arch.named_parameters():
        assert q.grad is not None and torch.isfinite(q.grad).all() and (q.grad != 0).any(), name
    before = [q.detach().clone() for q in params]
    opt = model.configure_optimizers()["optimizer"]
    assert isinstance(opt, torch.optim.AdamW)
    opt.step()
    for (name, q), b in zip(model.arch.named_parameters(), before):
        assert not torch.equal(q.detach(), b), name
    opt.zero_grad()
    loss2 = model.training_step(batch, 0)["loss"]
    assert torch.isfinite(loss2) and not torch.equal(loss2.detach(), loss.detach())
    # the prediction longer than the targets: cut, still differentiable
    short = model.training_step([x.to(dev) for x in _batch(8)], 0)["loss"]
    assert short.grad_fn is not None and torch.isfinite(short)
    # the default stays forward-only in train()
    plain = RS.MyModel(device="cuda:0", arch=make_net(dev, sd, leg)).to(dev).train()
    with pytest.raises(Exception, match="(?i)forward-only"):
        plain.training_step(batch, 0)
    # cal_loss without a gradient is what it was: no grad_fn, the same bits
    with torch.no_grad():
        pred, gt = model.eval()._forward_aligned(batch)
    a = model.cal_loss(pred_batch=pred, gt_batch=gt)
    assert a.grad_fn is None


# ------------------------------------------------------------------------------------------------------------------ #
# the C entry points' argument checks
# ------------------------------------------------------------------------------------------------------------------ #
def test_encoder_backward_bad_arguments_return_errors(dev):
    from fnssl import _lib, spatialnet as sn
    lib = _lib.load()
    nb, cin, nf, nt = 1, 10, 8, 6
    x = torch.randn(nb, cin, nf, nt, device=dev)
    wT, dwT, db = torch.randn(cin, 5, 96, device=dev), torch.zeros(cin, 5, 96, device=dev), torch.zeros(96, device=dev)
    dout, dx = sn._new_bfth(nb, nf, nt, dev).normal_(), torch.zeros_like(x)
    dv = sn._view(dout)
    ws = torch.zeros(lib.fnssl_sn_encoder_backward_workspace_bytes(nb, cin, nf, nt), dtype=torch.uint8, device=dev)
    assert ws.numel() > 0 and lib.fnssl_sn_encoder_backward_workspace_bytes(0, cin, nf, nt) == 0

    def call(xp=x.data_ptr(), nt_=nt, w=wT.data_ptr(), dp=dv.p, dsb=dv.sb, dw=dwT.data_ptr(), dbp=db.data_ptr(), dxp=dx.data_ptr(),
             wsp=ws.data_ptr(), wbytes=ws.numel()):
        return lib.fnssl_sn_encoder_backward(xp, *x.stride(), nb, cin, nf, nt_, w, dp, dsb, dv.st, dv.sf, dw, dbp, dxp, *dx.stride(),
                                             wsp, wbytes, None)

    def bad(needle, **kw):
        assert call(**kw) != 0, kw
        assert needle in lib.fnssl_last_error(), (kw, lib.fnssl_last_error())

    assert call() == 0 and call(dxp=None, w=None) == 0
    bad(b"null", xp=None)
    bad(b"null", dw=None)
    bad(b"null", dbp=None)
    bad(b"empty", nt_=0)
    bad(b"dout", dp=dv.p + 4)
    bad(b"dout", dp=None)
    bad(b"dout", dsb=dv.sb + 2)
    bad(b"dx needs", w=None)
    bad(b"workspace", wbytes=ws.numel() - 1)
    bad(b"workspace", wsp=None)
    torch.cuda.synchronize()


def test_head_backward_bad_arguments_return_errors(dev):
    from fnssl import _lib, spatialnet as sn
    lib = _lib.load()
    nb, nt2, nfc = 1, 2, 2
    x, dx = sn._new_bfth(nb, nfc, nt2, dev).normal_(), sn._new_bfth(nb, nfc, nt2, dev)
    w = [torch.randn(n, device=dev) for n in (16 * 16 * 96, 256, 256)]
    grads = [torch.zeros(n, device=dev) for n in (16 * 16 * 96, 256, 256, 16)]
    dout = torch.randn(nb, nt2, 32 * nfc, 4, 2, device=dev)
    xv, gv = sn._view(x), sn._view(dx)
    ws = torch.zeros(lib.fnssl_sn_head_backward_workspace_bytes(nb, nt2, nfc), dtype=torch.uint8, device=dev)
    assert ws.numel() > 0 and lib.fnssl_sn_head_backward_workspace_bytes(nb, 0, nfc) == 0

    def call(xview=xv, nt2_=nt2, wp=None, dp=dout.data_ptr(), gp=gv.p, gptrs=None, gnull=False, wsp=ws.data_ptr(), wbytes=ws.numel()):
        g = _lib.SnHeadGrads(*(gptrs or [t.data_ptr() for t in grads]))
        wp = wp or [t.data_ptr() for t in w]
        return lib.fnssl_sn_head_backward(C.byref(xview), nb, nt2_, nfc, *wp, dp, gp, gv.sb, gv.st, gv.sf,
                                          None if gnull else C.byref(g), wsp, wbytes, None)

    def bad(needle, **kw):
        assert call(**kw) != 0, kw
        assert needle in lib.fnssl_last_error(), (kw, lib.fnssl_last_error())

    assert call() == 0
    ptrs = [t.data_ptr() for t in grads]
    for i in range(4):
        bad(b"(g)", gptrs=ptrs[:i] + [None] + ptrs[i + 1:])
    bad(b"(g)", gnull=True)
    wptrs = [t.data_ptr() for t in w]
    for i in range(3):
        bad(b"weights", wp=wptrs[:i] + [None] + wptrs[i + 1:])
    bad(b"empty", nt2_=0)
    bad(b"dout", dp=None)
    bad(b"dout", dp=dout.data_ptr() + 4)
    bad(b"dx", gp=gv.p + 4)
    bad(b"x must", xview=_lib.BtfView(xv.p + 4, xv.sb, xv.st, xv.sf))
    bad(b"workspace", wbytes=ws.numel() - 1)
    bad(b"workspace", wsp=None)
    torch.cuda.synchronize()
