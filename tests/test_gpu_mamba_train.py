"""Training of one IPDnet2 Mamba block on the device (csrc/spatialnet_train.hip through fnssl.spatialnet_train and
IPDnet2.IPDnet2.SpatialNetLayer._mamba) against the float64 autograd restatement of tests/mamba_train_ref.py.

Every leg of R.legs() compares all 12 gradients (x + 11 parameters) with float64: max|got - f64| / max|f64| <= 8 x the
float32 restatement's own figure (R.GATE_F32: per tensor the largest over all legs, measured on the host, re-measured by
test_mamba_train_ref_host.py — none is chosen from what the kernels give).  Figures are printed before they are asserted.
Weights: fnssl.weights.make_ipdnet2_state; the chunk legs are placed around fnssl_sn_mamba_backward_chunk()."""
import functools

import numpy as np
import pytest

import mamba_train_ref as R

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
def state():
    from fnssl import weights as W
    return W.make_ipdnet2_state(0, num_layers=1)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(out, gradients) of a leg in float64 — computed once per leg, shared, never modified."""
    leg = LEGS[name]
    p = R.block_params(state(), bias_shift=leg[7])
    x, dout = R.leg_inputs(leg)
    return R.gradients(p, x, dout, leg[5], leg[4])


LEGS = {l[0]: l for l in R.legs()}


def modules(dev, bias_shift=0.0):
    """(LayerNorm, Mamba) holding the block's parameters on the device."""
    import IPDnet2.IPDnet2 as M
    p = R.block_params(state(), bias_shift=bias_shift)
    norm, mamba = M.LayerNorm(seq_last=False, normalized_shape=R.H), M.Mamba(R.H, R.NST, R.KC)
    norm.load_state_dict({"weight": torch.from_numpy(p["norm.weight"]), "bias": torch.from_numpy(p["norm.bias"])})
    mamba.load_state_dict({k: torch.from_numpy(p[k]) for k in R.PARAMS})
    return norm.to(dev), mamba.to(dev)


def place(x, layout, dev):
    """x [B, F, T, H] on the device, stored frame-major ([B, T, F, H]) or plainly contiguous."""
    t = torch.from_numpy(x).to(dev)
    if layout == "frame":
        t = t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    return t.requires_grad_(True)


def device_gradients(name, dev):
    from fnssl import spatialnet_train as T
    leg = LEGS[name]
    _, nb, nf, nt, pool, res, layout, shift = leg
    norm, mamba = modules(dev, shift)
    x, dout = R.leg_inputs(leg)
    xd = place(x, layout, dev)
    out = T.mamba_train(xd, norm, mamba, residual=res, time_pool=pool)
    out.backward(torch.from_numpy(dout).to(dev))
    torch.cuda.synchronize()
    g = {"x": xd.grad, "norm.weight": norm.weight.grad, "norm.bias": norm.bias.grad}
    g.update({k: v.grad for k, v in mamba.named_parameters()})
    return out.detach(), g


def check_leg(name, got_out, got):
    want_out, want = reference(name)
    ok = True
    e = R.rel_err(got_out.cpu().numpy(), want_out) if want_out.size else 0.0
    print("%-24s %-16s err %.3e" % (name, "out (forward)", e))
    for k in R.TENSORS:
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape, (k, g.shape, want[k].shape)
        assert np.isfinite(g).all(), k
        e, gate = R.rel_err(g, want[k]), R.gate(k)
        print("%-24s %-16s err %.3e  gate %.3e  (max|f64| %.3e)%s" % (name, k, e, gate, np.abs(want[k]).max(),
                                                                     "" if e <= gate else "   <-- FAIL"))
        ok &= e <= gate
    return ok


def test_chunk_is_the_one_the_tables_were_measured_for(dev):
    from fnssl import spatialnet_train as T
    assert T.backward_chunk() == R.TC, "re-measure R.GATE_F32 with legs placed around the new chunk"


@pytest.mark.parametrize("name", list(LEGS))
def test_gradients_vs_float64(dev, name):
    out, g = device_gradients(name, dev)
    assert check_leg(name, out, g), "%s: a gradient misses its gate (figures above)" % name


def test_frames_past_the_last_window_get_exactly_zero(dev):
    _, g = device_gradients("pooled_nt12", dev)
    dx = g["x"]
    assert (dx[:, :, 10:] == 0).all() and (dx[:, :, :10] != 0).any()
    _, want = reference("pooled_nt12")
    assert (want["x"][:, :, 10:] == 0).all()


def test_real_length_twice_is_bitwise_equal(dev):
    _, a = device_gradients("real_pool5", dev)
    _, b = device_gradients("real_pool5", dev)
    for k in R.TENSORS:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["real_pool1", "real_pool5", "short_nt3_branch_plain"])
def test_train_forward_is_the_eval_forward_bitwise(dev, name):
    from fnssl import spatialnet as sn
    leg = LEGS[name]
    out, _ = device_gradients(name, dev)
    p = R.block_params(state(), bias_shift=leg[7])
    sd = {"n.weight": p["norm.weight"], "n.bias": p["norm.bias"]}
    sd.update({"m." + k: p[k] for k in R.PARAMS})
    w, keep = sn.pack_mamba(sd, "n", "m", dev)
    x, _ = R.leg_inputs(leg)
    with torch.no_grad():
        want = sn.mamba(place(x, leg[6], dev).detach(), w, residual=leg[5], time_pool=leg[4])
    del keep
    assert torch.equal(out, want)


def test_bad_arguments_return_errors(dev):
    import ctypes as C
    from fnssl import _lib, spatialnet as sn
    lib = _lib.load()
    nb, nf, nt = 1, 2, 4
    x = sn._new_bfth(nb, nf, nt, dev).normal_()
    p = R.block_params(state())
    sd = {"n.weight": p["norm.weight"], "n.bias": p["norm.bias"]}
    sd.update({"m." + k: p[k] for k in R.PARAMS})
    w, keep = sn.pack_mamba(sd, "n", "m", dev)
    ws = torch.zeros(lib.fnssl_sn_mamba_workspace_bytes(nb, nt, nf), dtype=torch.uint8, device=dev)
    bws = torch.zeros(lib.fnssl_sn_mamba_backward_workspace_bytes(nb, nt, nf), dtype=torch.uint8, device=dev)
    grads = [torch.zeros(n, device=dev) for n in (96, 96, 96 * 384, 192 * 4, 192, 192 * 40, 192 * 6, 192, 192 * 16, 192, 192 * 96)]
    dout, dx = sn._new_bfth(nb, nf, nt, dev).normal_(), sn._new_bfth(nb, nf, nt, dev)
    xv, dv, gv = sn._view(x), sn._view(dout), sn._view(dx)

    def call(pool=1, gptrs=None, fbytes=None, dptr=None, bbytes=None):
        g = _lib.SnMambaGrads(*(gptrs or [t.data_ptr() for t in grads]))
        return lib.fnssl_sn_mamba_backward(C.byref(xv), nb, nt, nf, C.byref(w), 1, pool, ws.data_ptr(),
                                           ws.numel() if fbytes is None else fbytes, dptr or dv.p, dv.sb, dv.st, dv.sf, gv.p,
                                           gv.sb, gv.st, gv.sf, C.byref(g), bws.data_ptr(),
                                           bws.numel() if bbytes is None else bbytes, None)

    assert call(pool=0) != 0 and call(pool=17) != 0
    assert b"time_pool" in lib.fnssl_last_error()
    ptrs = [t.data_ptr() for t in grads]
    for i in range(len(ptrs)):
        assert call(gptrs=ptrs[:i] + [None] + ptrs[i + 1:]) != 0, i
    assert call(fbytes=ws.numel() - 4) != 0 and call(fbytes=ws.numel() + 4) != 0
    assert call(dptr=dv.p + 4) != 0
    assert call(bbytes=bws.numel() - 1) != 0
    torch.cuda.synchronize()
    del keep


# ------------------------------------------------------------------------------------------------------------------ #
# through the module
# ------------------------------------------------------------------------------------------------------------------ #
def make_layer(dev):
    import IPDnet2.IPDnet2 as M
    layer = M.SpatialNetLayer(dim_hidden=96, dim_squeeze=8, num_freqs=16, dropout=(0, 0, 0), kernel_size=(5, 3),
                              conv_groups=(8, 8), norms=["LN"] * 6, attention="mamba(16,4)", is_first=False)
    sd = state()
    layer.load_state_dict({k[len("layers.0."):]: torch.from_numpy(np.array(v)) for k, v in sd.items()
                           if k.startswith("layers.0.") and not k.startswith("layers.0.full.")}, strict=False)
    return layer.to(dev)


@pytest.mark.parametrize("which", ["mhsa", "tconvffn"])
def test_module_branch_trains(dev, which):
    from fnssl import spatialnet_train as T
    layer = make_layer(dev).train()
    mamba, norm = getattr(layer, which), getattr(layer, "norm_" + which)
    block = {id(p) for p in list(mamba.parameters()) + list(norm.parameters())}
    rs = np.random.RandomState(11)
    x = place(rs.standard_normal((2, 3, R.TC + 3, R.H)).astype(np.float32), "frame", dev)
    dout = torch.from_numpy(rs.standard_normal((2, 3, R.TC + 3, R.H)).astype(np.float32)).to(dev)
    y = layer._mamba(x, mamba, norm, layer.dropout_mhsa)
    assert y.grad_fn is not None and y.shape == x.shape
    y.backward(dout)
    with_grad = {id(p) for p in layer.parameters() if p.grad is not None}
    assert with_grad == block and len(block) == 11 and x.grad is not None
    # the function-level result (branch without the residual)
    x2 = x.detach().clone().requires_grad_(True)
    norm2, mamba2 = modules(dev)
    norm2.load_state_dict(norm.state_dict())
    mamba2.load_state_dict(mamba.state_dict())
    y2 = T.mamba_train(x2, norm2, mamba2, residual=False)
    y2.backward(dout)
    assert torch.equal(y, y2) and torch.equal(x.grad, x2.grad)
    for (k, a), (_, b) in zip(list(mamba.named_parameters()) + list(norm.named_parameters()),
                              list(mamba2.named_parameters()) + list(norm2.named_parameters())):
        assert torch.equal(a.grad, b.grad), k
    # one optimiser step, then the forward uses the new weights
    opt = torch.optim.AdamW(layer.parameters(), lr=1e-2)
    opt.step()
    y3 = layer._mamba(x, mamba, norm, layer.dropout_mhsa)
    assert not torch.equal(y3, y)
    with torch.no_grad():
        y4 = layer.eval()._mamba(x, mamba, norm, layer.dropout_mhsa)
    assert torch.equal(y3.detach(), y4), "the eval forward after the step is the train forward's bits"


def test_module_modes(dev):
    layer = make_layer(dev)
    x = place(np.random.RandomState(2).standard_normal((1, 3, 5, R.H)).astype(np.float32), "frame", dev)
    y = layer.eval()._mamba(x, layer.mhsa, layer.norm_mhsa, layer.dropout_mhsa)
    assert y.grad_fn is None
    with torch.no_grad():
        assert layer.train()._mamba(x, layer.mhsa, layer.norm_mhsa, layer.dropout_mhsa).grad_fn is None
    with pytest.raises(RuntimeError, match="forward-only"):
        layer.train()(x)
    with pytest.raises(RuntimeError, match="inference=True"):
        layer.train()._mamba(x, layer.mhsa, layer.norm_mhsa, layer.dropout_mhsa, inference=True)
    with pytest.raises(RuntimeError, match="fp32"):
        layer.bfloat16().train()._mamba(x, layer.mhsa, layer.norm_mhsa, layer.dropout_mhsa)
