"""Training of the f-conv branch, the full-band branch and a whole IPDnet2 SpatialNetLayer on the device
(csrc/spatialnet_layer_train.hip and csrc/spatialnet_train.hip through fnssl.spatialnet_train and
IPDnet2.IPDnet2.SpatialNetLayer) against the float64 autograd restatement of tests/layer_train_ref.py.

Every leg of R.legs(group) compares every gradient of its group (x + 5, x + 8, x + 40 parameters) with float64:
max|got - f64| / max|f64| <= 8 x the float32 restatement's own figure (R.GATE_F32: per tensor the largest over the legs of
the group, measured on the host, re-measured by test_layer_train_ref_host.py — none is chosen from what the kernels give).
Figures are printed before they are asserted.  Weights: fnssl.weights.make_ipdnet2_state; inputs: R.leg_inputs (no PReLU
input within 1e-4 of zero)."""
import ctypes as C
import functools

import numpy as np
import pytest

import layer_train_ref as R

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
    return W.make_ipdnet2_state(0, num_layers=2)


LEGS = {(g, l[0]): l for g in R.GROUPS for l in R.legs(g)}
IDS = ["%s-%s" % k for k in LEGS]


@functools.lru_cache(maxsize=None)
def inputs(key):
    """(parameters, x, dout) of a leg — computed once per leg, shared, never modified."""
    p = R.leg_params(key[0], LEGS[key], state())
    return (p,) + R.leg_inputs(key[0], LEGS[key], p)


@functools.lru_cache(maxsize=None)
def reference(key):
    """(out, gradients) of a leg in float64 — computed once per leg, shared, never modified."""
    p, x, dout = inputs(key)
    return R.gradients(key[0], LEGS[key], p, x, dout)


def make_layer(dev, p=None, nf=16, is_first=False):
    """A SpatialNetLayer on the device, holding ``p`` (R.LAYER_PARAMS' names) or, partially, the names of p it has."""
    import IPDnet2.IPDnet2 as M
    layer = M.SpatialNetLayer(dim_hidden=96, dim_squeeze=8, num_freqs=nf, dropout=(0, 0, 0), kernel_size=(5, 3),
                              conv_groups=(8, 8), norms=["LN"] * 6, attention="mamba(16,4)", is_first=is_first)
    if p is None:
        p = R.leg_params("layer", ("", 1, nf * (2 if is_first else 1), 1, is_first, 1, "frame", None), state())
    layer.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in p.items()}, strict=False)
    return layer.to(dev)


def place(x, layout, dev):
    """x [B, F, T, H] on the device, stored frame-major ([B, T, F, H]) or plainly contiguous."""
    t = torch.from_numpy(x).to(dev)
    if layout == "frame":
        t = t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    return t.requires_grad_(True)


def device_gradients(key, dev):
    from fnssl import spatialnet_train as T
    group, leg = key[0], LEGS[key]
    p, x, dout = inputs(key)
    xd = place(x, leg[6], dev)
    if group == "fconv":
        layer = make_layer(dev, {"fconv1." + k: v for k, v in p.items()})
        named = {k: layer.fconv1.get_parameter(k) for k in R.FCONV_PARAMS}
        out = T.fconv_train(xd, layer.fconv1, residual=leg[5], pool=leg[4])
    elif group == "full":
        layer = make_layer(dev, p, nf=leg[2])
        named = {k: layer.get_parameter(k) for k in R.FULL_PARAMS}
        out = T.full_train(xd, layer, residual=leg[5])
    else:
        layer = make_layer(dev, p, nf=leg[2] // 2 if leg[4] else leg[2], is_first=leg[4])
        named = {k: layer.get_parameter(k) for k in R.LAYER_PARAMS}
        out = T.layer_train(layer, xd, time_pool=leg[5])
    assert out.grad_fn is not None
    out.backward(torch.from_numpy(dout).to(dev))
    torch.cuda.synchronize()
    g = {"x": xd.grad}
    g.update({k: v.grad for k, v in named.items()})
    return out.detach(), g


def check_leg(key, got_out, got):
    want_out, want = reference(key)
    ok = True
    name = "%s/%s" % key
    e = R.rel_err(got_out.cpu().numpy(), want_out)
    print("%-28s %-28s err %.3e" % (name, "out (forward)", e))
    for k in R.TENSORS[key[0]]:
        assert got[k] is not None, k
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape, (k, g.shape, want[k].shape)
        assert np.isfinite(g).all(), k
        e, gate = R.rel_err(g, want[k]), R.gate(key[0], k)
        print("%-28s %-28s err %.3e  gate %.3e  (max|f64| %.3e)%s" % (name, k, e, gate, np.abs(want[k]).max(),
                                                                     "" if e <= gate else "   <-- FAIL"))
        ok &= e <= gate
    return ok


@pytest.mark.parametrize("key", list(LEGS), ids=IDS)
def test_gradients_vs_float64(dev, key):
    out, g = device_gradients(key, dev)
    assert check_leg(key, out, g), "%s/%s: a gradient misses its gate (figures above)" % key


@pytest.mark.parametrize("key", [("fconv", "f16_real"), ("fconv", "f256_300blocks"), ("full", "f16_real"),
                                 ("full", "f128_300frames")], ids=lambda k: "%s-%s" % k)
def test_real_length_twice_is_bitwise_equal(dev, key):
    _, a = device_gradients(key, dev)
    _, b = device_gradients(key, dev)
    for k in R.TENSORS[key[0]]:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("key", [("fconv", "f16_real"), ("fconv", "f128_pool8"), ("fconv", "f8_1frame_branch"),
                                 ("full", "f128_300frames"), ("full", "f32_branch"), ("layer", "later_layer"),
                                 ("layer", "first_layer")], ids=lambda k: "%s-%s" % k)
def test_train_forward_is_the_eval_forward_bitwise(dev, key):
    group, leg = key[0], LEGS[key]
    out, _ = device_gradients(key, dev)
    p, x, _ = inputs(key)
    xd = place(x, leg[6], dev).detach()
    with torch.no_grad():
        if group == "fconv":
            from fnssl import spatialnet as sn
            layer = make_layer(dev, {"fconv1." + k: v for k, v in p.items()}).eval()
            want = sn.fconv(xd, layer._packed(dev)[0], residual=leg[5], pool=leg[4])
        elif group == "full":
            from fnssl import spatialnet as sn
            layer = make_layer(dev, p, nf=leg[2]).eval()
            want = sn.full(xd, layer._packed(dev)[1], residual=leg[5])
        else:
            layer = make_layer(dev, p, nf=leg[2] // 2 if leg[4] else leg[2], is_first=leg[4]).eval()
            want = layer(xd)[0]
    assert torch.equal(out, want)


@pytest.mark.parametrize("which", ["point_lo", "point_hi"])
def test_single_point_reaches_exactly_the_rows_of_its_taps(dev, which):
    """dout is zero except one (b, t, f) point at the edge of the band: without the residual path's own row, dx is non-zero
    exactly in the 3 rows of that frame that the 5 taps reach inside [0, nf)."""
    key = ("fconv", "f16_" + which)
    _, g = device_gradients(key, dev)
    dx, nf = g["x"].cpu().numpy(), LEGS[key][2]
    rows = np.abs(dx).max(-1) != 0                           # [B, F, T]
    want = np.zeros_like(rows)
    want[0, slice(0, 3) if which == "point_lo" else slice(nf - 3, nf), 1] = True
    assert np.array_equal(rows, want)
    assert np.array_equal(np.abs(reference(key)[1]["x"]).max(-1) != 0, want)


def test_frames_past_the_last_time_window_get_exactly_zero(dev):
    key = ("layer", "later_layer_tpool5")
    _, g = device_gradients(key, dev)
    dx = g["x"]
    assert (dx[:, :, 10:] == 0).all() and (dx[:, :, :10] != 0).any()
    assert (reference(key)[1]["x"][:, :, 10:] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ #
# through the module
# ------------------------------------------------------------------------------------------------------------------ #
def _x(dev, nf=16, nt=5, seed=2):
    return place(np.random.RandomState(seed).standard_normal((2, nf, nt, R.H)).astype(np.float32), "frame", dev)


@pytest.mark.parametrize("which", ["fconv1", "fconv2", "full"])
def test_module_branch_trains(dev, which):
    layer = make_layer(dev).train()
    x = _x(dev)
    if which == "full":
        own = [layer.get_parameter(k) for k in R.FULL_PARAMS]
        call = lambda: layer._full(x)   # noqa: E731
    else:
        own = list(getattr(layer, which).parameters())
        call = lambda: layer._fconv(getattr(layer, which), x)   # noqa: E731
    y = call()
    assert y.grad_fn is not None and y.shape == x.shape
    y.backward(torch.ones_like(y))
    with_grad = {id(p) for p in layer.parameters() if p.grad is not None}
    assert with_grad == {id(p) for p in own} and len(own) == (8 if which == "full" else 5) and x.grad is not None
    with torch.no_grad():
        assert call().grad_fn is None
        y_eval = call()
    assert torch.equal(y_eval, y.detach())                   # the branch without the residual, the same bits
    layer.eval()
    assert call().grad_fn is None and torch.equal(call(), y.detach())


def test_module_layer_trains_and_steps(dev):
    layer = make_layer(dev).train()
    x = _x(dev, nt=R.TC + 3)
    y = layer.forward_train(x)
    assert y.grad_fn is not None and y.shape == x.shape
    y.backward(torch.randn(y.shape, device=dev, generator=torch.Generator(dev).manual_seed(1)))
    params = list(layer.parameters())
    assert len(params) == len(R.LAYER_PARAMS) == 40 and all(p.grad is not None for p in params) and x.grad is not None
    assert all(torch.isfinite(p.grad).all() for p in params)
    with torch.no_grad():
        assert torch.equal(layer.eval()(x)[0], y.detach())
    # one optimiser step, then the forward uses the new weights, in train() and in eval() alike
    torch.optim.AdamW(layer.parameters(), lr=1e-2).step()
    y2 = layer.train().forward_train(x)
    assert not torch.equal(y2, y)
    with torch.no_grad():
        assert torch.equal(layer.eval()(x)[0], y2.detach()), "the eval forward after the step is the train forward's bits"


def test_module_modes(dev):
    layer = make_layer(dev)
    x = _x(dev)
    with pytest.raises(RuntimeError, match="eval"):
        layer.eval().forward_train(x)
    with pytest.raises(RuntimeError, match="forward-only"):
        layer.train()(x)
    layer = layer.bfloat16().train()
    with pytest.raises(RuntimeError, match="fp32"):
        layer._fconv(layer.fconv1, x)
    with pytest.raises(RuntimeError, match="fp32"):
        layer._full(x)
    with pytest.raises(RuntimeError, match="fp32"):
        layer.forward_train(x)
    from fnssl import spatialnet_train as T
    with pytest.raises(RuntimeError, match="fp32"):
        T.fconv_train(x, layer.fconv1)
    with pytest.raises(RuntimeError, match="fp32"):
        T.full_train(x.detach().bfloat16(), layer)


# ------------------------------------------------------------------------------------------------------------------ #
# the C entry points' argument checks
# ------------------------------------------------------------------------------------------------------------------ #
def _c_setup(dev, which, nf=16):
    from fnssl import _lib, spatialnet as sn
    lib = _lib.load()
    nb, nt = 1, 3
    layer = make_layer(dev, nf=nf)
    w = layer._packed(dev)[0 if which == "fconv" else 1]
    sizes = (96, 96, 5760, 96, 96) if which == "fconv" else (96, 96, 768, 8, nf * nf, nf, 768, 96)
    grads = [torch.zeros(n, device=dev) for n in sizes]
    x, dout, dx = (sn._new_bfth(nb, nf, nt, dev).normal_() for _ in range(3))
    nbytes = getattr(lib, "fnssl_sn_%s_backward_workspace_bytes" % which)(nb, nt, nf)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    return lib, layer, w, grads, sn._view(x), sn._view(dout), sn._view(dx), ws, (nb, nt, nf), (x, dout, dx)


@pytest.mark.parametrize("which", ["fconv", "full"])
def test_bad_arguments_return_errors(dev, which):
    from fnssl import _lib
    lib, layer, w, grads, xv, dv, gv, ws, (nb, nt, nf), keep = _c_setup(dev, which)
    G = _lib.SnFconvGrads if which == "fconv" else _lib.SnFullGrads

    def call(nf=nf, pool=1, gptrs=None, xview=None, dptr=None, gptr=None, wsp=True, wbytes=None, wnull=False, gnull=False):
        g = G(*(gptrs or [t.data_ptr() for t in grads]))
        head = (C.byref(xview or xv), nb, nt, nf, None if wnull else C.byref(w), 1)
        tail = (dptr or dv.p, dv.sb, dv.st, dv.sf, gptr or gv.p, gv.sb, gv.st, gv.sf, None if gnull else C.byref(g),
                ws.data_ptr() if wsp else None, ws.numel() if wbytes is None else wbytes, None)
        if which == "fconv":
            return lib.fnssl_sn_fconv_backward(*head, pool, *tail)
        return lib.fnssl_sn_full_backward(*head, *tail)

    def bad(needle, **kw):
        assert call(**kw) != 0, kw
        assert needle in lib.fnssl_last_error(), (kw, lib.fnssl_last_error())

    assert call() == 0
    for n in (12, 4, 512):
        bad(b"nf", nf=n)
    if which == "fconv":
        bad(b"pool", pool=3)
    ptrs = [t.data_ptr() for t in grads]
    for i in range(len(ptrs)):
        bad(b"(g)", gptrs=ptrs[:i] + [None] + ptrs[i + 1:])
    bad(b"(g)", gnull=True)
    bad(b"(w)", wnull=True)
    bad(b"dout", dptr=dv.p + 4)
    bad(b"dx", gptr=gv.p + 4)
    bad(b"x must", xview=_lib.BtfView(xv.p + 4, xv.sb, xv.st, xv.sf))
    bad(b"x must", xview=_lib.BtfView(xv.p, xv.sb + 2, xv.st, xv.sf))
    bad(b"workspace", wbytes=ws.numel() - 1)
    bad(b"workspace", wsp=False)
    torch.cuda.synchronize()
    del keep, layer
