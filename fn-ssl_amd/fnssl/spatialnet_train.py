"""Training front of one IPDnet2 layer: ``torch.autograd`` around the forward entry points ``fnssl_sn_mamba`` /
``fnssl_sn_fconv`` / ``fnssl_sn_full`` and their backwards ``fnssl_sn_mamba_backward`` / ``fnssl_sn_fconv_backward`` /
``fnssl_sn_full_backward``, and around the network's two ends, ``fnssl_sn_encoder`` / ``fnssl_sn_head`` with
``fnssl_sn_encoder_backward`` / ``fnssl_sn_head_backward`` (include/fnssl.h).  fp32, whole sequences from zero state, ROCm
tensors only.

    y = mamba_train(x, norm, mamba, residual=True, time_pool=1)      # x logical [B, F, T, 96]
    y.backward(...)   # fills x.grad and the .grad of the LayerNorm's 2 and the Mamba's 9 parameters
    y = fconv_train(x, ml, residual=True, pool=1)                    # ml = ModuleList(LN, Conv1d, PReLU): 5 parameters
    y = full_train(x, layer, residual=True)                          # norm_full, squeeze, full, unsqueeze: 8 parameters
    y = layer_train(layer, x, time_pool=1)                           # the five branches of a SpatialNetLayer: 40
    y = encoder_train(x, conv)                                       # x [B, C, F, T] -> logical [B, F, T, 96]: 2
    y = head_train(x, freq_inverse, decoder)                         # logical [B, Fc, T', 96] -> [B, T', 2F, 4, 2]: 4
    y = net_train(net, x)                                            # a whole OnlineSpatialNet: 2 + 40 L + 4

Every forward is the inference call itself (same kernels, same bits).  The Mamba block saves the forward's workspace
(xz | dbl | y) plus x; the f-conv and full-band branches are local to a frame and save x alone, and so do the encoder and
the head.  ``net_train`` chains them: the prediction has the bits of ``net.eval()(x)`` and a ``grad_fn`` that reaches
every parameter of the network.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import SnFconvGrads, SnFconvW, SnFullGrads, SnFullW, SnHeadGrads, SnMambaGrads, SnMambaW, check
from .ops import _need_dev, _ptr, _stream
from .spatialnet import (DO, E, FP32, H, HS, KC, NST, RK, _conform, _new_bfth, _view, encoder, head, pack_fconv, pack_full,
                         pack_head, pack_mamba)

PARAMS = ("in_proj.weight", "conv1d.weight", "conv1d.bias", "x_proj.weight", "dt_proj.weight", "dt_proj.bias", "A_log", "D",
          "out_proj.weight")


def backward_chunk() -> int:
    """Steps between two checkpoints of the reverse scan (fnssl_sn_mamba_backward_chunk)."""
    return int(_lib.load().fnssl_sn_mamba_backward_chunk())


class MambaFunction(torch.autograd.Function):
    """pool_T(residual * x + Mamba(LN(x))) for x logical [B, F, T, 96]; arguments after ``time_pool``: LayerNorm weight
    and bias, then the Mamba parameters in ``PARAMS`` order."""

    @staticmethod
    def forward(ctx, x, residual, time_pool, *params):
        _need_dev(x, *params)
        if x.dtype != torch.float32 or any(p.dtype != torch.float32 for p in params):
            raise RuntimeError("fnssl.spatialnet_train: the Mamba block trains in fp32 (got %s)"
                               % sorted({str(t.dtype) for t in (x,) + params}))
        with torch.cuda.device(x.device):
            xc = _conform(x.detach())
            nb, nf, nt, _ = xc.shape
            sd = dict(zip(("n.weight", "n.bias") + tuple("m." + k for k in PARAMS), params))
            w, keep = pack_mamba(sd, "n", "m", x.device)
            packed = keep.tensors                            # the 11 packed tensors, in fnssl_sn_mamba_w's field order
            lib = _lib.load()
            ws = torch.empty(lib.fnssl_sn_mamba_workspace_bytes(nb, nt, nf), dtype=torch.uint8, device=x.device)
            out = _new_bfth(nb, nf, nt // time_pool, x.device)
            xv, ov = _view(xc), _view(out)
            check(lib.fnssl_sn_mamba(C.byref(xv), nb, nt, nf, C.byref(w), int(residual), int(time_pool), None, None, 0,
                                     ov.p, ov.sb, ov.st, ov.sf, _ptr(ws), ws.numel(), FP32, _stream()), "sn_mamba")
        ctx.save_for_backward(xc, ws, *packed)
        ctx.residual, ctx.time_pool = int(residual), int(time_pool)
        return out

    @staticmethod
    def backward(ctx, dout):
        xc, ws, *packed = ctx.saved_tensors
        with torch.cuda.device(xc.device):
            nb, nf, nt, _ = xc.shape
            dout = _conform(dout.float())
            lib = _lib.load()
            w = SnMambaW(*[t.data_ptr() for t in packed])
            grads = [torch.empty_like(t) for t in packed]
            g = SnMambaGrads(*[t.data_ptr() for t in grads])
            dx = _new_bfth(nb, nf, nt, xc.device)
            bws = torch.empty(lib.fnssl_sn_mamba_backward_workspace_bytes(nb, nt, nf), dtype=torch.uint8, device=xc.device)
            xv, dv, gv = _view(xc), _view(dout) if dout.numel() else None, _view(dx)
            check(lib.fnssl_sn_mamba_backward(C.byref(xv), nb, nt, nf, C.byref(w), ctx.residual, ctx.time_pool, _ptr(ws),
                                              ws.numel(), dv.p if dv else None, dv.sb if dv else 0, dv.st if dv else 0,
                                              dv.sf if dv else 0, gv.p, gv.sb, gv.st, gv.sf, C.byref(g), _ptr(bws),
                                              bws.numel(), _stream()), "sn_mamba_backward")
        gln_w, gln_b, gwinT, gcw, gcb, gwxT, gwdt, gbdt, ga, gd, gwoT = grads
        a = packed[8]                                      # A = -exp(A_log): dA_log = dA * A
        return (dx, None, None, gln_w, gln_b, gwinT.t(), gcw.view(E, 1, KC), gcb, gwxT[:, :RK + 2 * NST].t(), gwdt, gbdt,
                ga * a, gd, gwoT.t())


def mamba_train(x, norm, mamba, residual: bool = True, time_pool: int = 1):
    """pool_T(residual * x + mamba(norm(x))) along T with a ``grad_fn``.  ``norm``: the block's LayerNorm, ``mamba``: its
    ``Mamba`` parameter holder (IPDnet2.IPDnet2).  The forward's bits are ``fnssl.spatialnet.mamba``'s."""
    if x.dim() != 4 or x.shape[3] != H:
        raise RuntimeError("fnssl.spatialnet_train: expected [B, F, T, %d], got %s" % (H, tuple(x.shape)))
    sd = dict(mamba.named_parameters())
    return MambaFunction.apply(x, bool(residual), int(time_pool), norm.weight, norm.bias, *[sd[n] for n in PARAMS])


def _need_fp32(what, x, params):
    if x.dtype != torch.float32 or any(p.dtype != torch.float32 for p in params):
        raise RuntimeError("fnssl.spatialnet_train: %s trains in fp32 (got %s)"
                           % (what, sorted({str(t.dtype) for t in (x,) + tuple(params)})))


class FconvFunction(torch.autograd.Function):
    """pool_F(residual * x + PReLU(Conv1d_g(LN(x)))) along F for x logical [B, F, T, 96]; arguments after ``pool``:
    LayerNorm weight and bias, Conv1d weight [96, 12, 5] and bias, PReLU weight."""

    @staticmethod
    def forward(ctx, x, residual, pool, *params):
        _need_fp32("the f-conv branch", x, params)                 # before _need_dev, whose own message does not say fp32
        _need_dev(x, *params)
        with torch.cuda.device(x.device):
            xc = _conform(x.detach())
            nb, nf, nt, _ = xc.shape
            sd = dict(zip(("p.0.weight", "p.0.bias", "p.1.weight", "p.1.bias", "p.2.weight"), params))
            w, keep = pack_fconv(sd, "p", x.device)
            out = _new_bfth(nb, nf // pool, nt, x.device)              # fresh: never aliases x, which the backward reads
            xv, ov = _view(xc), _view(out)
            check(_lib.load().fnssl_sn_fconv(C.byref(xv), nb, nt, nf, C.byref(w), int(residual), int(pool), ov.p, ov.sb,
                                             ov.st, ov.sf, FP32, _stream()), "sn_fconv")
        ctx.save_for_backward(xc, *keep.tensors)                       # the 5 packed tensors, in fnssl_sn_fconv_w's order
        ctx.residual, ctx.pool = int(residual), int(pool)
        return out

    @staticmethod
    def backward(ctx, dout):
        xc, *packed = ctx.saved_tensors
        with torch.cuda.device(xc.device):
            nb, nf, nt, _ = xc.shape
            lib = _lib.load()
            w = SnFconvW(*[t.data_ptr() for t in packed])
            grads = [torch.empty_like(t) for t in packed]
            g = SnFconvGrads(*[t.data_ptr() for t in grads])
            dx = _new_bfth(nb, nf, nt, xc.device)
            ws = torch.empty(lib.fnssl_sn_fconv_backward_workspace_bytes(nb, nt, nf), dtype=torch.uint8, device=xc.device)
            dout = _conform(dout.float())
            xv, dv, gv = _view(xc), _view(dout), _view(dx)
            check(lib.fnssl_sn_fconv_backward(C.byref(xv), nb, nt, nf, C.byref(w), ctx.residual, ctx.pool, dv.p, dv.sb, dv.st,
                                              dv.sf, gv.p, gv.sb, gv.st, gv.sf, C.byref(g), _ptr(ws), ws.numel(), _stream()),
                  "sn_fconv_backward")
        gln_w, gln_b, gwT, gbias, gprelu = grads
        # wT is [g][tap][ci][o]: back to Conv1d's [g * 12 + o, ci, tap], the inverse of pack_fconv's permute
        gw = gwT.view(8, 5, 12, 12).permute(0, 3, 2, 1).reshape(H, 12, 5)
        return dx, None, None, gln_w, gln_b, gw, gbias, gprelu


class FullFunction(torch.autograd.Function):
    """residual * x + SiLU(unsqueeze(Linear_F(SiLU(squeeze(LN(x)))))) for x logical [B, F, T, 96]; arguments after
    ``residual``: norm_full weight, bias; squeeze.0 weight [8, 96, 1], bias; full weight [F, F], bias; unsqueeze.0 weight
    [96, 8, 1], bias."""

    @staticmethod
    def forward(ctx, x, residual, *params):
        _need_fp32("the full-band branch", x, params)                 # before _need_dev, whose own message does not say fp32
        _need_dev(x, *params)
        with torch.cuda.device(x.device):
            xc = _conform(x.detach())
            nb, nf, nt, _ = xc.shape
            sd = dict(zip(("norm_full.weight", "norm_full.bias", "squeeze.0.weight", "squeeze.0.bias", "full.weight",
                           "full.bias", "unsqueeze.0.weight", "unsqueeze.0.bias"), params))
            w, keep, nfull = pack_full(sd, "", x.device)
            if nfull != nf:
                raise RuntimeError("fnssl.spatialnet_train: full.weight is %d x %d, x has %d bins" % (nfull, nfull, nf))
            out = _new_bfth(nb, nf, nt, x.device)                      # fresh: never aliases x, which the backward reads
            xv, ov = _view(xc), _view(out)
            check(_lib.load().fnssl_sn_full(C.byref(xv), nb, nt, nf, C.byref(w), int(residual), ov.p, ov.sb, ov.st, ov.sf,
                                            FP32, _stream()), "sn_full")
        ctx.save_for_backward(xc, *keep.tensors)                       # the 8 packed tensors, in fnssl_sn_full_w's order
        ctx.residual = int(residual)
        return out

    @staticmethod
    def backward(ctx, dout):
        xc, *packed = ctx.saved_tensors
        with torch.cuda.device(xc.device):
            nb, nf, nt, _ = xc.shape
            lib = _lib.load()
            w = SnFullW(*[t.data_ptr() for t in packed])
            grads = [torch.empty_like(t) for t in packed]
            g = SnFullGrads(*[t.data_ptr() for t in grads])
            dx = _new_bfth(nb, nf, nt, xc.device)
            ws = torch.empty(lib.fnssl_sn_full_backward_workspace_bytes(nb, nt, nf), dtype=torch.uint8, device=xc.device)
            dout = _conform(dout.float())
            xv, dv, gv = _view(xc), _view(dout), _view(dx)
            check(lib.fnssl_sn_full_backward(C.byref(xv), nb, nt, nf, C.byref(w), ctx.residual, dv.p, dv.sb, dv.st, dv.sf,
                                             gv.p, gv.sb, gv.st, gv.sf, C.byref(g), _ptr(ws), ws.numel(), _stream()),
                  "sn_full_backward")
        gln_w, gln_b, gwsT, gbs, gwfT, gbf, gwuT, gbu = grads
        return (dx, None, gln_w, gln_b, gwsT.t().reshape(HS, H, 1), gbs, gwfT.t(), gbf, gwuT.t().reshape(H, HS, 1), gbu)


def _need_bfth(x):
    if x.dim() != 4 or x.shape[3] != H:
        raise RuntimeError("fnssl.spatialnet_train: expected [B, F, T, %d], got %s" % (H, tuple(x.shape)))


def fconv_train(x, ml, residual: bool = True, pool: int = 1):
    """pool_F(residual * x + PReLU(conv(LN(x)))) along F with a ``grad_fn``.  ``ml``: the branch's ModuleList (LayerNorm,
    Conv1d(96, 96, 5, groups 8), PReLU(96)).  The forward's bits are ``fnssl.spatialnet.fconv``'s in fp32."""
    _need_bfth(x)
    return FconvFunction.apply(x, bool(residual), int(pool), ml[0].weight, ml[0].bias, ml[1].weight, ml[1].bias, ml[2].weight)


def full_train(x, layer, residual: bool = True):
    """residual * x + the full-band branch of ``layer`` (norm_full, squeeze, full, unsqueeze) with a ``grad_fn``.  The
    forward's bits are ``fnssl.spatialnet.full``'s in fp32."""
    _need_bfth(x)
    return FullFunction.apply(x, bool(residual), layer.norm_full.weight, layer.norm_full.bias, layer.squeeze[0].weight,
                              layer.squeeze[0].bias, layer.full.weight, layer.full.bias, layer.unsqueeze[0].weight,
                              layer.unsqueeze[0].bias)


def layer_train(layer, x, time_pool: int = 1):
    """One ``SpatialNetLayer`` with a ``grad_fn``: the five branches composed as ``SpatialNetLayer.forward`` composes the
    five forward calls (residual inside each call, F pooled by 2 and by 8 in the first layer), ``time_pool`` handed to the
    second Mamba block.  x logical [B, F, T, 96] -> [B, F', T // time_pool, 96]; at time_pool 1 the bits of
    ``layer.eval()(x)[0]``."""
    first = bool(layer.is_first)
    y = fconv_train(x, layer.fconv1, True, 2 if first else 1)
    y = full_train(y, layer, True)
    y = fconv_train(y, layer.fconv2, True, 8 if first else 1)
    y = mamba_train(y, layer.norm_mhsa, layer.mhsa, True, 1)
    return mamba_train(y, layer.norm_tconvffn, layer.tconvffn, True, int(time_pool))


class EncoderFunction(torch.autograd.Function):
    """CausalConv1d(C -> 96, k 5) along T from zero state: x [B, C, F, T] (any strides) -> logical [B, F, T, 96];
    arguments after x: the conv's weight [96, C, 5] and bias [96].  dx is computed only when x requires a gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _need_fp32("the encoder", x, (weight, bias))                   # before _need_dev, whose own message does not say fp32
        _need_dev(x, weight, bias)
        xd = x.detach()
        wT = weight.detach().permute(1, 2, 0).contiguous()             # [c][k][o], the layout the kernels read
        out = encoder(xd, wT, bias.detach().contiguous())
        ctx.save_for_backward(xd, wT)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, wT = ctx.saved_tensors
        with torch.cuda.device(x.device):
            nb, cin, nf, nt = x.shape
            lib = _lib.load()
            dout = _conform(dout.float())
            dv = _view(dout)
            dwT, db = torch.empty_like(wT), torch.empty(H, dtype=torch.float32, device=x.device)
            dx = torch.empty(x.shape, dtype=torch.float32, device=x.device) if ctx.needs_input_grad[0] else None
            ws = torch.empty(lib.fnssl_sn_encoder_backward_workspace_bytes(nb, cin, nf, nt), dtype=torch.uint8, device=x.device)
            check(lib.fnssl_sn_encoder_backward(_ptr(x), *x.stride(), nb, cin, nf, nt, _ptr(wT), dv.p, dv.sb, dv.st, dv.sf,
                                                _ptr(dwT), _ptr(db), _ptr(dx), *(dx.stride() if dx is not None else (0,) * 4),
                                                _ptr(ws), ws.numel(), _stream()), "sn_encoder_backward")
        return dx, dwT.permute(2, 0, 1), db                            # back to Conv1d's [96, C, 5]


class HeadFunction(torch.autograd.Function):
    """FreqInverse + tanh + decoder + the output order: x logical [B, Fc, T', 96] -> [B, T', 2 * 16 Fc, 4, 2]; arguments
    after x: trans2.weight [256, 96, 1], trans2.bias [256], decoder.weight [16, 16], decoder.bias [16]."""

    @staticmethod
    def forward(ctx, x, *params):
        _need_fp32("the head", x, params)
        _need_dev(x, *params)
        xc = _conform(x.detach())
        sd = dict(zip(("freq_inverse.trans2.weight", "freq_inverse.trans2.bias", "decoder.weight", "decoder.bias"), params))
        ptrs, keep = pack_head(sd, x.device)
        out = head(xc, ptrs)
        ctx.save_for_backward(xc, *keep.tensors)                       # wfiP, bfiP, wdT, bd
        return out

    @staticmethod
    def backward(ctx, dout):
        xc, *packed = ctx.saved_tensors
        with torch.cuda.device(xc.device):
            nb, nfc, nt2, _ = xc.shape
            grads = [torch.empty_like(t) for t in packed]
            dx = _new_bfth(nb, nfc, nt2, xc.device)
            if xc.numel():
                lib = _lib.load()
                g = SnHeadGrads(*[t.data_ptr() for t in grads])
                dout = dout.float().contiguous()                       # a cut prediction's dpred is strided
                ws = torch.empty(lib.fnssl_sn_head_backward_workspace_bytes(nb, nt2, nfc), dtype=torch.uint8, device=xc.device)
                xv, gv = _view(xc), _view(dx)
                check(lib.fnssl_sn_head_backward(C.byref(xv), nb, nt2, nfc, _ptr(packed[0]), _ptr(packed[1]), _ptr(packed[2]),
                                                 _ptr(dout), gv.p, gv.sb, gv.st, gv.sf, C.byref(g), _ptr(ws), ws.numel(),
                                                 _stream()), "sn_head_backward")
            else:
                for t in grads:
                    t.zero_()
        gwfi, gbfi, gwdT, gbd = grads
        # wfiP is [r][o][h] = trans2.weight[o * 16 + r, h], bfiP [r][o]: the inverse of pack_head's re-layout
        return dx, gwfi.permute(1, 0, 2).reshape(16 * DO, H, 1), gbfi.t().reshape(16 * DO), gwdT.t(), gbd


def encoder_train(x, conv):
    """The encoder with a ``grad_fn``: x [B, C, F, T] -> logical [B, F, T, 96].  ``conv``: the network's ``CausalConv1d``
    (out 96, k 5, bias).  The forward's bits are ``fnssl.spatialnet.encoder``'s in fp32; x.grad is formed only if
    ``x.requires_grad``."""
    if x.dim() != 4 or tuple(conv.weight.shape) != (H, x.shape[1], 5) or conv.bias is None:
        raise RuntimeError("fnssl.spatialnet_train: the encoder takes [B, C, F, T] and a conv weight [%d, C, 5] with bias, got "
                           "%s and %s" % (H, tuple(x.shape), tuple(conv.weight.shape)))
    return EncoderFunction.apply(x, conv.weight, conv.bias)


def head_train(x, freq_inverse, decoder):
    """The head with a ``grad_fn``: x logical [B, Fc, T', 96] -> [B, T', 2 * 16 Fc, 4, 2].  ``freq_inverse``: the network's
    ``FreqInverse`` (trans2), ``decoder``: its Linear(16, 16).  The forward's bits are ``fnssl.spatialnet.head``'s."""
    _need_bfth(x)
    return HeadFunction.apply(x, freq_inverse.trans2.weight, freq_inverse.trans2.bias, decoder.weight, decoder.bias)


def net_train(net, x):
    """A whole ``OnlineSpatialNet`` with a ``grad_fn``: x [B, dim_input, F, T] -> [B, T // ratio, 2F, 4, 2], the bits of
    ``net.eval()(x)``; the backward reaches the encoder's 2, every layer's 40 and the head's 4 parameters (and x, if it
    requires a gradient).  Time is pooled by ``net.time_compression_ratio`` at the end of layer 0."""
    ratio = int(net.time_compression_ratio)
    if x.dim() != 4 or x.shape[3] < ratio:
        raise RuntimeError("fnssl.spatialnet_train: training needs [B, C, F, T] with at least one pooled frame (T >= %d), "
                           "got %s" % (ratio, tuple(x.shape)))
    y = encoder_train(x, net.encoder)
    for l, layer in enumerate(net.layers):
        y = layer_train(layer, y, ratio if l == 0 else 1)
    return head_train(y, net.freq_inverse, net.decoder)
