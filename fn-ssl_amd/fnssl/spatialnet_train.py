"""Training front of one IPDnet2 Mamba block: ``torch.autograd`` around ``fnssl_sn_mamba`` (forward) and
``fnssl_sn_mamba_backward`` (include/fnssl.h).  fp32, whole sequences from zero state, ROCm tensors only.

    y = mamba_train(x, norm, mamba, residual=True, time_pool=1)      # x logical [B, F, T, 96]
    y.backward(...)   # fills x.grad and the .grad of the LayerNorm's 2 and the Mamba's 9 parameters

The forward is the inference call itself (same kernels, same bits) into a workspace tensor of its own, which is what the
backward recomputes from: xz | dbl | y as the forward left them, plus x.  The rest of the network (f-conv, full-band
branch, encoder, head) has no backward yet, so ``OnlineSpatialNet`` stays forward-only.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import SnMambaGrads, SnMambaW, check
from .ops import _need_dev, _ptr, _stream
from .spatialnet import E, FP32, H, KC, NST, RK, _conform, _new_bfth, _view, pack_mamba

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
