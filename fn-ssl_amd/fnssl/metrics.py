"""DOA evaluation on device: the tensor front of ``fnssl_doa_metrics`` / ``fnssl_doa_metrics_ex`` (csrc/metrics.hip),
``fnssl_ipd2doa_tracks`` and ``fnssl_ipd2doa_mse_tracks`` (csrc/doa.hip).

Reference: ``getMetric.forward`` (FN-SSL/Lightning/Module.py:126-276, IPDnet/Module.py:92-237, IPDnet2/Module.py:67-278),
``PredDOA.pred2DOA`` (IPDnet/Module.py:463-579) and IPDnet2's MSE search (IPDnet2/Module.py:548-666).  Everything here takes and returns device tensors; nothing is read
back and nothing synchronises.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .ops import _need_dev, _ptr, _stream, on_device

MAX_SOURCES = 4
SOURCE_MODE = {"single": 0, "multiple": 1}
AE_MODE = {"azi": 1, "ele": 2, "aziele": 4}
# slots of the metrics vector (include/fnssl.h: fnssl_doa_metrics)
SLOT_ACC, SLOT_MDR, SLOT_FAR, SLOT_MAE, SLOT_RMSE, NUM_SLOTS = 0, 1, 2, 3, 6, 9
AE_SLOT = {"azi": 0, "ele": 1, "aziele": 2}


def ae_mask(ae_mode) -> int:
    modes = [ae_mode] if isinstance(ae_mode, str) else list(ae_mode)
    if not modes or any(m not in AE_MODE for m in modes):
        raise Exception('Angle error mode unrecognized')                 # Module.py:134 / :305
    mask = 0
    for m in modes:
        mask |= AE_MODE[m]
    return mask


def _strides(t, n):
    return (C.c_longlong * n)(*t.stride())


@on_device
def doa_metrics(doa_gt: torch.Tensor, vad_gt, doa_est: torch.Tensor, vad_est, source_mode: str = "multiple",
                ae_mode=("azi",), ae_TH: float = 30, useVAD: bool = True, vad_TH=(0.5, 0.5), radians: bool = False,
                large_number: float = 10000, eps: float = 1e-5, est_below: bool = False, ratio_eps: float = 0.0):
    """doa_gt [nb, nt, 2, ns_gt], vad_gt [nb, nt, ns_gt], doa_est [nb, nt, 2, ns_est], vad_est [nb, nt, ns_est]
    (float32 device tensors of any strides, read in place) -> (metrics float32 [9], K_gt, K_est, K_corr int32 [nb]).

    metrics: [0] ACC, [1] MDR, [2] FAR, [3:6] MAE (azi, ele, aziele), [6:9] RMSE (azi, ele, aziele); 'single' fills ACC
    and MAE; only the modes named in ``ae_mode`` are formed.  ``radians``: the DOAs are radians and the kernel forms
    the degrees (``x * 180 / np.pi`` in fp32); a pair ``(gt_radians, est_radians)`` gives each side its own unit.
    ``est_below``: an estimate is active when ``vad_est < vad_TH[1]`` (IPDnet2, whose activity is an MSE) instead of
    ``>``; ``ratio_eps`` is added to the K_gt denominators of ACC / MDR / FAR (IPDnet2: 1e-6; 0 keeps 0 / 0 = NaN)."""
    if source_mode not in SOURCE_MODE:
        raise RuntimeError("fnssl.metrics.doa_metrics: source_mode must be 'single' or 'multiple', got %r" % (source_mode,))
    _need_dev(doa_gt, doa_est)
    if doa_gt.ndim != 4 or doa_est.ndim != 4 or doa_gt.shape[2] != 2 or doa_est.shape[2] != 2 \
            or tuple(doa_gt.shape[:2]) != tuple(doa_est.shape[:2]):
        raise RuntimeError("fnssl.metrics.doa_metrics: DOAs must be [nb, nt, 2, ns] with equal nb, nt, got %s and %s"
                           % (tuple(doa_gt.shape), tuple(doa_est.shape)))
    nb, nt, _, ns_gt = doa_gt.shape
    ns_est = doa_est.shape[3]
    if useVAD:
        _need_dev(vad_gt, vad_est)
        if vad_gt is None or vad_est is None or tuple(vad_gt.shape) != (nb, nt, ns_gt) or tuple(vad_est.shape) != (nb, nt, ns_est):
            raise RuntimeError("fnssl.metrics.doa_metrics: VADs must be [nb, nt, ns] like the DOAs %s / %s"
                               % (tuple(doa_gt.shape), tuple(doa_est.shape)))
    dev = doa_gt.device
    metrics = torch.empty(NUM_SLOTS, dtype=torch.float32, device=dev)
    per_utt = torch.empty((nb, NUM_SLOTS), dtype=torch.float32, device=dev)
    counts = torch.empty((3, nb), dtype=torch.int32, device=dev)
    head = (_ptr(doa_gt), _strides(doa_gt, 4), _ptr(vad_gt if useVAD else None), _strides(vad_gt, 3) if useVAD else None,
            _ptr(doa_est), _strides(doa_est, 4), _ptr(vad_est if useVAD else None), _strides(vad_est, 3) if useVAD else None,
            nb, nt, ns_gt, ns_est, SOURCE_MODE[source_mode], ae_mask(ae_mode), float(ae_TH), float(vad_TH[0]), float(vad_TH[1]),
            1 if useVAD else 0)
    tail = (float(large_number), float(eps), _ptr(metrics), _ptr(per_utt), C.c_void_p(counts[0].data_ptr()),
            C.c_void_p(counts[1].data_ptr()), C.c_void_p(counts[2].data_ptr()), _stream())
    pair = isinstance(radians, (tuple, list))
    if pair or est_below or ratio_eps:
        gt_rad, est_rad = radians if pair else (radians, radians)
        if not float(ratio_eps) >= 0.0:
            raise RuntimeError("fnssl.metrics.doa_metrics: ratio_eps must not be negative, got %r" % (ratio_eps,))
        _lib.check(_lib.load().fnssl_doa_metrics_ex(*head, 1 if gt_rad else 0, 1 if est_rad else 0, 1 if est_below else 0,
                                                    float(ratio_eps), *tail), "doa_metrics_ex")
    else:
        _lib.check(_lib.load().fnssl_doa_metrics(*head, 1 if radians else 0, *tail), "doa_metrics")
    return metrics, counts[0], counts[1], counts[2]


@on_device
def localize_tracks(pred: torch.Tensor, bank: torch.Tensor, max_num_sources: int = 1, source_num_mode: str = "UnkNum"):
    """The template search for every track of IPDnet's output in one launch.

    pred [nb, nt2, 2nf, nmic - 1, ntrack] (any strides — the forward's permuted view is read in place); bank
    [nele, nazi, 2nf, nmic - 1].  Returns (idx int32 [ntrack, nb, nt2, ns], vad [ntrack, nb, nt2, ns],
    ss [ntrack, nb, nt2, nele, nazi]); track r equals ``fnssl.doa.localize(pred[..., r], ...)`` bit for bit."""
    _need_dev(pred, bank)
    if source_num_mode not in ("KNum", "UnkNum", "kNum", "unkNum"):
        raise RuntimeError("source_num_mode must be 'KNum' or 'UnkNum'")
    if pred.ndim != 5:
        raise RuntimeError("fnssl.metrics.localize_tracks: pred must be [nb, nt2, 2nf, nmic - 1, ntrack]")
    bank = bank.contiguous()
    nele, nazi, nf2, np_ = bank.shape
    nb, nt, nf2p, npp, ntrack = pred.shape
    if nf2p != nf2 or npp != np_:
        raise RuntimeError("fnssl.metrics.localize_tracks: pred %s does not match the bank %s" % (tuple(pred.shape), tuple(bank.shape)))
    sb, st, sk, sp, sr = pred.stride()
    ns = int(max_num_sources)
    ss = torch.empty((ntrack, nb, nt, nele, nazi), dtype=torch.float32, device=pred.device)
    idx = torch.empty((ntrack, nb, nt, ns), dtype=torch.int32, device=pred.device)
    vad = torch.empty((ntrack, nb, nt, ns), dtype=torch.float32, device=pred.device)
    _lib.check(_lib.load().fnssl_ipd2doa_tracks(_ptr(pred), sb, sp, st, sk, sr, _ptr(bank), nb, np_, nt, nf2, nele * nazi, ns,
                                                ntrack, 1 if source_num_mode in ("UnkNum", "unkNum") else 0, _ptr(ss),
                                                C.c_void_p(idx.data_ptr()), _ptr(vad), _stream()), "ipd2doa_tracks")
    return idx, vad, ss


MAX_MSE_LDS_BYTES = 60 * 1024          # include/fnssl.h: fnssl_ipd2doa_mse_tracks


@on_device
def localize_tracks_mse(pred: torch.Tensor, bank: torch.Tensor, max_num_sources: int = 1, source_num_mode: str = "UnkNum"):
    """IPDnet2's MSE template search (IPDnet2/Module.py:573-666) for every track in one launch.

    pred [nb, nt, 2nf, nmic - 1, ntrack] float32 (any strides - the forward's output is read in place); bank
    [nele, nazi, 2nf, nmic - 1] float32.  Returns (doa_idx int32 [ntrack, nb, nt, ns] into the flattened (ele, azi) grid: the
    first minimum of the MSE, torch.argmin's NaN rule; vad [ntrack, nb, nt, ns]: that MSE ('UnkNum') or 1 ('KNum');
    ss [ntrack, nb, nt, nele, nazi]: the MSE of every candidate before any subtraction).  For ``max_num_sources`` > 1 the
    winning template is subtracted whole and the search repeats (:652)."""
    if source_num_mode not in ("KNum", "UnkNum"):
        raise RuntimeError("source_num_mode must be 'KNum' or 'UnkNum'")
    _need_dev(pred, bank)
    if pred.ndim != 5 or bank.ndim != 4:
        raise RuntimeError("fnssl.metrics.localize_tracks_mse: pred must be [nb, nt, 2nf, nmic - 1, ntrack] and bank [nele, nazi, "
                           "2nf, nmic - 1], got %s and %s" % (tuple(pred.shape), tuple(bank.shape)))
    if pred.dtype != torch.float32 or bank.dtype != torch.float32:
        raise RuntimeError("fnssl.metrics.localize_tracks_mse: float32 tensors, got %s and %s" % (pred.dtype, bank.dtype))
    nele, nazi, nf2, np_ = bank.shape
    nb, nt, nf2p, npp, ntrack = pred.shape
    if nf2p != nf2 or npp != np_:
        raise RuntimeError("fnssl.metrics.localize_tracks_mse: pred %s does not match the bank %s" % (tuple(pred.shape), tuple(bank.shape)))
    ns = int(max_num_sources)
    if not 1 <= ns <= MAX_SOURCES:
        raise RuntimeError("fnssl.metrics.localize_tracks_mse: max_num_sources must be 1..%d, got %r" % (MAX_SOURCES, max_num_sources))
    if (nf2 * np_ + nele * nazi) * 4 > MAX_MSE_LDS_BYTES:
        raise RuntimeError("fnssl.metrics.localize_tracks_mse: 2nf * (nmic - 1) = %d values and %d candidates do not fit the "
                           "kernel's %d bytes of LDS" % (nf2 * np_, nele * nazi, MAX_MSE_LDS_BYTES))
    bank = bank.contiguous()
    sb, st, sk, sp, sr = pred.stride()
    ss = torch.empty((ntrack, nb, nt, nele, nazi), dtype=torch.float32, device=pred.device)
    idx = torch.empty((ntrack, nb, nt, ns), dtype=torch.int32, device=pred.device)
    vad = torch.empty((ntrack, nb, nt, ns), dtype=torch.float32, device=pred.device)
    _lib.check(_lib.load().fnssl_ipd2doa_mse_tracks(_ptr(pred), sb, sp, st, sk, sr, _ptr(bank), nb, np_, nt, nf2, nele * nazi, ns,
                                                    ntrack, 1 if source_num_mode == "UnkNum" else 0, _ptr(ss),
                                                    C.c_void_p(idx.data_ptr()), _ptr(vad), _stream()), "ipd2doa_mse_tracks")
    return idx, vad, ss
