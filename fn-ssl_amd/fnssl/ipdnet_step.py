"""The data and loss half of IPDnet's training step on device (csrc/ipdnet_step.hip; reference
IPDnet/runIPDnetOn.py:144-154, 196-290):

    pit_mse(pred, gt)            cal_loss with its gradient: (loss, dpred, perm) from one kernel call
    PitMSE.apply(pred, gt)       the same as a differentiable scalar (``torch.autograd.Function``)
    dp_vad(mix_spec, dp_spec)    cal_vad from the spectra ``ops.stft`` writes
    ipdnet_targets(...)          per-source DP-IPD targets, DP-VAD gate, Bessel target in silent slots
    non_source_target(mic_pos)   that Bessel target (host, numpy only), ``non_source_device`` its cached upload
    ipdnet2_targets(...)         IPDnet2's near-field targets (IPDnet2/run_IPDnet2.py:290-322), gated by the label VAD
    ipdnet2_geometry(mic, dev)   per geometry, cached: the float64 table, its Bessel target and PredDOA's candidate bank

ROCm tensors only: there is no CPU implementation and no ATen fall-back.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .ops import NBIN, SEG_FRAMES, _need_dev, _ptr, _stream, on_device

MAX_SOURCES = 4


@on_device
def pit_mse(pred: torch.Tensor, gt: torch.Tensor, n_total: int = 0, loss: torch.Tensor = None, want_perm: bool = False):
    """pred [nb, nt2, 2nf, nmic - 1, nsrc] (any non-overlapping strides: the train-mode ``IPDnet.forward`` returns a
    permuted view, read in place), gt the same logical shape, or the reference's ``view(nb * nt2, 2nf, nmic - 1, nsrc)``.
    Returns (loss [1], dpred with pred's strides, perm int32 [nb * nt2] or None).  ``n_total`` (default: pred's element
    count) and ``loss`` (accumulated into when given) process a batch in chunks, as ``fnssl_mse_loss``."""
    _need_dev(pred, gt)
    if pred.ndim != 5:
        raise RuntimeError("fnssl.pit_mse: pred must be [nb, nt2, 2nf, nmic - 1, nsrc], got %s" % (tuple(pred.shape),))
    nb, nt2, nf2, nm1, nsrc = pred.shape
    if gt.numel() != pred.numel() or tuple(gt.shape[-3:]) != (nf2, nm1, nsrc):
        raise RuntimeError("fnssl.pit_mse: gt %s does not match pred %s" % (tuple(gt.shape), tuple(pred.shape)))
    gt = gt.contiguous()
    dev = pred.device
    dpred = torch.empty_strided(pred.shape, pred.stride(), dtype=torch.float32, device=dev)
    accumulate = loss is not None
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
    perm = torch.empty(nb * nt2, dtype=torch.int32, device=dev) if want_perm else None
    lib = _lib.load()
    ws = torch.empty(max(1, lib.fnssl_pit_mse_workspace_bytes(nb * nt2) // 4), dtype=torch.float32, device=dev)
    strides = (C.c_longlong * 5)(*pred.stride())
    _lib.check(lib.fnssl_pit_mse_loss(_ptr(pred), strides, _ptr(gt), nb, nt2, nf2, nm1, nsrc, int(n_total) or pred.numel(),
                                      _ptr(dpred), _ptr(loss), 1 if accumulate else 0, _ptr(perm), _ptr(ws), ws.numel() * 4,
                                      _stream()), "pit_mse_loss")
    return loss, dpred, perm


class PitMSE(torch.autograd.Function):
    """cal_loss (runIPDnetOn.py:196-206) as one kernel call with its gradient: forward keeps d loss / d pred, backward
    scales it."""

    @staticmethod
    def forward(ctx, pred, gt):
        loss, dpred, _ = pit_mse(pred.detach(), gt.detach())
        ctx.dpred = dpred
        return loss.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return ctx.dpred * g, None


@on_device
def dp_vad(mix_spec: torch.Tensor, dp_spec: torch.Tensor):
    """mix_spec [nb, nch, nt, 257, 2], dp_spec [nb, nsrc, nt, 257, 2] (``ops.stft`` of the mixture and of
    ``dp_signal[:, :, 0, :]``) -> dp_vad [nb, nt // 12, nsrc]."""
    _need_dev(mix_spec, dp_spec)
    if (mix_spec.ndim != 5 or dp_spec.ndim != 5 or tuple(mix_spec.shape[3:]) != (NBIN, 2) or tuple(dp_spec.shape[3:]) != (NBIN, 2)
            or mix_spec.shape[0] != dp_spec.shape[0] or mix_spec.shape[2] != dp_spec.shape[2]):
        raise RuntimeError("fnssl.dp_vad: expected spectra [nb, nch, nt, 257, 2] and [nb, nsrc, nt, 257, 2], got %s and %s"
                           % (tuple(mix_spec.shape), tuple(dp_spec.shape)))
    mix_spec, dp_spec = mix_spec.contiguous(), dp_spec.contiguous()
    nb, nch, nt = mix_spec.shape[:3]
    nsrc = dp_spec.shape[1]
    out = torch.empty((nb, nt // SEG_FRAMES, nsrc), dtype=torch.float32, device=mix_spec.device)
    _lib.check(_lib.load().fnssl_dp_vad(_ptr(mix_spec), _ptr(dp_spec), nb, nch, nsrc, nt, _ptr(out), _stream()), "dp_vad")
    return out


def bessel_j0(x):
    """J0(x) = mean over theta in (0, pi) of cos(x sin theta), by the mid-point rule on 1024 points: the integrand is
    periodic and analytic, so the rule converges geometrically (4.5e-16 against scipy.special.jn(0, x) up to x = 148,
    a 1-m aperture at 8 kHz).  numpy only: scipy may be absent where the library runs."""
    th = (np.arange(1024) + 0.5) * (np.pi / 1024)
    return np.cos(np.asarray(x, dtype=np.float64)[..., None] * np.sin(th)).mean(axis=-1)


def non_source_target(mic_pos, bins=range(1, 257)) -> np.ndarray:
    """euclidean_distances_to_bessel (runIPDnetOn.py:209-221): [512, nmic - 1] float32 =
    [J0(2 pi f_k d_m / 340) | zeros(256)], d_m the distance of microphone m from microphone 0,
    f = linspace(0, 8000, 257)[bins].  The reference's ``mic_pos`` is a float32 tensor; pass float32 to reproduce it."""
    mic = np.asarray(mic_pos).reshape(-1, 3)          # distances in the array's own dtype, as the reference forms them
    if mic.shape[0] < 2:
        raise RuntimeError("fnssl.non_source_target: at least two microphones")
    dist = np.sqrt(np.sum((mic[1:] - mic[0]) ** 2, axis=1))
    freq = (2 * np.pi * np.linspace(0, 8000, 257) / 340)[list(bins)]
    if len(freq) != 256:
        raise RuntimeError("fnssl.non_source_target: the reference pairs 256 bins with 256 zeros")
    return np.concatenate((bessel_j0(freq[:, None] * dist[None, :]), np.zeros((256, len(dist)))), axis=0).astype(np.float32)


_geometry_cache = {}


def non_source_device(mic_pos, device):
    """(mic_loc [nmic, 3], non_source [512, nmic - 1]) on ``device``: computed once per geometry and uploaded once."""
    mic = np.ascontiguousarray(np.asarray(mic_pos, dtype=np.float32).reshape(-1, 3))
    key = (mic.tobytes(), str(device))
    if key not in _geometry_cache:
        _geometry_cache[key] = (torch.from_numpy(mic).to(device), torch.from_numpy(non_source_target(mic)).to(device))
    return _geometry_cache[key]


@on_device
def ipdnet_targets(doa: torch.Tensor, vad, mic_loc: torch.Tensor, non_source, bin0: int = 1, nf_used: int = 256,
                   nbins: int = 257, fre_max: float = 8000.0, speed: float = 340.0, vad_th: float = 0.001):
    """doa [nb, nseg, 2, nsrc] (elevation, azimuth), vad [nb, nseg, nsrc] or None (all active), mic_loc [nmic, 3] and
    non_source [2 nf_used, nmic - 1] on the device -> ipd [nb, nseg, 2 nf_used, nmic - 1, nsrc]."""
    _need_dev(doa, vad, mic_loc, non_source)
    if doa.ndim != 4 or doa.shape[2] != 2:
        raise RuntimeError("fnssl.ipdnet_targets: doa must be [nb, nseg, 2, nsource], got %s" % (tuple(doa.shape),))
    nb, nseg, _, nsrc = doa.shape
    if vad is not None and tuple(vad.shape) != (nb, nseg, nsrc):
        raise RuntimeError("fnssl.ipdnet_targets: vad %s does not match doa %s" % (tuple(vad.shape), tuple(doa.shape)))
    if mic_loc.ndim != 2 or mic_loc.shape[1] != 3:
        raise RuntimeError("fnssl.ipdnet_targets: mic_loc must be [nmic, 3], got %s" % (tuple(mic_loc.shape),))
    nmic = mic_loc.shape[0]
    if non_source is not None and tuple(non_source.shape) != (2 * nf_used, nmic - 1):
        raise RuntimeError("fnssl.ipdnet_targets: non_source %s is not [%d, %d]" % (tuple(non_source.shape), 2 * nf_used, nmic - 1))
    doa, mic_loc = doa.contiguous(), mic_loc.contiguous()
    vad = None if vad is None else vad.contiguous()
    non_source = None if non_source is None else non_source.contiguous()
    ipd = torch.empty((nb, nseg, 2 * nf_used, nmic - 1, nsrc), dtype=torch.float32, device=doa.device)
    _lib.check(_lib.load().fnssl_ipdnet_targets(_ptr(doa), _ptr(vad), nb, nseg, nsrc, _ptr(mic_loc), nmic, _ptr(non_source),
                                                int(bin0), int(nf_used), int(nbins), float(fre_max), float(speed),
                                                float(vad_th), _ptr(ipd), _stream()), "ipdnet_targets")
    return ipd


_geometry2_cache = {}


def ipdnet2_geometry(mic_pos, device, res_the: int = 1, res_phi: int = 360, nfft: int = 512, fre_max: float = 8000.0,
                     speed: float = 340.0):
    """What IPDnet2's evaluation needs of one array, computed once per (geometry, grid, device) and uploaded once:

        mic         float64 [nmic, 3] on ``device`` (the reference keeps the table in float64: ``fnssl_ipdnet2_targets``)
        non_source  float32 [512, nmic - 1]: euclidean_distances_to_bessel (run_IPDnet2.py:252-264) of that table
        bank        float32 [res_the, res_phi, 2 * (nfft // 2), nmic - 1]: DPIPD2.__init__'s far-field templates
                    (IPDnet2/Module.py:416-441; equal to DPIPD's: elevation pi / 2, azimuth linspace(-pi, pi, res_phi),
                    reference-microphone pairs), [cos | sin] of bins 1 .. nfft / 2 as pred2DOA_track takes them (:585)
        ele, azi    float32 candidate grids on ``device``
    """
    from . import doa as fdoa
    mic = np.ascontiguousarray(np.asarray(mic_pos, dtype=np.float64).reshape(-1, 3))
    key = (mic.tobytes(), str(device), int(res_the), int(res_phi), int(nfft), float(fre_max), float(speed))
    if key not in _geometry2_cache:
        nf = int(nfft / 2) + 1
        template, cand = fdoa.dpipd_templates(mic, int(res_the), int(res_phi), nf, fre_max, "M", speed,
                                              search_space_ele=(np.pi / 2, np.pi / 2), search_space_azi=(-np.pi, np.pi))
        k = list(range(1, nf))
        bank = np.ascontiguousarray(np.concatenate((template.real[:, :, k, :], template.imag[:, :, k, :]), axis=2).astype(np.float32))
        non_source = non_source_target(mic) if nf == 257 and fre_max == 8000.0 and speed == 340.0 else None
        _geometry2_cache[key] = {
            "mic": torch.from_numpy(mic).to(device),
            "non_source": None if non_source is None else torch.from_numpy(non_source).to(device),
            "bank": torch.from_numpy(bank).to(device),
            "ele": torch.from_numpy(cand[0].astype(np.float32)).to(device),
            "azi": torch.from_numpy(cand[1].astype(np.float32)).to(device),
        }
    return _geometry2_cache[key]


@on_device
def ipdnet2_targets(doa: torch.Tensor, distance: torch.Tensor, vad, mic_loc: torch.Tensor, non_source, bin0: int = 1,
                    nf_used: int = 256, nbins: int = 257, fre_max: float = 8000.0, speed: float = 340.0, vad_th: float = 0.0):
    """doa [nb, nt, 2, nsrc] (elevation, azimuth; radians), distance [nb, nt, nsrc] (metres), vad [nb, nt, nsrc] or None
    (all active): float32; mic_loc FLOAT64 [nmic, 3] and non_source float32 [2 nf_used, nmic - 1], all on the device
    -> ipd [nb, nt, 2 nf_used, nmic - 1, nsrc].  ``vad > vad_th`` gives the near-field DP-IPD of DPIPD2.forward, otherwise
    the ``non_source`` column; a NaN VAD gives NaN."""
    _need_dev(doa, distance, vad, non_source)
    if not isinstance(mic_loc, torch.Tensor) or not mic_loc.is_cuda or mic_loc.dtype != torch.float64:
        raise RuntimeError("fnssl.ipdnet2_targets: mic_loc must be a float64 ROCm tensor (fnssl.ipdnet_step.ipdnet2_geometry)")
    if doa.ndim != 4 or doa.shape[2] != 2:
        raise RuntimeError("fnssl.ipdnet2_targets: doa must be [nb, nt, 2, nsource], got %s" % (tuple(doa.shape),))
    nb, nseg, _, nsrc = doa.shape
    if not 1 <= nsrc <= MAX_SOURCES:
        raise RuntimeError("fnssl.ipdnet2_targets: 1..%d sources, got %d" % (MAX_SOURCES, nsrc))
    if tuple(distance.shape) != (nb, nseg, nsrc):
        raise RuntimeError("fnssl.ipdnet2_targets: distance %s does not match doa %s" % (tuple(distance.shape), tuple(doa.shape)))
    if vad is not None and tuple(vad.shape) != (nb, nseg, nsrc):
        raise RuntimeError("fnssl.ipdnet2_targets: vad %s does not match doa %s" % (tuple(vad.shape), tuple(doa.shape)))
    if mic_loc.ndim != 2 or mic_loc.shape[1] != 3 or not 2 <= mic_loc.shape[0] <= 64:
        raise RuntimeError("fnssl.ipdnet2_targets: mic_loc must be [nmic, 3] with 2..64 microphones, got %s" % (tuple(mic_loc.shape),))
    nmic = mic_loc.shape[0]
    if vad is not None and non_source is None:
        raise RuntimeError("fnssl.ipdnet2_targets: a VAD needs the non_source target of the silent slots")
    if non_source is not None and tuple(non_source.shape) != (2 * nf_used, nmic - 1):
        raise RuntimeError("fnssl.ipdnet2_targets: non_source %s is not [%d, %d]" % (tuple(non_source.shape), 2 * nf_used, nmic - 1))
    doa, distance, mic_loc = doa.contiguous(), distance.contiguous(), mic_loc.contiguous()
    vad = None if vad is None else vad.contiguous()
    non_source = None if non_source is None else non_source.contiguous()
    ipd = torch.empty((nb, nseg, 2 * nf_used, nmic - 1, nsrc), dtype=torch.float32, device=doa.device)
    if ipd.numel() == 0:
        return ipd
    _lib.check(_lib.load().fnssl_ipdnet2_targets(_ptr(doa), _ptr(distance), _ptr(vad), nb, nseg, nsrc, _ptr(mic_loc), nmic,
                                                 _ptr(non_source), int(bin0), int(nf_used), int(nbins), float(fre_max),
                                                 float(speed), float(vad_th), _ptr(ipd), _stream()), "ipdnet2_targets")
    return ipd
