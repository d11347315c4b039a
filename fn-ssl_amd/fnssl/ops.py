"""Torch-tensor front of the C-ABI library: PyTorch supplies device memory and
the current HIP stream, every numeric op is a HIP kernel in libfnssl_hip.so.

No function here computes on the CPU or with ATen kernels; non-ROCm tensors are
rejected (``RuntimeError``), mirroring how the reference surfaces shape errors.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch

from . import _lib
from ._lib import LstmBwdDesc, CH_MODE, LstmDesc, Net, View, check

SEG_FRAMES = 12
NBIN = 257
NF = 256


def _need_dev(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("fnssl: expected a ROCm device tensor (this path has no CPU implementation), got %s"
                               % (t.device if isinstance(t, torch.Tensor) else type(t)))
        if t.dtype != torch.float32:
            raise RuntimeError("fnssl: expected float32, got %s" % t.dtype)


def _first_device(objs):
    for a in objs:
        if isinstance(a, torch.Tensor):
            if a.is_cuda:
                return a.device
        elif isinstance(a, (list, tuple)):
            d = _first_device(a)
            if d is not None:
                return d
    return None


def on_device(fn):
    """Run ``fn`` with the HIP current device set to the device of its first ROCm tensor argument, so that the
    kernels launch on that device and ``_stream()`` is that device's current stream (a model on ``cuda:1`` must
    not launch on device 0's stream).  Without a device tensor the call goes through unchanged (and the op's own
    ``_need_dev`` raises)."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        dev = _first_device(args) or _first_device(kwargs.values())
        if dev is None:
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapped


def _need_dev_act(*tensors):
    """Activation tensors of the wide bf16 path: ROCm tensors of float32 or bfloat16."""
    for t in tensors:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("fnssl: expected a ROCm device tensor (this path has no CPU implementation), got %s"
                               % (t.device if isinstance(t, torch.Tensor) else type(t)))
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError("fnssl: expected float32 or bfloat16, got %s" % t.dtype)


def _stream():
    """The current HIP stream of the current device (ops run under ``on_device``)."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# --------------------------------------------------------------------------- #
# front end
# --------------------------------------------------------------------------- #
def num_frames(ns: int, hop: int = 256, center: bool = False) -> int:
    if hop == 256 and not center:
        return _lib.load().fnssl_num_frames(int(ns))
    return _lib.load().fnssl_num_frames_ex(int(ns), int(hop), int(bool(center)))


def num_pairs(nch: int, ch_mode: str) -> int:
    return _lib.load().fnssl_num_pairs(int(nch), CH_MODE[ch_mode])


@on_device
def stft(sig: torch.Tensor, hop: int = 256, center: bool = False):
    """sig [nb, ns, nch] -> (spec [nb, nch, nt, 257, 2], magsum [nb, nch, nt]).  Module.py:48-68; with hop 320 and
    center=True (reflect padding) it is IPDnet2's transform, IPDnet2/Module.py:47-64."""
    _need_dev(sig)
    if sig.ndim != 3:
        raise RuntimeError("fnssl.stft: expected [nb, ns, nch], got %s" % (tuple(sig.shape),))
    nb, ns, nch = sig.shape          # any strides: a permuted [nb, nch, ns] batch is read in place
    nt = num_frames(ns, hop, center)
    spec = torch.empty((nb, nch, max(nt, 0), NBIN, 2), dtype=torch.float32, device=sig.device)
    magsum = torch.empty((nb, nch, max(nt, 0)), dtype=torch.float32, device=sig.device)
    sb, sn, sc = sig.stride()
    check(_lib.load().fnssl_stft_ex(_ptr(sig), nb, ns, nch, sb, sn, sc, int(hop), int(bool(center)), _ptr(spec),
                                    _ptr(magsum), _stream()), "stft")
    return spec, magsum


_coef_cache = {}


def forgetting_coefs_host(nt: int, sample_length: int = 298):
    a = np.empty(nt, dtype=np.float32)
    b = np.empty(nt, dtype=np.float32)
    check(_lib.load().fnssl_forgetting_coefs(nt, sample_length, a.ctypes.data_as(C.c_void_p),
                                             b.ctypes.data_as(C.c_void_p)), "forgetting_coefs")
    return a, b


def forgetting_coefs(nt: int, sample_length: int, device):
    key = (nt, sample_length, str(device))
    if key not in _coef_cache:
        a, b = forgetting_coefs_host(nt, sample_length)
        _coef_cache[key] = (torch.from_numpy(a).to(device), torch.from_numpy(b).to(device))
    return _coef_cache[key]


@on_device
def pair_features(spec, magsum, ch_mode: str = "MM", eps: float = 1e-6, sample_length: int = 298,
                  layout: int = 0, normalise: bool = True):
    """main.py:207-225.  Returns (x, mu); x is [nb', nt, 256, 4] (layout 0) or [nb', 4, 256, nt] (layout 1).
    ``normalise=False`` = the reference's ``nor_flag=False`` branch (main.py:219-221: real / imag parts as they are): the same
    kernels with a zero recursion (mu = 0) and eps = 1, i.e. an exact division by one."""
    _need_dev(spec, magsum)
    nb, nch, nt = magsum.shape
    np_ = num_pairs(nch, ch_mode)
    if np_ <= 0:
        raise RuntimeError("fnssl.pair_features: need at least 2 channels, got %d" % nch)
    ca, cb = forgetting_coefs(nt, sample_length, spec.device)
    if not normalise:
        ca, cb, eps = torch.zeros_like(ca), torch.zeros_like(cb), 1.0
    mu = torch.empty((nb * np_, nt), dtype=torch.float32, device=spec.device)
    shape = (nb * np_, nt, NF, 4) if layout == 0 else (nb * np_, 4, NF, nt)
    x = torch.empty(shape, dtype=torch.float32, device=spec.device)
    check(_lib.load().fnssl_pair_features(_ptr(spec), _ptr(magsum), _ptr(ca), _ptr(cb), nb, nch, nt,
                                          CH_MODE[ch_mode], eps, _ptr(mu), _ptr(x), layout, _stream()),
          "pair_features")
    return x, mu


def preprocess(sig, ch_mode: str = "MM", eps: float = 1e-6, sample_length: int = 298, layout: int = 0, normalise: bool = True):
    """Waveforms [nb, ns, nch] -> network features (data_preprocess, main.py:200-225)."""
    spec, magsum = stft(sig)
    x, _ = pair_features(spec, magsum, ch_mode, eps, sample_length, layout, normalise)
    return x


@on_device
def array_features(spec, magsum, eps: float = 1e-6, sample_length: int = 280, layout: int = 1):
    """IPDnet's all-channel features (runIPDnetOn.py:246-254).  Returns (x, mu); x is
    [nb, 2*nch, 256, nt] (layout 1, the reference's tensor) or [nb, nt, 256, 2*nch] (layout 0)."""
    _need_dev(spec, magsum)
    nb, nch, nt = magsum.shape
    ca, cb = forgetting_coefs(nt, sample_length, spec.device)
    mu = torch.empty((nb, nt), dtype=torch.float32, device=spec.device)
    shape = (nb, nt, NF, 2 * nch) if layout == 0 else (nb, 2 * nch, NF, nt)
    x = torch.empty(shape, dtype=torch.float32, device=spec.device)
    check(_lib.load().fnssl_array_features(_ptr(spec), _ptr(magsum), _ptr(ca), _ptr(cb), nb, nch, nt, eps,
                                           _ptr(mu), _ptr(x), layout, _stream()), "array_features")
    return x, mu


def preprocess_array(sig, eps: float = 1e-6, sample_length: int = 280, layout: int = 1, hop: int = 256,
                     center: bool = False):
    """Waveforms [nb, ns, nch] -> IPDnet input features (runIPDnetOn.py:237-254); with ``hop=320, center=True,
    sample_length=249`` the features of IPDnet2 (IPDnet2/run_IPDnet2.py:277-288, see ``preprocess_ipdnet2``).

    layout 1 returns the reference's tensor [nb, 2*nch, 256, nt] as a VIEW of the frame-major storage
    [nb, nt, 256, 2*nch] the network consumes (same shape and values for every reader; ``IPDnet.forward`` then skips
    its own transposition pass, and the front end writes whole rows instead of one float per 1200-byte stride).
    ``array_features(..., layout=1)`` still produces the contiguous NCHW tensor."""
    spec, magsum = stft(sig, hop, center)
    x, _ = array_features(spec, magsum, eps, sample_length, 0)
    return x if layout == 0 else x.permute(0, 3, 2, 1)


@on_device
def array_frontend(sig, eps: float = 1e-6, sample_length: int = 280, hop: int = 256, center: bool = False):
    """Waveforms [nb, ns, nch] (any strides) -> features [nb, nt, 256, 2*nch] in ONE library call that never writes the
    spectrum (``fnssl_array_frontend``: magnitude pass, recursive mean, transform + normalise + store pass) — the
    low-memory variant of ``preprocess_array(layout=0)``: no [nb, nch, nt, 257] complex buffer (493 MB at BASELINE
    config 5), same values.  It transforms every frame twice, and the transform (VALU + LDS bound), not the traffic, is
    what the front end costs: 0.92 ms against 0.74 ms for the two-step path at config 5, so the default stays two-step."""
    _need_dev(sig)
    if sig.ndim != 3:
        raise RuntimeError("fnssl.array_frontend: expected [nb, ns, nch], got %s" % (tuple(sig.shape),))
    nb, ns, nch = sig.shape
    nt = num_frames(ns, hop, center)
    if nt <= 0:
        raise RuntimeError("fnssl.array_frontend: signal of %d samples is too short" % ns)
    ca, cb = forgetting_coefs(nt, sample_length, sig.device)
    magsum = torch.empty((nb, nch, nt), dtype=torch.float32, device=sig.device)
    mu = torch.empty((nb, nt), dtype=torch.float32, device=sig.device)
    x = torch.empty((nb, nt, NF, 2 * nch), dtype=torch.float32, device=sig.device)
    sb, sn, sc = sig.stride()
    check(_lib.load().fnssl_array_frontend(_ptr(sig), nb, ns, nch, sb, sn, sc, int(hop), int(bool(center)), _ptr(ca), _ptr(cb),
                                           eps, _ptr(magsum), _ptr(mu), _ptr(x), _stream()), "array_frontend")
    return x


def preprocess_ipdnet2(sig, eps: float = 1e-6, sample_length: int = 249, frame_major: bool = False):
    """Waveforms [nb, ns, nch] -> IPDnet2's network input [nb, 2*nch, 256, nt], nt = ns // 320 + 1
    (IPDnet2/run_IPDnet2.py:277-288: STFT nfft 512 / hop 320 / center=True (IPDnet2/Module.py:47-64), abs,
    forgetting_norm over ALL channels with sample_length 249, real / imag normalise, cat, DC drop).  The returned
    tensor has the reference's shape and values, contiguous like the reference's (frames fastest: the layout the
    encoder kernel's frame-per-lane loads coalesce on); ``frame_major=True`` returns the same tensor as a view of
    [nb, nt, 256, 2*nch] storage instead."""
    if frame_major:
        return preprocess_array(sig, eps, sample_length, 1, hop=320, center=True)
    spec, magsum = stft(sig, 320, True)
    return array_features(spec, magsum, eps, sample_length, 1)[0]   # the reference's contiguous [nb, 2 nch, 256, nt]


@on_device
def nchw_to_seq(x):
    """[n, c, nf, nt] -> [n, nt, nf, c] (Model.py:73) as a contiguous tensor."""
    _need_dev(x)
    xs = x.permute(0, 3, 2, 1)
    if xs.is_contiguous():          # already stored frame-major (e.g. what preprocess_array hands over): nothing to move
        return xs
    x = x.contiguous()
    n, c, nf, nt = x.shape
    y = torch.empty((n, nt, nf, c), dtype=torch.float32, device=x.device)
    check(_lib.load().fnssl_nchw_to_seq(_ptr(x), n, c, nf, nt, _ptr(y), _stream()), "nchw_to_seq")
    return y


# --------------------------------------------------------------------------- #
# LSTM
# --------------------------------------------------------------------------- #
def pack_lstm_host(w_ih, w_hh, b_ih, b_hh, c0: int, c2: int) -> np.ndarray:
    """Pack one direction's nn.LSTM parameters (numpy / CPU tensors) into the kernel's weight stream."""
    arrs = [np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)
            for a in (w_ih, w_hh, b_ih, b_hh)]
    hidden = arrs[1].shape[1]
    if arrs[0].shape != (4 * hidden, c0 + c2) or arrs[1].shape != (4 * hidden, hidden):
        raise RuntimeError("fnssl.pack_lstm: weight shapes %s / %s do not match c0+c2=%d, H=%d"
                           % (arrs[0].shape, arrs[1].shape, c0 + c2, hidden))
    lib = _lib.load()
    n = lib.fnssl_lstm_packed_floats(c0, c2, hidden)
    if n == 0:
        raise RuntimeError("fnssl.pack_lstm: unsupported sizes c0=%d c2=%d H=%d (multiples of 4 / 16)" % (c0, c2, hidden))
    out = np.empty(n, dtype=np.float32)
    check(lib.fnssl_lstm_pack(*[a.ctypes.data_as(C.c_void_p) for a in arrs], c0, c2, hidden,
                              out.ctypes.data_as(C.c_void_p)), "lstm_pack")
    return out


def pack_lstm(w_ih, w_hh, b_ih, b_hh, c0: int, c2: int, device) -> torch.Tensor:
    return torch.from_numpy(pack_lstm_host(w_ih, w_hh, b_ih, b_hh, c0, c2)).to(device)


def pack_lstm_bf16(w_ih, w_hh, b_ih, b_hh, c0: int, c2: int, device) -> torch.Tensor:
    """Weight stream of the bf16-MFMA kernels: weights rounded to bf16 (nearest even), bias fp32.
    c0, c2 multiples of 16, hidden a multiple of 32."""
    arrs = [np.ascontiguousarray(a.detach().float().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)
            for a in (w_ih, w_hh, b_ih, b_hh)]
    hidden = arrs[1].shape[1]
    if arrs[0].shape != (4 * hidden, c0 + c2) or arrs[1].shape != (4 * hidden, hidden):
        raise RuntimeError("fnssl.pack_lstm_bf16: weight shapes %s / %s do not match c0+c2=%d, H=%d"
                           % (arrs[0].shape, arrs[1].shape, c0 + c2, hidden))
    lib = _lib.load()
    n = lib.fnssl_lstm_packed_floats_bf16(c0, c2, hidden)
    if n == 0:
        raise RuntimeError("fnssl.pack_lstm_bf16: unsupported sizes c0=%d c2=%d H=%d (16 / 16 / 32)" % (c0, c2, hidden))
    out = np.empty(n, dtype=np.float32)
    check(lib.fnssl_lstm_pack_bf16(*[a.ctypes.data_as(C.c_void_p) for a in arrs], c0, c2, hidden,
                                   out.ctypes.data_as(C.c_void_p)), "lstm_pack_bf16")
    return torch.from_numpy(out).to(device)


def pack_lstm_bf16w(w_ih, w_hh, b_ih, b_hh, c0: int, c2: int, device) -> torch.Tensor:
    """Weight stream of the WIDE bf16 kernels (32 sequences per wave, lstm_bf16w.h): gate-row tiles of bf16
    A operands, the bias as three bf16 terms of a constant-one block.  c0, c2, hidden multiples of 16."""
    arrs = [np.ascontiguousarray(a.detach().float().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)
            for a in (w_ih, w_hh, b_ih, b_hh)]
    hidden = arrs[1].shape[1]
    if arrs[0].shape != (4 * hidden, c0 + c2) or arrs[1].shape != (4 * hidden, hidden):
        raise RuntimeError("fnssl.pack_lstm_bf16w: weight shapes %s / %s do not match c0+c2=%d, H=%d"
                           % (arrs[0].shape, arrs[1].shape, c0 + c2, hidden))
    lib = _lib.load()
    n = lib.fnssl_lstm_packed_floats_bf16w(c0, c2, hidden)
    if n == 0:
        raise RuntimeError("fnssl.pack_lstm_bf16w: unsupported sizes c0=%d c2=%d H=%d (multiples of 16)" % (c0, c2, hidden))
    out = np.empty(n, dtype=np.float32)
    check(lib.fnssl_lstm_pack_bf16w(*[a.ctypes.data_as(C.c_void_p) for a in arrs], c0, c2, hidden,
                                    out.ctypes.data_as(C.c_void_p)), "lstm_pack_bf16w")
    return torch.from_numpy(out).to(device)


def _view(t, mode):
    """4-D logical [nb, nt, nf, C] tensor -> (View, q_inner) for 'full' (seq=(b,t), step=f) or
    'narrow' (seq=(b,f), step=t)."""
    sb, st, sf, sc = t.stride()
    if sc != 1:
        raise RuntimeError("fnssl.lstm: channel dimension must be contiguous")
    if mode == "full":
        return View(t.data_ptr(), sb, st, sf)
    return View(t.data_ptr(), sb, sf, st)


def _conform(t):
    """Channel-contiguous, 16-byte aligned, strides multiples of 4 floats (8 bf16) — else copy (plumbing only)."""
    if t is None:
        return None
    m = 8 if t.dtype == torch.bfloat16 else 4
    ok = t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(s % m == 0 for s in t.stride()[:-1])
    return t if ok else t.contiguous()


_ws_cache = {}
_fb_counters = {}
_fb_nets = None      # weak set of DeviceNet objects (each owns the counter its fnssl_net hands to the library)


def fallback_counter(device):
    """The per-device int32 counter every LSTM call of this binding hands to the library unless the caller passes its own
    (fnssl_lstm_desc.fallback_count / fnssl_lstm_bwd_desc.fallback_count): launches whose cluster-resident kernel gave up on
    a hand-off and were recomputed by the guarded fallback kernels of the same call.  Results are correct either way; a
    non-zero count means the device could not keep a cluster's member workgroups resident (shared, partitioned or busy
    device) and throughput numbers taken meanwhile are not the kernels'."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    c = _fb_counters.get(device.index)
    if c is None:
        c = torch.zeros(1, dtype=torch.int32, device=device)
        _fb_counters[device.index] = c
    return c


def cluster_fallbacks(device=None, reset: bool = False) -> int:
    """Fallbacks counted on ``device`` so far: ``fallback_counter(device)`` plus the counters of the live ``DeviceNet``s
    (SYNCHRONISES the device: measurement code calls it outside timed regions).  ``reset``: zero them afterwards."""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    cs = [fallback_counter(device)] + [n.fallbacks for n in (_fb_nets or ()) if n.device == device or
                                       (n.device.index is None and device.index == torch.cuda.current_device())]
    total = sum(int(c.item()) for c in cs)
    if reset:
        for c in cs:
            c.zero_()
        for n in (_fb_nets or ()):
            n._fb_seen = 0
    return total



def _ws_key(device, tag: str):
    """Key of the workspace cache: (device index, that device's current stream, tag)."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return (device.index, torch.cuda.current_stream(device).cuda_stream, tag)


def _workspace(nbytes: int, device, tag: str):
    """Scratch buffer for one op, cached per (device, stream, tag): two forwards issued on different HIP streams
    never share scratch, and on one stream the ops that use a tag are ordered anyway.  A buffer that has to
    grow is replaced; the old one goes back to torch's caching allocator, which keeps it reserved for this
    stream's pending work."""
    key = _ws_key(device, tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=torch.device("cuda", key[0]))
        _ws_cache[key] = buf
    return buf


def release_workspaces():
    _ws_cache.clear()


@on_device
def lstm_layer(mode: str, x0, x1, x2, packed, hidden: int, out, variant: int = 0, skip=None, out_sum=None,
               reserve=None, carry_workspace=None, carry=False, bf16=False, wide=False, fallback_count=None, plan_only=False,
               tuning=None):
    """One (bi)LSTM layer over strided views.

    ``fallback_count`` (optional 1-element int32 device tensor, caller-zeroed): counts the layers whose cluster-resident
    kernel gave up on a hand-off and were recomputed by the guarded fallback kernels of the same call (results are
    correct either way).  ``tuning`` (a ``_lib.Tuning``, e.g. ``_lib.make_tuning(reserved_cus=16)``): this call's knobs
    instead of the process default (fnssl_lstm_desc.tuning).  ``plan_only=True`` launches nothing and returns ``(family, rounds)`` — the kernel family
    ``fnssl_lstm_forward`` takes for exactly this call (``_lib.LSTM_FAMILY`` names), see ``lstm_plan``.

    mode 'full': sequences are (b, t) rows, steps run over f; 'narrow': sequences (b, f), steps over t.
    x0 (+ x1) is the summed input, x2 the concatenated one (either may be None); all are logical
    [nb, nt, nf, C] tensors with arbitrary strides.  ``packed`` is a list of 1 or 2 device weight
    streams; ``out`` a logical [nb, nt, nf, ndir*hidden] tensor (any strides) that is written in place.
    With ``skip``/``out_sum`` (both logical [nb, nt, nf, ndir*hidden]; out_sum with out's strides) the
    kernel also stores out_sum = h + skip, i.e. the next layer's residual input.
    ``reserve`` (a float32 device buffer of ``lstm_reserve_floats`` elements) switches to the training
    forward, which also saves the gate activations and cell states for ``lstm_backward``.
    Streaming (uni-directional layers): pass a persistent ``carry_workspace`` (``lstm_state_workspace``); with
    ``carry=True`` the recurrence continues from the cell state in it and from the h row one step before
    ``out`` in memory (the caller's buffer holds the previous call's last h there).
    ``bf16=True``: ``packed`` comes from ``pack_lstm_bf16`` and the matrix product runs on bf16 MFMAs (operands
    rounded to bf16, fp32 accumulate; all tensors stay fp32).
    ``wide=True`` (with bf16): the 32-sequences-per-wave kernels — ``packed`` from ``pack_lstm_bf16w``; x0 / x2 /
    out may each be float32 or bfloat16 tensors (bf16 between layers: the values are rounded to bf16 on entry to
    the next MFMA anyway), no x1 / skip / reserve / carry.
    """
    if wide:
        _need_dev_act(x0, x2, out)
        _need_dev(x1, skip, out_sum, *packed)
    else:
        _need_dev(x0, x1, x2, out, skip, out_sum, *packed)
    if mode not in ("full", "narrow"):
        raise RuntimeError("fnssl.lstm_layer: mode must be 'full' or 'narrow'")
    ref = x0 if x0 is not None else x2
    if ref is None:
        raise RuntimeError("fnssl.lstm_layer: no input")
    x0, x1, x2 = _conform(x0), _conform(x1), _conform(x2)
    nb, nt, nf = ref.shape[:3]
    ndir = len(packed)
    if tuple(out.shape) != (nb, nt, nf, ndir * hidden):
        raise RuntimeError("fnssl.lstm_layer: out shape %s != %s" % (tuple(out.shape), (nb, nt, nf, ndir * hidden)))
    d = LstmDesc()
    if x0 is not None:
        d.src0 = _view(x0, mode)
        d.c0 = x0.shape[3]
    if x1 is not None:
        if x0 is None or x1.shape != x0.shape:
            raise RuntimeError("fnssl.lstm_layer: x1 must match x0")
        d.src1 = _view(x1, mode)
    if x2 is not None:
        d.src2 = _view(x2, mode)
        d.c2 = x2.shape[3]
    ov = _view(out, mode)
    d.out, d.out_so, d.out_si, d.out_st = ov.p, ov.so, ov.si, ov.st
    if (skip is None) != (out_sum is None):
        raise RuntimeError("fnssl.lstm_layer: skip and out_sum go together")
    if out_sum is not None:
        if out_sum.shape != out.shape or out_sum.stride() != out.stride() or skip.shape != out.shape:
            raise RuntimeError("fnssl.lstm_layer: out_sum must have out's shape and strides, skip out's shape")
        skip = _conform(skip)
        d.skip = _view(skip, mode)
        d.out_sum = out_sum.data_ptr()
    d.hidden, d.ndir = hidden, ndir
    d.nseq = nb * (nt if mode == "full" else nf)
    d.q_inner = nt if mode == "full" else nf
    d.nsteps = nf if mode == "full" else nt
    d.wpack[0] = packed[0].data_ptr()
    d.wpack[1] = packed[1].data_ptr() if ndir == 2 else 0
    lib = _lib.load()
    precision = (2 if wide else 1) if bf16 else 0
    wsb = lib.fnssl_lstm_workspace_bytes_ex(d.nseq, hidden, ndir, precision)
    if carry_workspace is not None:
        _need_dev(carry_workspace)
        if carry_workspace.numel() * 4 < wsb:
            raise RuntimeError("fnssl.lstm_layer: carry workspace too small")
        d.workspace, d.workspace_bytes = carry_workspace.data_ptr(), carry_workspace.numel() * 4
        d.carry_state = 1 if carry else 0
    else:
        if carry:
            raise RuntimeError("fnssl.lstm_layer: carry=True needs the persistent carry_workspace")
        ws = _workspace(wsb, out.device, "lstm")
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    d.variant = variant
    d.precision = precision
    if wide:
        if not bf16:
            raise RuntimeError("fnssl.lstm_layer: wide=True is a bf16 mode")
        d.f32_mask = ((1 if (x0 is not None and x0.dtype == torch.float32) else 0) |
                      (2 if (x2 is not None and x2.dtype == torch.float32) else 0) |
                      (4 if out.dtype == torch.float32 else 0))
    if reserve is not None:
        _need_dev(reserve)
        d.reserve, d.reserve_bytes = reserve.data_ptr(), reserve.numel() * 4
    if fallback_count is None:
        fallback_count = fallback_counter(out.device)
    if not isinstance(fallback_count, torch.Tensor) or not fallback_count.is_cuda or fallback_count.dtype != torch.int32 \
            or fallback_count.numel() < 1:
        raise RuntimeError("fnssl.lstm_layer: fallback_count must be an int32 device tensor")
    d.fallback_count = fallback_count.data_ptr()
    if tuning is not None:
        d.tuning = C.pointer(tuning)
    if plan_only:
        fam, rounds = C.c_int(0), C.c_int(0)
        check(lib.fnssl_lstm_plan(C.byref(d), C.byref(fam), C.byref(rounds)), "lstm_plan")
        return _lib.LSTM_FAMILY.get(int(fam.value), "unknown(%d)" % fam.value), int(rounds.value)
    check(lib.fnssl_lstm_forward(C.byref(d), _stream()), "lstm_forward")
    return out


def lstm_plan(*args, **kwargs):
    """``(family, rounds)`` of the ``lstm_layer`` call with the same arguments: which kernel family the library would
    launch on this device with the current environment, without launching anything (fnssl_lstm_plan)."""
    kwargs["plan_only"] = True
    return lstm_layer(*args, **kwargs)


def mfma_f32_peak(iters: int = 20000, waves_per_simd: int = 2, reps: int = 3, device=None) -> float:
    """The device's own fp32-MFMA ceiling in TFLOP/s (fnssl_mfma_f32_peak timed with HIP events on the current stream;
    best of ``reps``): the calibration bench.py reports as roofline.peak_measured."""
    lib = _lib.load()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    ncu = torch.cuda.get_device_properties(device).multi_processor_count
    out = torch.empty(ncu * waves_per_simd * 256, dtype=torch.float32, device=device)
    best = 0.0
    for r in range(reps + 1):
        flop = C.c_double(0.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.fnssl_mfma_f32_peak(out.data_ptr(), out.numel(), iters, waves_per_simd, C.byref(flop), _stream()), "mfma_f32_peak")
        e1.record()
        e1.synchronize()
        if r > 0:   # (the first launch carries the code-object load)
            best = max(best, flop.value / (e0.elapsed_time(e1) * 1e-3) / 1e12)
    return best


def mfma_f32_peak_sustained(seconds: float = 2.0, iters: int = 20000, waves_per_simd: int = 2, device=None) -> dict:
    """The same ceiling held for ``seconds`` of back-to-back launches (fnssl_mfma_f32_peak_clocks): what the matrix pipe
    delivers once the power / thermal management has settled, which is the regime the 85 – 115 ms LSTM kernels of a 10-s
    timed region run in — a 35-ms burst does not show it.  Returns TFLOP/s of the whole window and of its last quarter,
    and the clock (MHz, shader cycles per 100 MHz tick of wave 0 of every workgroup) per XCD during the LAST launch."""
    lib = _lib.load()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    ncu = torch.cuda.get_device_properties(device).multi_processor_count
    nblk = ncu * waves_per_simd
    out = torch.empty(nblk * 256, dtype=torch.float32, device=device)
    clk = torch.zeros(nblk * 3, dtype=torch.int64, device=device)
    flop = C.c_double(0.0)

    def launch(with_clocks):
        check(lib.fnssl_mfma_f32_peak_clocks(out.data_ptr(), out.numel(), iters, waves_per_simd, C.byref(flop),
                                             clk.data_ptr() if with_clocks else None, clk.numel() if with_clocks else 0,
                                             _stream()), "mfma_f32_peak_clocks")

    launch(False)                                       # code-object load + one-launch duration
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch(False)
    e1.record()
    e1.synchronize()
    one_ms = max(e0.elapsed_time(e1), 1e-3)
    n = max(4, int(seconds * 1e3 / one_ms + 0.999))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record()
    for k in range(n):
        launch(k == n - 1)
        ev[k + 1].record()
    ev[n].synchronize()
    total_ms = ev[0].elapsed_time(ev[n])
    q = max(1, n // 4)
    last_ms = ev[n - q].elapsed_time(ev[n])
    c = clk.cpu().numpy().reshape(nblk, 3)
    mhz = c[:, 0] / np.maximum(c[:, 1], 1) * 100.0
    per_xcd = {}
    for x in sorted(set(int(v) for v in c[:, 2])):
        m = mhz[c[:, 2] == x]
        per_xcd[x] = round(float(m.mean()), 1)
    return {"tflops": flop.value * n / (total_ms * 1e-3) / 1e12, "tflops_last_quarter": flop.value * q / (last_ms * 1e-3) / 1e12,
            "seconds": total_ms * 1e-3, "launches": n, "xcd_mhz": per_xcd,
            "slowest_xcd_mhz": min(per_xcd.values()), "fastest_xcd_mhz": max(per_xcd.values())}


def lstm_cluster_status(nseq: int, hidden: int, ndir: int, device=None) -> int:
    """Status word the cluster-resident LSTM kernels left in the current stream's LSTM workspace (0 = every hand-off
    arrived; otherwise the layer was recomputed by the guarded fallback kernels of the same call — see
    fnssl_lstm_cluster_status).  `nseq, hidden, ndir` as in the lstm_layer call that used the workspace."""
    lib = _lib.load()
    ws = _ws_cache.get(_ws_key("cuda" if device is None else device, "lstm"))
    if ws is None:
        raise RuntimeError("fnssl.lstm_cluster_status: no LSTM call has run on this device's current stream yet "
                           "(there is no LSTM workspace to read the status word from)")
    out = C.c_uint(0xffffffff)
    check(lib.fnssl_lstm_cluster_status(ws.data_ptr(), ws.numel(), nseq, hidden, ndir, _stream(), C.byref(out)),
          "lstm_cluster_status")
    return int(out.value)


def lstm_state_workspace(nseq: int, hidden: int, device):
    """Persistent per-layer cell-state buffer for streaming (uni-directional) LSTM calls."""
    n = _lib.load().fnssl_lstm_workspace_bytes_ex(nseq, hidden, 1, 0)
    return torch.zeros((n + 3) // 4, dtype=torch.float32, device=device)


def lstm_reserve_floats(nseq: int, hidden: int, ndir: int, nsteps: int) -> int:
    return _lib.load().fnssl_lstm_reserve_bytes(nseq, hidden, ndir, nsteps) // 4


def pack_lstm_bwd_host(w_ih, w_hh, c0g: int) -> np.ndarray:
    """Pack one direction's [W_ih[:, :c0g] | W_hh]^T into the backward kernel's weight stream."""
    arrs = [np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)
            for a in (w_ih, w_hh)]
    hidden = arrs[1].shape[1]
    c_in = arrs[0].shape[1]
    lib = _lib.load()
    n = lib.fnssl_lstm_bwd_packed_floats(c0g, hidden)
    if n == 0 or arrs[0].shape[0] != 4 * hidden or arrs[1].shape[0] != 4 * hidden:
        raise RuntimeError("fnssl.pack_lstm_bwd: unsupported sizes c0g=%d H=%d" % (c0g, hidden))
    out = np.empty(n, dtype=np.float32)
    check(lib.fnssl_lstm_pack_bwd(arrs[0].ctypes.data_as(C.c_void_p), arrs[1].ctypes.data_as(C.c_void_p), c_in, c0g,
                                  hidden, out.ctypes.data_as(C.c_void_p)), "lstm_pack_bwd")
    return out


@on_device
def lstm_backward(mode: str, reserve, dh, da, dx, packed_bwd, hidden: int, c0g: int, plan_only: bool = False,
                  status: bool = False, fallback_count=None, tuning=None):
    """Back-propagation through time of one (bi)LSTM layer.

    dh: upstream gradient, logical [nb, nt, nf, ndir*hidden]; da (written): logical [nb, nt, nf, ndir*4*hidden]
    pre-activation gate gradients; dx (written, or None when c0g == 0): logical [nb, nt, nf, ndir*c0g], one slab
    per direction.  ``mode`` as in lstm_layer.  ``plan_only``: launch nothing, return the kernel family name the call
    would take (fnssl_lstm_backward_plan); ``status``: also return the cluster kernel's status word (synchronises).
    ``fallback_count`` (int32 device tensor, caller-zeroed): incremented when the cluster-resident BPTT kernel gave up on a
    hand-off and the split kernels of the same call recomputed the layer; ``tuning``: this call's knobs (a ``_lib.Tuning``)."""
    _need_dev(reserve, dh, da, dx, *packed_bwd)
    ndir = len(packed_bwd)
    nb, nt, nf = dh.shape[:3]
    if tuple(dh.shape) != (nb, nt, nf, ndir * hidden) or tuple(da.shape) != (nb, nt, nf, ndir * 4 * hidden):
        raise RuntimeError("fnssl.lstm_backward: dh / da shapes %s / %s" % (tuple(dh.shape), tuple(da.shape)))
    if (c0g > 0) != (dx is not None) or (dx is not None and tuple(dx.shape) != (nb, nt, nf, ndir * c0g)):
        raise RuntimeError("fnssl.lstm_backward: dx must be [nb, nt, nf, ndir*c0g] (None when c0g == 0)")
    dh = _conform(dh)
    d = LstmBwdDesc()
    d.reserve = reserve.data_ptr()
    d.dh = _view(dh, mode)
    v = _view(da, mode)
    d.da, d.da_so, d.da_si, d.da_st = v.p, v.so, v.si, v.st
    if dx is not None:
        v = _view(dx, mode)
        d.dx, d.dx_so, d.dx_si, d.dx_st = v.p, v.so, v.si, v.st
    d.c0g, d.hidden, d.ndir = c0g, hidden, ndir
    d.nseq = nb * (nt if mode == "full" else nf)
    d.q_inner = nt if mode == "full" else nf
    d.nsteps = nf if mode == "full" else nt
    if reserve.numel() < lstm_reserve_floats(d.nseq, hidden, ndir, d.nsteps):
        raise RuntimeError("fnssl.lstm_backward: reserve buffer too small")
    d.wpack_bwd[0] = packed_bwd[0].data_ptr()
    d.wpack_bwd[1] = packed_bwd[1].data_ptr() if ndir == 2 else 0
    lib = _lib.load()
    ws = _workspace(lib.fnssl_lstm_bwd_workspace_bytes(d.nseq, hidden, ndir), dh.device, "lstm_bwd")
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    if fallback_count is None:
        fallback_count = fallback_counter(dh.device)
    if not isinstance(fallback_count, torch.Tensor) or not fallback_count.is_cuda or fallback_count.dtype != torch.int32:
        raise RuntimeError("fnssl.lstm_backward: fallback_count must be an int32 device tensor")
    d.fallback_count = fallback_count.data_ptr()
    if tuning is not None:
        d.tuning = C.pointer(tuning)
    if plan_only:
        fam = C.c_int(0)
        check(lib.fnssl_lstm_backward_plan(C.byref(d), C.byref(fam)), "lstm_backward_plan")
        return _lib.LSTM_FAMILY[fam.value]
    check(lib.fnssl_lstm_backward(C.byref(d), _stream()), "lstm_backward")
    if status:
        word = C.c_uint(0)
        check(lib.fnssl_lstm_backward_status(ws.data_ptr(), ws.numel(), d.nseq, hidden, ndir, _stream(), C.byref(word)),
              "lstm_backward_status")
        return da, dx, word.value
    return da, dx


# --------------------------------------------------------------------------- #
# causal 3x3 conv + time pooling (IPDnet head)
# --------------------------------------------------------------------------- #
def pack_conv3x3(weight, ca: int, cb: int, device, bf16: bool = False) -> torch.Tensor:
    """Pack a Conv2d weight [cout, ca + cb, 3, 3] into the conv kernel's weight stream (``bf16``: the bf16-MFMA
    stream; ca, cb multiples of 16)."""
    w = np.ascontiguousarray(weight.detach().float().cpu().numpy() if isinstance(weight, torch.Tensor) else weight,
                             dtype=np.float32)
    cout = w.shape[0]
    if w.shape != (cout, ca + cb, 3, 3):
        raise RuntimeError("fnssl.pack_conv3x3: weight shape %s does not match [cout, %d + %d, 3, 3]"
                           % (w.shape, ca, cb))
    lib = _lib.load()
    n = (lib.fnssl_conv3x3_packed_floats_bf16 if bf16 else lib.fnssl_conv3x3_packed_floats)(cout, ca, cb)
    if n == 0:
        raise RuntimeError("fnssl.pack_conv3x3: unsupported sizes cout=%d ca=%d cb=%d" % (cout, ca, cb))
    out = np.empty(n, dtype=np.float32)
    check((lib.fnssl_conv3x3_pack_bf16 if bf16 else lib.fnssl_conv3x3_pack)(
        w.ctypes.data_as(C.c_void_p), cout, ca, cb, out.ctypes.data_as(C.c_void_p)), "conv3x3_pack")
    return torch.from_numpy(out).to(device)


@on_device
def conv3x3_causal(xa, xb, packed, cout: int, act: str = "none", bf16: bool = False):
    """Causal 3x3 conv over (bin, time) of the channel concatenation [xa | xb].

    xa / xb: logical [nb, nf, nt, C] tensors with arbitrary batch / bin / time strides and a
    contiguous channel dimension (xb may be None).  Returns [nb, nf, nt, ceil4(cout)] channels-last
    (padding channels are 0)."""
    _need_dev_act(xa)
    _need_dev(xb, packed)
    a_bf = xa.dtype == torch.bfloat16
    if a_bf and not bf16:
        raise RuntimeError("fnssl.conv3x3_causal: a bfloat16 input needs the bf16 kernel (bf16=True)")
    xa, xb = _conform(xa), _conform(xb)
    nb, nf, nt, ca = xa.shape
    cb = 0 if xb is None else xb.shape[3]
    if xb is not None and tuple(xb.shape[:3]) != (nb, nf, nt):
        raise RuntimeError("fnssl.conv3x3_causal: xb must match xa's [nb, nf, nt]")
    if xa.stride(3) != 1 or (xb is not None and xb.stride(3) != 1):
        raise RuntimeError("fnssl.conv3x3_causal: channel dimension must be contiguous")
    cs = (cout + 3) // 4 * 4
    out = torch.empty((nb, nf, nt, cs), dtype=torch.float32, device=xa.device)   # pad channels come out 0
    sa = xa.stride()
    sb_ = xb.stride() if xb is not None else (0, 0, 0, 1)
    code = {"none": 0, "relu": 1, "tanh": 2}[act]
    lib = _lib.load()
    fn = (lib.fnssl_conv3x3_causal_bf16a if a_bf else lib.fnssl_conv3x3_causal_bf16) if bf16 else lib.fnssl_conv3x3_causal
    check(fn(_ptr(xa), sa[0], sa[1], sa[2], ca,
             _ptr(xb) if xb is not None else None, sb_[0], sb_[1], sb_[2], cb,
             _ptr(packed), cout, nb, nf, nt, code, _ptr(out), cs, _stream()),
          "conv3x3_causal")
    return out


def conv3x3_bf16x_supported(cout: int, ca: int, cb: int) -> bool:
    """Whether the LDS-staged bf16 conv kernel (conv_bf16x.hip) takes these channel counts."""
    return _lib.load().fnssl_conv3x3_packed_bytes_bf16x(cout, ca, cb) > 0


def pack_conv3x3_bf16x(weight, ca: int, cb: int, device) -> torch.Tensor:
    """Pack a Conv2d weight [cout, ca + cb, 3, 3] into the weight stream of ``conv3x3_causal_bf16x``."""
    w = np.ascontiguousarray(weight.detach().float().cpu().numpy() if isinstance(weight, torch.Tensor) else weight,
                             dtype=np.float32)
    cout = w.shape[0]
    if w.shape != (cout, ca + cb, 3, 3):
        raise RuntimeError("fnssl.pack_conv3x3_bf16x: weight shape %s does not match [cout, %d + %d, 3, 3]"
                           % (w.shape, ca, cb))
    lib = _lib.load()
    n = lib.fnssl_conv3x3_packed_bytes_bf16x(cout, ca, cb)
    if n == 0:
        raise RuntimeError("fnssl.pack_conv3x3_bf16x: unsupported sizes cout=%d ca=%d cb=%d" % (cout, ca, cb))
    out = np.empty(n // 4, dtype=np.float32)       # raw stream bytes, carried as a float32 tensor like the others
    check(lib.fnssl_conv3x3_pack_bf16x(w.ctypes.data_as(C.c_void_p), cout, ca, cb, out.ctypes.data_as(C.c_void_p)),
          "conv3x3_pack_bf16x")
    return torch.from_numpy(out).to(device)


@on_device
def conv3x3_causal_bf16x(xa, xb, packed, cout: int, act: str = "none", pool: int = 1, bf16_out: bool = False):
    """``conv3x3_causal`` for a bfloat16 ``xa`` (and an optional fp32 ``xb``) through the LDS-staged kernel, with the
    time pooling that follows it in CausCnnBlock fused into the epilogue (``pool`` 1 / 3 / 4).
    Returns [nb, nf, nt // pool, cout], float32 or (``bf16_out``) bfloat16."""
    _need_dev_act(xa)
    _need_dev(xb, packed)
    if xa.dtype != torch.bfloat16 or (xb is not None and xb.dtype != torch.float32):
        raise RuntimeError("fnssl.conv3x3_causal_bf16x: xa must be bfloat16 and xb float32")
    nb, nf, nt, ca = xa.shape
    cb = 0 if xb is None else xb.shape[3]
    if xb is not None and tuple(xb.shape[:3]) != (nb, nf, nt):
        raise RuntimeError("fnssl.conv3x3_causal_bf16x: xb must match xa's [nb, nf, nt]")
    if xa.stride(3) != 1 or (xb is not None and xb.stride(3) != 1):
        raise RuntimeError("fnssl.conv3x3_causal_bf16x: channel dimension must be contiguous")
    out = torch.empty((nb, nf, nt // pool, cout), dtype=torch.bfloat16 if bf16_out else torch.float32, device=xa.device)
    if out.numel() == 0:
        return out
    sa = xa.stride()
    sb_ = xb.stride() if xb is not None else (0, 0, 0, 1)
    code = {"none": 0, "relu": 1, "tanh": 2}[act]
    check(_lib.load().fnssl_conv3x3_causal_bf16x(
        _ptr(xa), sa[0], sa[1], sa[2], ca, _ptr(xb) if xb is not None else None, sb_[0], sb_[1], sb_[2], cb,
        _ptr(packed), cout, nb, nf, nt, code, pool, int(bf16_out), _ptr(out), cout, _stream()), "conv3x3_causal_bf16x")
    return out


@on_device
def avgpool_time(x, k: int, bf16_out: bool = False):
    """[nb, nf, nt, C] channels-last -> [nb, nf, nt // k, C] (AvgPool2d((1, k)) of the NCHW view); ``bf16_out``
    rounds the result to bfloat16 (the operand rounding of the bf16 conv that follows, done once here)."""
    _need_dev(x)
    x = x.contiguous()
    nb, nf, nt, c = x.shape
    y = torch.empty((nb, nf, nt // k, c), dtype=torch.bfloat16 if bf16_out else torch.float32, device=x.device)
    if y.numel():
        fn = _lib.load().fnssl_avgpool_time_bf16 if bf16_out else _lib.load().fnssl_avgpool_time
        check(fn(_ptr(x), nb * nf, nt, c, k, _ptr(y), _stream()), "avgpool_time")
    return y


def pack_conv3x3_backward_data(weight, cin_g: int, device) -> torch.Tensor:
    """Pack a Conv2d weight [cout, cin, 3, 3] (transposed, bin-flipped) for ``conv3x3_causal_backward_data`` — the
    gradient of the first ``cin_g`` input channels."""
    w = np.ascontiguousarray(weight.detach().float().cpu().numpy() if isinstance(weight, torch.Tensor) else weight,
                             dtype=np.float32)
    if w.ndim != 4 or w.shape[2:] != (3, 3):
        raise RuntimeError("fnssl.pack_conv3x3_backward_data: weight shape %s is not [cout, cin, 3, 3]" % (w.shape,))
    cout, cin = w.shape[:2]
    lib = _lib.load()
    n = lib.fnssl_conv3x3_packed_floats_backward_data(cout, cin, cin_g)
    if n == 0:
        raise RuntimeError("fnssl.pack_conv3x3_backward_data: unsupported sizes cout=%d cin=%d cin_g=%d" % (cout, cin, cin_g))
    out = np.empty(n, dtype=np.float32)
    check(lib.fnssl_conv3x3_pack_backward_data(w.ctypes.data_as(C.c_void_p), cout, cin, cin_g,
                                               out.ctypes.data_as(C.c_void_p)), "conv3x3_pack_backward_data")
    return torch.from_numpy(out).to(device)


def _chlast(t, what):
    """A logical [nb, nf, nt, C] fp32 device tensor with a contiguous channel dimension, 16-byte aligned, strides
    multiples of 4 floats (else a copy: plumbing only)."""
    if t.dim() != 4 or t.dtype != torch.float32:
        raise RuntimeError("fnssl.%s: expected a 4-D float32 tensor, got %s %s" % (what, tuple(t.shape), t.dtype))
    return _conform(t)


@on_device
def conv3x3_act_pool_backward(dp, y, k: int, act: str):
    """Activation + AvgPool2d((1, k)) backward of one CausCnnBlock stage: y [nb, nf, nt, C] (saved post-activation
    output), dp [nb, nf, nt // k, C] -> dz [nb, nf, nt, C] (pre-activation gradient), all channels-last."""
    _need_dev(dp, y)
    y, dp = y.contiguous(), dp.contiguous()
    nb, nf, nt, c = y.shape
    if tuple(dp.shape) != (nb, nf, nt // k, c):
        raise RuntimeError("fnssl.conv3x3_act_pool_backward: dp %s does not match y %s pooled by %d"
                           % (tuple(dp.shape), tuple(y.shape), k))
    dz = torch.empty_like(y)
    check(_lib.load().fnssl_conv3x3_act_pool_backward(_ptr(dp), _ptr(y), nb, nf, nt, c, k,
                                                      {"none": 0, "relu": 1, "tanh": 2}[act], _ptr(dz), _stream()),
          "conv3x3_act_pool_backward")
    return dz


@on_device
def conv3x3_causal_backward_data(dz, packed, cin_g: int, out=None):
    """Input gradient of ``conv3x3_causal`` for its first ``cin_g`` input channels.  dz: the pre-activation gradient,
    logical [nb, nf, nt, cout] (any batch / bin / time strides); ``packed`` from ``pack_conv3x3_backward_data``.
    Returns (or writes into ``out``, a contiguous [nb, nf, nt, >= cin_g] tensor) dx [nb, nf, nt, cin_g]."""
    _need_dev(dz, packed, out)
    dz = _chlast(dz, "conv3x3_causal_backward_data")
    nb, nf, nt, cout = dz.shape
    if out is None:
        out = torch.empty((nb, nf, nt, cin_g), dtype=torch.float32, device=dz.device)
    if tuple(out.shape[:3]) != (nb, nf, nt) or out.shape[3] < cin_g or not out.is_contiguous():
        raise RuntimeError("fnssl.conv3x3_causal_backward_data: out must be a contiguous [%d, %d, %d, >= %d] tensor"
                           % (nb, nf, nt, cin_g))
    s = dz.stride()
    check(_lib.load().fnssl_conv3x3_causal_backward_data(_ptr(dz), s[0], s[1], s[2], cout, _ptr(packed), cin_g, nb, nf,
                                                         nt, _ptr(out), out.shape[3], _stream()),
          "conv3x3_causal_backward_data")
    return out


@on_device
def conv3x3_weight_grads(dz, xa, xb, grad):
    """grad [cout, ca + cb, 3, 3] += the weight gradient of ``conv3x3_causal(xa, xb, ...)`` given its pre-activation
    gradient dz [nb, nf, nt, cout]; xa / xb / dz logical [nb, nf, nt, C] with any batch / bin / time strides."""
    _need_dev(dz, xa, xb, grad)
    dz = _chlast(dz, "conv3x3_weight_grads")
    xa = _chlast(xa, "conv3x3_weight_grads")
    xb = _chlast(xb, "conv3x3_weight_grads") if xb is not None else None
    nb, nf, nt, cout = dz.shape
    ca = xa.shape[3]
    cb = 0 if xb is None else xb.shape[3]
    if tuple(xa.shape[:3]) != (nb, nf, nt) or (xb is not None and tuple(xb.shape[:3]) != (nb, nf, nt)):
        raise RuntimeError("fnssl.conv3x3_weight_grads: xa / xb must match dz's [nb, nf, nt]")
    if tuple(grad.shape) != (cout, ca + cb, 3, 3) or not grad.is_contiguous() or grad.dtype != torch.float32:
        raise RuntimeError("fnssl.conv3x3_weight_grads: grad must be a contiguous fp32 [%d, %d, 3, 3]" % (cout, ca + cb))
    lib = _lib.load()
    ws = _workspace(lib.fnssl_conv3x3_weight_grads_workspace_bytes(nb, nf, nt, cout, ca, cb), dz.device, "conv_wgrad")
    sz, sa = dz.stride(), xa.stride()
    sb_ = xb.stride() if xb is not None else (0, 0, 0, 1)
    check(lib.fnssl_conv3x3_weight_grads(_ptr(dz), sz[0], sz[1], sz[2], cout, _ptr(xa), sa[0], sa[1], sa[2], ca,
                                         _ptr(xb) if xb is not None else None, sb_[0], sb_[1], sb_[2], cb, nb, nf, nt,
                                         _ptr(grad), _ptr(ws), ws.numel(), _stream()), "conv3x3_weight_grads")
    return grad


@on_device
def lstm_weight_grads(da, x0, x2, h, hidden: int, ndir: int, nsteps: int, g_wih, g_whh, g_bih, g_bhh):
    """Accumulate one LSTM layer's weight gradients (``fnssl_lstm_weight_grads``, csrc/wgrad.hip): g_wih[d] [4H, c0+c2]
    += dA_d^T [x0 | x2], g_whh[d] [4H, H] += dA_d^T h_prev_d, g_bih[d] = g_bhh[d] [4H] += sum_r dA_d[r].
    da [rows, ndir*4H], x0 [rows, c0] / x2 [rows, c2] (either may be None), h [rows, ndir*H]: row-major matrices with
    rows = sequences x steps in the layer's natural layout (any row stride).  g_*: lists of ndir contiguous tensors."""
    from ._lib import WgradDesc
    _need_dev(da, x0, x2, h, *g_wih, *g_whh, *g_bih, *g_bhh)
    rows = da.shape[0]
    d = WgradDesc()
    d.da, d.lda = _ptr(da), da.stride(0)
    d.x0, d.ldx0, d.c0 = (_ptr(x0), x0.stride(0), x0.shape[1]) if x0 is not None else (None, 0, 0)
    d.x2, d.ldx2, d.c2 = (_ptr(x2), x2.stride(0), x2.shape[1]) if x2 is not None else (None, 0, 0)
    d.h, d.ldh = _ptr(h), h.stride(0)
    for t in (da, x0, x2, h):
        if t is not None and (t.stride(1) != 1 or t.dtype != torch.float32):
            raise RuntimeError("fnssl.lstm_weight_grads: operands must be fp32 row-major matrices")
    if rows % nsteps or h.shape[0] != rows or da.shape[1] != ndir * 4 * hidden or h.shape[1] != ndir * hidden:
        raise RuntimeError("fnssl.lstm_weight_grads: shapes da %s / h %s do not match hidden %d, ndir %d, nsteps %d"
                           % (tuple(da.shape), tuple(h.shape), hidden, ndir, nsteps))
    d.nseq, d.nsteps, d.hidden, d.ndir = rows // nsteps, nsteps, hidden, ndir
    for k in range(ndir):
        for name, lst, shape in (("g_wih", g_wih, (4 * hidden, d.c0 + d.c2)), ("g_whh", g_whh, (4 * hidden, hidden)),
                                 ("g_bih", g_bih, (4 * hidden,)), ("g_bhh", g_bhh, (4 * hidden,))):
            t = lst[k]
            if tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32:
                raise RuntimeError("fnssl.lstm_weight_grads: %s[%d] must be a contiguous fp32 %s" % (name, k, shape))
            getattr(d, name)[k] = t.data_ptr()
    lib = _lib.load()
    ws = _workspace(lib.fnssl_lstm_weight_grads_workspace_bytes(rows, hidden, ndir, d.c0, d.c2), da.device, "wgrad")
    d.workspace, d.workspace_bytes = _ptr(ws), ws.numel()
    check(lib.fnssl_lstm_weight_grads(C.byref(d), _stream()), "lstm_weight_grads")


# --------------------------------------------------------------------------- #
# head / whole network
# --------------------------------------------------------------------------- #
@on_device
def head(x, w, b):
    """x [nb, nf, nt, 256] -> [nb, nt//12, 2*nf]  (Model.py:79-87)."""
    _need_dev(x, w, b)
    x = x.contiguous()
    nb, nf, nt, c = x.shape
    if c != 256:
        raise RuntimeError("fnssl.head: emb2ipd is Linear(256, 2); got %d channels" % c)
    out = torch.empty((nb, nt // SEG_FRAMES, 2 * nf), dtype=torch.float32, device=x.device)
    check(_lib.load().fnssl_head(_ptr(x), nb, nf, nt, _ptr(w.contiguous()), _ptr(b.contiguous()), _ptr(out),
                                 _stream()), "head")
    return out


@on_device
def linear(x, wt, b):
    """y = x @ wt + b with wt = weight^T [k, n_out]."""
    _need_dev(x, wt, b)
    x = x.contiguous()
    k = x.shape[-1]
    m = x.numel() // k
    n_out = wt.shape[1]
    y = torch.empty(tuple(x.shape[:-1]) + (n_out,), dtype=torch.float32, device=x.device)
    check(_lib.load().fnssl_linear(_ptr(x), m, k, _ptr(wt.contiguous()), _ptr(b), n_out, _ptr(y), _stream()),
          "linear")
    return y


class DeviceNet:
    """Device-resident packed parameters of an FN_SSL network (the ``fnssl_net`` struct)."""

    def __init__(self, state: dict, device, is_online: bool = True, is_doa: bool = False, input_size: int = 4,
                 prefix: str = ""):
        self.device = torch.device(device)
        self.is_online, self.is_doa, self.input_size = bool(is_online), bool(is_doa), int(input_size)
        self._keep = []
        net = Net()
        g = lambda k: state[prefix + k]  # noqa: E731
        for blk in range(3):
            bp = "block_%d." % (blk + 1)
            fin = input_size if blk == 0 else 256
            specs = [("fullLstm.", fin, 0, True),
                     ("narrLstm.", 256, input_size if blk == 0 else 0, not is_online)]
            for li, (lp, c0, c2, bidir) in enumerate(specs):
                for di, sfx in enumerate(["", "_reverse"] if bidir else [""]):
                    t = pack_lstm(g(bp + lp + "weight_ih_l0" + sfx), g(bp + lp + "weight_hh_l0" + sfx),
                                  g(bp + lp + "bias_ih_l0" + sfx), g(bp + lp + "bias_hh_l0" + sfx), c0, c2,
                                  self.device)
                    self._keep.append(t)
                    net.wpack[blk][li][di] = t.data_ptr()
        self.emb_w = self._dev(g("emb2ipd.weight"))
        self.emb_b = self._dev(g("emb2ipd.bias"))
        net.emb_w, net.emb_b = self.emb_w.data_ptr(), self.emb_b.data_ptr()
        if is_doa:
            self.doa_wt = self._dev(g("ipd2doa.weight")).t().contiguous()
            self.doa_b = self._dev(g("ipd2doa.bias"))
            net.doa_wt, net.doa_b = self.doa_wt.data_ptr(), self.doa_b.data_ptr()
        net.input_size, net.is_online = self.input_size, int(self.is_online)
        # layers whose cluster-resident kernel gave up on a hand-off and were recomputed by the guarded fallback kernels of
        # the same call (fnssl_lstm_forward): counted on the device, read back asynchronously (4 bytes per forward, no
        # synchronisation) and reported one forward later as a RuntimeWarning — results are correct either way
        self.fallbacks = torch.zeros(1, dtype=torch.int32, device=self.device)
        global _fb_nets
        if _fb_nets is None:
            import weakref
            _fb_nets = weakref.WeakSet()
        _fb_nets.add(self)
        self._fb_host = torch.zeros(1, dtype=torch.int32).pin_memory() if self.device.type == "cuda" else None
        self._fb_event, self._fb_seen = None, 0
        net.fallback_count = self.fallbacks.data_ptr()
        self.net = net

    def _report_fallbacks(self):
        if self._fb_event is not None and self._fb_event.query():
            n = int(self._fb_host[0])
            if n > self._fb_seen:
                import warnings
                warnings.warn("fnssl: %d LSTM layer launch(es) so far could not keep every member workgroup of a cluster-resident "
                              "kernel resident (shared, partitioned or busy device?) and were recomputed by the per-wave kernels: "
                              "results are unaffected, throughput is" % n, RuntimeWarning, stacklevel=3)
                self._fb_seen = n
            self._fb_event = None

    def _poll_fallbacks(self):
        if self._fb_host is not None and self._fb_event is None:
            self._fb_host.copy_(self.fallbacks, non_blocking=True)
            self._fb_event = torch.cuda.Event()
            self._fb_event.record(torch.cuda.current_stream(self.device))

    def _dev(self, a):
        t = a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, dtype=np.float32))
        return t.to(self.device, torch.float32).contiguous()

    def _run(self, x0, out, chunk_pairs):
        nb, nt, nf, _ = x0.shape
        lib = _lib.load()
        ws = _workspace(lib.fnssl_forward_workspace_bytes(nb, nf, nt, int(self.is_online), chunk_pairs), x0.device, "forward")
        check(lib.fnssl_forward(C.byref(self.net), _ptr(x0), nb, nf, nt, _ptr(out), _ptr(ws), ws.numel(),
                                chunk_pairs, _stream()), "forward")

    @on_device
    def forward(self, x0: torch.Tensor, chunk_pairs: int = 0) -> torch.Tensor:
        """x0 [nb', nt, nf, input_size] -> [nb', nt//12, 2*nf] (or [.., 180] with the DOA layer)."""
        _need_dev(x0)
        x0 = x0.contiguous()
        nb, nt, nf, cin = x0.shape
        if cin != self.input_size:
            raise RuntimeError("fnssl.forward: expected %d input channels, got %d" % (self.input_size, cin))
        last = 180 if self.is_doa else 2 * nf
        out = torch.empty((nb, nt // SEG_FRAMES, last), dtype=torch.float32, device=x0.device)
        self._report_fallbacks()
        self._run(x0, out, chunk_pairs)
        self._poll_fallbacks()
        return out


# --------------------------------------------------------------------------- #
# measurement hooks
# --------------------------------------------------------------------------- #
@on_device
def occupy_cus(nblocks: int, stop, max_ms: int = 2000, lds_bytes: int = 160 * 1024, stream=None):
    """Diagnostic (fnssl_occupy_cus): ``nblocks`` workgroups, each holding ``lds_bytes`` of LDS (default: a whole CU), idle on
    ``stream`` (default: the current one) until ``stop[0]`` is non-zero or ``max_ms`` pass — what RCCL's persistent all-reduce
    kernels do to the CUs under an overlapped backward.  ``stop``: int32 tensor of 1 + nblocks words in pinned host (or
    device) memory, zeroed by the caller; workgroup b sets ``stop[1 + b]`` when it has become resident."""
    if stop.dtype != torch.int32 or stop.numel() < 1 + int(nblocks):
        raise RuntimeError("fnssl.occupy_cus: stop must hold 1 + nblocks int32 words")
    s = C.c_void_p(stream.cuda_stream) if stream is not None else _stream()
    check(_lib.load().fnssl_occupy_cus(int(nblocks), int(lds_bytes), C.c_void_p(stop.data_ptr()), int(max_ms), s), "occupy_cus")



def timing_enable(on: bool):
    check(_lib.load().fnssl_timing_enable(1 if on else 0), "timing_enable")


def timing_select(name=None):
    """Bracket only launches of kernel ``name`` (None: all)."""
    check(_lib.load().fnssl_timing_select(name.encode() if name else None), "timing_select")


def timing_collect(cap: int = 64):
    names = ((C.c_char * 64) * cap)()
    ms = (C.c_double * cap)()
    cnt = (C.c_longlong * cap)()
    fl = (C.c_double * cap)()
    n = _lib.load().fnssl_timing_collect(cap, names, ms, cnt, fl)
    return {names[i].value.decode(): {"ms": ms[i], "count": cnt[i], "flops": fl[i]} for i in range(n)}


# --------------------------------------------------------------------------- #
# room simulation (csrc/rir.hip; the gpuRIR-named surface is fnssl/rir.py)
# --------------------------------------------------------------------------- #
def _rir_host(room_sz, beta, nb_img):
    room = [float(v) for v in np.asarray(room_sz, dtype=np.float64).reshape(-1)]
    bet = [float(v) for v in np.asarray(beta, dtype=np.float64).reshape(-1)]
    if len(room) != 3 or len(bet) != 6:
        raise ValueError("fnssl.rir: room_sz has 3 entries and beta 6, got %d and %d" % (len(room), len(bet)))
    out = [(C.c_float * 3)(*room), (C.c_float * 6)(*bet)]
    if nb_img is not None:
        nb = [int(v) for v in np.asarray(nb_img).reshape(-1)]
        if len(nb) != 3:
            raise ValueError("fnssl.rir: nb_img has 3 entries, got %d" % len(nb))
        out.append((C.c_int * 3)(*nb))
    return out


def rir_plan(m_src: int, m_rcv: int, nb_img, nism: int, cus: int = 0) -> dict:
    """Host only (fnssl_rir_plan): the image chunks per RIR and the launch geometry ``rir_ism`` takes for these sizes on a
    device of ``cus`` compute units (0: the current device)."""
    nb = (C.c_int * 3)(*[int(v) for v in nb_img])
    info = _lib.RirPlanInfo()
    check(_lib.load().fnssl_rir_plan(int(m_src), int(m_rcv), C.byref(nb), int(nism), int(cus), C.byref(info)), "rir_plan")
    return {n: int(getattr(info, n)) for n, _ in _lib.RirPlanInfo._fields_}


def _rir_positions(pos_src, pos_rcv):
    _need_dev(pos_src, pos_rcv)
    if pos_src.ndim != 2 or pos_src.shape[1] != 3 or pos_rcv.ndim != 2 or pos_rcv.shape[1] != 3:
        raise RuntimeError("fnssl.rir: positions are [M, 3], got %s and %s" % (tuple(pos_src.shape), tuple(pos_rcv.shape)))
    return pos_src.contiguous(), pos_rcv.contiguous()


@on_device
def rir_ism(pos_src, pos_rcv, room_sz, beta, nb_img, nism: int, nsamples: int, fs: float, c: float = 343.0, out=None):
    """Image-source part (fnssl_rir_ism): pos_src [M_src, 3], pos_rcv [M_rcv, 3] -> RIRs [M_src, M_rcv, nsamples] with samples
    [0, nism) written (the rest zero unless ``out`` is given)."""
    pos_src, pos_rcv = _rir_positions(pos_src, pos_rcv)
    room, bet, nb = _rir_host(room_sz, beta, nb_img)
    ms, mr = pos_src.shape[0], pos_rcv.shape[0]
    lib = _lib.load()
    if out is None:
        out = torch.zeros((ms, mr, int(nsamples)), dtype=torch.float32, device=pos_src.device)
    else:
        _need_dev(out)
        if tuple(out.shape) != (ms, mr, int(nsamples)) or not out.is_contiguous() or out.device != pos_src.device:
            raise RuntimeError("fnssl.rir_ism: out must be a contiguous [%d, %d, %d] on %s, got %s on %s"
                               % (ms, mr, int(nsamples), pos_src.device, tuple(out.shape), out.device))
    wsb = lib.fnssl_rir_workspace_bytes(ms, mr, C.byref(nb), int(nism), 0)
    ws = torch.empty(max(wsb, 4) // 4, dtype=torch.float32, device=pos_src.device)
    check(lib.fnssl_rir_ism(C.byref(room), C.byref(bet), _ptr(pos_src), ms, _ptr(pos_rcv), mr, C.byref(nb), int(nism),
                            int(nsamples), float(fs), float(c), _ptr(out), _ptr(ws), ws.numel() * 4, _stream()), "rir_ism")
    return out


@on_device
def rir_tail(rir, pos_src, pos_rcv, room_sz, beta, nism: int, fs: float, c: float = 343.0, seed: int = 0):
    """Diffuse tail (fnssl_rir_tail), in place: samples [nism, nsamples) of ``rir`` [M_src, M_rcv, nsamples] from its samples
    [0, nism).  Returns ``rir``."""
    pos_src, pos_rcv = _rir_positions(pos_src, pos_rcv)
    _need_dev(rir)
    ms, mr = pos_src.shape[0], pos_rcv.shape[0]
    if rir.ndim != 3 or tuple(rir.shape[:2]) != (ms, mr) or not rir.is_contiguous():
        raise RuntimeError("fnssl.rir_tail: expected a contiguous [%d, %d, nSamples], got %s" % (ms, mr, tuple(rir.shape)))
    room, bet = _rir_host(room_sz, beta, None)
    check(_lib.load().fnssl_rir_tail(C.byref(room), C.byref(bet), _ptr(pos_src), ms, _ptr(pos_rcv), mr, int(nism),
                                     int(rir.shape[2]), float(fs), float(c), int(seed) & (2 ** 64 - 1), _ptr(rir), _stream()),
          "rir_tail")
    return rir


@on_device
def rir_trajectory_batch(signals, rirs, w_inis):
    """Moving-source mixing of several independent (signal [ns], RIRs [npts, M, len], w_ini int32 [npts + 1]) triples in one
    launch (fnssl_rir_trajectory) -> list of [ns + len - 1, M]."""
    n = len(signals)
    if not (n == len(rirs) == len(w_inis)) or n < 1:
        raise RuntimeError("fnssl.rir_trajectory_batch: %d signals, %d RIR sets, %d w_ini" % (n, len(rirs), len(w_inis)))
    outs, keep = [], []
    items = (_lib.RirTrajItem * _lib.RIR_TRAJ_MAX_BATCH)()
    lib = _lib.load()
    for k0 in range(0, n, _lib.RIR_TRAJ_MAX_BATCH):
        k1 = min(n, k0 + _lib.RIR_TRAJ_MAX_BATCH)
        for k in range(k0, k1):
            x, r, w = signals[k], rirs[k], w_inis[k]
            _need_dev(x, r)
            if not isinstance(w, torch.Tensor) or not w.is_cuda or w.dtype != torch.int32:
                raise RuntimeError("fnssl.rir_trajectory_batch: w_ini must be an int32 ROCm tensor")
            if x.ndim != 1 or r.ndim != 3 or w.ndim != 1 or w.numel() != r.shape[0] + 1 or x.numel() < 1:
                raise RuntimeError("fnssl.rir_trajectory_batch: item %d: signal %s, RIRs %s, w_ini %s"
                                   % (k, tuple(x.shape), tuple(r.shape), tuple(w.shape)))
            x, r, w = x.contiguous(), r.contiguous(), w.contiguous()
            y = torch.empty((x.numel() + r.shape[2] - 1, r.shape[1]), dtype=torch.float32, device=x.device)
            keep.append((x, r, w))
            outs.append(y)
            items[k - k0] = _lib.RirTrajItem(x.data_ptr(), r.data_ptr(), w.data_ptr(), y.data_ptr(), x.numel(), r.shape[2],
                                             r.shape[0], r.shape[1])
        check(lib.fnssl_rir_trajectory(items, k1 - k0, _stream()), "rir_trajectory")
    return outs


def _rir_jobs(jobs, outs, who, need_device=True):
    """The fnssl_rir_job array of ``jobs``: dicts with ``rir_ism``'s arguments under their names (pos_src, pos_rcv, room_sz,
    beta, nb_img, nism, nsamples, fs and optionally c, seed).  Without ``need_device`` (planning) m_src / m_rcv may stand in
    for the positions."""
    jobs = list(jobs)
    if not jobs:
        raise RuntimeError("fnssl.%s: no job" % who)
    arr = (_lib.RirJob * len(jobs))()
    keep = []
    for k, job in enumerate(jobs):
        j = arr[k]
        try:
            room, bet, nb = _rir_host(job["room_sz"], job.get("beta", [0.0] * 6), job["nb_img"])
        except ValueError as e:
            raise ValueError("fnssl.%s: job %d: %s" % (who, k, e)) from None
        j.room_sz, j.beta, j.nb_img = room, bet, nb
        if need_device:
            try:
                src, rcv = _rir_positions(job["pos_src"], job["pos_rcv"])
            except RuntimeError as e:
                raise RuntimeError("fnssl.%s: job %d: %s" % (who, k, e)) from None
            keep.append((src, rcv))
            j.pos_src, j.pos_rcv, j.m_src, j.m_rcv = src.data_ptr(), rcv.data_ptr(), src.shape[0], rcv.shape[0]
        else:
            j.m_src = int(job["m_src"] if "m_src" in job else job["pos_src"].shape[0])
            j.m_rcv = int(job["m_rcv"] if "m_rcv" in job else job["pos_rcv"].shape[0])
        j.nism = int(job["nism"])
        j.nsamples = int(job.get("nsamples", job["nism"]))
        j.fs, j.c = float(job.get("fs", 16000.0)), float(job.get("c", 343.0))
        j.seed = int(job.get("seed", 0)) & (2 ** 64 - 1)
        if outs is not None:
            out = outs[k]
            _need_dev(out)
            if tuple(out.shape) != (j.m_src, j.m_rcv, j.nsamples) or not out.is_contiguous() or out.device != keep[k][0].device:
                raise RuntimeError("fnssl.%s: job %d: the RIRs must be a contiguous [%d, %d, %d] on %s, got %s on %s"
                                   % (who, k, j.m_src, j.m_rcv, j.nsamples, keep[k][0].device, tuple(out.shape), out.device))
            j.rir = out.data_ptr()
    return arr, keep


def rir_batch_plan(jobs, cus: int = 0):
    """Host only (fnssl_rir_batch_plan): per job ``rir_plan`` of the job alone plus ``workspace_offset``, its slice of the
    batch's workspace, and the workspace's size (fnssl_rir_batch_workspace_bytes) -> (list of dicts, bytes)."""
    arr, _ = _rir_jobs(jobs, None, "rir_batch_plan", need_device=False)
    lib = _lib.load()
    plans = (_lib.RirJobPlan * len(arr))()
    check(lib.fnssl_rir_batch_plan(arr, len(arr), int(cus), plans), "rir_batch_plan")
    out = []
    for pl in plans:
        d = {n: int(getattr(pl.plan, n)) for n, _ in _lib.RirPlanInfo._fields_}
        d["workspace_offset"] = int(pl.workspace_offset)
        out.append(d)
    return out, int(lib.fnssl_rir_batch_workspace_bytes(arr, len(arr), int(cus)))


@on_device
def rir_ism_batch(jobs, outs=None):
    """Image-source part of several jobs in one launch set (fnssl_rir_ism_batch): ``jobs`` are dicts of ``rir_ism``'s
    arguments -> list of RIRs [M_src, M_rcv, nsamples], each bit for bit what ``rir_ism`` gives the job alone.  ``outs``:
    the RIRs to write (samples [nism, nsamples) are left alone), else zeros.  Every job is checked before the first launch;
    a refused job is named by its index."""
    jobs = list(jobs)
    if outs is None:
        arr, keep = _rir_jobs(jobs, None, "rir_ism_batch")
        outs = [torch.zeros((j.m_src, j.m_rcv, max(j.nsamples, 0)), dtype=torch.float32, device=keep[k][0].device)
                for k, j in enumerate(arr)]
        for k, out in enumerate(outs):
            arr[k].rir = out.data_ptr()
    else:
        outs = list(outs)
        if len(outs) != len(jobs):
            raise RuntimeError("fnssl.rir_ism_batch: %d outputs for %d jobs" % (len(outs), len(jobs)))
        arr, keep = _rir_jobs(jobs, outs, "rir_ism_batch")
    lib = _lib.load()
    wsb = lib.fnssl_rir_batch_workspace_bytes(arr, len(arr), 0)
    ws = torch.empty(max(wsb, 4) // 4, dtype=torch.float32, device=keep[0][0].device)
    check(lib.fnssl_rir_ism_batch(arr, len(arr), _ptr(ws), ws.numel() * 4, _stream()), "rir_ism_batch")
    return outs


@on_device
def rir_tail_batch(jobs, rirs):
    """Diffuse tails of several jobs in one launch set (fnssl_rir_tail_batch), in place: ``rirs[k]`` [M_src, M_rcv, nsamples]
    of job k (``rir_tail``'s arguments under their names, ``nsamples`` taken from the RIRs).  Jobs with nsamples == nism have
    no tail and take no slot.  Returns ``rirs``."""
    jobs, rirs = list(jobs), list(rirs)
    if len(rirs) != len(jobs):
        raise RuntimeError("fnssl.rir_tail_batch: %d RIR sets for %d jobs" % (len(rirs), len(jobs)))
    for k, r in enumerate(rirs):
        if not isinstance(r, torch.Tensor) or r.ndim != 3:
            raise RuntimeError("fnssl.rir_tail_batch: job %d: expected a contiguous [M_src, M_rcv, nSamples]" % k)
    arr, keep = _rir_jobs([dict(j, nsamples=int(r.shape[2])) for j, r in zip(jobs, rirs)], rirs, "rir_tail_batch")
    check(_lib.load().fnssl_rir_tail_batch(arr, len(arr), _stream()), "rir_tail_batch")
    return rirs


# --------------------------------------------------------------------------- #
# scene finish (csrc/scene.hip; the reference-named surface is fnssl/scene.py)
# --------------------------------------------------------------------------- #
def _need_dev_f64(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("fnssl: expected a ROCm device tensor (this path has no CPU implementation), got %s"
                           % (t.device if isinstance(t, torch.Tensor) else type(t)))
    if t.dtype != torch.float64:
        raise RuntimeError("fnssl.%s: expected float64 (pivots of 1e-7 next to ones do not fit float32), got %s" % (what, t.dtype))


@on_device
def anf_coherence(mic_pos, fs: float, nfft: int = 256, c: float = 343.0):
    """Spherical coherence (fnssl_anf_coherence): mic_pos [B, M, 3] float64 -> DC [B, M, M, nfft / 2 + 1] float64."""
    _need_dev_f64(mic_pos, "anf_coherence")
    if mic_pos.ndim != 3 or mic_pos.shape[2] != 3:
        raise RuntimeError("fnssl.anf_coherence: mic_pos is [B, M, 3], got %s" % (tuple(mic_pos.shape),))
    mic_pos = mic_pos.contiguous()
    nb, m = mic_pos.shape[0], mic_pos.shape[1]
    dc = torch.empty((nb, m, m, int(nfft) // 2 + 1), dtype=torch.float64, device=mic_pos.device)
    check(_lib.load().fnssl_anf_coherence(_ptr(mic_pos), nb, m, float(fs), int(nfft), float(c), _ptr(dc), _stream()), "anf_coherence")
    return dc


@on_device
def anf_factor(dc, sync: bool = True):
    """Upper Cholesky factor per bin (fnssl_anf_factor): DC [B, M, M, bins] float64 -> (C, status).  C [B, M, M, 129] float32
    is a view of the kernel's [B, 16, 16, 129] store (what ``anf_mix`` takes), C[b, :, :, k]^T C[b, :, :, k] = DC[b, :, :, k]
    for k >= 1, slot 0 unused.  ``sync``: read the status words (synchronises) and raise ``numpy.linalg.LinAlgError`` naming
    the first bin that is not positive definite, as scipy.linalg.cholesky does in the reference; else the caller reads
    ``status`` (int32 view: -1 = fine) itself."""
    _need_dev_f64(dc, "anf_factor")
    if dc.ndim != 4 or dc.shape[1] != dc.shape[2]:
        raise RuntimeError("fnssl.anf_factor: DC is [B, M, M, bins], got %s" % (tuple(dc.shape),))
    dc = dc.contiguous()
    nb, m, nfft = dc.shape[0], dc.shape[1], 2 * (dc.shape[3] - 1)
    lib = _lib.load()
    store = torch.zeros((nb, _lib.ANF_MAX_MICS, _lib.ANF_MAX_MICS, _lib.ANF_BINS), dtype=torch.float32, device=dc.device)
    status = torch.empty((nb,), dtype=torch.int32, device=dc.device)
    check(lib.fnssl_anf_factor(_ptr(dc), nb, m, nfft, _ptr(store), _ptr(status), _stream()), "anf_factor")
    if sync:
        words = (C.c_uint * nb)()
        check(lib.fnssl_anf_status(_ptr(status), nb, _stream(), words), "anf_status")
        bad = [(b, int(w)) for b, w in enumerate(words) if w != 0xFFFFFFFF]
        if bad:
            raise np.linalg.LinAlgError("fnssl.anf_factor: the coherence matrix of bin %d is not positive definite%s"
                                        % (bad[0][1], " (item %d)" % bad[0][0] if nb > 1 else ""))
    return store[:, :m, :m, :], status


def _anf_store(cfac):
    want = (_lib.ANF_MAX_MICS * _lib.ANF_MAX_MICS * _lib.ANF_BINS, _lib.ANF_MAX_MICS * _lib.ANF_BINS, _lib.ANF_BINS, 1)
    if cfac.ndim != 4 or cfac.shape[1] != cfac.shape[2] or cfac.shape[3] != _lib.ANF_BINS or \
            (cfac.shape[0] > 1 and cfac.stride(0) != want[0]) or tuple(cfac.stride()[1:]) != want[1:]:
        raise RuntimeError("fnssl.anf_mix: the factor must be what anf_factor returned ([B, M, M, 129] in its [B, 16, 16, 129] store), "
                           "got %s with strides %s" % (tuple(cfac.shape), tuple(cfac.stride())))


@on_device
def anf_mean(x):
    """Mean of every row of x [B, count] (fnssl_anf_mean; rows contiguous) -> [B]."""
    _need_dev(x)
    if x.ndim != 2 or x.stride(1) != 1 or x.shape[1] < 1:
        raise RuntimeError("fnssl.anf_mean: expected [B, count] with contiguous rows, got %s" % (tuple(x.shape),))
    nb, count = x.shape
    nchunks = (count + _lib.ANF_MEAN_CHUNK - 1) // _lib.ANF_MEAN_CHUNK
    part = torch.empty((nb * nchunks,), dtype=torch.float32, device=x.device)
    mean = torch.empty((nb,), dtype=torch.float32, device=x.device)
    check(_lib.load().fnssl_anf_mean(_ptr(x), nb, count, x.stride(0) if nb > 1 else 0, _ptr(part), part.numel(), _ptr(mean),
                                     _stream()), "anf_mean")
    return mean


@on_device
def anf_mix(x, cfac, mean=None, nfft: int = 256, _tile_hops: int = 0):
    """Habets' mixing (fnssl_anf_mix): x [B, L, M] (any strides), the factor of ``anf_factor`` (one item for all, or B) and
    optionally mean [B] (subtracted from the samples, never from the padding) -> [B, L + ((-L) mod 64), M].
    ``_tile_hops`` is for tests: the output hops one wave owns; the bits do not depend on it."""
    _need_dev(x, cfac, mean)
    if x.ndim != 3:
        raise RuntimeError("fnssl.anf_mix: expected [B, L, M], got %s" % (tuple(x.shape),))
    nb, length, m = x.shape
    if m <= _lib.ANF_MAX_MICS:
        _anf_store(cfac)
        if cfac.shape[1] != m or cfac.shape[0] not in (1, nb):
            raise RuntimeError("fnssl.anf_mix: a factor %s for signals %s" % (tuple(cfac.shape), tuple(x.shape)))
    if mean is not None and (mean.shape != (nb,) or not mean.is_contiguous()):
        raise RuntimeError("fnssl.anf_mix: mean is [B], got %s" % (tuple(mean.shape),))
    y = torch.empty((nb, length + (-length) % 64, m), dtype=torch.float32, device=x.device)
    sb, sn, sm = x.stride()
    check(_lib.load().fnssl_anf_mix(_ptr(x), sb, sn, sm, _ptr(mean), _ptr(cfac), cfac.shape[0], nb, length, m, int(nfft),
                                    int(_tile_hops), _ptr(y), _stream()), "anf_mix")
    return y


def _scene_rows(sigs, n, m, who):
    arr = (C.c_void_p * _lib.SCENE_MAX_SOURCES)()
    keep = []
    for k, a in enumerate(sigs):
        _need_dev(a)
        if a.ndim != 2 or a.shape[1] != m or a.shape[0] < n:
            raise RuntimeError("fnssl.%s: signal %d is %s, expected at least [%d, %d]" % (who, k, tuple(a.shape), n, m))
        a = a.contiguous()
        keep.append(a)
        if k < _lib.SCENE_MAX_SOURCES:
            arr[k] = a.data_ptr()
    return arr, keep


@on_device
def scene_power(sigs, n: int = None):
    """``acoustic_power`` of every channel of the sum of ``sigs`` (a tensor or a list of up to 4, each [>= n, M]; rows [0, n))
    (fnssl_scene_power) -> [M]."""
    sigs = [sigs] if isinstance(sigs, torch.Tensor) else list(sigs)
    if not sigs or not isinstance(sigs[0], torch.Tensor) or sigs[0].ndim != 2:
        raise RuntimeError("fnssl.scene_power: expected [n, M] signals")
    n = sigs[0].shape[0] if n is None else int(n)
    m = sigs[0].shape[1]
    arr, keep = _scene_rows(sigs, n, m, "scene_power")
    blocks = torch.empty((max(m * (n // 256), 1),), dtype=torch.float32, device=sigs[0].device)
    power = torch.empty((m,), dtype=torch.float32, device=sigs[0].device)
    check(_lib.load().fnssl_scene_power(arr, len(sigs), n, m, _ptr(blocks), blocks.numel(), _ptr(power), _stream()), "scene_power")
    return power


@on_device
def scene_finish(sigs, noise, p, pn, snr_db: float, n: int, vads=None):
    """The SNR mix and the VAD (fnssl_scene_finish): sigs / vads lists of [>= n, M], noise [>= n, M], p / pn [M] -> dict with
    mic [n, M], g [1] and, with vads, vmax [S], vad_sources [n, S] and vad [n] (uint8)."""
    sigs = list(sigs)
    _need_dev(noise, p, pn)
    m = noise.shape[1] if noise.ndim == 2 else -1
    if noise.ndim != 2 or noise.shape[0] < n or p.shape != (m,) or pn.shape != (m,):
        raise RuntimeError("fnssl.scene_finish: noise %s, powers %s and %s for n = %d" % (tuple(noise.shape), tuple(p.shape), tuple(pn.shape), n))
    arr, keep = _scene_rows(sigs, n, m, "scene_finish")
    noise, p, pn = noise.contiguous(), p.contiguous(), pn.contiguous()
    dev = noise.device
    ns = len(sigs)
    out = {"mic": torch.empty((n, m), dtype=torch.float32, device=dev), "g": torch.empty((1,), dtype=torch.float32, device=dev)}
    varr = None
    if vads is not None:
        if len(vads) != ns:
            raise RuntimeError("fnssl.scene_finish: %d VAD signals for %d sources" % (len(vads), ns))
        varr, vkeep = _scene_rows(vads, n, m, "scene_finish")
        keep += vkeep
        out["vmax"] = torch.empty((ns,), dtype=torch.float32, device=dev)
        out["vad_sources"] = torch.empty((n, ns), dtype=torch.uint8, device=dev)
        out["vad"] = torch.empty((n,), dtype=torch.uint8, device=dev)
    check(_lib.load().fnssl_scene_finish(arr, ns, _ptr(noise), varr, int(n), m, _ptr(p), _ptr(pn), 10.0 ** (float(snr_db) / 10.0),
                                         _ptr(out["mic"]), _ptr(out["g"]), _ptr(out.get("vmax")), _ptr(out.get("vad_sources")),
                                         _ptr(out.get("vad")), _stream()), "scene_finish")
    return out


@on_device
def scene_mix_batch(scenes, n: int):
    """Power and finish of a batch of scenes in one launch set (fnssl_scene_power_batch, fnssl_scene_finish_batch).  ``scenes``:
    dicts with ``dp`` and ``sig`` (lists of S_b <= 4 signals [>= n, M]), ``noise`` [>= n, M] (its WHOLE length enters its
    power), ``snr_db`` and optionally ``vads`` (S_b signals).  n and M are shared.  Returns a dict: mic [B, n, M], g [B],
    power and power_noise [B, M], vad [B, n] and, per scene, vmax [S_b] and vad_sources [n, S_b] (uint8; None without VAD) —
    every entry bit for bit what ``scene_power`` / ``scene_finish`` give the scene alone.  Nothing is read back."""
    scenes = list(scenes)
    nb, n = len(scenes), int(n)
    if nb < 1:
        raise RuntimeError("fnssl.scene_mix_batch: no scene")
    noise0 = scenes[0]["noise"]
    _need_dev(noise0)
    if noise0.ndim != 2:
        raise RuntimeError("fnssl.scene_mix_batch: noise is [>= n, M], got %s" % (tuple(noise0.shape),))
    m, dev = noise0.shape[1], noise0.device
    nblk = max(n // 256, 1)
    nlen = []
    for b, sc in enumerate(scenes):
        _need_dev(sc["noise"])
        if sc["noise"].ndim != 2 or sc["noise"].shape[1] != m or sc["noise"].shape[0] < n:
            raise RuntimeError("fnssl.scene_mix_batch: scene %d: noise %s for [>= %d, %d]" % (b, tuple(sc["noise"].shape), n, m))
        nlen.append(int(sc["noise"].shape[0]))
        if len(sc["dp"]) != len(sc["sig"]) or (sc.get("vads") is not None and len(sc["vads"]) != len(sc["sig"])):
            raise RuntimeError("fnssl.scene_mix_batch: scene %d: %d direct-path, %d full and %s VAD signals"
                               % (b, len(sc["dp"]), len(sc["sig"]), "no" if sc.get("vads") is None else len(sc["vads"])))
    nsrc = [len(sc["sig"]) for sc in scenes]
    nblk_noise = [max(v // 256, 1) for v in nlen]
    blocks = torch.empty((m * (nb * nblk + sum(nblk_noise)),), dtype=torch.float32, device=dev)
    out = {"mic": torch.empty((nb, n, m), dtype=torch.float32, device=dev), "g": torch.empty((nb,), dtype=torch.float32, device=dev),
           "power": torch.empty((nb, m), dtype=torch.float32, device=dev),
           "power_noise": torch.empty((nb, m), dtype=torch.float32, device=dev), "vmax": [None] * nb, "vad_sources": [None] * nb}
    with_vad = [sc.get("vads") is not None for sc in scenes]
    nv = sum(s for s, w in zip(nsrc, with_vad) if w)
    vmax = torch.empty((max(nv, 1),), dtype=torch.float32, device=dev)
    vsrc = torch.empty((max(nv, 1) * n,), dtype=torch.uint8, device=dev)
    out["vad"] = vany = torch.empty((nb, n), dtype=torch.uint8, device=dev)        # rows of scenes without VAD are not written
    descs = (_lib.SceneDesc * nb)()
    keep, boff, voff = [], 0, 0
    for b, sc in enumerate(scenes):
        d = descs[b]
        for name, field in (("dp", d.dp), ("sig", d.sig)) + ((("vads", d.vad_in),) if with_vad[b] else ()):
            arr, kept = _scene_rows(sc[name], n, m, "scene_mix_batch: scene %d" % b)
            keep += kept
            for s in range(min(nsrc[b], _lib.SCENE_MAX_SOURCES)):
                field[s] = arr[s]
        noise = sc["noise"].contiguous()
        keep.append(noise)
        d.noise, d.ns, d.noise_len, d.with_vad = noise.data_ptr(), nsrc[b], nlen[b], int(with_vad[b])
        d.snr_lin = 10.0 ** (float(sc["snr_db"]) / 10.0)
        d.blocks, d.blocks_floats = blocks[boff:].data_ptr(), m * nblk
        boff += m * nblk
        d.blocks_noise, d.blocks_noise_floats = blocks[boff:].data_ptr(), m * nblk_noise[b]
        boff += m * nblk_noise[b]
        d.power, d.power_noise = out["power"][b].data_ptr(), out["power_noise"][b].data_ptr()
        d.mic, d.g = out["mic"][b].data_ptr(), out["g"][b:].data_ptr()
        if with_vad[b]:
            out["vmax"][b] = vmax[voff:voff + nsrc[b]]
            out["vad_sources"][b] = vsrc[voff * n:(voff + nsrc[b]) * n].view(n, nsrc[b])
            d.vmax, d.vad_sources, d.vad = out["vmax"][b].data_ptr(), out["vad_sources"][b].data_ptr(), vany[b].data_ptr()
            voff += nsrc[b]
    lib = _lib.load()
    check(lib.fnssl_scene_power_batch(descs, nb, n, m, _stream()), "scene_power_batch")
    check(lib.fnssl_scene_finish_batch(descs, nb, n, m, _stream()), "scene_finish_batch")
    return out


# --------------------------------------------------------------------------- #
# training labels of a batch of scenes (csrc/labels.hip)
# --------------------------------------------------------------------------- #
def _need_dev_as(t, dtype, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("fnssl: expected a ROCm device tensor (this path has no CPU implementation), got %s"
                           % (t.device if isinstance(t, torch.Tensor) else type(t)))
    if t.dtype != dtype:
        raise RuntimeError("fnssl.%s: expected %s, got %s" % (what, dtype, t.dtype))


@on_device
def scene_doa_batch(items):
    """Trajectory and DOA of every scene in one launch set (fnssl_scene_doa_batch).  ``items``: dicts with ``traj_pts``
    [P, 3, S] and ``timestamps`` [P] (float64 device tensors), ``n``, ``fs`` and ``array_pos`` (three host numbers) -> a list of
    (trajectory [n, 3, S], DOA [n, 2, S]) float64 tensors, views of two batch allocations."""
    items = list(items)
    if not items:
        raise RuntimeError("fnssl.scene_doa_batch: no scene")
    descs = (_lib.SceneDoaDesc * len(items))()
    keep, rows = [], []
    for b, it in enumerate(items):
        pts, ts = it["traj_pts"], it["timestamps"]
        _need_dev_as(pts, torch.float64, "scene_doa_batch")
        _need_dev_as(ts, torch.float64, "scene_doa_batch")
        if pts.ndim != 3 or pts.shape[1] != 3 or ts.ndim != 1 or ts.shape[0] != pts.shape[0] or pts.shape[0] < 1:
            raise RuntimeError("fnssl.scene_doa_batch: scene %d: traj_pts is [P, 3, S] and timestamps [P], got %s and %s"
                               % (b, tuple(pts.shape), tuple(ts.shape)))
        pts, ts = pts.contiguous(), ts.contiguous()
        keep += [pts, ts]
        rows.append(int(it["n"]) * int(pts.shape[2]))
        d = descs[b]
        d.traj_pts, d.timestamps, d.fs = pts.data_ptr(), ts.data_ptr(), float(it["fs"])
        d.npts, d.ns, d.n = int(pts.shape[0]), int(pts.shape[2]), int(it["n"])
        for i in range(3):
            d.array_pos[i] = float(it["array_pos"][i])
    dev = items[0]["traj_pts"].device
    traj = torch.empty((3 * max(sum(rows), 1),), dtype=torch.float64, device=dev)
    doa = torch.empty((2 * max(sum(rows), 1),), dtype=torch.float64, device=dev)
    out, off = [], 0
    for b, it in enumerate(items):
        n, s = descs[b].n, descs[b].ns
        t, a = traj[3 * off:3 * (off + rows[b])], doa[2 * off:2 * (off + rows[b])]
        descs[b].trajectory, descs[b].doa = t.data_ptr(), a.data_ptr()
        out.append((t.view(n, 3, s), a.view(n, 2, s)))
        off += rows[b]
    check(_lib.load().fnssl_scene_doa_batch(descs, len(items), _stream()), "scene_doa_batch")
    return out


@on_device
def scene_segment_batch(items, length: int, K: int, step: int, nw: int, smax: int, with_doa: bool = True, with_vad: bool = True):
    """The windows of every scene in one launch set (fnssl_scene_segment_batch).  ``items``: dicts with ``doa`` [>= (nw - 1) step
    + K, 2, S_b] float64 (needed with ``with_doa``), ``vad_sources`` [Lv, S_b] and ``vad`` [Lv] uint8 / bool (or None: zeros), Lv <= length, and
    ``ns`` = S_b.  Returns a dict: doa [B, nw, 2, smax] float64 (``with_doa``), vad_sources [B, nw, K, smax] and vad [B, nw, K]
    uint8 and vad_count [B, nw, smax] int32 (``with_vad``)."""
    items = list(items)
    nb = len(items)
    if nb < 1:
        raise RuntimeError("fnssl.scene_segment_batch: no scene")
    descs = (_lib.SceneSegmentDesc * nb)()
    keep, dev = [], None
    for b, it in enumerate(items):
        d = descs[b]
        d.ns = int(it["ns"])
        doa = it.get("doa") if with_doa else None
        if with_doa and doa is None:
            raise RuntimeError("fnssl.scene_segment_batch: scene %d: no DOA (its rows of the output would stay unwritten)" % b)
        if doa is not None:
            _need_dev_as(doa, torch.float64, "scene_segment_batch")
            if doa.ndim != 3 or doa.shape[1] != 2 or doa.shape[2] != d.ns:
                raise RuntimeError("fnssl.scene_segment_batch: scene %d: DOA is [n, 2, %d], got %s" % (b, d.ns, tuple(doa.shape)))
            doa = doa.contiguous()
            keep.append(doa)
            d.doa, d.doa_len, dev = doa.data_ptr(), int(doa.shape[0]), doa.device
        lens = []
        for name, shape in (("vad_sources", (d.ns,)), ("vad", ())):
            v = it.get(name) if with_vad else None
            if v is None:
                continue
            if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype not in (torch.uint8, torch.bool):
                raise RuntimeError("fnssl.scene_segment_batch: scene %d: %s must be a uint8 / bool ROCm tensor" % (b, name))
            if tuple(v.shape[1:]) != shape:
                raise RuntimeError("fnssl.scene_segment_batch: scene %d: %s is %s, got %s"
                                   % (b, name, "[n, %d]" % d.ns if shape else "[n]", tuple(v.shape)))
            v = v.contiguous().view(torch.uint8)
            keep.append(v)
            setattr(d, name, v.data_ptr())
            lens.append(int(v.shape[0]))
            dev = v.device
        if len(set(lens)) > 1:
            raise RuntimeError("fnssl.scene_segment_batch: scene %d: vad_sources has %d rows, vad %d" % (b, lens[0], lens[1]))
        d.vad_len = lens[0] if lens else 0
    if dev is None:
        raise RuntimeError("fnssl.scene_segment_batch: no device tensor in the batch")
    out = {}
    if with_doa:
        out["doa"] = torch.empty((nb, nw, 2, smax), dtype=torch.float64, device=dev)
    if with_vad:
        out["vad_sources"] = torch.empty((nb, nw, K, smax), dtype=torch.uint8, device=dev)
        out["vad"] = torch.empty((nb, nw, K), dtype=torch.uint8, device=dev)
        out["vad_count"] = torch.empty((nb, nw, smax), dtype=torch.int32, device=dev)
    check(_lib.load().fnssl_scene_segment_batch(descs, nb, int(length), int(K), int(step), int(nw), int(smax), _ptr(out.get("doa")),
                                                _ptr(out.get("vad_sources")), _ptr(out.get("vad")), _ptr(out.get("vad_count")),
                                                _stream()), "scene_segment_batch")
    return out


@on_device
def scene_pack_batch(scenes, n: int, m: int, smax: int):
    """``scenes``: per scene its S_b <= smax direct-path signals, a list of [>= n, M] tensors or ONE tensor [>= n, M, S_b] of any
    strides (what ``simulate_batch`` leaves on a scene; read in place) -> dp_signal [B, n, M, smax], absent sources zero
    (fnssl_scene_pack_batch)."""
    scenes = list(scenes)
    nb = len(scenes)
    if nb < 1:
        raise RuntimeError("fnssl.scene_pack_batch: no scene")
    descs = (_lib.ScenePackDesc * nb)()
    keep = []
    for b, sigs in enumerate(scenes):
        d = descs[b]
        stacked = isinstance(sigs, torch.Tensor)
        ns = int(sigs.shape[2]) if stacked and sigs.ndim == 3 else -1 if stacked else len(sigs)
        if not 1 <= ns <= min(smax, _lib.SCENE_MAX_SOURCES):
            raise RuntimeError("fnssl.scene_pack_batch: scene %d: %d sources (1 .. max_source = %d)" % (b, ns, smax))
        d.ns = ns
        if stacked:
            _need_dev(sigs)
            if sigs.shape[0] < n or sigs.shape[1] != m:
                raise RuntimeError("fnssl.scene_pack_batch: scene %d: signals %s, expected at least [%d, %d, S]" % (b, tuple(sigs.shape), n, m))
            if min(sigs.stride()) < 1:
                sigs = sigs.contiguous()
            keep.append(sigs)
            d.stride_t, d.stride_c = sigs.stride(0), sigs.stride(1)
            for s in range(ns):
                d.dp[s] = sigs.data_ptr() + 4 * s * sigs.stride(2)
        else:
            arr, kept = _scene_rows(sigs, n, m, "scene_pack_batch: scene %d" % b)
            keep += kept
            d.stride_t, d.stride_c = m, 1
            for s in range(ns):
                d.dp[s] = arr[s]
    out = torch.empty((nb, n, m, smax), dtype=torch.float32, device=keep[0].device)
    check(_lib.load().fnssl_scene_pack_batch(descs, nb, int(n), int(m), int(smax), _ptr(out), _stream()), "scene_pack_batch")
    return out
