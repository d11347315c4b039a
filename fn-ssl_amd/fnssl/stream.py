"""Online use: microphone samples in, features / DP-IPD / DOA out, chunk by chunk.

``StreamFrontEnd`` is the streamed counterpart of ``ops.preprocess`` (FN-SSL, mode ``'pair'``) and
``ops.preprocess_array`` (IPDnet, mode ``'array'``): ``push`` takes the next samples, keeps the ones whose frames are
not complete yet in a device-side tail, and returns the features of every new whole group of ``segment_frames`` frames
from ONE launch of ``fnssl_stream_frontend`` — bit for bit what the whole-signal path gives on the same frames (the
hop-256 transform is not centred, so a frame depends on its own 512 samples only, and the recursive normalisation
continues from the carried ``mu`` with the coefficients of the ABSOLUTE frame index).

``OnlineLocalizer`` chains a front end to a model's ``forward_stream`` (and optionally a prediction -> DOA callable);
the Lightning drop-ins expose it as ``predict_stream``.

IPDnet2 does not stream here: its transform is centred with hop 320 and its last frames depend on the end of the signal.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from ._lib import CH_MODE, STREAM_MODE, check

WIN = 512
HOP = 256
DEFAULT_SAMPLE_LENGTH = {"pair": 298, "array": 280}     # main.py:207-225 / runIPDnetOn.py:246-254


# --------------------------------------------------------------------------- #
# count arithmetic (pure: tests/test_stream_host.py holds it to a brute-force count)
# --------------------------------------------------------------------------- #
def frames_ready(nsamples: int) -> int:
    """Frames complete once ``nsamples`` samples have arrived: frame t exists when sample 256 t + 511 has."""
    return 0 if nsamples < WIN else (nsamples - WIN) // HOP + 1


def plan_push(tail: int, new: int, segment_frames: int):
    """The tail holds ``tail`` samples, the first one being the first sample of the next frame to emit; ``new`` samples
    arrive.  Returns (frames to emit now — whole groups of ``segment_frames`` —, samples the tail keeps afterwards)."""
    if tail < 0 or new < 0 or segment_frames <= 0:
        raise ValueError("plan_push: tail %r, new %r, segment_frames %r" % (tail, new, segment_frames))
    have = tail + new
    emit = frames_ready(have) // segment_frames * segment_frames
    return emit, have - HOP * emit


def tail_bound(segment_frames: int) -> int:
    """The tail never keeps this many samples: fewer than ``segment_frames`` complete frames plus less than one hop."""
    return HOP * segment_frames + WIN


def stream_coefs_host(sample_length: int):
    """The host function's own table of ``sample_length + 1`` entries; frame t reads entry ``min(t, sample_length)``
    (from ``sample_length`` on the coefficients are constant, and b_t there is a different expression)."""
    return ops.forgetting_coefs_host(sample_length + 1, sample_length)


_coef_cache = {}


def _stream_coefs(sample_length: int, normalise: bool, device):
    key = (sample_length, bool(normalise), str(device))
    if key not in _coef_cache:
        a, b = stream_coefs_host(sample_length)
        if not normalise:                 # nor_flag = False: zero recursion, eps = 1 (ops.pair_features does the same)
            a, b = np.zeros_like(a), np.zeros_like(b)
        _coef_cache[key] = (torch.from_numpy(a).to(device), torch.from_numpy(b).to(device))
    return _coef_cache[key]


# --------------------------------------------------------------------------- #
# front end
# --------------------------------------------------------------------------- #
class StreamFrontEnd:
    """``push(chunk [nb, n, nch]) -> features`` of the frames completed by it, in groups of ``segment_frames``:
    ``[nb * np, T, 256, 4]`` (mode ``'pair'``, ``ch_mode`` 'M' / 'MM') or ``[nb, T, 256, 2 * nch]`` (mode ``'array'``),
    T possibly 0.  ``frames`` counts the frames emitted so far; ``reset()`` starts over."""

    def __init__(self, mode: str, nch: int, ch_mode: str = "MM", sample_length: int = None, eps: float = 1e-6,
                 normalise: bool = True, segment_frames: int = 12):
        if mode not in STREAM_MODE:
            raise ValueError("StreamFrontEnd: mode must be 'pair' or 'array', got %r" % (mode,))
        if mode == "pair" and ch_mode not in CH_MODE:
            raise ValueError("StreamFrontEnd: ch_mode must be 'M' or 'MM', got %r" % (ch_mode,))
        if int(segment_frames) <= 0:
            raise ValueError("StreamFrontEnd: segment_frames must be positive, got %r" % (segment_frames,))
        self.mode, self.nch, self.ch_mode = mode, int(nch), ch_mode if mode == "pair" else "M"
        if self.nch < (2 if mode == "pair" else 1):
            raise ValueError("StreamFrontEnd: %d channels" % self.nch)
        self.sample_length = int(DEFAULT_SAMPLE_LENGTH[mode] if sample_length is None else sample_length)
        self.normalise = bool(normalise)
        self.eps = float(eps) if self.normalise else 1.0
        self.segment_frames = int(segment_frames)
        self.nrows = ops.num_pairs(self.nch, self.ch_mode) if mode == "pair" else 1     # feature rows per utterance
        self.width = 4 if mode == "pair" else 2 * self.nch
        self.reset()

    def reset(self):
        """Forget the stream: the next push is sample 0 again (of any batch size, on any device)."""
        self.frames = 0
        self.nb = None
        self._buf = None                 # [nb, capacity, nch]; the tail is _buf[:, _start:_start + _len]
        self._start = self._len = 0
        self._state = None

    @property
    def tail_samples(self) -> int:
        """Samples kept for frames not emitted yet (< ``tail_bound(segment_frames)``)."""
        return self._len

    @property
    def buffer_samples(self) -> int:
        """Capacity of the device-side sample buffer, per channel and utterance."""
        return 0 if self._buf is None else self._buf.shape[1]

    def _open(self, chunk):
        nb = chunk.shape[0]
        self.nb = nb
        lib = _lib.load()
        nbytes = lib.fnssl_stream_frontend_state_bytes(nb, self.nch, STREAM_MODE[self.mode], CH_MODE[self.ch_mode], 1 << 20)
        if nbytes == 0:
            raise RuntimeError("fnssl.stream: no streamed front end for %d utterances x %d channels (mode %r)"
                               % (nb, self.nch, self.mode))
        self._state = torch.zeros(nbytes, dtype=torch.uint8, device=chunk.device)      # mu_{-1} = 0
        self._buf = torch.empty((nb, 2 * tail_bound(self.segment_frames), self.nch), dtype=torch.float32,
                                device=chunk.device)

    def _append(self, chunk):
        n = chunk.shape[1]
        if self._start + self._len + n > self._buf.shape[1]:
            # move the tail to the front of a buffer that holds it and the chunk; the capacity follows the largest push,
            # not the length of the stream
            cap = self._buf.shape[1] if self._len + n <= self._buf.shape[1] else 2 * (self._len + n)
            buf = self._buf if cap == self._buf.shape[1] else torch.empty((self.nb, cap, self.nch), dtype=torch.float32,
                                                                           device=self._buf.device)
            tail = self._buf[:, self._start:self._start + self._len]
            buf[:, :self._len].copy_(tail.clone() if buf is self._buf else tail)
            self._buf, self._start = buf, 0
        self._buf[:, self._start + self._len:self._start + self._len + n].copy_(chunk)   # any strides: read in place
        self._len += n

    @ops.on_device
    def push(self, chunk):
        ops._need_dev(chunk)
        if chunk.ndim != 3 or chunk.shape[2] != self.nch:
            raise RuntimeError("fnssl.stream: expected a chunk [nb, n, %d], got %s" % (self.nch, tuple(chunk.shape)))
        if self.nb is None:
            self._open(chunk)
        elif chunk.shape[0] != self.nb or chunk.device != self._buf.device:
            raise RuntimeError("fnssl.stream: the stream was opened with %d utterances on %s, got %d on %s (reset() first)"
                               % (self.nb, self._buf.device, chunk.shape[0], chunk.device))
        emit, keep = plan_push(self._len, chunk.shape[1], self.segment_frames)
        if chunk.shape[1]:
            self._append(chunk)
        x = torch.empty((self.nb * self.nrows, emit, ops.NF, self.width), dtype=torch.float32, device=chunk.device)
        if emit == 0:
            return x
        win = self._buf[:, self._start:self._start + self._len]
        ca, cb = _stream_coefs(self.sample_length, self.normalise, chunk.device)
        sb, sn, sc = win.stride()
        check(_lib.load().fnssl_stream_frontend(
            ops._ptr(win), self.nb, self._len, self.nch, sb, sn, sc, STREAM_MODE[self.mode], CH_MODE[self.ch_mode],
            self.frames, emit, ops._ptr(ca), ops._ptr(cb), self.sample_length, self.eps, ops._ptr(self._state),
            self._state.numel(), ops._ptr(x), ops._stream()), "stream_frontend")
        self.frames += emit
        self._start += HOP * emit         # consumed samples are dropped: the next append moves what is left
        self._len = keep
        return x


# --------------------------------------------------------------------------- #
# front end -> network -> DOA
# --------------------------------------------------------------------------- #
class OnlineLocalizer:
    """``push(chunk [nb, n, nch]) -> (pred, doa)``: the emitted features go through ``model.forward_stream`` with its
    carried state; ``localize`` (a callable on the new prediction, e.g. the template search of ``PredDOA``) gives ``doa``.
    Both are None while the push completes no segment.  ``model`` is an online fp32 ``FN_SSL`` / ``IPDnet``; the errors
    for offline or bf16 modules are ``forward_stream``'s own."""

    def __init__(self, model, frontend: StreamFrontEnd, localize=None):
        if frontend.segment_frames % ops.SEG_FRAMES:
            raise ValueError("OnlineLocalizer: the network consumes groups of %d frames, the front end emits groups of %d"
                             % (ops.SEG_FRAMES, frontend.segment_frames))
        if getattr(model, "input_size", frontend.width) != frontend.width:
            raise ValueError("OnlineLocalizer: the front end emits %d feature channels, the network takes %d"
                             % (frontend.width, model.input_size))
        self.model, self.frontend, self.localize = model, frontend, localize
        self.state = None
        # fail at construction, not at the first completed segment: a zero-frame call runs forward_stream's checks of
        # the module (eval mode, online, fp32) and stops at its shape check
        self._check_model()

    def _check_model(self):
        probe = torch.zeros((1, self.frontend.width, ops.NF, 0))
        try:
            self.model.forward_stream(probe)
        except RuntimeError as e:
            if "expected [nb" not in str(e):
                raise

    def reset(self):
        self.frontend.reset()
        self.state = None

    def push(self, chunk):
        x = self.frontend.push(chunk)
        if x.shape[1] == 0:
            return None, None
        pred, self.state = self.model.forward_stream(x.permute(0, 3, 2, 1), self.state)   # a view: nothing is moved
        return pred, (self.localize(pred) if self.localize is not None else None)
