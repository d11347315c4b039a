"""Online use: microphone samples in, features / DP-IPD / DOA out, chunk by chunk.

``StreamFrontEnd`` is the streamed counterpart of ``ops.preprocess`` (FN-SSL, mode ``'pair'``) and
``ops.preprocess_array`` (IPDnet, mode ``'array'``): ``push`` takes the next samples, keeps the ones whose frames are
not complete yet in a device-side tail, and returns the features of every new whole group of ``segment_frames`` frames
from ONE launch of ``fnssl_stream_frontend`` — bit for bit what the whole-signal path gives on the same frames (the
hop-256 transform is not centred, so a frame depends on its own 512 samples only, and the recursive normalisation
continues from the carried ``mu`` with the coefficients of the ABSOLUTE frame index).

``CentredStreamFrontEnd`` is the streamed counterpart of ``ops.preprocess_ipdnet2`` (IPDnet2: centred Hann-512
transform with hop 320 and reflect padding, normalisation over all channels), from ONE launch of
``fnssl_stream_frontend_centred`` per push, with the same bit-for-bit promise.  A centred frame t covers samples
320 t - 256 .. 320 t + 255, so it is complete 256 samples (16 ms) after its centre; the start reflection touches frame
0 only, and the end reflection only the very last frame of a signal, which ``finish()`` emits once the length is known
(the ``centred_*`` functions below are the arithmetic; DESIGN.md derives it).

``OnlineLocalizer`` chains a front end to a model's ``forward_stream`` (and optionally a prediction -> DOA callable);
the Lightning drop-ins of FN-SSL, IPDnet and IPDnet2 expose it as ``predict_stream``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from ._lib import CH_MODE, STREAM_MODE, check

WIN = 512
HOP = 256
CENTRED_HOP = 320                                        # IPDnet2: win_shift_ratio 0.625 (IPDnet2/run_IPDnet2.py:90-93)
DEFAULT_SAMPLE_LENGTH = {"pair": 298, "array": 280}     # main.py:207-225 / runIPDnetOn.py:246-254
CENTRED_SAMPLE_LENGTH = 249                              # IPDnet2/run_IPDnet2.py:277-288


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


# the centred hop-320 transform of IPDnet2 (pure: tests/test_stream2_host.py holds it to a count that folds indices)
def centred_frames_ready(nsamples: int) -> int:
    """Frames of the centred transform that are complete once ``nsamples`` samples have arrived and the end of the signal
    is not known: frame t >= 1 when its last sample 320 t + 255 has, frame 0 when sample 256 has (its index -256 folds
    to it).  Such a frame never touches the end reflection, however long the signal turns out to be."""
    return 0 if nsamples <= WIN // 2 else (nsamples - WIN // 2) // CENTRED_HOP + 1


def centred_tail_start(frames: int) -> int:
    """Absolute index of the first sample still needed once ``frames`` frames have been emitted: frame ``frames`` starts at
    320 frames - 256, and if it turns out to be the LAST frame of a signal of exactly 320 frames samples its end
    reflection reaches one sample further back."""
    return max(0, CENTRED_HOP * frames - WIN // 2 - 1)


def centred_plan_push(tail: int, new: int, segment_frames: int, frames: int):
    """``frames`` frames have been emitted, the tail holds the ``tail`` samples from ``centred_tail_start(frames)`` on,
    ``new`` samples arrive.  Returns (frames to emit now — whole groups of ``segment_frames`` —, samples the tail keeps
    afterwards)."""
    if tail < 0 or new < 0 or segment_frames <= 0 or frames < 0 or frames % segment_frames:
        raise ValueError("centred_plan_push: tail %r, new %r, segment_frames %r, frames %r" % (tail, new, segment_frames, frames))
    arrived = centred_tail_start(frames) + tail + new
    emit = max(0, centred_frames_ready(arrived) - frames) // segment_frames * segment_frames
    return emit, arrived - centred_tail_start(frames + emit)


def centred_plan_finish(total: int, segment_frames: int, frames: int):
    """The stream ends after ``total`` samples with ``frames`` frames emitted: the signal has total // 320 + 1 frames, of
    which the whole groups are emitted and the rest dropped, as the network's time pooling drops them.  Returns (frames
    to emit now, samples kept afterwards = 0)."""
    if total <= WIN // 2 or segment_frames <= 0 or frames < 0 or frames % segment_frames:
        raise ValueError("centred_plan_finish: total %r, segment_frames %r, frames %r" % (total, segment_frames, frames))
    emit = (total // CENTRED_HOP + 1) // segment_frames * segment_frames - frames
    if emit < 0:
        raise ValueError("centred_plan_finish: %d frames emitted, a signal of %d samples has %d" % (frames, total, emit + frames))
    return emit, 0


def centred_tail_bound(segment_frames: int) -> int:
    """The centred tail never keeps this many samples: it starts one sample before the next frame to emit, and the last
    sample of the frame ``segment_frames - 1`` hops later would complete the group."""
    return CENTRED_HOP * (segment_frames - 1) + WIN + 1


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
# front ends
# --------------------------------------------------------------------------- #
class _SampleTail:
    """The device-side sample buffer of a streamed front end: the samples of the frames not emitted yet (the tail) in a
    buffer whose capacity follows the largest push, and the kernel's carried state beside it."""

    def reset(self):
        """Forget the stream: the next push is sample 0 again (of any batch size, on any device)."""
        self.frames = 0
        self.nb = None
        self._buf = None                 # [nb, capacity, nch]; the tail is _buf[:, _start:_start + _len]
        self._start = self._len = 0
        self._state = None

    @property
    def tail_samples(self) -> int:
        """Samples kept for frames not emitted yet (below the front end's tail bound)."""
        return self._len

    @property
    def buffer_samples(self) -> int:
        """Capacity of the device-side sample buffer, per channel and utterance."""
        return 0 if self._buf is None else self._buf.shape[1]

    def _allocate(self, chunk, state_bytes: int, bound: int):
        self.nb = chunk.shape[0]
        self._state = torch.zeros(state_bytes, dtype=torch.uint8, device=chunk.device)      # mu_{-1} = 0
        self._buf = torch.empty((self.nb, 2 * bound, self.nch), dtype=torch.float32, device=chunk.device)

    def _accept(self, chunk):
        """The checks of a pushed chunk; opens the stream on the first one."""
        ops._need_dev(chunk)
        if chunk.ndim != 3 or chunk.shape[2] != self.nch:
            raise RuntimeError("fnssl.stream: expected a chunk [nb, n, %d], got %s" % (self.nch, tuple(chunk.shape)))
        if self.nb is None:
            self._open(chunk)
        elif chunk.shape[0] != self.nb or chunk.device != self._buf.device:
            raise RuntimeError("fnssl.stream: the stream was opened with %d utterances on %s, got %d on %s (reset() first)"
                               % (self.nb, self._buf.device, chunk.shape[0], chunk.device))

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


class StreamFrontEnd(_SampleTail):
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

    def _open(self, chunk):
        nb = chunk.shape[0]
        lib = _lib.load()
        nbytes = lib.fnssl_stream_frontend_state_bytes(nb, self.nch, STREAM_MODE[self.mode], CH_MODE[self.ch_mode], 1 << 20)
        if nbytes == 0:
            raise RuntimeError("fnssl.stream: no streamed front end for %d utterances x %d channels (mode %r)"
                               % (nb, self.nch, self.mode))
        self._allocate(chunk, nbytes, tail_bound(self.segment_frames))

    @ops.on_device
    def push(self, chunk):
        self._accept(chunk)
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

    def finish(self):
        """The end of the stream completes nothing here: a hop-256 frame depends on its own samples only."""
        return None


class CentredStreamFrontEnd(_SampleTail):
    """IPDnet2's front end from a stream: ``push(chunk [nb, n, nch]) -> [nb, T, 256, 2 * nch]``, the features of the frames
    the chunk completes, in groups of ``segment_frames`` (T possibly 0); ``finish()`` says that the stream has ended and
    returns the frames only the known end completes (the last frame may reflect at it), again in whole groups, the rest
    being dropped as the network's time pooling drops them.  Pushes and ``finish`` together give the bits of
    ``ops.preprocess_ipdnet2`` on the whole signal, cut to whole groups.  After ``finish()`` only ``reset()`` starts a new
    stream."""

    def __init__(self, nch: int, sample_length: int = CENTRED_SAMPLE_LENGTH, eps: float = 1e-6, normalise: bool = True,
                 segment_frames: int = 5):
        if int(segment_frames) <= 0:
            raise ValueError("CentredStreamFrontEnd: segment_frames must be positive, got %r" % (segment_frames,))
        if int(nch) < 1:
            raise ValueError("CentredStreamFrontEnd: %d channels" % int(nch))
        if int(sample_length) <= 0:
            raise ValueError("CentredStreamFrontEnd: sample_length must be positive, got %r" % (sample_length,))
        self.nch = int(nch)
        self.sample_length = int(sample_length)
        self.normalise = bool(normalise)
        self.eps = float(eps) if self.normalise else 1.0
        self.segment_frames = int(segment_frames)
        self.nrows = 1
        self.width = 2 * self.nch
        self.reset()

    def reset(self):
        super().reset()
        self.finished = False

    @property
    def samples(self) -> int:
        """Samples pushed so far."""
        return centred_tail_start(self.frames) + self._len

    def _open(self, chunk):
        nb = chunk.shape[0]
        nbytes = _lib.load().fnssl_stream_frontend_centred_state_bytes(nb, self.nch, 1 << 20)
        if nbytes == 0:
            raise RuntimeError("fnssl.stream: no centred streamed front end for %d utterances x %d channels" % (nb, self.nch))
        self._allocate(chunk, nbytes, centred_tail_bound(self.segment_frames))

    def _emit(self, emit: int, total: int):
        """Frames [frames, frames + emit) from the tail; ``total`` < 0 while the stream is open."""
        dev = self._buf.device
        x = torch.empty((self.nb, emit, ops.NF, self.width), dtype=torch.float32, device=dev)
        if emit == 0:
            return x
        win = self._buf[:, self._start:self._start + self._len]
        ca, cb = _stream_coefs(self.sample_length, self.normalise, dev)
        sb, sn, sc = win.stride()
        check(_lib.load().fnssl_stream_frontend_centred(
            ops._ptr(win), self.nb, self._len, self.nch, sb, sn, sc, centred_tail_start(self.frames), self.frames, emit,
            total, ops._ptr(ca), ops._ptr(cb), self.sample_length, self.eps, ops._ptr(self._state), self._state.numel(),
            ops._ptr(x), ops._stream()), "stream_frontend_centred")
        drop = centred_tail_start(self.frames + emit) - centred_tail_start(self.frames)
        self.frames += emit
        self._start += drop               # consumed samples are dropped: the next append moves what is left
        self._len -= drop
        return x

    @ops.on_device
    def push(self, chunk):
        if self.finished:
            raise RuntimeError("fnssl.stream: the stream has been finished (reset() starts a new one)")
        self._accept(chunk)
        emit, keep = centred_plan_push(self._len, chunk.shape[1], self.segment_frames, self.frames)
        if chunk.shape[1]:
            self._append(chunk)
        x = self._emit(emit, -1)
        assert self._len == keep
        return x

    def finish(self):
        if self.finished:
            raise RuntimeError("fnssl.stream: the stream has been finished (reset() starts a new one)")
        total = self.samples
        if total <= WIN // 2:             # the whole-signal transform's own condition (torch.stft's for reflect padding)
            raise RuntimeError("fnssl.stream: signal of %d samples is too short for reflect padding of %d" % (total, WIN // 2))
        emit, _ = centred_plan_finish(total, self.segment_frames, self.frames)
        with torch.cuda.device(self._buf.device):
            x = self._emit(emit, total)
        self.finished = True
        self._start = self._len = 0
        return x


# --------------------------------------------------------------------------- #
# front end -> network -> DOA
# --------------------------------------------------------------------------- #
class OnlineLocalizer:
    """``push(chunk [nb, n, nch]) -> (pred, doa)``: the emitted features go through ``model.forward_stream`` with its
    carried state; ``localize`` (a callable on the new prediction, e.g. the template search of ``PredDOA``) gives ``doa``.
    Both are None while the push completes no segment.  ``finish() -> (pred, doa)`` ends the stream: the same for the
    frames only the known end completes (``CentredStreamFrontEnd``), (None, None) otherwise.  ``model`` is an online fp32
    ``FN_SSL`` / ``IPDnet`` with a ``StreamFrontEnd``, or an ``OnlineSpatialNet`` (IPDnet2, fp32 or bf16) with a
    ``CentredStreamFrontEnd``; the errors for offline, bf16 LSTM or ``train()``-mode modules are ``forward_stream``'s own."""

    def __init__(self, model, frontend, localize=None):
        group = getattr(model, "time_compression_ratio", ops.SEG_FRAMES)      # OnlineSpatialNet pools 5 frames, the LSTMs 12
        if frontend.segment_frames % group:
            raise ValueError("OnlineLocalizer: the network consumes groups of %d frames, the front end emits groups of %d"
                             % (group, frontend.segment_frames))
        if hasattr(model, "time_compression_ratio"):
            takes = model.encoder.in_channels
        else:
            takes = getattr(model, "input_size", frontend.width)
        if takes != frontend.width:
            raise ValueError("OnlineLocalizer: the front end emits %d feature channels, the network takes %d"
                             % (frontend.width, takes))
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
            # the shape errors of FN_SSL / IPDnet and of OnlineSpatialNet: the module itself was accepted
            if "expected [nb" not in str(e) and "chunks must be positive multiples" not in str(e):
                raise

    def reset(self):
        self.frontend.reset()
        self.state = None

    def _forward(self, x):
        if x is None or x.shape[1] == 0:
            return None, None
        pred, self.state = self.model.forward_stream(x.permute(0, 3, 2, 1), self.state)   # a view: nothing is moved
        return pred, (self.localize(pred) if self.localize is not None else None)

    def push(self, chunk):
        return self._forward(self.frontend.push(chunk))

    def finish(self):
        return self._forward(self.frontend.finish())
