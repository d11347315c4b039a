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

``StreamPool`` (front end alone: ``PoolFrontEnd``) serves independent IPDnet2 streams, each with its own start, chunk
sizes and end, with one set of launches per push: ``pool_plan_push`` is the host arithmetic, DESIGN.md 3.3b the design.
``LstmStreamPool`` (front end alone: ``HopPoolFrontEnd``) is the same for the hop-256 models, FN-SSL and IPDnet, whose
carried state is ``forward_stream``'s dict of tensors and LSTM workspaces: ``hop_pool_plan_push``, DESIGN.md 3.3c.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

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
class _TailBuffer:
    """Device sample storage ``[rows, capacity, nch]`` for streamed front ends.  The rows are grouped into lanes that
    advance on their own: lane k keeps the samples of its frames not emitted yet (its tail) at
    ``buf[rows_k, start[k]:start[k] + len[k]]``.  A lock-step front end has one lane of all its rows, a pool one lane per
    slot.  The capacity follows the largest push, not the length of a stream: an append that does not fit behind a
    lane's tail moves that tail to the front, and one that does not fit the buffer doubles it (every lane's tail then
    moves to the front of the new buffer)."""

    def __init__(self, rows: int, nch: int, capacity: int, device, lanes: int = 1):
        self.buf = torch.empty((rows, capacity, nch), dtype=torch.float32, device=device)
        self.lane_rows = [slice(None)] if lanes == 1 else [slice(k, k + 1) for k in range(lanes)]
        self.start = [0] * lanes
        self.len = [0] * lanes

    @property
    def capacity(self) -> int:
        return self.buf.shape[1]

    def window(self, k: int = 0):
        return self.buf[self.lane_rows[k], self.start[k]:self.start[k] + self.len[k]]

    def _to_front(self, k: int, buf):
        """Lane k's tail to the front of ``buf`` (the buffer itself, or its larger successor)."""
        n = self.len[k]
        if n and (buf is not self.buf or self.start[k]):
            tail = self.window(k)
            buf[self.lane_rows[k], :n].copy_(tail.clone() if buf is self.buf else tail)
        self.start[k] = 0

    def append(self, k: int, chunk):
        """``chunk [rows of lane k, n, nch]`` (any strides: read in place) behind lane k's tail."""
        n = chunk.shape[1]
        if self.start[k] + self.len[k] + n > self.capacity:
            if self.len[k] + n <= self.capacity:
                self._to_front(k, self.buf)
            else:
                buf = torch.empty((self.buf.shape[0], 2 * (self.len[k] + n), self.buf.shape[2]), dtype=torch.float32,
                                  device=self.buf.device)
                for j in range(len(self.len)):
                    self._to_front(j, buf)
                self.buf = buf
        at = self.start[k] + self.len[k]
        self.buf[self.lane_rows[k], at:at + n].copy_(chunk)
        self.len[k] += n

    def drop(self, k: int, n: int):
        """Lane k has consumed its first ``n`` samples: the next append moves what is left."""
        self.start[k] += n
        self.len[k] -= n

    def clear(self, k: int):
        self.start[k] = self.len[k] = 0


class _SampleTail:
    """The device-side sample buffer of a streamed front end: the samples of the frames not emitted yet (the tail) in a
    one-lane ``_TailBuffer``, and the kernel's carried state beside it."""

    def reset(self):
        """Forget the stream: the next push is sample 0 again (of any batch size, on any device)."""
        self.frames = 0
        self.nb = None
        self._tail = None                # the one-lane _TailBuffer [nb, capacity, nch], allocated by the first push
        self._state = None

    @property
    def tail_samples(self) -> int:
        """Samples kept for frames not emitted yet (below the front end's tail bound)."""
        return 0 if self._tail is None else self._tail.len[0]

    @property
    def buffer_samples(self) -> int:
        """Capacity of the device-side sample buffer, per channel and utterance."""
        return 0 if self._tail is None else self._tail.capacity

    def _allocate(self, chunk, state_bytes: int, bound: int):
        self.nb = chunk.shape[0]
        self._state = torch.zeros(state_bytes, dtype=torch.uint8, device=chunk.device)      # mu_{-1} = 0
        self._tail = _TailBuffer(self.nb, self.nch, 2 * bound, chunk.device)

    def _accept(self, chunk):
        """The checks of a pushed chunk; opens the stream on the first one."""
        ops._need_dev(chunk)
        if chunk.ndim != 3 or chunk.shape[2] != self.nch:
            raise RuntimeError("fnssl.stream: expected a chunk [nb, n, %d], got %s" % (self.nch, tuple(chunk.shape)))
        if self.nb is None:
            self._open(chunk)
        elif chunk.shape[0] != self.nb or chunk.device != self._tail.buf.device:
            raise RuntimeError("fnssl.stream: the stream was opened with %d utterances on %s, got %d on %s (reset() first)"
                               % (self.nb, self._tail.buf.device, chunk.shape[0], chunk.device))

    def _append(self, chunk):
        self._tail.append(0, chunk)


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
        emit, keep = plan_push(self.tail_samples, chunk.shape[1], self.segment_frames)
        if chunk.shape[1]:
            self._append(chunk)
        x = torch.empty((self.nb * self.nrows, emit, ops.NF, self.width), dtype=torch.float32, device=chunk.device)
        if emit == 0:
            return x
        win = self._tail.window()
        ca, cb = _stream_coefs(self.sample_length, self.normalise, chunk.device)
        sb, sn, sc = win.stride()
        check(_lib.load().fnssl_stream_frontend(
            ops._ptr(win), self.nb, win.shape[1], self.nch, sb, sn, sc, STREAM_MODE[self.mode], CH_MODE[self.ch_mode],
            self.frames, emit, ops._ptr(ca), ops._ptr(cb), self.sample_length, self.eps, ops._ptr(self._state),
            self._state.numel(), ops._ptr(x), ops._stream()), "stream_frontend")
        self.frames += emit
        self._tail.drop(0, HOP * emit)    # consumed samples are dropped: the next append moves what is left
        assert self.tail_samples == keep
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
        return centred_tail_start(self.frames) + self.tail_samples

    def _open(self, chunk):
        nb = chunk.shape[0]
        nbytes = _lib.load().fnssl_stream_frontend_centred_state_bytes(nb, self.nch, 1 << 20)
        if nbytes == 0:
            raise RuntimeError("fnssl.stream: no centred streamed front end for %d utterances x %d channels" % (nb, self.nch))
        self._allocate(chunk, nbytes, centred_tail_bound(self.segment_frames))

    def _emit(self, emit: int, total: int):
        """Frames [frames, frames + emit) from the tail; ``total`` < 0 while the stream is open."""
        dev = self._tail.buf.device
        x = torch.empty((self.nb, emit, ops.NF, self.width), dtype=torch.float32, device=dev)
        if emit == 0:
            return x
        win = self._tail.window()
        ca, cb = _stream_coefs(self.sample_length, self.normalise, dev)
        sb, sn, sc = win.stride()
        check(_lib.load().fnssl_stream_frontend_centred(
            ops._ptr(win), self.nb, win.shape[1], self.nch, sb, sn, sc, centred_tail_start(self.frames), self.frames, emit,
            total, ops._ptr(ca), ops._ptr(cb), self.sample_length, self.eps, ops._ptr(self._state), self._state.numel(),
            ops._ptr(x), ops._stream()), "stream_frontend_centred")
        drop = centred_tail_start(self.frames + emit) - centred_tail_start(self.frames)
        self.frames += emit
        self._tail.drop(0, drop)          # consumed samples are dropped: the next append moves what is left
        return x

    @ops.on_device
    def push(self, chunk):
        if self.finished:
            raise RuntimeError("fnssl.stream: the stream has been finished (reset() starts a new one)")
        self._accept(chunk)
        emit, keep = centred_plan_push(self.tail_samples, chunk.shape[1], self.segment_frames, self.frames)
        if chunk.shape[1]:
            self._append(chunk)
        x = self._emit(emit, -1)
        assert self.tail_samples == keep
        return x

    def finish(self):
        if self.finished:
            raise RuntimeError("fnssl.stream: the stream has been finished (reset() starts a new one)")
        total = self.samples
        if total <= WIN // 2:             # the whole-signal transform's own condition (torch.stft's for reflect padding)
            raise RuntimeError("fnssl.stream: signal of %d samples is too short for reflect padding of %d" % (total, WIN // 2))
        emit, _ = centred_plan_finish(total, self.segment_frames, self.frames)
        with torch.cuda.device(self._tail.buf.device):
            x = self._emit(emit, total)
        self.finished = True
        self._tail.clear(0)
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


# --------------------------------------------------------------------------- #
# a pool of independent IPDnet2 streams
# --------------------------------------------------------------------------- #
class PoolGroup(NamedTuple):
    """One group of ``group`` frames that one slot emits in one round of a pool push."""
    slot: int
    frame0: int          # absolute index of the group's first frame
    sample0: int         # absolute index of the first sample the slot still holds = centred_tail_start(frame0)
    ns: int              # samples it holds from there on
    total: int           # length of the slot's whole signal where this group needs it (it follows the end), else -1
    fresh: bool          # the slot's first group: mu and the network state start from zero


def pool_plan_push(streams: dict, new: dict, last=(), group: int = 5):
    """The host arithmetic of ``StreamPool.push``.  ``streams``: slot -> (frames emitted, samples in the tail) of every
    open, unfinished slot; ``new``: slot -> samples arriving; ``last``: the slots whose signal ends with them.  Returns
    (rounds, after): in round r every slot that completes more than r groups emits exactly its r-th one (a ``PoolGroup``,
    in slot order), so every row of a round has the same frame count; ``after``: slot -> (frames, tail) once the push is
    done (a finished slot keeps no tail).  The groups of a slot are those of ``centred_plan_push`` on the arriving samples
    and then, for a slot in ``last``, of ``centred_plan_finish`` on the length that is then known.  Nothing is modified;
    an error (unknown slot, a signal of 256 samples or fewer that ends) is raised before anything is planned."""
    last = set(last)
    for slot in list(new) + list(last):
        if slot not in streams:
            raise KeyError("pool_plan_push: slot %r is not an open, unfinished stream" % (slot,))
    per_slot, after = {}, {}
    for slot in sorted(set(new) | last):
        frames, tail = streams[slot]
        n = int(new.get(slot, 0))
        emit, keep = centred_plan_push(tail, n, group, frames)
        arrived = centred_tail_start(frames) + tail + n
        totals = [-1] * (emit // group)
        if slot in last:
            if arrived <= WIN // 2:
                raise RuntimeError("fnssl.stream: slot %d ends after %d samples, too short for reflect padding of %d"
                                   % (slot, arrived, WIN // 2))
            more, keep = centred_plan_finish(arrived, group, frames + emit)
            totals += [arrived] * (more // group)
        per_slot[slot] = [PoolGroup(slot, f0, centred_tail_start(f0), arrived - centred_tail_start(f0), total, f0 == 0)
                          for f0, total in ((frames + group * r, t) for r, t in enumerate(totals))]
        after[slot] = (frames + group * len(totals), keep)
    depth = max([len(g) for g in per_slot.values()], default=0)
    rounds = [[g[r] for g in per_slot.values() if len(g) > r] for r in range(depth)]
    return rounds, after


def pool_pack_descriptors(groups, group: int, sig_offset_of):
    """The ``PoolGroup``s of a round -> the ctypes descriptor array of ``fnssl_stream_frontend_centred_pool`` (row a of
    the output belongs to groups[a]; the library cuts the array into launches of ``_lib.STREAM_POOL_MAX_DESC``) and the
    sizes of those launches.  ``sig_offset_of(g)``: floats from the storage's base to the slot's sample ``g.sample0``."""
    descs = (_lib.StreamPoolDesc * len(groups))()
    for a, g in enumerate(groups):
        descs[a] = _lib.StreamPoolDesc(slot=g.slot, frame0=g.frame0, nframes=group, out_row=a, fresh=int(g.fresh), ns=g.ns,
                                       sample0=g.sample0, total=g.total, sig_offset=sig_offset_of(g))
    m = _lib.STREAM_POOL_MAX_DESC
    return descs, [min(m, len(groups) - i) for i in range(0, len(groups), m)]


class _Slot:
    """Host-side position of one stream of a pool."""
    __slots__ = ("frames", "finished")

    def __init__(self):
        self.frames, self.finished = 0, False


class PoolFrontEnd:
    """IPDnet2's front end for ``slots`` independent streams: ``open() -> slot``, ``push({slot: chunk [n, nch]}, last=())
    -> [(groups, x [A, segment_frames, 256, 2 * nch]), ...]``, one entry per round of ``pool_plan_push`` and ONE
    ``fnssl_stream_frontend_centred_pool`` call each (row a of x holds the frames of groups[a]); ``close(slot)`` frees a
    slot, whose next stream starts from mu = 0 by descriptor, without a launch; ``reset()`` closes all.  Every slot's
    emitted frames are the bits of ``ops.preprocess_ipdnet2`` on its own signal, cut to whole groups."""

    def __init__(self, nch: int, slots: int, sample_length: int = CENTRED_SAMPLE_LENGTH, eps: float = 1e-6,
                 segment_frames: int = 5):
        if int(slots) <= 0:
            raise ValueError("PoolFrontEnd: %r slots" % (slots,))
        if int(nch) < 1:
            raise ValueError("PoolFrontEnd: %d channels" % int(nch))
        if int(sample_length) <= 0 or int(segment_frames) <= 0:
            raise ValueError("PoolFrontEnd: sample_length %r, segment_frames %r" % (sample_length, segment_frames))
        self.nch, self.nslots = int(nch), int(slots)
        self.sample_length, self.eps, self.group = int(sample_length), float(eps), int(segment_frames)
        self.launches = 0                # kernel launches so far (a call cuts its descriptors into launches of 64)
        self._tails = self._state = None
        self.reset()

    def reset(self):
        """Close every slot.  The device buffers stay as they are: nothing is zeroed."""
        self._slots = {}
        if self._tails is not None:
            for k in range(self.nslots):
                self._tails.clear(k)

    def open(self) -> int:
        for slot in range(self.nslots):
            if slot not in self._slots:
                self._slots[slot] = _Slot()
                return slot
        raise RuntimeError("fnssl.stream: all %d slots of the pool are open" % self.nslots)

    def close(self, slot: int):
        self._stream(slot, finished_ok=True)
        del self._slots[slot]
        if self._tails is not None:
            self._tails.clear(slot)

    def _stream(self, slot, finished_ok=False):
        st = self._slots.get(slot)
        if st is None:
            raise KeyError("fnssl.stream: slot %r of the pool is not open" % (slot,))
        if st.finished and not finished_ok:
            raise RuntimeError("fnssl.stream: the stream of slot %d has been finished (close() it; open() starts a new one)" % slot)
        return st

    def frames(self, slot: int) -> int:
        """Frames the slot's stream has emitted so far."""
        return self._stream(slot, True).frames

    def finished(self, slot: int) -> bool:
        return self._stream(slot, True).finished

    def tail_samples(self, slot: int) -> int:
        self._stream(slot, True)
        return 0 if self._tails is None else self._tails.len[slot]

    def samples(self, slot: int) -> int:
        """Samples pushed into the slot's stream so far (0 once it is finished: its tail is dropped)."""
        return centred_tail_start(self._stream(slot, True).frames) + self.tail_samples(slot)

    @property
    def buffer_samples(self) -> int:
        return 0 if self._tails is None else self._tails.capacity

    @property
    def device(self):
        return None if self._tails is None else self._tails.buf.device

    def _allocate(self, device):
        nbytes = _lib.load().fnssl_stream_frontend_centred_state_bytes(self.nslots, self.nch, 1 << 20)
        if nbytes == 0:
            raise RuntimeError("fnssl.stream: no centred streamed front end for %d slots x %d channels" % (self.nslots, self.nch))
        self._state = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self._tails = _TailBuffer(self.nslots, self.nch, 2 * centred_tail_bound(self.group), device, lanes=self.nslots)

    def _launch(self, groups):
        buf = self._tails.buf
        x = torch.empty((len(groups), self.group, ops.NF, 2 * self.nch), dtype=torch.float32, device=buf.device)
        sb, sn, sc = buf.stride()
        base = {g.slot: centred_tail_start(self._slots[g.slot].frames) for g in groups}     # absolute index of the tail's first sample

        def sig_offset(g):
            at = g.sample0 - base[g.slot]
            assert at >= 0 and at + g.ns == self._tails.len[g.slot]       # the window lies inside the slot's tail
            return g.slot * sb + (self._tails.start[g.slot] + at) * sn

        descs, launches = pool_pack_descriptors(groups, self.group, sig_offset)
        ca, cb = _stream_coefs(self.sample_length, True, buf.device)
        check(_lib.load().fnssl_stream_frontend_centred_pool(
            ops._ptr(buf), self.nslots, self.nch, sn, sc, descs, len(groups), ops._ptr(ca), ops._ptr(cb), self.sample_length,
            self.eps, ops._ptr(self._state), self._state.numel(), ops._ptr(x), len(groups), self.group, ops._stream()),
            "stream_frontend_centred_pool")
        self.launches += len(launches)
        return x

    def push(self, chunks: dict, last=()):
        last = tuple(last)
        for slot in list(chunks) + list(last):
            self._stream(slot)
        device = self.device
        for slot, chunk in chunks.items():
            if not isinstance(chunk, torch.Tensor) or chunk.ndim != 2 or chunk.shape[1] != self.nch:
                raise RuntimeError("fnssl.stream: slot %d: expected a chunk [n, %d], got %s"
                                   % (slot, self.nch, tuple(getattr(chunk, "shape", ()))))
            ops._need_dev(chunk)
            device = chunk.device if device is None else device
            if chunk.device != device:
                raise RuntimeError("fnssl.stream: the pool lives on %s, slot %d was pushed a chunk on %s" % (device, slot, chunk.device))
        tail = (lambda s: 0) if self._tails is None else (lambda s: self._tails.len[s])
        streams = {s: (st.frames, tail(s)) for s, st in self._slots.items() if not st.finished}
        rounds, after = pool_plan_push(streams, {s: c.shape[0] for s, c in chunks.items()}, last, self.group)
        out = []
        if device is not None:           # (no device yet: nothing has ever been pushed, and nothing was planned)
            with torch.cuda.device(device):
                if self._tails is None:
                    self._allocate(device)
                for slot, chunk in chunks.items():
                    if chunk.shape[0]:
                        self._tails.append(slot, chunk.unsqueeze(0))
                out = [(groups, self._launch(groups)) for groups in rounds]
        for slot, (frames, keep) in after.items():
            st = self._slots[slot]
            if slot in last:
                st.finished = True
                if self._tails is not None:
                    self._tails.clear(slot)
            elif self._tails is not None:
                self._tails.drop(slot, centred_tail_start(frames) - centred_tail_start(st.frames))
                assert self._tails.len[slot] == keep
            st.frames = frames
        return out

    def finish(self, slot: int):
        """The slot's signal has ended: a push of no samples with the slot in ``last``."""
        return self.push({}, last=(slot,))


class StreamPool:
    """``slots`` independent IPDnet2 streams on one device, each with its own sample tail, frame count, normalisation
    ``mu``, network state and end; ``model`` is an ``OnlineSpatialNet`` (fp32 or bf16) in eval mode.

    ``open() -> slot``; ``push({slot: chunk [n, nch]}, last=()) -> {slot: (pred [g, 512, nmic - 1, 2], doa)}`` for the
    slots that completed g >= 1 groups of 5 frames (n is free per slot, 0 allowed; slots in ``last`` end with their chunk
    and also emit what only the known end completes); ``finish(slot)``; ``close(slot)`` frees a slot, whose next
    ``open()`` starts from zero without a launch; ``reset()`` closes all.  ``doa`` is None without ``localize``, else a
    list with one entry per group: what ``localize(pred [A, 1, 512, nmic - 1, 2])`` returned for the A rows of a network
    call, narrowed to this stream along ``localize_batch_dim`` (1: the layout of ``PredDOA._search``).

    The device work of a push is per ROUND (a real-time push is one round; a catch-up push that completes several groups
    of a slot takes one per group), whatever the number of slots: one ``fnssl_stream_frontend_centred_pool`` call
    (``PoolFrontEnd``), ONE ``fnssl_sn_forward`` on the round's rows — in place on the pool's state when they are all
    slots in order and none is fresh, otherwise on a compact state between one gather and one scatter
    (``fnssl_sn_state_rows``) —, and ``localize``.  Fresh rows (a stream's first group) ride in the carried rows' call:
    the gather hands them zeros, and a zeroed state under ``carry=True`` gives the bits of ``forward_stream(x, None)``, in
    fp32 and in bf16 (tests/test_gpu_stream_pool.py::test_first_group_finding)."""

    def __init__(self, model, nch: int, slots: int, localize=None, sample_length: int = CENTRED_SAMPLE_LENGTH,
                 eps: float = 1e-6, localize_batch_dim: int = 1):
        if not hasattr(model, "time_compression_ratio") or not hasattr(model, "device_net"):
            raise ValueError("StreamPool: the model must be an OnlineSpatialNet (IPDnet2), got %s" % type(model).__name__)
        self.frontend = PoolFrontEnd(nch, slots, sample_length, eps, model.time_compression_ratio)
        if model.encoder.in_channels != 2 * self.frontend.nch:
            raise ValueError("StreamPool: the front end emits %d feature channels, the network takes %d"
                             % (2 * self.frontend.nch, model.encoder.in_channels))
        self.model, self.localize, self.localize_batch_dim = model, localize, int(localize_batch_dim)
        self.nslots = self.frontend.nslots
        # as OnlineLocalizer: a zero-frame call runs forward_stream's checks of the module (eval mode) and stops at its
        # shape check, so a module in train() mode fails here and not at the first completed group
        try:
            model.forward_stream(torch.zeros((1, 2 * self.frontend.nch, ops.NF, 0)))
        except RuntimeError as e:
            if "chunks must be positive multiples" not in str(e):
                raise
        self.in_place = True             # False: every call of the network goes through gather and scatter (tests)
        self.gathers = self.scatters = 0
        self._dn = self._net_state = self._compact = None

    def open(self) -> int:
        return self.frontend.open()

    def close(self, slot: int):
        self.frontend.close(slot)

    def reset(self):
        self.frontend.reset()

    def _rows(self, slots, direction, fresh=None):
        n = len(slots)
        check(_lib.load().fnssl_sn_state_rows(
            C.byref(self._dn.net), self.nslots, self._dn.num_freqs, ops._ptr(self._net_state), n, ops._ptr(self._compact),
            (C.c_int * n)(*slots), None if fresh is None else (C.c_ubyte * n)(*[int(f) for f in fresh]), direction,
            ops._stream()), "sn_state_rows")
        if direction == _lib.SN_ROWS_GATHER:
            self.gathers += 1
        else:
            self.scatters += 1

    def _network(self, x, groups):
        """The network on a round's rows ``x [n, 5, 256, 2 nch]``.  In place on the pool's state when the rows are all
        slots in order and all carried (or all fresh: ``carry=False`` reads no state); else on the compact state: gather
        (zeros for fresh rows; skipped when all rows are fresh), forward, scatter."""
        # fetched per call, as forward_stream does: weights or a dtype changed since the last push are picked up (the
        # model re-packs them when its parameters changed), while the carried state keeps its layout
        self._dn = self.model.device_net(x.device)
        if self._net_state is None:
            self._net_state = self._dn.new_state(self.nslots)
        slots = [g.slot for g in groups]
        fresh = [g.fresh for g in groups]
        carry = not all(fresh)
        xv = x.permute(0, 3, 2, 1)                                        # a view: nothing is moved
        if self.in_place and slots == list(range(self.nslots)) and (not carry or not any(fresh)):
            return self._dn.forward(xv, state=self._net_state, carry=carry)
        if self._compact is None:        # as large as the pool's state: holds the compact state of any number of rows
            self._compact = torch.empty_like(self._net_state)
        if carry:
            self._rows(slots, _lib.SN_ROWS_GATHER, fresh)
        nfloats = _lib.load().fnssl_sn_state_floats(C.byref(self._dn.net), len(slots), self._dn.num_freqs)
        pred = self._dn.forward(xv, state=self._compact[:nfloats], carry=carry)
        self._rows(slots, _lib.SN_ROWS_SCATTER)
        return pred

    @torch.no_grad()
    def push(self, chunks: dict, last=()):
        out = {}
        for groups, x in self.frontend.push(chunks, last):
            with torch.cuda.device(x.device):
                pred = self._network(x, groups)
                doa = self.localize(pred) if self.localize is not None else None
            for a, g in enumerate(groups):
                preds, doas = out.setdefault(g.slot, ([], []))
                preds.append(pred[a])
                if doa is not None:
                    one = lambda t: t.narrow(self.localize_batch_dim, a, 1)   # noqa: E731
                    doas.append(tuple(one(t) for t in doa) if isinstance(doa, (tuple, list)) else one(doa))
        return {slot: (torch.cat(preds, dim=0), doas if self.localize is not None else None)
                for slot, (preds, doas) in out.items()}

    def finish(self, slot: int):
        """``push({slot: no samples}, last=(slot,))``: the groups only the known end completes."""
        return self.push({}, last=(slot,))


# --------------------------------------------------------------------------- #
# a pool of independent hop-256 streams: FN-SSL / IPDnet
# --------------------------------------------------------------------------- #
def hop_pool_plan_push(streams: dict, new: dict, group: int = 12):
    """The host arithmetic of ``HopPoolFrontEnd.push``.  ``streams``: slot -> (frames emitted, samples in the tail) of every
    open slot; ``new``: slot -> samples arriving.  Returns (rounds, after) as ``pool_plan_push`` does: in round r every slot
    that completes more than r groups emits its r-th one (a ``PoolGroup`` with ``total = -1``, in slot order); ``after``:
    slot -> (frames, tail) once the push is done, which is ``plan_push`` per slot.  There is no ``last``: a hop-256 frame
    depends on its own samples only, so the end of a stream completes nothing (``StreamFrontEnd.finish``).  Nothing is
    modified; an unknown slot raises before anything is planned."""
    for slot in new:
        if slot not in streams:
            raise KeyError("hop_pool_plan_push: slot %r is not an open stream" % (slot,))
    per_slot, after = {}, {}
    for slot in sorted(new):
        frames, tail = streams[slot]
        have = tail + int(new[slot])
        emit, keep = plan_push(tail, int(new[slot]), group)
        per_slot[slot] = [PoolGroup(slot, f0, HOP * f0, have - HOP * (f0 - frames), -1, f0 == 0)
                          for f0 in range(frames, frames + emit, group)]
        after[slot] = (frames + emit, keep)
    depth = max([len(g) for g in per_slot.values()], default=0)
    rounds = [[g[r] for g in per_slot.values() if len(g) > r] for r in range(depth)]
    return rounds, after


class HopPoolFrontEnd(PoolFrontEnd):
    """The front end of FN-SSL (mode ``'pair'``) / IPDnet (mode ``'array'``) for ``slots`` independent streams, with the
    surface of ``PoolFrontEnd`` (no ``last`` / ``finish``: the end of a hop-256 stream completes nothing): ``push({slot:
    chunk [n, nch]}) -> [(groups, x), ...]``, one entry per round of ``hop_pool_plan_push`` and ONE
    ``fnssl_stream_frontend_pool`` call each.  The frames of groups[a] are rows ``a * nrows .. a * nrows + nrows - 1`` of
    ``x [A * nrows, segment_frames, 256, 4]`` (pair mode, ``nrows`` = microphone pairs) or row a of ``x [A, segment_frames,
    256, 2 * nch]`` (array mode).  Every slot's emitted frames are the bits of ``ops.pair_features`` /
    ``ops.array_features`` on its own signal."""

    def __init__(self, mode: str, nch: int, slots: int, ch_mode: str = "MM", sample_length: int = None, eps: float = 1e-6,
                 segment_frames: int = 12):
        if mode not in STREAM_MODE:
            raise ValueError("HopPoolFrontEnd: mode must be 'pair' or 'array', got %r" % (mode,))
        if mode == "pair" and ch_mode not in CH_MODE:
            raise ValueError("HopPoolFrontEnd: ch_mode must be 'M' or 'MM', got %r" % (ch_mode,))
        if int(slots) <= 0:
            raise ValueError("HopPoolFrontEnd: %r slots" % (slots,))
        if int(nch) < (2 if mode == "pair" else 1):
            raise ValueError("HopPoolFrontEnd: %d channels" % int(nch))
        sample_length = DEFAULT_SAMPLE_LENGTH[mode] if sample_length is None else sample_length
        if int(sample_length) <= 0 or int(segment_frames) <= 0:
            raise ValueError("HopPoolFrontEnd: sample_length %r, segment_frames %r" % (sample_length, segment_frames))
        self.mode, self.ch_mode = mode, ch_mode if mode == "pair" else "M"
        self.nch, self.nslots = int(nch), int(slots)
        self.sample_length, self.eps, self.group = int(sample_length), float(eps), int(segment_frames)
        self.nrows = ops.num_pairs(self.nch, self.ch_mode) if mode == "pair" else 1      # feature rows per slot
        self.width = 4 if mode == "pair" else 2 * self.nch
        self.launches = 0
        self._tails = self._state = None
        self.reset()

    def samples(self, slot: int) -> int:
        """Samples pushed into the slot's stream so far."""
        return HOP * self._stream(slot).frames + self.tail_samples(slot)

    def _allocate(self, device):
        # sized for full 12-frame tiles, as the library spaces the scratch rows of arrays that do not fit the LDS
        nbytes = _lib.load().fnssl_stream_frontend_state_bytes(self.nslots, self.nch, STREAM_MODE[self.mode],
                                                               CH_MODE[self.ch_mode], ops.SEG_FRAMES)
        if nbytes == 0:
            raise RuntimeError("fnssl.stream: no streamed front end for %d slots x %d channels (mode %r)"
                               % (self.nslots, self.nch, self.mode))
        self._state = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self._tails = _TailBuffer(self.nslots, self.nch, 2 * tail_bound(self.group), device, lanes=self.nslots)

    def _launch(self, groups):
        buf = self._tails.buf
        x = torch.empty((len(groups) * self.nrows, self.group, ops.NF, self.width), dtype=torch.float32, device=buf.device)
        sb, sn, sc = buf.stride()

        def sig_offset(g):
            at = g.sample0 - HOP * self._slots[g.slot].frames             # the lane starts with the next frame to emit
            assert at >= 0 and at + g.ns == self._tails.len[g.slot]       # the window lies inside the slot's tail
            return g.slot * sb + (self._tails.start[g.slot] + at) * sn

        descs, launches = pool_pack_descriptors(groups, self.group, sig_offset)
        ca, cb = _stream_coefs(self.sample_length, True, buf.device)
        check(_lib.load().fnssl_stream_frontend_pool(
            ops._ptr(buf), self.nslots, self.nch, sn, sc, STREAM_MODE[self.mode], CH_MODE[self.ch_mode], descs, len(groups),
            ops._ptr(ca), ops._ptr(cb), self.sample_length, self.eps, ops._ptr(self._state), self._state.numel(), ops._ptr(x),
            len(groups), self.group, ops._stream()), "stream_frontend_pool")
        self.launches += len(launches)
        return x

    def push(self, chunks: dict):
        for slot in chunks:
            self._stream(slot)
        device = self.device
        for slot, chunk in chunks.items():
            if not isinstance(chunk, torch.Tensor) or chunk.ndim != 2 or chunk.shape[1] != self.nch:
                raise RuntimeError("fnssl.stream: slot %d: expected a chunk [n, %d], got %s"
                                   % (slot, self.nch, tuple(getattr(chunk, "shape", ()))))
            ops._need_dev(chunk)
            device = chunk.device if device is None else device
            if chunk.device != device:
                raise RuntimeError("fnssl.stream: the pool lives on %s, slot %d was pushed a chunk on %s" % (device, slot, chunk.device))
        tail = (lambda s: 0) if self._tails is None else (lambda s: self._tails.len[s])
        streams = {s: (st.frames, tail(s)) for s, st in self._slots.items()}
        rounds, after = hop_pool_plan_push(streams, {s: c.shape[0] for s, c in chunks.items()}, self.group)
        out = []
        if device is not None:           # (no device yet: nothing has ever been pushed, and nothing was planned)
            with torch.cuda.device(device):
                if self._tails is None:
                    self._allocate(device)
                for slot, chunk in chunks.items():
                    if chunk.shape[0]:
                        self._tails.append(slot, chunk.unsqueeze(0))
                out = [(groups, self._launch(groups)) for groups in rounds]
        for slot, (frames, keep) in after.items():
            st = self._slots[slot]
            if self._tails is not None:
                self._tails.drop(slot, HOP * (frames - st.frames))
                assert self._tails.len[slot] == keep
            st.frames = frames
        return out

    def finish(self, slot: int):
        """The end of a stream completes nothing here: a hop-256 frame depends on its own samples only."""
        self._stream(slot)
        return []


def _lstm_pool_kind(model):
    """'pair' for an ``FN_SSL``, 'array' for a fixed-array ``IPDnet``: told apart by the modules ``forward_stream`` of
    each walks."""
    if all(hasattr(model, a) for a in ("block_1", "block_2", "block_3", "emb2ipd", "forward_stream")):
        return "pair"
    if all(hasattr(model, a) for a in ("block_1", "block_2", "conv", "cnn_out_dim", "forward_stream")):
        return "array"
    raise ValueError("LstmStreamPool: the model must be an FN_SSL or a fixed-array IPDnet, got %s" % type(model).__name__)


class LstmStreamPool:
    """``slots`` independent FN-SSL / IPDnet streams on one device, each with its own sample tail, frame count,
    normalisation ``mu`` and network state; ``model`` is an online fp32 ``FN_SSL`` (front end 'pair') or ``IPDnet`` (front
    end 'array') in eval mode — the errors for anything else are ``forward_stream``'s own, raised here.

    ``open() -> slot``; ``push({slot: chunk [n, nch]}) -> {slot: (pred, doa)}`` for the slots that completed g >= 1 groups
    of 12 frames (n is free per slot, 0 allowed): ``pred`` is the slot's rows of ``forward_stream``'s prediction — ``[np, g,
    512]`` (FN-SSL) or ``[1, g, 512, nch - 1, ntrack]`` (IPDnet) —; ``close(slot)`` frees a slot, whose next ``open()``
    starts from zero without a launch; ``reset()`` closes all.  ``doa`` is None without ``localize``, else a list with one
    entry per group: what ``localize(pred of the call's rows)`` returned (a tensor, or a tuple / list / dict of tensors),
    narrowed to this slot's rows along ``localize_batch_dim``.

    The device work of a push is per ROUND (a real-time push is one round), whatever the number of slots: one
    ``fnssl_stream_frontend_pool`` call and ONE ``model.forward_stream`` call on the round's rows.  The state is
    ``forward_stream``'s dict for ``slots`` streams: the call runs in place on it when its rows are all slots in order and
    all carried, otherwise on a compact dict between one gather and one scatter (``fnssl_state_rows``) over the segments of
    ``_segments``: per narrow-band layer the slot's cell records at the front of the LSTM workspace
    (``fnssl_lstm_cell_group_floats``; everything behind them is rebuilt by each call) and the h / tail tensors.  Fresh
    rows (a stream's first group) ride in the carried rows' call: the gather hands them zeros, and a zeroed state under
    carry gives the bits of ``forward_stream(x, None)`` (DESIGN 3.3c;
    tests/test_gpu_stream_pool_lstm.py::test_first_group_finding)."""

    # forward_stream's carried tensors beside the workspaces: (key, index in the list or None)
    _TENSORS = {"pair": (("h", 0), ("h", 1), ("h", 2)),
                "array": (("n_tail", 0), ("n_tail", 1), ("x_tail", None), ("p_tail", 0), ("p_tail", 1))}

    def __init__(self, model, nch: int, slots: int, ch_mode: str = "MM", localize=None, localize_batch_dim: int = 0,
                 sample_length: int = None, eps: float = 1e-6):
        self.kind = _lstm_pool_kind(model)
        self.frontend = HopPoolFrontEnd(self.kind, nch, slots, ch_mode, sample_length, eps, ops.SEG_FRAMES)
        if model.input_size != self.frontend.width:
            raise ValueError("LstmStreamPool: the front end emits %d feature channels, the network takes %d"
                             % (self.frontend.width, model.input_size))
        self.model, self.localize, self.localize_batch_dim = model, localize, int(localize_batch_dim)
        self.nslots, self.np = self.frontend.nslots, self.frontend.nrows
        # as OnlineLocalizer: a zero-frame call runs forward_stream's checks of the module (eval mode, online, fp32) and
        # stops at its shape check
        try:
            model.forward_stream(torch.zeros((1, self.frontend.width, ops.NF, 0)))
        except RuntimeError as e:
            if "expected [nb" not in str(e):
                raise
        self.in_place = True             # False: every call of the network goes through gather and scatter (tests)
        self.gathers = self.scatters = 0
        self._pool = self._compact = None

    def open(self) -> int:
        return self.frontend.open()

    def close(self, slot: int):
        self.frontend.close(slot)

    def reset(self):
        self.frontend.reset()

    # ---- the state ---------------------------------------------------------
    def _blocks(self):
        m = self.model
        return (m.block_1, m.block_2, m.block_3) if self.kind == "pair" else (m.block_1, m.block_2)

    def _new_state(self, device):
        """``forward_stream``'s dict for ``nslots`` streams, all zero (what its own ``state=None`` branch builds, with the
        h tensors of FN-SSL present)."""
        rows, nf = self.nslots * self.np, ops.NF
        blocks = self._blocks()
        state = {"ws": [ops.lstm_state_workspace(rows * nf, b.narr_hidden_size, device) for b in blocks],
                 "shape": (rows, nf), "frames": 0}
        if self.kind == "pair":
            state["h"] = [torch.zeros((rows, nf, b.narr_hidden_size), device=device) for b in blocks]
        else:
            hid = self.model.conv.cnn_hidden_dim
            state["n_tail"] = [torch.zeros((rows, nf, 2, b.narr_hidden_size), device=device) for b in blocks]
            state["x_tail"] = torch.zeros((rows, 2, nf, self.model.input_size), device=device)
            state["p_tail"] = [torch.zeros((rows, nf, 2, hid), device=device) for _ in range(2)]
        return state

    @staticmethod
    def _get(state, key, idx):
        return state[key] if idx is None else state[key][idx]

    def _call_state(self, store, rows):
        """The dict of one ``forward_stream`` call on the first ``rows`` batch rows of ``store`` (views: a call on fewer
        rows uses the front of every tensor, and of every workspace — its check only asks for enough bytes), carried."""
        state = {"ws": store["ws"], "shape": (rows, ops.NF), "frames": ops.SEG_FRAMES}
        for key, idx in self._TENSORS[self.kind]:
            t = self._get(store, key, idx)[:rows]
            if idx is None:
                state[key] = t
            else:
                state.setdefault(key, [None] * len(store[key]))[idx] = t
        return state

    def _segments(self, pool, compact):
        """The ctypes segment table of ``fnssl_state_rows``: per block the slot's cell records in the workspace, then the
        carried tensors.  Rebuilt from ``data_ptr()`` per call: ``forward_stream`` replaces the tensors it returns."""
        lib = _lib.load()
        segs = []
        for k, b in enumerate(self._blocks()):
            cell = lib.fnssl_lstm_cell_group_floats(b.narr_hidden_size)
            if cell == 0:
                raise RuntimeError("fnssl.stream: no streaming LSTM kernel for hidden size %d" % b.narr_hidden_size)
            segs.append((pool["ws"][k], compact["ws"][k], self.np * (ops.NF // 16) * cell))
        for key, idx in self._TENSORS[self.kind]:
            p, c = self._get(pool, key, idx), self._get(compact, key, idx)
            segs.append((p, c, self.np * p[0].numel()))
        table = (_lib.StateSeg * len(segs))()
        for j, (p, c, row) in enumerate(segs):
            if not (p.is_contiguous() and c.is_contiguous() and p.dtype == c.dtype == torch.float32):
                raise RuntimeError("fnssl.stream: segment %d of the carried state is not a dense float32 tensor" % j)
            table[j] = _lib.StateSeg(p.data_ptr(), c.data_ptr(), row)
        return table

    def _rows(self, pool, compact, slots, direction, fresh=None):
        n = len(slots)
        table = self._segments(pool, compact)
        check(_lib.load().fnssl_state_rows(
            table, len(table), self.nslots, n, (C.c_int * n)(*slots),
            None if fresh is None else (C.c_ubyte * n)(*[int(f) for f in fresh]), direction, ops._stream()), "state_rows")
        if direction == _lib.SN_ROWS_GATHER:
            self.gathers += 1
        else:
            self.scatters += 1

    def _adopt(self, store, returned):
        """``forward_stream`` replaced the carried tensors of the call's dict: the ones of a full-size call become the store's."""
        for key, idx in self._TENSORS[self.kind]:
            if idx is None:
                store[key] = returned[key]
            else:
                store[key][idx] = returned[key][idx]

    def _network(self, x, groups):
        """The network on a round's rows ``x [n * np, 12, 256, C]``.  In place on the pool's state when the rows are all
        slots in order and all carried; else on the compact state: gather (zeros for fresh rows), forward, scatter."""
        if self._pool is None:
            self._pool = self._new_state(x.device)
        slots = [g.slot for g in groups]
        fresh = [g.fresh for g in groups]
        xv = x.permute(0, 3, 2, 1)                                        # a view: nothing is moved
        if self.in_place and slots == list(range(self.nslots)) and not any(fresh):
            pred, state = self.model.forward_stream(xv, self._call_state(self._pool, x.shape[0]))
            self._adopt(self._pool, state)
            return pred
        if self._compact is None:        # as large as the pool's state: holds the compact state of any number of rows
            self._compact = self._new_state(x.device)
        self._rows(self._pool, self._compact, slots, _lib.SN_ROWS_GATHER, fresh)
        pred, state = self.model.forward_stream(xv, self._call_state(self._compact, x.shape[0]))
        # the scatter reads the tensors the call returned; the compact store keeps its own full-size ones
        self._rows(self._pool, state, slots, _lib.SN_ROWS_SCATTER)
        return pred

    def _narrow(self, out, a, n):
        """Row a of n of what ``localize`` returned."""
        if isinstance(out, dict):
            return {k: self._narrow(v, a, n) for k, v in out.items()}
        if isinstance(out, (tuple, list)):
            return tuple(self._narrow(v, a, n) for v in out)
        if not isinstance(out, torch.Tensor):
            return out
        per = out.shape[self.localize_batch_dim] // n
        return out.narrow(self.localize_batch_dim, a * per, per)

    @torch.no_grad()
    def push(self, chunks: dict):
        out = {}
        for groups, x in self.frontend.push(chunks):
            with torch.cuda.device(x.device):
                pred = self._network(x, groups)
                doa = self.localize(pred) if self.localize is not None else None
            for a, g in enumerate(groups):
                preds, doas = out.setdefault(g.slot, ([], []))
                preds.append(pred[a * self.np:(a + 1) * self.np])
                if doa is not None:
                    doas.append(self._narrow(doa, a, len(groups)))
        return {slot: (torch.cat(preds, dim=1), doas if self.localize is not None else None)
                for slot, (preds, doas) in out.items()}
