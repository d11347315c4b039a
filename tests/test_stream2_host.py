"""Host-side checks of IPDnet2's streamed front end (no GPU): the two entry points are declared, listed and exported;
every invalid argument is refused with FNSSL_E_INVALID, i.e. before any launch; the centred frame arithmetic of
fnssl/stream.py equals a brute-force count that literally folds indices as the whole-signal kernel does; CPU tensors and
bad settings are refused; OnlineLocalizer takes an OnlineSpatialNet with a 5-frame front end."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from fnssl import _lib, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fnssl_stream_frontend_centred_state_bytes", "fnssl_stream_frontend_centred")
E_INVALID = -1
SIZES = [0, 1, 63, 64, 255, 256, 257, 319, 320, 321, 1600, 4000]


def test_centred_symbols_declared_listed_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fnssl.h")).read()
    declared = set(re.findall(r"\b(fnssl_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.fnssl_abi_version() == 19 == _lib.ABI_VERSION
    assert _lib.STREAM_MODE == {"pair": 0, "array": 1}                    # no third mode: the centred entry is its own


def test_centred_state_bytes():
    sb = _lib.load().fnssl_stream_frontend_centred_state_bytes
    assert sb(0, 5, 10) == 0 and sb(2, 0, 10) == 0 and sb(2, 17, 10) == 0 and sb(2, 5, 0) == 0
    # up to 6 channels a 10-frame tile of spectra stays in LDS: the carried mu alone; from 7 on it is staged in the state
    for nch in (1, 2, 5, 6):
        assert 0 < sb(2, nch, 1 << 20) < 4096, nch
    assert sb(2, 7, 1 << 20) >= 2 * 10 * 7 * 256 * 8
    wide = sb(2, 8, 10)
    assert wide >= 2 * 10 * 8 * 256 * 8 and sb(2, 8, 4000) == wide        # stops growing at the 10-frame tile
    assert sb(2, 8, 5) < 4096                                             # one 5-frame group of 8 channels fits the LDS
    assert sb(2, 8, 1) <= sb(2, 8, 9) <= wide


def call(lib, sig=64, nb=2, ns=1536, nch=5, sample0=0, frame0=0, nframes=5, total=-1, ca=64, cb=64, sl=249, eps=1e-6,
         state=64, state_bytes=1 << 20, x=64):
    """fnssl_stream_frontend_centred on never-dereferenced pointers: every call of the test must fail validation first.
    The default is a valid request: frames 0..4 read samples 0..1535."""
    p = lambda v: None if v is None else C.c_void_p(v)      # noqa: E731
    return lib.fnssl_stream_frontend_centred(p(sig), nb, ns, nch, nch * ns, nch, 1, sample0, frame0, nframes, total, p(ca),
                                             p(cb), sl, eps, p(state), state_bytes, p(x), None)


@pytest.mark.parametrize("kw, word", [
    (dict(sig=None), "null"), (dict(ca=None), "null"), (dict(cb=None), "null"), (dict(state=None), "null"),
    (dict(x=None), "null"),
    (dict(nch=0), "channels"), (dict(nch=17), "channels"),
    (dict(nb=0), "batch"),
    (dict(nframes=0), "frame count"), (dict(nframes=-3), "frame count"),
    (dict(frame0=-1), "first frame"),
    (dict(sl=0), "sample_length"),
    (dict(ns=1535), "the window holds"),                                  # frame 4 ends at sample 1535
    (dict(nframes=1, ns=256), "the window holds"),                        # frame 0 folds index -256 to sample 256
    (dict(sample0=1), "the window holds"),                                # frame 0 reads sample 0
    (dict(ns=0), "window of"), (dict(sample0=-1), "window of"),
    (dict(frame0=5, nframes=1, sample0=1344, ns=192), "the window holds"),  # open: frame 5 reads 1344..1855
    # the retention edge: total = 320 * 5, frame 5 starts at 1344 and its end reflection reaches back to 1343
    (dict(frame0=5, nframes=1, sample0=1344, ns=256, total=1600), "reads samples 1343..1599"),
    (dict(total=256), "too short"), (dict(total=0), "too short"),
    (dict(total=1000, ns=1000), "does not exist"),                        # a signal of 1000 samples has frames 0..3
    (dict(state_bytes=0), "state"),
    (dict(nch=8, nframes=10, ns=3136, state_bytes=4096), "state"),        # no room for the spectra scratch
    (dict(sig=66), "misaligned"), (dict(ca=66), "misaligned"), (dict(cb=70), "misaligned"),
    (dict(state=72), "misaligned"), (dict(x=72), "misaligned"),
])
def test_invalid_arguments_fail_before_any_launch(kw, word):
    lib = _lib.load()
    assert call(lib, **kw) == E_INVALID                                   # FNSSL_E_HIP (-2) would mean a launch was tried
    assert word in lib.fnssl_last_error().decode(), lib.fnssl_last_error()


# ---- the brute-force side: indices folded one by one, as csrc/frontend.hip folds them ---------------------------------
@functools.lru_cache(maxsize=None)
def reads(t, ns):
    """(lowest, highest) signal index frame t reads; ns = None: the end is unknown, only the start fold applies."""
    i = np.arange(320 * t - 256, 320 * t + 256)
    i = np.where(i < 0, -i, i)
    if ns is not None:
        i = np.where(i >= ns, 2 * (ns - 1) - i, i)
    return int(i.min()), int(i.max())


def brute_ready(n):
    """Frames whose every start-folded index has arrived: they read the same samples whatever the final length."""
    t = 0
    while reads(t, None)[1] < n:
        t += 1
    return t


def test_centred_frames_ready_against_brute_force():
    for n in range(0, 4001):
        assert stream.centred_frames_ready(n) == brute_ready(n), n
    assert stream.centred_frames_ready(256) == 0 and stream.centred_frames_ready(257) == 1      # frame 0 waits for sample 256
    assert stream.centred_frames_ready(575) == 1 and stream.centred_frames_ready(576) == 2
    # a ready frame reads the same samples under every final length: no end reflection
    for n in (257, 576, 600, 1856, 3999):
        for t in range(brute_ready(n)):
            for ns in (n, n + 1, n + 255, n + 320):
                assert reads(t, ns) == reads(t, None), (n, t, ns)


def test_centred_tail_start_is_the_lowest_index_a_later_frame_can_read():
    """With f frames emitted, over every final length that has a frame f, the lowest index frames f.. read; the minimum
    is taken at ns = 320 f, one sample before frame f's own first sample."""
    for f in range(0, 13):
        lowest = min(reads(t, ns)[0] for ns in range(max(257, 320 * f), 320 * f + 700) for t in range(f, ns // 320 + 1))
        assert stream.centred_tail_start(f) == lowest, f
    assert stream.centred_tail_start(0) == 0 and stream.centred_tail_start(1) == 63 and stream.centred_tail_start(5) == 1343
    assert reads(5, 1600) == (1343, 1599) and reads(5, 1601)[0] == 1344
    # at most the last frame is end-reflected, and only for a residue of at most 255
    for ns in range(257, 4001):
        last = ns // 320
        assert all(reads(t, ns) == reads(t, None) for t in range(last)), ns
        assert (reads(last, ns) != reads(last, None)) == (ns % 320 <= 255), ns


@pytest.mark.parametrize("seg", [1, 5, 10])
def test_centred_plan_against_brute_force(seg):
    """Every total length 257..4000 over a random schedule, then finish: the frames emitted are exactly the whole groups
    among ns // 320 + 1; every index an emitted frame reads after folding lies inside the tail it is emitted from; the
    tail is the contiguous run from centred_tail_start on (nothing lost, nothing kept twice) and stays below the bound."""
    rng = np.random.RandomState(180 + seg)
    bound = stream.centred_tail_bound(seg)
    assert bound == 320 * (seg - 1) + 513
    for ns in range(257, 4001):
        arrived = frames = tail = 0
        while arrived < ns:
            new = min(int(rng.choice(SIZES)), ns - arrived)
            emit, keep = stream.centred_plan_push(tail, new, seg, frames)
            lo = arrived - tail                                           # the window the frames are emitted from
            arrived += new
            assert frames + emit == brute_ready(arrived) // seg * seg, (ns, arrived)
            for t in range(frames, frames + emit):
                assert reads(t, ns) == reads(t, None) and lo <= reads(t, ns)[0] and reads(t, ns)[1] < arrived, (ns, t)
            frames += emit
            tail = keep
            assert tail == arrived - stream.centred_tail_start(frames) and 0 <= tail < bound, (ns, arrived)
        emit, keep = stream.centred_plan_finish(ns, seg, frames)
        for t in range(frames, frames + emit):
            assert ns - tail <= reads(t, ns)[0] and reads(t, ns)[1] < ns, (ns, t)
        assert frames + emit == (ns // 320 + 1) // seg * seg and keep == 0, ns
    with pytest.raises(ValueError):
        stream.centred_plan_push(-1, 5, 5, 0)
    with pytest.raises(ValueError):
        stream.centred_plan_push(0, 5, 0, 0)
    with pytest.raises(ValueError):
        stream.centred_plan_push(0, 5, 5, 3)                              # frames are emitted in whole groups
    with pytest.raises(ValueError):
        stream.centred_plan_finish(256, 5, 0)


def test_single_pushes_from_every_kind_of_tail():
    for seg in (1, 5, 10):
        for frames in (0, seg, 2 * seg):
            start = stream.centred_tail_start(frames)
            for tail in (0, 1, 63, 64, 256, 257, 320):
                for new in range(0, 4001, 7):
                    emit, keep = stream.centred_plan_push(tail, new, seg, frames)
                    ready = max(brute_ready(start + tail + new), frames)
                    assert frames + emit == ready // seg * seg, (seg, frames, tail, new)
                    assert keep == start + tail + new - stream.centred_tail_start(frames + emit)


def test_cpu_tensors_and_bad_settings_are_refused():
    fe = stream.CentredStreamFrontEnd(5)
    assert (fe.sample_length, fe.segment_frames, fe.frames, fe.nrows, fe.width, fe.eps) == (249, 5, 0, 1, 10, 1e-6)
    assert (fe.tail_samples, fe.buffer_samples, fe.samples, fe.finished) == (0, 0, 0, False)
    assert stream.CentredStreamFrontEnd(5, normalise=False).eps == 1.0
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        fe.push(torch.zeros(2, 100, 5))
    with pytest.raises(RuntimeError, match="too short for reflect padding"):
        fe.finish()                                                       # nothing pushed: 0 samples
    assert not fe.finished
    for bad in (lambda: stream.CentredStreamFrontEnd(0), lambda: stream.CentredStreamFrontEnd(5, segment_frames=0),
                lambda: stream.CentredStreamFrontEnd(5, sample_length=0), lambda: stream.StreamFrontEnd("centre", 4)):
        with pytest.raises(ValueError):
            bad()


def spatialnet(**kw):
    from IPDnet2.IPDnet2 import OnlineSpatialNet
    cfg = dict(dim_input=10, dim_output=16, num_layers=1, dim_hidden=96, num_heads=4, kernel_size=(5, 3), conv_groups=(8, 8),
               norms=["LN", "LN", "GN", "LN", "LN", "LN"], dim_squeeze=8, num_freqs=256, attention="mamba(16,4)", rope=False,
               time_compression_layer=0, fre_compression_ratio=16, time_compression_ratio=5)
    cfg.update(kw)
    return OnlineSpatialNet(**cfg)


def test_online_localizer_accepts_online_spatialnet():
    import Model
    net = spatialnet().eval()
    fe = stream.CentredStreamFrontEnd(5)
    loc = stream.OnlineLocalizer(net, fe)
    assert loc.state is None and loc.frontend is fe
    stream.OnlineLocalizer(net, stream.CentredStreamFrontEnd(5, segment_frames=10))            # whole groups of 5
    stream.OnlineLocalizer(spatialnet().bfloat16().eval(), fe)                                # both precisions
    with pytest.raises(ValueError, match="groups of 5 frames, the front end emits groups of 12"):
        stream.OnlineLocalizer(net, stream.CentredStreamFrontEnd(5, segment_frames=12))
    with pytest.raises(ValueError, match="emits 8 feature channels, the network takes 10"):
        stream.OnlineLocalizer(net, stream.CentredStreamFrontEnd(4))
    with pytest.raises(RuntimeError, match=r"call \.eval\(\) first"):
        stream.OnlineLocalizer(spatialnet().train(), fe)
    # the LSTM models keep their group of 12, and the end of a stream completes nothing for them
    with pytest.raises(ValueError, match="groups of 12"):
        stream.OnlineLocalizer(Model.FN_SSL().eval(), stream.StreamFrontEnd("pair", 2, segment_frames=5))
    old = stream.OnlineLocalizer(Model.FN_SSL().eval(), stream.StreamFrontEnd("pair", 2))
    assert old.finish() == (None, None)
