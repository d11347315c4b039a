"""Host-side checks of the streamed front end (no GPU): the two entry points are declared, listed and exported; every
invalid argument is refused with FNSSL_E_INVALID, i.e. before any launch; the frames-ready / tail arithmetic of
fnssl/stream.py equals a brute-force count; the coefficient table is indexed as the whole-signal table is; CPU tensors
are refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from fnssl import _lib, ops, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fnssl_stream_frontend_state_bytes", "fnssl_stream_frontend")
E_INVALID = -1
PAIR, ARRAY = 0, 1
M, MM = 0, 1


def test_stream_symbols_declared_listed_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fnssl.h")).read()
    declared = set(re.findall(r"\b(fnssl_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.fnssl_abi_version() == 19
    assert _lib.STREAM_MODE == {"pair": PAIR, "array": ARRAY}
    for name, value in (("FNSSL_STREAM_PAIR", PAIR), ("FNSSL_STREAM_ARRAY", ARRAY)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name


def test_state_bytes():
    sb = _lib.load().fnssl_stream_frontend_state_bytes
    assert sb(0, 4, PAIR, MM, 12) == 0 and sb(2, 1, PAIR, MM, 12) == 0 and sb(2, 4, PAIR, 2, 12) == 0
    assert sb(2, 4, 2, MM, 12) == 0 and sb(2, 4, PAIR, MM, 0) == 0 and sb(2, 17, ARRAY, M, 12) == 0
    assert sb(2, 1, ARRAY, M, 12) > 0                                     # one channel has no pair but is an array
    # 4 channels: the carried mu alone (a 12-frame tile of spectra is 96 KiB of LDS); 8 channels: + 192 KiB per utterance
    small, wide = sb(2, 4, ARRAY, M, 12), sb(2, 8, ARRAY, M, 12)
    assert 0 < small < 4096 and sb(2, 4, PAIR, MM, 12) >= 2 * 6 * 4
    assert wide >= 2 * 12 * 8 * 256 * 8
    assert sb(2, 8, ARRAY, M, 4000) == wide                               # stops growing at the 12-frame tile
    assert sb(2, 8, ARRAY, M, 1) <= sb(2, 8, ARRAY, M, 6) <= wide         # monotone in the frame count


def call(lib, sig=64, nb=2, ns=3328, nch=4, mode=PAIR, ch_mode=MM, frame0=0, nframes=12, ca=64, cb=64, sl=298, eps=1e-6,
         state=64, state_bytes=1 << 20, x=64):
    """fnssl_stream_frontend on never-dereferenced pointers: every call of the test must fail validation first."""
    p = lambda v: None if v is None else C.c_void_p(v)      # noqa: E731
    return lib.fnssl_stream_frontend(p(sig), nb, ns, nch, 4 * ns, 4, 1, mode, ch_mode, frame0, nframes, p(ca), p(cb), sl,
                                     eps, p(state), state_bytes, p(x), None)


@pytest.mark.parametrize("kw, word", [
    (dict(sig=None), "null"), (dict(ca=None), "null"), (dict(cb=None), "null"), (dict(state=None), "null"),
    (dict(x=None), "null"),
    (dict(nch=1), "channels"),                                            # pair mode needs two
    (dict(nch=17, mode=ARRAY), "channels"),
    (dict(mode=2), "mode"), (dict(ch_mode=2), "ch_mode"),
    (dict(nb=0), "batch"),
    (dict(nframes=0), "frame count"), (dict(nframes=-3), "frame count"),
    (dict(frame0=-1), "first frame"),
    (dict(sl=0), "sample_length"),
    (dict(ns=3327), "samples"),                                           # 12 frames need 11 * 256 + 512
    (dict(state_bytes=16), "state"),                                      # 2 x 6 pairs of mu do not fit
    (dict(nch=8, mode=ARRAY, ns=3328, state_bytes=4096), "state"),        # no room for the spectra scratch
    (dict(sig=66), "misaligned"), (dict(ca=66), "misaligned"), (dict(cb=70), "misaligned"),
    (dict(state=72), "misaligned"), (dict(x=72), "misaligned"),
])
def test_invalid_arguments_fail_before_any_launch(kw, word):
    lib = _lib.load()
    assert call(lib, **kw) == E_INVALID                                   # FNSSL_E_HIP (-2) would mean a launch was tried
    assert word in lib.fnssl_last_error().decode(), lib.fnssl_last_error()


def brute_frames(nsamples):
    """Frames t whose last sample 256 t + 511 has arrived."""
    t = 0
    while 256 * t + 511 < nsamples:
        t += 1
    return t


def test_frames_ready_against_brute_force():
    for k in range(0, 4001):
        assert stream.frames_ready(k) == brute_frames(k), k
    assert stream.frames_ready(511) == 0 and stream.frames_ready(512) == 1 and stream.frames_ready(767) == 1
    assert stream.frames_ready(768) == 2


@pytest.mark.parametrize("seg", [1, 5, 12])
def test_plan_push_against_brute_force(seg):
    """Single pushes of 0..4000 samples from every kind of tail, then random schedules: the frames emitted so far are the
    whole groups among the frames complete so far, the tail starts at the first sample of the next frame to emit, keeps
    every sample from there on and stays below the bound."""
    for tail in (0, 1, 255, 256, 511, 512, 700, 256 * seg + 511):
        for new in range(0, 4001):
            emit, keep = stream.plan_push(tail, new, seg)
            ready = brute_frames(tail + new)
            assert emit == ready // seg * seg and keep == tail + new - 256 * emit, (tail, new)
    rng = np.random.RandomState(77 + seg)
    for _ in range(40):
        total = emitted = tail = 0
        for new in rng.choice([0, 1, 100, 255, 256, 257, 511, 512, 3072, 3073, 4000, 9000], size=60):
            emit, tail = stream.plan_push(tail, int(new), seg)
            total += int(new)
            emitted += emit
            assert emitted == brute_frames(total) // seg * seg
            assert tail == total - 256 * emitted                          # nothing lost, nothing kept twice
            assert 0 <= tail < stream.tail_bound(seg)
    with pytest.raises(ValueError):
        stream.plan_push(-1, 5, 12)
    with pytest.raises(ValueError):
        stream.plan_push(0, 5, 0)


@pytest.mark.parametrize("sl", [8, 280, 298])
def test_coefficient_table_index_clamp(sl):
    """The streamed kernel reads entry min(t, sample_length) of a table of sample_length + 1 entries: that is the
    whole-signal table at every t, in particular at sample_length - 1, sample_length and beyond, where b_t changes
    from 1.0f - alp to (float)(1.0 - alpha)."""
    a, b = stream.stream_coefs_host(sl)
    assert a.shape == b.shape == (sl + 1,)
    la, lb = ops.forgetting_coefs_host(sl + 700, sl)
    for t in list(range(0, sl + 3)) + [sl + 50, sl + 699]:
        assert a[min(t, sl)] == la[t] and b[min(t, sl)] == lb[t], t
    assert np.all(la[sl:] == la[sl]) and np.all(lb[sl:] == lb[sl])       # constant from sample_length on
    assert stream.DEFAULT_SAMPLE_LENGTH == {"pair": 298, "array": 280}


def test_cpu_tensors_and_bad_settings_are_refused():
    fe = stream.StreamFrontEnd("pair", 4)
    assert (fe.sample_length, fe.segment_frames, fe.frames, fe.nrows, fe.width) == (298, 12, 0, 6, 4)
    assert stream.StreamFrontEnd("array", 4).sample_length == 280
    assert stream.StreamFrontEnd("pair", 4, "M").nrows == 3
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        fe.push(torch.zeros(2, 100, 4))
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        stream.StreamFrontEnd("array", 8).push(torch.zeros(1, 3328, 8))
    for bad in (lambda: stream.StreamFrontEnd("centre", 4), lambda: stream.StreamFrontEnd("pair", 1),
                lambda: stream.StreamFrontEnd("pair", 4, "XX"), lambda: stream.StreamFrontEnd("pair", 4, segment_frames=0)):
        with pytest.raises(ValueError):
            bad()


def test_online_localizer_rejects_modules_that_do_not_stream():
    """Offline and bf16 modules raise forward_stream's own errors when the localizer is built, and a front end whose
    groups the network cannot consume is refused."""
    import Model
    from IPDnet.FixedAarryIPDnet import IPDnet
    fe = stream.StreamFrontEnd("pair", 2)
    with pytest.raises(RuntimeError, match="only the online model"):
        stream.OnlineLocalizer(Model.FN_SSL(is_online=False).eval(), fe)
    with pytest.raises(RuntimeError, match="fp32 model only"):
        stream.OnlineLocalizer(Model.FN_SSL().bfloat16().eval(), fe)
    fa = stream.StreamFrontEnd("array", 4)
    with pytest.raises(RuntimeError, match="online fp32 model only"):
        stream.OnlineLocalizer(IPDnet(8, 256, 2, False).eval(), fa)
    with pytest.raises(RuntimeError, match="online fp32 model only"):
        stream.OnlineLocalizer(IPDnet(8, 256, 2, True).bfloat16().eval(), fa)
    with pytest.raises(ValueError, match="groups of 12"):
        stream.OnlineLocalizer(Model.FN_SSL().eval(), stream.StreamFrontEnd("pair", 2, segment_frames=1))
    with pytest.raises(ValueError, match="feature channels"):
        stream.OnlineLocalizer(IPDnet(8, 256, 2, True).eval(), stream.StreamFrontEnd("array", 2))
    loc = stream.OnlineLocalizer(Model.FN_SSL().eval(), fe)               # an online fp32 model passes
    assert loc.state is None and loc.frontend is fe
