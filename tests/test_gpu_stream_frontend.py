"""GPU tests of the streamed front end (csrc/frontend_stream.hip, fnssl/stream.py): whatever the push schedule, the
concatenated features are the BITS of the whole-signal path (ops.stft + ops.pair_features / ops.array_features, layout
0) on the frames emitted — torch.equal, no tolerance: both run the arithmetic of csrc/frontend_core.h, and the
whole-signal path is held to float64 and to the reference's golden vectors by tests/test_gpu_frontend.py and
tests/test_gpu_parity.py.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from conftest import rs_randn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NB = 2
PAIR_FRAMES, ARRAY_FRAMES, LONG_FRAMES = 312, 300, 1044      # cross t = 298 / 280 (coefficient form), 1024 (recursion tile)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


def samples_of(nframes):
    return 512 + 256 * (nframes - 1)


_whole = {}


def whole_signal(dev, mode, nch, ch_mode, nframes, seed, normalise=True):
    """(signal [NB, ns, nch] on the device, whole-signal features layout 0); computed once per case and left unchanged."""
    from fnssl import ops
    key = (mode, nch, ch_mode, nframes, seed, normalise)
    if key not in _whole:
        sig = torch.from_numpy(rs_randn(seed, (NB, samples_of(nframes), nch), 0.1)).to(dev)
        spec, magsum = ops.stft(sig)
        if mode == "pair":
            x, _ = ops.pair_features(spec, magsum, ch_mode, 1e-6, 298, 0, normalise)
        else:
            x, _ = ops.array_features(spec, magsum, 1e-6, 280, 0)
        assert x.shape[1] == nframes
        _whole[key] = (sig, x)
    return _whole[key]


def ragged_schedule(ns, seed):
    """Push sizes that sum to ns: a first push too short for a frame, a 100-sample push that completes nothing, a push
    that completes several segments, an empty push, then seeded pushes around one segment (3072 samples)."""
    rng = np.random.RandomState(seed)
    sizes = [300, 100, 10000, 0, 3072, 3072, 100]
    while sum(sizes) < ns:
        sizes.append(int(rng.choice([3072, 3072, int(rng.randint(2800, 3400)), int(rng.randint(1, 700)), 6500])))
    sizes[-1] -= sum(sizes) - ns
    return sizes


def stream_through(fe, sig, sizes):
    """Push sig [nb, ns, nch] in pieces; returns (features concatenated over frames, frames emitted per push)."""
    outs, emitted, lo = [], [], 0
    for n in sizes:
        x = fe.push(sig[:, lo:lo + n])
        lo += n
        emitted.append(x.shape[1])
        outs.append(x)
    assert lo == sig.shape[1]
    return torch.cat(outs, dim=1), emitted


CASES = [("pair", 4, "MM", PAIR_FRAMES), ("pair", 4, "M", PAIR_FRAMES), ("pair", 2, "MM", PAIR_FRAMES),
         ("array", 4, "M", ARRAY_FRAMES), ("array", 8, "M", ARRAY_FRAMES)]


@pytest.mark.parametrize("mode, nch, ch_mode, nframes", CASES, ids=["MM4", "M4", "MM2", "array4", "array8"])
def test_streamed_equals_whole_signal(dev, mode, nch, ch_mode, nframes):
    """Every mode, NB = 2, a ragged seeded schedule; 4 channels keep the tile's spectra in LDS, 8 stage them in the
    state's scratch."""
    from fnssl import _lib, ops, stream
    sig, want = whole_signal(dev, mode, nch, ch_mode, nframes, 5100 + nch)
    fe = stream.StreamFrontEnd(mode, nch, ch_mode)
    sizes = ragged_schedule(sig.shape[1], 5200 + nch)
    got, emitted = stream_through(fe, sig, sizes)
    # the schedule is what the test says it is
    assert sizes[0] < 512 and emitted[0] == 0                                  # too short for one frame
    assert sizes[1] == 100 and emitted[1] == 0 and sizes[6] == 100 and emitted[6] == 0
    assert emitted[2] >= 36 and sizes[3] == 0 and emitted[3] == 0              # several segments at once; an empty push
    assert emitted.count(12) >= 5 and all(e % 12 == 0 for e in emitted)
    assert fe.frames == sum(emitted) == nframes == ops.num_frames(sig.shape[1])
    rows = NB * (ops.num_pairs(nch, ch_mode) if mode == "pair" else 1)
    assert tuple(got.shape) == (rows, nframes, 256, 4 if mode == "pair" else 2 * nch) == tuple(want.shape)
    scratch = _lib.load().fnssl_stream_frontend_state_bytes(NB, nch, _lib.STREAM_MODE[mode], _lib.CH_MODE[ch_mode], 12) > 4096
    assert scratch == (nch == 8)
    diff = (got != want)
    assert torch.equal(got, want), "%d of %d values differ, first frame %d" % (
        int(diff.sum()), diff.numel(), int(diff.any(dim=3).any(dim=2).any(dim=0).nonzero()[0]))


@pytest.mark.parametrize("mode, nch", [("pair", 2), ("array", 4)])
def test_long_stream_crosses_the_recursion_tile_with_a_bounded_tail(dev, mode, nch):
    """1044 frames: the whole-signal recursion continues from its carried mu after 1024 frames, the streamed one does so
    at every push.  The tail and the sample buffer follow the pushes, not the length of the stream."""
    from fnssl import stream
    sig, want = whole_signal(dev, mode, nch, "MM", LONG_FRAMES, 5300 + nch)
    fe = stream.StreamFrontEnd(mode, nch)
    rng = np.random.RandomState(5301)
    lo, outs, worst_tail, worst_buf, largest = 0, [], 0, 0, 0
    while lo < sig.shape[1]:
        n = min(int(rng.choice([3072, 3072, 1, 4000, 7000, int(rng.randint(0, 3072))])), sig.shape[1] - lo)
        outs.append(fe.push(sig[:, lo:lo + n]))
        lo += n
        largest = max(largest, n)
        worst_tail, worst_buf = max(worst_tail, fe.tail_samples), max(worst_buf, fe.buffer_samples)
    assert fe.frames == LONG_FRAMES
    assert worst_tail < stream.tail_bound(12) == 256 * 12 + 512
    assert worst_buf <= 2 * (stream.tail_bound(12) + largest)
    assert torch.equal(torch.cat(outs, dim=1), want)


def test_segment_of_one_frame_and_normalisation_off(dev):
    """segment_frames = 1 (ragged tiles: 14 frames = 12 + 2, single frames) equals segment_frames = 12 on the frames both
    have emitted; normalise = False equals the whole-signal normalise = False (zero recursion, eps = 1)."""
    from fnssl import stream
    sig, want = whole_signal(dev, "pair", 4, "MM", 60, 5400)
    sizes = [700, 3500, 256, 256, 1, 3000, 100, 4000]
    sizes.append(sig.shape[1] - 100 - sum(sizes))                             # leave the last 100 samples out
    one, e1 = stream_through(stream.StreamFrontEnd("pair", 4, segment_frames=1), sig[:, :-100], sizes)
    twelve, e12 = stream_through(stream.StreamFrontEnd("pair", 4, segment_frames=12), sig[:, :-100], sizes)
    assert one.shape[1] == 59 and twelve.shape[1] == 48 and 14 in e1 and 1 in e1 and sorted(set(e12)) == [0, 12]
    assert torch.equal(one[:, :48], twelve) and torch.equal(one, want[:, :59])
    sig8, want8 = whole_signal(dev, "array", 8, "M", 60, 5401)
    one8, _ = stream_through(stream.StreamFrontEnd("array", 8, segment_frames=1), sig8[:, :-100], sizes)
    assert torch.equal(one8, want8[:, :59])                                   # short tiles of 8 channels fit the LDS
    _, plain = whole_signal(dev, "pair", 4, "MM", 60, 5400, normalise=False)
    off, _ = stream_through(stream.StreamFrontEnd("pair", 4, normalise=False), sig, [5000, 3072, sig.shape[1] - 8072])
    assert off.shape[1] == 60 and torch.equal(off, plain)
    assert not torch.equal(off, want)


def test_strided_chunks_are_read_in_place(dev):
    """A [nb, nch, n] recording pushed as its permuted view equals the contiguous push."""
    from fnssl import stream
    for mode, nch in (("pair", 4), ("array", 8)):
        sig, want = whole_signal(dev, mode, nch, "MM" if mode == "pair" else "M", 60, 5400 if mode == "pair" else 5401)
        planar = sig.permute(0, 2, 1).contiguous()                           # [nb, nch, ns]
        view = planar.permute(0, 2, 1)
        assert view.stride(1) == 1 and not view.is_contiguous()
        got, _ = stream_through(stream.StreamFrontEnd(mode, nch), view, [3333, 5000, view.shape[1] - 8333])
        assert got.shape[1] == 60 and torch.equal(got, want)


def test_independent_states_and_reset(dev):
    """Two front ends pushed alternately with different signals give what each gives alone; reset() replays identically;
    a changed batch or channel count raises."""
    from fnssl import stream
    sig_a, want_a = whole_signal(dev, "pair", 4, "MM", 60, 5400)
    sig_b, want_b = whole_signal(dev, "pair", 4, "MM", 60, 5500)
    fa, fb = stream.StreamFrontEnd("pair", 4), stream.StreamFrontEnd("pair", 4)
    sizes = [4000, 3072, 100, 5000, sig_a.shape[1] - 12172]
    outs_a, outs_b, lo = [], [], 0
    for n in sizes:
        outs_a.append(fa.push(sig_a[:, lo:lo + n]))
        outs_b.append(fb.push(sig_b[:, lo:lo + n]))
        lo += n
    got_a, got_b = torch.cat(outs_a, dim=1), torch.cat(outs_b, dim=1)
    assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b) and not torch.equal(got_a, got_b)
    with pytest.raises(RuntimeError, match="opened with 2 utterances"):
        fa.push(sig_a[:1, :100])
    with pytest.raises(RuntimeError, match="expected a chunk"):
        fa.push(sig_a[:, :100, :3])
    fa.reset()
    assert fa.frames == 0 and fa.tail_samples == 0
    again, _ = stream_through(fa, sig_a, sizes)
    assert torch.equal(again, want_a)
    fa.reset()
    one = fa.push(sig_a[:1, :3328])                                           # after reset() another batch size is a new stream
    assert tuple(one.shape) == (6, 12, 256, 4) and torch.equal(one, want_a[:6, :12])
