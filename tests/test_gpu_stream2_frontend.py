"""GPU tests of IPDnet2's streamed front end (csrc/frontend_stream.hip: fnssl_stream_frontend_centred; fnssl/stream.py:
CentredStreamFrontEnd): whatever the push schedule, the features of the pushes and of ``finish()``, concatenated, are the
BITS of the whole-signal path (``ops.preprocess_ipdnet2(sig, frame_major=True)``) cut to the whole groups — torch.equal,
no tolerance: both run the arithmetic of csrc/frontend_core.h on the same folded samples, and the whole-signal path is
held to the reference's golden vectors by tests/test_gpu_ipdnet2.py.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from conftest import rs_randn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NB = 2
BASE = 320 * 22                                           # + r: 23 frames whatever the residue


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


_whole = {}


def whole_signal(dev, nch, ns, seed):
    """(signal [NB, ns, nch] on the device, whole-signal features [NB, nt, 256, 2 nch]); computed once per case and left
    unchanged."""
    from fnssl import ops
    key = (nch, ns, seed)
    if key not in _whole:
        sig = torch.from_numpy(rs_randn(seed, (NB, ns, nch), 0.1)).to(dev)
        x = ops.preprocess_ipdnet2(sig, frame_major=True).permute(0, 3, 2, 1)
        assert tuple(x.shape) == (NB, ns // 320 + 1, 256, 2 * nch) and x.is_contiguous()
        _whole[key] = (sig, x)
    return _whole[key]


def schedule(ns):
    """Push sizes that sum to ns: an empty push, 256 samples (one short of frame 0), the 1 sample that completes frame 0,
    an empty push, 319, a push that completes several groups of 5, another empty one, 64 that complete nothing, one more
    group, the rest."""
    sizes = [0, 256, 1, 0, 319, 4000, 0, 64, 1600]
    return sizes + [ns - sum(sizes)]


def stream_through(fe, sig, sizes, finish=True):
    """Push sig [nb, ns, nch] in pieces, then finish; returns (features concatenated over frames, frames emitted per
    push, frames emitted by finish)."""
    outs, emitted, lo = [], [], 0
    for n in sizes:
        x = fe.push(sig[:, lo:lo + n])
        lo += n
        emitted.append(x.shape[1])
        outs.append(x)
    assert lo == sig.shape[1]
    if not finish:
        return torch.cat(outs, dim=1), emitted, None
    outs.append(fe.finish())
    return torch.cat(outs, dim=1), emitted, outs[-1].shape[1]


def assert_same(got, want):
    assert tuple(got.shape) == tuple(want.shape)
    diff = (got != want)
    assert torch.equal(got, want), "%d of %d values differ, first frame %d" % (
        int(diff.sum()), diff.numel(), int(diff.any(dim=3).any(dim=2).any(dim=0).nonzero()[0]))


@pytest.mark.parametrize("r", [0, 1, 255, 256, 319])
@pytest.mark.parametrize("nch", [1, 2, 5, 8])
def test_streamed_equals_whole_signal(dev, nch, r):
    """NB = 2, every channel count, total lengths 320 * 22 + r: r = 0 is the retention edge (the last frame's end
    reflection reaches one sample before its own first sample), 255 the last residue whose last frame is reflected, 256
    the first whose last frame is not.  Groups of 5 (of 23 frames the last three are dropped: finish completes none) and
    groups of 1 (finish completes the reflected frame).  5 channels keep a tile's spectra in LDS, 8 stage them in the
    state's scratch."""
    from fnssl import _lib, stream
    ns = BASE + r
    sig, want = whole_signal(dev, nch, ns, 7100 + nch)
    sizes = schedule(ns)
    fe5 = stream.CentredStreamFrontEnd(nch)
    got5, e5, fin5 = stream_through(fe5, sig, sizes)
    assert e5 == [0, 0, 0, 0, 0, 10, 0, 0, 5, 5] and fin5 == 0 and fe5.frames == 20 and fe5.finished
    assert_same(got5, want[:, :20])
    fe1 = stream.CentredStreamFrontEnd(nch, segment_frames=1)
    got1, e1, fin1 = stream_through(fe1, sig, sizes)
    reflected = r <= 255
    assert e1[:9] == [0, 0, 1, 0, 1, 12, 0, 0, 5]                              # 256 samples: nothing; the 257th: frame 0
    assert fin1 == (1 if reflected else 0) and sum(e1) + fin1 == 23 == fe1.frames
    assert_same(got1, want)
    sb = _lib.load().fnssl_stream_frontend_centred_state_bytes
    assert (sb(NB, nch, max(e5)) > 4096) == (nch == 8) == (sb(NB, nch, max(e1)) > 4096)      # which path the widest push ran


@pytest.mark.parametrize("nch", [5, 8])
def test_finish_completes_the_group_with_the_reflected_frame(dev, nch):
    """25 frames, residue 3: frames 20..23 are complete when the last sample arrives, frame 24 reflects at the end, and
    finish emits the five together."""
    from fnssl import stream
    ns = 320 * 24 + 3
    sig, want = whole_signal(dev, nch, ns, 7200 + nch)
    fe = stream.CentredStreamFrontEnd(nch)
    got, emitted, fin = stream_through(fe, sig, schedule(ns))
    assert emitted == [0, 0, 0, 0, 0, 10, 0, 0, 5, 5] and fin == 5 and fe.frames == 25 and fe.tail_samples == 0
    assert_same(got, want)
    fe.reset()                                                                 # one push, one finish: other tiles, same bits
    got, emitted, fin = stream_through(fe, sig, [ns])
    assert emitted == [20] and fin == 5
    assert_same(got, want)


def test_segment_sizes_and_normalisation_off(dev):
    """segment_frames = 10 equals segment_frames = 1 on the frames both emit, at 5 channels (LDS) and 8 (scratch: a
    10-frame tile); normalise = False gives the transform itself (zero recursion, eps = 1: a division by one)."""
    from fnssl import ops, stream
    ns = BASE + 1
    for nch in (5, 8):
        sig, want = whole_signal(dev, nch, ns, 7100 + nch)
        ten, e10, fin10 = stream_through(stream.CentredStreamFrontEnd(nch, segment_frames=10), sig, schedule(ns))
        assert e10 == [0, 0, 0, 0, 0, 10, 0, 0, 0, 10] and fin10 == 0
        assert_same(ten, want[:, :20])
    sig, want = whole_signal(dev, 5, ns, 7105)
    spec, _ = ops.stft(sig, 320, True)                                         # [NB, 5, 23, 257, 2]
    plain = torch.cat((spec[..., 1:, 0].permute(0, 2, 3, 1), spec[..., 1:, 1].permute(0, 2, 3, 1)), dim=3)
    off, _, fin = stream_through(stream.CentredStreamFrontEnd(5, normalise=False, segment_frames=1), sig, schedule(ns))
    assert fin == 1
    assert_same(off, plain)
    assert not torch.equal(off, want)


def test_strided_chunks_are_read_in_place(dev):
    """A [nb, nch, n] recording pushed as its permuted view equals the contiguous push."""
    from fnssl import stream
    ns = BASE + 255
    for nch in (5, 8):
        sig, want = whole_signal(dev, nch, ns, 7100 + nch)
        planar = sig.permute(0, 2, 1).contiguous()                            # [nb, nch, ns]
        view = planar.permute(0, 2, 1)
        assert view.stride(1) == 1 and not view.is_contiguous()
        got, _, fin = stream_through(stream.CentredStreamFrontEnd(nch, segment_frames=1), view, [3333, 10, ns - 3343])
        assert fin == 1
        assert_same(got, want)


def test_long_stream_crosses_the_recursion_tile_with_a_bounded_tail(dev):
    """1030 frames: the whole-signal recursion continues from its carried mu after 1024 frames, the streamed one does so
    at every push.  The tail and the sample buffer follow the pushes, not the length of the stream."""
    from fnssl import stream
    ns = 320 * 1029 + 5
    sig, want = whole_signal(dev, 2, ns, 7300)
    fe = stream.CentredStreamFrontEnd(2)
    rng = np.random.RandomState(7301)
    lo, outs, worst_tail, worst_buf, largest = 0, [], 0, 0, 0
    while lo < ns:
        n = min(int(rng.choice([1600, 1600, 1, 4000, 7000, int(rng.randint(0, 1600))])), ns - lo)
        outs.append(fe.push(sig[:, lo:lo + n]))
        lo += n
        largest = max(largest, n)
        worst_tail, worst_buf = max(worst_tail, fe.tail_samples), max(worst_buf, fe.buffer_samples)
    assert fe.frames == 1025 and fe.samples == ns
    outs.append(fe.finish())
    assert outs[-1].shape[1] == 5 and fe.frames == 1030
    assert worst_tail < stream.centred_tail_bound(5) == 320 * 4 + 513
    assert worst_buf <= 2 * (stream.centred_tail_bound(5) + largest)
    assert_same(torch.cat(outs, dim=1), want)


def test_independent_states_reset_and_finish(dev):
    """Two front ends pushed alternately with different signals give what each gives alone; reset() replays identically;
    a push after finish raises until reset(); a changed batch or channel count raises."""
    from fnssl import stream
    ns = BASE
    sig_a, want_a = whole_signal(dev, 5, ns, 7105)
    sig_b, want_b = whole_signal(dev, 5, ns, 7400)
    fa, fb = stream.CentredStreamFrontEnd(5, segment_frames=1), stream.CentredStreamFrontEnd(5, segment_frames=1)
    sizes = [2000, 1600, 100, 3000, ns - 6700]
    outs_a, outs_b, lo = [], [], 0
    for n in sizes:
        outs_a.append(fa.push(sig_a[:, lo:lo + n]))
        outs_b.append(fb.push(sig_b[:, lo:lo + n]))
        lo += n
    with pytest.raises(RuntimeError, match="opened with 2 utterances"):
        fa.push(sig_a[:1, :100])
    with pytest.raises(RuntimeError, match="expected a chunk"):
        fa.push(sig_a[:, :100, :3])
    outs_a.append(fa.finish())
    outs_b.append(fb.finish())
    got_a, got_b = torch.cat(outs_a, dim=1), torch.cat(outs_b, dim=1)
    assert_same(got_a, want_a)
    assert_same(got_b, want_b)
    assert not torch.equal(got_a, got_b)
    with pytest.raises(RuntimeError, match="has been finished"):
        fa.push(sig_a[:, :100])
    with pytest.raises(RuntimeError, match="has been finished"):
        fa.finish()
    fa.reset()
    assert fa.frames == 0 and fa.tail_samples == 0 and fa.samples == 0 and not fa.finished
    again, _, _ = stream_through(fa, sig_a, sizes)
    assert_same(again, want_a)
    fa.reset()
    one = fa.push(sig_a[:1, :1600])                                            # after reset() another batch size is a new stream
    assert tuple(one.shape) == (1, 5, 256, 10) and torch.equal(one, want_a[:1, :5])


def test_a_stream_too_short_to_reflect_is_refused_at_finish(dev):
    """256 samples in all: the whole-signal transform refuses the signal (reflect padding needs more than 256 samples), and
    so does finish; the front end can be reset and used again."""
    from fnssl import ops, stream
    sig, want = whole_signal(dev, 2, BASE, 7102)
    fe = stream.CentredStreamFrontEnd(2)
    assert fe.push(sig[:, :200]).shape[1] == 0 and fe.push(sig[:, 200:256]).shape[1] == 0
    with pytest.raises(RuntimeError, match="too short for reflect padding"):
        ops.preprocess_ipdnet2(sig[:, :256], frame_major=True)
    with pytest.raises(RuntimeError, match="signal of 256 samples is too short for reflect padding"):
        fe.finish()
    fe.reset()
    got, _, _ = stream_through(fe, sig, [BASE])
    assert_same(got, want[:, :20])
