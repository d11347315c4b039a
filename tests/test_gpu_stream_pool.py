"""GPU tests of the stream pool (csrc/frontend_stream.hip: fnssl_stream_frontend_centred_pool; csrc/spatialnet.hip:
fnssl_sn_state_rows; fnssl/stream.py: PoolFrontEnd, StreamPool; ``IPDnet2.run_step.MyModel.open_stream_pool``): independent
IPDnet2 streams that start, advance and end on their own give, each of them, the bits the single-stream path gives on its
own signal — features ``torch.equal`` to ``ops.preprocess_ipdnet2``, predictions ``torch.equal`` to ``forward_stream``
replayed in groups of 5 frames at batch 1 (tests/test_gpu_ipdnet2.py pins batch rows to be bit-independent; equality across
different chunk cuttings is not claimed, hence groups of 5).  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from conftest import rs_randn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NS25 = 320 * 24 + 3                                      # 25 frames: the fifth group holds the end-reflected frame
MICS5 = np.array(((0.0, 0.0, 0.0), (0.04, 0.0, 0.0), (0.0, 0.04, 0.0), (-0.04, 0.0, 0.0), (0.0, -0.04, 0.0)))
GROUP = 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


def signal(dev, seed, ns, nch):
    return torch.from_numpy(rs_randn(seed, (ns, nch), 0.1)).to(dev)


def whole_features(sig, sample_length=249):
    """[nt, 256, 2 nch]: the whole-signal front end on one signal [ns, nch]."""
    from fnssl import ops
    return ops.preprocess_ipdnet2(sig[None], 1e-6, sample_length, frame_major=True).permute(0, 3, 2, 1)[0]


class Feed:
    """One stream of a test: a signal, the sizes of its pushes, the push it opens at."""

    def __init__(self, sig, sizes, first_push, finish=False):
        assert sum(sizes) <= sig.shape[0] and (not finish or sum(sizes) == sig.shape[0])
        self.sig, self.sizes, self.first, self.finish = sig, sizes, first_push, finish
        self.slot, self.lo, self.got = None, 0, []

    def chunk_at(self, push):
        """(chunk, is it the last one) or None when the stream is not being pushed."""
        i = push - self.first
        if i < 0 or i >= len(self.sizes):
            return None
        chunk = self.sig[self.lo:self.lo + self.sizes[i]]
        self.lo += self.sizes[i]
        return chunk, self.finish and i == len(self.sizes) - 1

    def frames_due(self):
        from fnssl import stream
        if self.finish:
            return (self.sig.shape[0] // 320 + 1) // GROUP * GROUP
        return stream.centred_frames_ready(self.lo) // GROUP * GROUP


def drive_one(pool, feeds, push):
    """Push ``push``: open the feeds that start here, push the chunks of all running feeds in ONE call; -> (what the push
    returned, slot -> feed for the feeds that were pushed).  The feeds keep their positions between calls."""
    chunks, last, feeds_of = {}, [], {}
    for f in feeds:
        if f.first == push:
            f.slot = pool.open()
        c = f.chunk_at(push)
        if c is not None:
            chunks[f.slot], feeds_of[f.slot] = c[0], f
            if c[1]:
                last.append(f.slot)
    return pool.push(chunks, last), feeds_of


# ---- 1. the front end ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [5, 7], ids=["5ch_lds", "7ch_scratch"])
def test_frontend_of_independent_streams_equals_whole_signal(dev, nch):
    """Four streams in a pool of five slots (slot 4 stays idle): two open at push 0, one at push 2, one at push 3; one
    ends at NS25 (its last frame reflects at the end); one is closed at push 3 and its slot reopened with another signal.
    sample_length = 7: the frames cross into the constant-coefficient range at different pushes per stream.  Before the
    first group the whole state (every mu, the scratch) is poisoned: fresh slots must not read it, and the idle slot's mu
    and scratch row keep their bits."""
    from fnssl import _lib, stream
    fe = stream.PoolFrontEnd(nch, 5, sample_length=7)
    a1 = Feed(signal(dev, 8301, 5000, nch), [1600, 1700, 300], 0)                      # closed before push 3
    b = Feed(signal(dev, 8302, NS25, nch), [256, 1, 1400, 3300, 64, NS25 - 5021], 0, finish=True)
    c = Feed(signal(dev, 8303, 9000, nch), [1599, 1601, 320, 3300], 2)
    a2 = Feed(signal(dev, 8304, 9000, nch), [3300, 0, 1600, 257], 3)                   # reopens a1's slot
    d = Feed(signal(dev, 8305, 9000, nch), [4000, 319, 1600], 3)
    assert fe.push({fe.open(): a1.sig[:0]}) == []                                       # allocates; nothing arrives
    fe.close(0)
    state = fe._state.view(torch.float32)
    state.copy_(torch.arange(state.numel(), dtype=torch.float32, device=dev) + 1000.0)
    poison = state.clone()
    assert (fe._state.numel() > 4096) == (nch == 7)                                     # 7 channels: spectra in the scratch

    emitted_per_push = []
    for push in range(7):
        if push == 3:
            assert a1.slot == 0
            fe.close(a1.slot)
        rounds, feeds_of = drive_one(fe, [a1, b, c, a2, d], push)
        emitted_per_push.append(sum(len(groups) for groups, _ in rounds))
        for groups, x in rounds:
            assert tuple(x.shape) == (len(groups), GROUP, 256, 2 * nch)
            for row, g in enumerate(groups):
                feeds_of[g.slot].got.append(x[row])
    assert (a1.slot, b.slot, c.slot, a2.slot, d.slot) == (0, 1, 2, 0, 3)
    for f in (a1, b, c, a2, d):
        got = torch.cat(f.got, dim=0)
        want = whole_features(f.sig, 7)
        assert got.shape[0] == f.frames_due() > 7
        assert torch.equal(got, want[:got.shape[0]])
    assert fe.finished(b.slot) and fe.frames(b.slot) == 25 and fe.tail_samples(b.slot) == 0
    assert sum(emitted_per_push) == sum(f.frames_due() for f in (a1, b, c, a2, d)) // GROUP
    mu_bytes = 256                                                                       # mu[5] rounded up to the state's alignment
    assert torch.equal(state[4], poison[4]) and torch.equal(state[5:mu_bytes // 4], poison[5:mu_bytes // 4])
    assert not torch.equal(state[:4], poison[:4])
    if nch == 7:
        row = 10 * nch * 256 * 2                                                         # floats of a slot's scratch row
        scratch, was = state[mu_bytes // 4:].view(5, row), poison[mu_bytes // 4:].view(5, row)
        assert torch.equal(scratch[4], was[4])
        assert all(not torch.equal(scratch[s], was[s]) for s in range(4))
    assert _lib.load().fnssl_stream_frontend_centred_state_bytes(5, nch, 10) == fe._state.numel()


# ---- 2. more descriptors than one launch carries ----------------------------------------------------------------------
def test_more_than_64_active_slots_take_two_launches(dev):
    from fnssl import stream
    sig = torch.from_numpy(rs_randn(8310, (70, 1600, 2), 0.1)).to(dev)
    fe = stream.PoolFrontEnd(2, 70)
    rounds = fe.push({fe.open(): sig[s] for s in range(70)})
    assert len(rounds) == 1 and fe.launches == 2
    groups, x = rounds[0]
    assert [g.slot for g in groups] == list(range(70)) and tuple(x.shape) == (70, GROUP, 256, 4)
    want = stream.CentredStreamFrontEnd(2).push(sig)                                     # the single-stream entry, batch 70
    assert tuple(want.shape) == tuple(x.shape)
    for s in range(70):
        assert torch.equal(x[s], want[s]), "slot %d" % s


# ---- 3. state rows ---------------------------------------------------------------------------------------------------
def net_of(dev, layers, bf16=False, seed=8100):
    from IPDnet2.IPDnet2 import OnlineSpatialNet
    from fnssl import weights as W
    key = (layers, bf16, seed)
    if key not in _nets:
        net = OnlineSpatialNet(dim_input=10, dim_output=16, num_layers=layers, dim_hidden=96, num_heads=4, kernel_size=(5, 3),
                               conv_groups=(8, 8), norms=["LN", "LN", "GN", "LN", "LN", "LN"], dim_squeeze=8, num_freqs=256,
                               attention='mamba(16,4)', rope=False, time_compression_layer=0, fre_compression_ratio=16,
                               time_compression_ratio=5)
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in W.make_ipdnet2_state(seed, num_layers=layers).items()})
        _nets[key] = (net.bfloat16() if bf16 else net).to(dev).eval()
    return _nets[key]


_nets = {}


def segments(state, n, layers):
    """The segments of a carried state of batch n as [n, row] views: encoder taps, then per Mamba block conv taps and SSM
    state (include/fnssl.h, fnssl_sn_state_rows)."""
    rows = [10 * 256 * 4] + [16 * 3 * 192, 16 * 192 * 16] * (2 * layers)
    out, at = [], 0
    for r in rows:
        out.append(state[at:at + n * r].view(n, r))
        at += n * r
    return out, at


@pytest.mark.parametrize("slots,fresh", [((5, 0, 3), (0, 1, 0)), ((2,), (0,)), ((4, 5, 0, 1, 3, 2), (0, 0, 0, 0, 0, 1)),
                                         ((0, 1, 2, 3, 4, 5), None)], ids=["partial", "one", "all_permuted", "all_in_order"])
def test_state_rows_gather_and_scatter(dev, slots, fresh):
    from fnssl import _lib
    lib, S, L, A = _lib.load(), 6, 3, len(slots)
    dn = net_of(dev, L).device_net(dev)
    total = lib.fnssl_sn_state_floats(C.byref(dn.net), S, 256)
    pool = torch.arange(total, dtype=torch.float32, device=dev) + 1.0                    # distinct per row and segment, exact
    assert total < 2 ** 24 and segments(pool, S, L)[1] == total
    assert total // S == 10240 + 6 * 58368                                               # one slot of a 3-layer net
    before = pool.clone()
    compact = torch.full((total,), -1.0, dtype=torch.float32, device=dev)

    def rows(direction):
        return lib.fnssl_sn_state_rows(C.byref(dn.net), S, 256, pool.data_ptr(), A, compact.data_ptr(), (C.c_int * A)(*slots),
                                       None if fresh is None else (C.c_ubyte * A)(*fresh), direction,
                                       torch.cuda.current_stream().cuda_stream)

    assert rows(_lib.SN_ROWS_GATHER) == 0
    csegs, used = segments(compact, A, L)
    assert used == lib.fnssl_sn_state_floats(C.byref(dn.net), A, 256)
    for cs, ps in zip(csegs, segments(before, S, L)[0]):
        for a, s in enumerate(slots):
            if fresh is not None and fresh[a]:
                assert not cs[a].any()                                                   # exactly zero
            else:
                assert torch.equal(cs[a], ps[s])
    assert torch.equal(pool, before) and bool((compact[used:] == -1.0).all())
    compact[:used] += 0.5                                                                # what a forward would have changed
    assert rows(_lib.SN_ROWS_SCATTER) == 0
    want = before.clone()
    for ws, cs in zip(segments(want, S, L)[0], csegs):
        for a, s in enumerate(slots):
            ws[s] = cs[a]
    assert torch.equal(pool, want)                                                       # listed rows updated, all else unchanged
    assert int((pool != before).sum()) == A * (total // S)


# ---- 4. the pool against a replay of each stream ----------------------------------------------------------------------
def replay(arch, sig):
    """``forward_stream`` at batch 1 on the stream's whole-signal features in groups of exactly 5 frames -> [groups, 512, 4, 2]."""
    from fnssl import ops
    feats = ops.preprocess_ipdnet2(sig[None], frame_major=True)
    st, outs = None, []
    for t0 in range(0, feats.shape[3] // GROUP * GROUP, GROUP):
        o, st = arch.forward_stream(feats[..., t0:t0 + GROUP], st)
        outs.append(o[0])
    return torch.cat(outs, dim=0)


class ForwardCounter:
    """Counts the ``fnssl_sn_forward`` calls by wrapping ``DeviceSpatialNet.forward`` while active."""

    def __enter__(self):
        from fnssl import spatialnet
        self.cls, self.orig, self.calls = spatialnet.DeviceSpatialNet, spatialnet.DeviceSpatialNet.forward, []
        counter = self

        def counting(dn, x, state=None, carry=False):
            counter.calls.append((x.shape[0], bool(carry)))
            return counter.orig(dn, x, state=state, carry=carry)

        self.cls.forward = counting
        return self

    def __exit__(self, *exc):
        self.cls.forward = self.orig


def three_feeds(dev):
    """Staggered starts, ragged chunks; push 2 completes two groups of c; push 3 is the full in-order carried set; a ends
    at NS25 in push 5 (its reflected group comes with the end)."""
    a = Feed(signal(dev, 8321, NS25, 5), [1600, 1600, 1600, 1600, 100, NS25 - 6500], 0, finish=True)
    b = Feed(signal(dev, 8322, 9000, 5), [1700, 1500, 1600, 1600, 0], 1)
    c = Feed(signal(dev, 8323, 9000, 5), [3300, 1600, 0, 1700], 2)
    return [a, b, c]


@pytest.mark.parametrize("layers,bf16", [(3, False), (8, False), (8, True)], ids=["3layers_fp32", "shipped_fp32", "shipped_bf16"])
def test_pool_equals_per_stream_replay(dev, layers, bf16):
    from fnssl import stream
    arch = net_of(dev, layers, bf16)
    pool = stream.StreamPool(arch, 5, 3)
    feeds = three_feeds(dev)
    first_done = set()
    with torch.no_grad():
        for push in range(6):
            with ForwardCounter() as fc:
                res, feeds_of = drive_one(pool, feeds, push)
            # ONE call per round, also for a round that mixes fresh and carried rows (fresh rows ride along); only a
            # round of fresh rows alone runs without carry
            ngroups = {s: p.shape[0] for s, (p, _) in res.items()}
            want_calls = []
            for r in range(max(ngroups.values(), default=0)):
                rows = [s for s, g in ngroups.items() if g > r]
                fresh = [s for s in rows if r == 0 and s not in first_done]
                want_calls.append((len(rows), len(fresh) < len(rows)))
            first_done |= set(ngroups)
            assert fc.calls == want_calls, (push, fc.calls)
            if push == 1:
                assert fc.calls == [(2, True)]                                           # b fresh beside a carried: one call
            for s, (pred, doa) in res.items():
                assert doa is None and tuple(pred.shape[1:]) == (512, 4, 2) and pred.dtype == torch.float32
                feeds_of[s].got.append(pred)
            if push == 2:
                assert ngroups == {0: 1, 1: 1, 2: 2}
            if push == 3:
                assert fc.calls == [(3, True)] and ngroups == {0: 1, 1: 1, 2: 1}
        assert pool.frontend.finished(feeds[0].slot)
        with pytest.raises(RuntimeError, match="has been finished"):
            pool.push({feeds[0].slot: feeds[0].sig[:100]})
        for f in feeds:
            got = torch.cat(f.got, dim=0)
            want = replay(arch, f.sig[:f.lo])
            assert got.shape[0] == f.frames_due() // GROUP >= 3
            assert torch.equal(got, want[:got.shape[0]]), "stream of slot %d" % f.slot


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_first_group_finding(dev, bf16):
    """A zeroed state under carry=True gives the bits of carry=False (= ``forward_stream(x, None)``), prediction and new
    state, in fp32 and in bf16: that is why fresh rows ride in the carried rows' call (DESIGN 3.3b has the reason)."""
    from fnssl import ops
    arch = net_of(dev, 8, bf16)
    dn = arch.device_net(dev)
    x = ops.preprocess_ipdnet2(signal(dev, 8330, 1600, 5)[None], frame_major=True)[..., :GROUP]
    with torch.no_grad():
        s0, s1 = dn.new_state(1), dn.new_state(1)
        cold = dn.forward(x, state=s0, carry=False)
        warm = dn.forward(x, state=s1, carry=True)
    same = torch.equal(cold, warm) and torch.equal(s0, s1)
    print("first group, %s: zero state under carry=True %s the bits of carry=False (max |diff| %.3g)"
          % ("bf16" if bf16 else "fp32", "gives" if same else "does NOT give", float((cold - warm).abs().max())))
    assert same


# ---- 5. the in-place path --------------------------------------------------------------------------------------------
def test_full_in_order_set_runs_in_place(dev):
    from fnssl import stream
    arch = net_of(dev, 3)
    sigs = [signal(dev, 8340 + s, 6400, 5) for s in range(3)]

    def run(in_place):
        pool = stream.StreamPool(arch, 5, 3)
        pool.in_place = in_place
        slots = [pool.open() for _ in range(3)]
        outs = []
        for lo in range(0, 6400, 1600):
            res = pool.push({s: sigs[s][lo:lo + 1600] for s in slots})
            assert sorted(res) == slots
            outs.append(torch.stack([res[s][0] for s in slots]))
        return torch.cat(outs, dim=1), pool

    with torch.no_grad():
        got, pool = run(True)
        assert (pool.gathers, pool.scatters) == (0, 0)                                   # fresh in order, then carried in order
        forced, pool2 = run(False)
        assert (pool2.gathers, pool2.scatters) == (3, 4)                                 # a call of fresh rows alone gathers nothing
        assert tuple(got.shape) == (3, 4, 512, 4, 2) and torch.equal(got, forced)
        for s in range(3):
            assert torch.equal(got[s], replay(arch, sigs[s]))


# ---- 6. DOA ----------------------------------------------------------------------------------------------------------
def test_doa_of_every_slot_equals_the_search_on_its_replay_and_reset(dev):
    from IPDnet2.Module import PredDOA
    from fnssl import stream
    arch = net_of(dev, 3)
    pd = PredDOA(mic_location=MICS5, dev="cuda:0")
    entry = lambda p: pd._search(p[..., :2], 1)                                          # noqa: E731
    pool = stream.StreamPool(arch, 5, 3, localize=entry)

    def one_pass():
        feeds = three_feeds(dev)
        out = {}
        for push in range(6):
            res, _ = drive_one(pool, feeds, push)
            for s, (pred, doa) in res.items():
                assert len(doa) == pred.shape[0]
                out.setdefault(s, []).extend(zip(pred, doa))
        return feeds, out

    with torch.no_grad():
        feeds, first = one_pass()
        for f in feeds:
            want = replay(arch, f.sig[:f.lo])
            assert len(first[f.slot]) == f.frames_due() // GROUP
            for k, (pred, doa) in enumerate(first[f.slot]):
                assert torch.equal(pred, want[k])
                wdoa = entry(want[k][None, None])
                assert tuple(doa[0].shape) == (2, 1, 1, 2, 1) and tuple(doa[1].shape) == (2, 1, 1, 1)
                assert len(doa) == len(wdoa) == 3 and all(torch.equal(x, y) for x, y in zip(doa, wdoa))
        pool.reset()
        _, second = one_pass()
        assert sorted(second) == sorted(first)
        for s in first:
            for (p1, d1), (p2, d2) in zip(first[s], second[s]):
                assert torch.equal(p1, p2) and all(torch.equal(x, y) for x, y in zip(d1, d2))


# ---- 7. validation at the ABI ---------------------------------------------------------------------------------------
def test_invalid_descriptors_are_refused_before_any_launch(dev):
    from fnssl import _lib, stream
    lib, S, nch, ns = _lib.load(), 4, 2, 1700
    sig = torch.from_numpy(rs_randn(8350, (S, ns, nch), 0.1)).to(dev)
    nbytes = lib.fnssl_stream_frontend_centred_state_bytes(S, nch, 10)
    state = (torch.arange(nbytes // 4, dtype=torch.float32, device=dev) + 7.0)
    x = torch.full((2, GROUP, 256, 2 * nch), -3.0, dtype=torch.float32, device=dev)
    state0, x0 = state.clone(), x.clone()
    ca, cb = stream._stream_coefs(249, True, dev)

    def call(*descs):
        arr = (_lib.StreamPoolDesc * len(descs))(*[_lib.StreamPoolDesc(**d) for d in descs])
        return lib.fnssl_stream_frontend_centred_pool(
            sig.data_ptr(), S, nch, nch, 1, arr, len(descs), ca.data_ptr(), cb.data_ptr(), 249, 1e-6, state.data_ptr(), nbytes,
            x.data_ptr(), 2, GROUP, torch.cuda.current_stream().cuda_stream)

    def desc(slot, out_row, **kw):
        d = dict(slot=slot, frame0=0, nframes=GROUP, out_row=out_row, fresh=1, ns=ns, sample0=0, total=-1,
                 sig_offset=slot * ns * nch)
        d.update(kw)
        return d

    bad = {
        "the window holds": (desc(0, 0), desc(1, 1, ns=1535)),                          # frame 4 reads up to sample 1535
        "slot 4 of 4": (desc(0, 0), desc(4, 1)),
        "slot 1 appears twice": (desc(1, 0), desc(1, 1)),
        "output row 0 appears twice": (desc(0, 0), desc(1, 0)),
        "output row 2 of 2": (desc(0, 0), desc(1, 2)),
        "total length 256 is too short": (desc(0, 0), desc(1, 1, total=256)),
        "total length 0 is too short": (desc(0, 0), desc(1, 1, total=0)),
        "does not exist in a signal of total length 1000": (desc(0, 0), desc(1, 1, total=1000)),
        "0 frames in rows of 5": (desc(0, 0), desc(1, 1, nframes=0)),
    }
    for message, descs in bad.items():
        assert call(*descs) == -1, message                                               # FNSSL_E_INVALID
        err = lib.fnssl_last_error().decode()
        assert message in err and "descriptor 1" in err, err
    torch.cuda.synchronize()
    assert torch.equal(state, state0) and torch.equal(x, x0)                             # nothing was launched
    assert call(desc(0, 0), desc(1, 1)) == 0                                             # the same call, valid
    want = stream.CentredStreamFrontEnd(nch).push(sig[:2])
    assert torch.equal(x, want)
    assert torch.equal(state[2:], state0[2:]) and not torch.equal(state[:2], state0[:2])  # mu of slots 0 and 1 only


# ---- 8. the drop-in ----------------------------------------------------------------------------------------------------
def shipped_model(dev):
    from IPDnet2.run_step import MyModel
    m = MyModel(device="cuda:0")
    m.arch = net_of(dev, 8)
    return m.to(dev).eval()


def test_open_stream_pool_drop_in(dev):
    from fnssl import stream
    model = shipped_model(dev)
    sig = signal(dev, 8360, 1600, 5)
    with torch.no_grad():
        want = replay(model.arch, sig)
        pool = model.open_stream_pool(5, 2)
        assert isinstance(pool, stream.StreamPool)
        s = pool.open()
        (pred, doa), = pool.push({s: sig}).values()
        assert doa is None and torch.equal(pred, want)
        pool = model.open_stream_pool(5, 2, localize=True, mic_location=MICS5)
        s = pool.open()
        (pred, doa), = pool.push({s: sig}).values()
        assert torch.equal(pred, want) and len(doa) == 1 and tuple(doa[0][0].shape) == (2, 1, 1, 2, 1)
    with pytest.raises(ValueError, match="mic_location"):
        model.open_stream_pool(5, 2, localize=True)


def test_train_mode_is_refused(dev):
    from IPDnet2.run_step import MyModel
    model = MyModel(device="cuda:0").to(dev).train()
    with pytest.raises(RuntimeError, match=r"call \.eval\(\) first"):
        model.open_stream_pool(5, 2)


def test_pool_follows_changed_weights(dev):
    """The pool fetches the packed network per call, as ``forward_stream`` does: weights loaded after the first push are
    the ones a stream opened afterwards runs on."""
    from fnssl import stream
    from fnssl import weights as W
    arch = net_of(dev, 3, seed=8371)                                                     # this test's own net: it is modified
    sig = signal(dev, 8370, 1600, 5)
    pool = stream.StreamPool(arch, 5, 2)
    with torch.no_grad():
        (before, _), = pool.push({pool.open(): sig}).values()
        assert torch.equal(before, replay(arch, sig))
        arch.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in W.make_ipdnet2_state(8372, num_layers=3).items()})
        (after, _), = pool.push({pool.open(): sig}).values()
        assert torch.equal(after, replay(arch, sig)) and not torch.equal(after, before)
