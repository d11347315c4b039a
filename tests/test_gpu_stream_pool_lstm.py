"""GPU tests of the hop-256 stream pool (csrc/frontend_stream.hip: fnssl_stream_frontend_pool; csrc/state_rows.hip:
fnssl_state_rows; fnssl/stream.py: HopPoolFrontEnd, LstmStreamPool; ``open_stream_pool`` of the FN-SSL and IPDnet drop-ins):
independent FN-SSL / IPDnet streams that start and advance on their own give, each of them, the bits the single-stream
path gives on its own signal — features ``torch.equal`` to ``ops.pair_features`` / ``ops.array_features`` of the whole
signal, predictions ``torch.equal`` to ``forward_stream`` replayed on the stream's own features in the same groups of 12
frames.  torch.equal throughout: the streamed path is held bit for bit to the whole-signal path
(tests/test_gpu_stream_frontend.py, tests/test_gpu_stream_localize.py).  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from conftest import rs_randn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GROUP = 12
MICS4 = np.array(((-0.04, 0.0, 0.0), (0.04, 0.0, 0.0), (0.0, 0.05, 0.01), (0.02, -0.03, 0.0)), dtype=np.float32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


def signal(dev, seed, ns, nch):
    return torch.from_numpy(rs_randn(seed, (ns, nch), 0.1)).to(dev)


def whole_features(sig, mode, ch_mode, sample_length):
    """The whole-signal front end on one signal [ns, nch]: [np, nt, 256, 4] (pair) or [1, nt, 256, 2 nch] (array)."""
    from fnssl import ops
    spec, magsum = ops.stft(sig[None])
    if mode == "pair":
        return ops.pair_features(spec, magsum, ch_mode, 1e-6, sample_length, 0, True)[0]
    return ops.array_features(spec, magsum, 1e-6, sample_length, 0)[0]


def frames_due(nsamples):
    from fnssl import stream
    return stream.frames_ready(nsamples) // GROUP * GROUP


class Feed:
    """One stream of a test: a signal, the sizes of its pushes (None: the stream sits this push out), the push it opens at."""

    def __init__(self, sig, sizes, first_push):
        assert sum(n or 0 for n in sizes) <= sig.shape[0]
        self.sig, self.sizes, self.first = sig, sizes, first_push
        self.slot, self.lo, self.got = None, 0, []

    def chunk_at(self, push):
        i = push - self.first
        if i < 0 or i >= len(self.sizes) or self.sizes[i] is None:
            return None
        chunk = self.sig[self.lo:self.lo + self.sizes[i]]
        self.lo += self.sizes[i]
        return chunk


def drive_one(pool, feeds, push):
    """Push ``push``: open the feeds that start here, push the chunks of all running feeds in ONE call; -> (what the push
    returned, slot -> feed for the feeds that were pushed).  The feeds keep their positions between calls."""
    chunks, feeds_of = {}, {}
    for f in feeds:
        if f.first == push:
            f.slot = pool.open()
        c = f.chunk_at(push)
        if c is not None:
            chunks[f.slot], feeds_of[f.slot] = c, f
    return pool.push(chunks), feeds_of


# ---- 1. the front end ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode, nch, ch_mode", [("pair", 2, "M"), ("pair", 4, "MM"), ("array", 4, "M"), ("array", 8, "M")],
                         ids=["pair2_M", "pair4_MM", "array4_lds", "array8_scratch"])
def test_frontend_of_independent_streams_equals_whole_signal(dev, mode, nch, ch_mode):
    """Four streams in a pool of five slots (slot 4 stays idle): two open at push 0, one at push 2, two at push 3, one of
    them in the slot of a stream closed just before.  The chunks are ragged (0, 1, 255, 3 071, 3 072 and 7 000 samples
    among them; 7 000 completes two groups, so that push takes two rounds).  sample_length = 20: the frames cross into the
    constant-coefficient range at different pushes per stream.  Before the first group the whole state (every mu, the
    scratch) is poisoned: fresh slots must not read it, and the idle slot's mu and scratch row keep their bits."""
    from fnssl import _lib, ops, stream
    SL = 20
    fe = stream.HopPoolFrontEnd(mode, nch, 5, ch_mode, sample_length=SL)
    np_ = ops.num_pairs(nch, ch_mode) if mode == "pair" else 1
    width = 4 if mode == "pair" else 2 * nch
    a1 = Feed(signal(dev, 9301, 11000, nch), [7000, 255, 3072], 0)                      # closed before push 3
    b = Feed(signal(dev, 9302, 17000, nch), [0, 1, 255, 3071, 3072, 7000, 3072], 0)
    c = Feed(signal(dev, 9303, 17000, nch), [3584, 3072, 3072, 100, 6500], 2)
    a2 = Feed(signal(dev, 9304, 14000, nch), [7000, 0, 3072, 3584], 3)                  # reopens a1's slot
    d = Feed(signal(dev, 9305, 11000, nch), [4000, 3071, 3073], 3)
    assert fe.push({fe.open(): a1.sig[:0]}) == []                                       # allocates; nothing arrives
    fe.close(0)
    state = fe._state.view(torch.float32)
    state.copy_(torch.arange(state.numel(), dtype=torch.float32, device=dev) + 1000.0)
    poison = state.clone()
    assert (fe._state.numel() > 4096) == (nch == 8)                                     # 8 channels: spectra in the scratch
    assert _lib.load().fnssl_stream_frontend_state_bytes(5, nch, _lib.STREAM_MODE[mode], _lib.CH_MODE[ch_mode], 12) == fe._state.numel()

    total_rounds = 0
    for push in range(7):
        if push == 3:
            assert a1.slot == 0
            fe.close(a1.slot)
        before = fe.launches
        rounds, feeds_of = drive_one(fe, [a1, b, c, a2, d], push)
        assert fe.launches - before == len(rounds)                                      # ONE launch per round
        total_rounds += len(rounds)
        for groups, x in rounds:
            assert tuple(x.shape) == (len(groups) * np_, GROUP, 256, width)
            for row, g in enumerate(groups):
                feeds_of[g.slot].got.append(x[row * np_:(row + 1) * np_])
        if push == 0:
            assert [len(groups) for groups, _ in rounds] == [1, 1]                      # a1's 7 000 samples: two rounds
    assert (a1.slot, b.slot, c.slot, a2.slot, d.slot) == (0, 1, 2, 0, 3) and total_rounds >= 8
    for f in (a1, b, c, a2, d):
        got = torch.cat(f.got, dim=1)
        want = whole_features(f.sig, mode, ch_mode, SL)
        assert got.shape[1] == frames_due(f.lo) >= 36 > SL
        if f is not a1:                                                                  # (a1's slot belongs to a2 by now)
            assert fe.frames(f.slot) == got.shape[1] and fe.tail_samples(f.slot) == f.lo - 256 * got.shape[1]
            assert fe.samples(f.slot) == f.lo
        assert torch.equal(got, want[:, :got.shape[1]]), "stream of slot %d" % f.slot
    nchain = np_
    mu_floats = (5 * nchain * 4 + 255) // 256 * 64                                      # mu[5][chains] rounded up to the state's alignment
    assert torch.equal(state[4 * nchain:mu_floats], poison[4 * nchain:mu_floats])       # the idle slot's mu and the padding
    assert not torch.equal(state[:4 * nchain], poison[:4 * nchain])
    if nch == 8:
        row = 12 * nch * 256 * 2                                                         # floats of a slot's scratch row
        scratch, was = state[mu_floats:].view(5, row), poison[mu_floats:].view(5, row)
        assert torch.equal(scratch[4], was[4])
        assert all(not torch.equal(scratch[s], was[s]) for s in range(4))
    # reset(): every slot is free again, and the next stream of a slot starts from zero
    fe.reset()
    e = Feed(signal(dev, 9306, 7000, nch), [7000], 0)
    e.slot = fe.open()
    assert e.slot == 0 and fe.frames(0) == 0 and fe.tail_samples(0) == 0
    rounds = fe.push({0: e.chunk_at(0)})
    got = torch.cat([x for _, x in rounds], dim=1)
    assert got.shape[1] == 24 and torch.equal(got, whole_features(e.sig, mode, ch_mode, SL)[:, :24])


# ---- 2. more descriptors than one launch carries ----------------------------------------------------------------------
def test_more_than_64_active_slots_take_two_launches(dev):
    from fnssl import stream
    sig = torch.from_numpy(rs_randn(9310, (70, 3584, 1), 0.1)).to(dev)
    fe = stream.HopPoolFrontEnd("array", 1, 70)
    rounds = fe.push({fe.open(): sig[s] for s in range(70)})
    assert len(rounds) == 1 and fe.launches == 2
    groups, x = rounds[0]
    assert [g.slot for g in groups] == list(range(70)) and tuple(x.shape) == (70, GROUP, 256, 2)
    want = stream.StreamFrontEnd("array", 1).push(sig)                                   # the single-stream entry, batch 70
    assert tuple(want.shape) == tuple(x.shape)
    for s in range(70):
        assert torch.equal(x[s], want[s]), "slot %d" % s


# ---- 3. state rows ---------------------------------------------------------------------------------------------------
ROW_FLOATS = (4, 4096, 1572864)


def seg_table(pool, compact, rows=ROW_FLOATS):
    from fnssl import _lib
    return (_lib.StateSeg * len(pool))(*[_lib.StateSeg(p.data_ptr(), c.data_ptr(), r) for p, c, r in zip(pool, compact, rows)])


@pytest.mark.parametrize("slots,fresh", [((5, 0, 3), (0, 1, 0)), ((2,), (0,)), ((4, 5, 0, 1, 3, 2), (0, 0, 0, 0, 0, 1)),
                                         ((3, 1, 5), None)], ids=["partial", "one", "all_permuted", "no_flags"])
def test_state_rows_gather_and_scatter(dev, slots, fresh):
    from fnssl import _lib
    lib, S, A = _lib.load(), 6, len(slots)
    # distinct per segment, row and float, exact in fp32 (the largest value is below 2^24)
    pool = [torch.arange(S * r, dtype=torch.float32, device=dev).view(S, r) + float(k + 1) for k, r in enumerate(ROW_FLOATS)]
    assert S * ROW_FLOATS[2] + 3 < 2 ** 24
    before = [p.clone() for p in pool]
    compact = [torch.full((S, r), -1.0, dtype=torch.float32, device=dev) for r in ROW_FLOATS]

    def rows(direction):
        return lib.fnssl_state_rows(seg_table(pool, compact), 3, S, A, (C.c_int * A)(*slots),
                                    None if fresh is None else (C.c_ubyte * A)(*fresh), direction,
                                    torch.cuda.current_stream().cuda_stream)

    assert rows(_lib.SN_ROWS_GATHER) == 0
    for cs, ps, now in zip(compact, before, pool):
        for a, s in enumerate(slots):
            if fresh is not None and fresh[a]:
                assert not cs[a].any()                                                   # exactly zero
            else:
                assert torch.equal(cs[a], ps[s])
        assert torch.equal(now, ps) and bool((cs[A:] == -1.0).all())                     # the pool is read only; rows past A untouched
    for cs in compact:
        cs[:A] = -cs[:A] - 1.0                                  # what a forward would have changed: exact, and never what was there
    assert rows(_lib.SN_ROWS_SCATTER) == 0
    for now, ps, cs, r in zip(pool, before, compact, ROW_FLOATS):
        want = ps.clone()
        for a, s in enumerate(slots):
            want[s] = cs[a]
        assert torch.equal(now, want)                                                    # listed rows updated, all else unchanged
        assert int((now != ps).sum()) == A * r


def test_state_rows_refuses_bad_arguments_before_any_launch(dev):
    from fnssl import _lib
    lib, S = _lib.load(), 4
    rows_ = (4, 64)
    pool = [torch.arange(S * r, dtype=torch.float32, device=dev).view(S, r) + 1.0 for r in rows_]
    compact = [torch.full((S, r), -1.0, dtype=torch.float32, device=dev) for r in rows_]
    keep = [t.clone() for t in pool + compact]
    Seg = _lib.StateSeg

    def call(table, nsegs, nrows, slots, direction=_lib.SN_ROWS_GATHER, nslots=S):
        return lib.fnssl_state_rows(table, nsegs, nslots, nrows, (C.c_int * len(slots))(*slots), None, direction,
                                    torch.cuda.current_stream().cuda_stream)

    good = seg_table(pool, compact, rows_)
    p0, c0, p1, c1 = pool[0].data_ptr(), compact[0].data_ptr(), pool[1].data_ptr(), compact[1].data_ptr()
    nine = (Seg * 9)(*[Seg(p0, c0, 4)] * 9)
    bad = {
        "segment 1: the tensors must be 16-byte aligned": ((Seg * 2)(Seg(p0, c0, 4), Seg(p1 + 4, c1, 60)), 2, 2, (0, 1)),
        "segment 0: the tensors must be 16-byte aligned": ((Seg * 2)(Seg(p0, c0 + 8, 4), Seg(p1, c1, 64)), 2, 2, (0, 1)),
        "segment 1 shares a tensor with segment 0": ((Seg * 2)(Seg(p0, c0, 4), Seg(p1, c0, 64)), 2, 2, (0, 1)),
        "segment 1: pool and compact tensor are the same": ((Seg * 2)(Seg(p0, c0, 4), Seg(p1, p1, 64)), 2, 2, (0, 1)),
        "segment 1: a row of 62 floats": ((Seg * 2)(Seg(p0, c0, 4), Seg(p1, c1, 62)), 2, 2, (0, 1)),
        "segment 0: a row of 0 floats": ((Seg * 2)(Seg(p0, c0, 0), Seg(p1, c1, 64)), 2, 2, (0, 1)),
        "segment 1: a row of 4294967296 floats": ((Seg * 2)(Seg(p0, c0, 4), Seg(p1, c1, 1 << 32)), 2, 2, (0, 1)),
        "segment 1: null pointer": ((Seg * 2)(Seg(p0, c0, 4), Seg(p1, None, 64)), 2, 2, (0, 1)),
        "9 segments": (nine, 9, 2, (0, 1)),
        "0 segments": (good, 0, 2, (0, 1)),
        "row 1: slot 2 appears twice": (good, 2, 2, (2, 2)),
        "row 1: slot 4 of 4": (good, 2, 2, (0, 4)),
        "row 0: slot -1 of 4": (good, 2, 2, (-1, 1)),
        "5 rows of 4 slots": (good, 2, 5, (0, 1, 2, 3, 0)),
        "0 rows of 4 slots": (good, 2, 0, (0,)),
    }
    for message, (table, nsegs, nrows, slots) in bad.items():
        for direction in (_lib.SN_ROWS_GATHER, _lib.SN_ROWS_SCATTER):
            assert call(table, nsegs, nrows, slots, direction) == -1, message            # FNSSL_E_INVALID
            assert message in lib.fnssl_last_error().decode(), lib.fnssl_last_error().decode()
    assert call(good, 2, 2, (0, 1), direction=2) == -1 and "direction 2" in lib.fnssl_last_error().decode()
    torch.cuda.synchronize()
    assert all(torch.equal(t, k) for t, k in zip(pool + compact, keep))                  # nothing was launched
    assert call(good, 2, 2, (3, 1)) == 0                                                 # the same table, valid
    assert all(torch.equal(c[0], p[3]) and torch.equal(c[1], p[1]) for p, c in zip(pool, compact))


# ---- 4. the pool against a replay of each stream ----------------------------------------------------------------------
_models = {}


def fnssl_module(dev):
    """The FN-SSL Lightning drop-in around ``FN_SSL()`` as the reference builds it; two microphones give one pair."""
    if "fnssl" not in _models:
        import predict_step as ps
        from fnssl import weights as W
        model = ps.MyModel(device="cuda:0")
        model.arch.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in W.make_fnssl_state(9100).items()})
        _models["fnssl"] = model.to(dev).eval()
    return _models["fnssl"]


def ipdnet_module(dev, wide=False):
    """The IPDnet drop-in around ``IPDnet()`` as the reference builds it (2 microphones, hidden 128) or, ``wide``, around the
    4-microphone hidden-256 net of tests/test_gpu_stream_localize.py."""
    key = "ipdnet_wide" if wide else "ipdnet"
    if key not in _models:
        from IPDnet.FixedAarryIPDnet import IPDnet
        from IPDnet.train_step import MyModel
        from fnssl import weights as W
        args = (8, 256, 2, True) if wide else (4, 128, 2, True)
        net = IPDnet(*args)
        net.load_state_dict({k: torch.from_numpy(np.array(v, dtype=np.float32)) for k, v in W.make_ipdnet_state(9200, *args).items()})
        mics = MICS4 if wide else MICS4[:2]
        _models[key] = MyModel(arch=net, mic_pos=torch.from_numpy(mics), device="cuda:0").to(dev).eval()
    return _models[key]


def model_of(dev, name):
    """-> (arch, front-end mode, microphones, ch_mode, sample_length)"""
    if name == "fnssl":
        m = fnssl_module(dev)
        return m.arch, "pair", 2, "M", 298
    return ipdnet_module(dev).arch, "array", 2, "M", 280


def replay(arch, sig, mode, ch_mode, sample_length):
    """``forward_stream`` on the stream's own whole-signal features, in groups of exactly 12 frames -> [np, groups, ...]."""
    feats = whole_features(sig, mode, ch_mode, sample_length).permute(0, 3, 2, 1)        # [np, C, 256, nt]
    st, outs = None, []
    for t0 in range(0, feats.shape[3] // GROUP * GROUP, GROUP):
        o, st = arch.forward_stream(feats[..., t0:t0 + GROUP], st)
        outs.append(o)
    return torch.cat(outs, dim=1)


class ForwardCounter:
    """Counts the ``forward_stream`` calls of ``arch`` while active: (batch rows, frames) of each."""

    def __init__(self, arch):
        self.arch, self.calls = arch, []

    def __enter__(self):
        orig = self.arch.forward_stream

        def counting(x, state=None):
            self.calls.append((x.shape[0], x.shape[3]))
            return orig(x, state)

        self.arch.forward_stream = counting                                              # an instance attribute over the method
        return self

    def __exit__(self, *exc):
        del self.arch.forward_stream


def narrow_family(arch, rows, dev):
    """The kernel family ``forward_stream`` of ``arch`` takes for its narrow-band layers on ``rows`` batch rows of one
    12-frame group under carry: the plan of the call it makes for each block (nothing is launched)."""
    from fnssl import ops
    fams = []
    blocks = [b for b in (arch.block_1, arch.block_2, getattr(arch, "block_3", None)) if b is not None]
    concat = hasattr(arch, "conv")                                                       # IPDnet: every narrow layer reads cat(f, x)
    for blk in blocks:
        H, C2 = blk.narr_hidden_size, 2 * blk.full_hidden_size
        narr_w = blk._streams(dev)[1]
        ws = ops.lstm_state_workspace(rows * 256, H, dev)
        if concat:                                                                       # the tensors as IPDnet.forward_stream lays them out
            f = torch.empty((rows, GROUP, 256, C2), device=dev)
            x2 = torch.empty((rows, GROUP + 2, 256, arch.input_size), device=dev)[:, 2:]
            out = torch.empty((rows, 256, GROUP + 2, H), device=dev)[:, :, 2:].permute(0, 2, 1, 3)
        else:                                                                            # ... and as FN_SSL.forward_stream does
            out = torch.empty((rows, 256, GROUP + 1, H), device=dev)[:, :, 1:].permute(0, 2, 1, 3)
            if blk.is_first:
                f, x2 = torch.empty((rows, GROUP, 256, C2), device=dev), torch.empty((rows, GROUP, 256, arch.input_size), device=dev)
            else:
                f, x2 = torch.empty((rows, 256, GROUP, C2), device=dev).permute(0, 2, 1, 3), None
        fams.append(ops.lstm_plan("narrow", f, None, x2, narr_w, H, out, carry_workspace=ws, carry=True)[0])
    return fams


# the narrow-band family per layer, for every count of batch rows a pool of up to 32 two-microphone slots can reach (1 = one
# stream alone): the planner's answers on an MI355X, see test_pool_equals_per_stream_replay
FAMILIES = {"fnssl": ["f32_cluster"] * 3, "ipdnet": ["split"] * 2}


@pytest.mark.parametrize("name", ["fnssl", "ipdnet"])
def test_pool_equals_per_stream_replay(dev, name):
    """Four slots, three pushes.  Push 0: slots 0, 1, 2 start (fresh rows only); slot 2 is closed afterwards.  Push 1: slot
    1 sits out, slot 2 is reopened with another signal and two groups — round 0 is a carried row (slot 0) and a fresh one
    (slot 2, over the state its first stream left) in ONE call, round 1 slot 2 alone.  Push 2: slot 3 starts, so the full
    in-order set holds three carried rows and a fresh one; slot 0 completes two groups.  Every call goes through gather
    and scatter here (a partial set, or a fresh row among carried ones); test_full_in_order_set_runs_in_place has the
    other path.

    The family of the narrow-band LSTM calls is planned (``ops.lstm_plan``, nothing launched) for the batch rows a pool
    reaches: a pool's call has 256 x rows sequences where one stream's has 256.  On an MI355X the planner answers the same
    family from 1 row to 32 — f32_cluster for every layer of FN-SSL (H = 256), split for both of IPDnet (H = 128) — so a
    pool of at most 32 two-microphone slots cannot reach a row count whose family differs from one stream's, and there is
    no leg for another family; test_pool_of_32_slots_equals_per_stream_replay runs the largest such pool."""
    from fnssl import stream
    arch, mode, nch, ch_mode, SL = model_of(dev, name)
    pool = stream.LstmStreamPool(arch, nch, 4, ch_mode)
    a = Feed(signal(dev, 9321, 13000, nch), [3584, 3072, 6144], 0)
    b = Feed(signal(dev, 9322, 7000, nch), [3584, None, 3072], 0)
    c1 = Feed(signal(dev, 9323, 4000, nch), [3584], 0)                                   # closed after push 0
    c2 = Feed(signal(dev, 9324, 10000, nch), [6656, 3072], 1)                            # reopens c1's slot
    d = Feed(signal(dev, 9325, 4000, nch), [3584], 2)
    feeds = [a, b, c1, c2, d]
    want_calls = {0: [(3, 12)], 1: [(2, 12), (1, 12)], 2: [(4, 12), (1, 12)]}
    with torch.no_grad():
        for push in range(3):
            if push == 1:
                pool.close(c1.slot)
            before = pool.frontend.launches
            with ForwardCounter(arch) as fc:
                res, feeds_of = drive_one(pool, feeds, push)
            assert fc.calls == want_calls[push], (push, fc.calls)                        # ONE network call per round
            assert pool.frontend.launches - before == len(fc.calls)                      # and one front-end launch
            for s, (pred, doa) in res.items():
                assert doa is None and pred.shape[0] == pool.np and pred.dtype == torch.float32
                feeds_of[s].got.append(pred)
        assert (a.slot, b.slot, c1.slot, c2.slot, d.slot) == (0, 1, 2, 2, 3)
        assert pool.gathers == 5 and pool.scatters == 5 and pool.gathers > 0
        for f in feeds:
            got = torch.cat(f.got, dim=1)
            want = replay(arch, f.sig[:f.lo], mode, ch_mode, SL)
            assert got.shape[1] == frames_due(f.lo) // GROUP >= 1
            assert torch.equal(got, want[:, :got.shape[1]]), "stream of slot %d" % f.slot
        fams = {rows: narrow_family(arch, rows, dev) for rows in (1, 2, 3, 4, 8, 16, 31, 32)}
        print("narrow-band families of %s per batch rows: %s" % (name, fams))
        assert all(f == FAMILIES[name] for f in fams.values()), fams


@pytest.mark.parametrize("name", ["fnssl", "ipdnet"])
def test_pool_of_32_slots_equals_per_stream_replay(dev, name):
    """The largest row count the family assertion of test_pool_equals_per_stream_replay covers: 32 two-microphone slots
    (8 192 sequences per narrow-band call, 32 cell blocks per gather), two pushes (fresh rows through gather / scatter,
    then the full carried set in place); every fourth slot is held to its replay."""
    from fnssl import stream
    arch, mode, nch, ch_mode, SL = model_of(dev, name)
    pool = stream.LstmStreamPool(arch, nch, 32, ch_mode)
    sigs = torch.from_numpy(rs_randn(9326, (32, 3584 + 3072, nch), 0.1)).to(dev)
    with torch.no_grad():
        slots = [pool.open() for _ in range(32)]
        first = pool.push({s: sigs[s, :3584] for s in slots})
        second = pool.push({s: sigs[s, 3584:] for s in slots})
        assert (pool.gathers, pool.scatters) == (1, 1) and sorted(second) == slots
        for s in range(0, 32, 4):
            got = torch.cat((first[s][0], second[s][0]), dim=1)
            assert torch.equal(got, replay(arch, sigs[s], mode, ch_mode, SL)), "slot %d" % s


@pytest.mark.parametrize("name", ["fnssl", "ipdnet"])
def test_first_group_finding(dev, name):
    """One group through ``forward_stream(x, None)`` against the same rows with a zeroed state under carry — prediction,
    carried tensors and cell records: the same bits.  carry = 1 differs from carry = 0 only in the W_hh h_{-1} product and
    the c_{-1} load of step 0, which add +-0 with zeros.  That is why fresh rows ride in the carried rows' call
    (DESIGN 3.3c)."""
    from fnssl import _lib, stream
    arch, mode, nch, ch_mode, SL = model_of(dev, name)
    x = whole_features(signal(dev, 9330, 3584, nch), mode, ch_mode, SL).permute(0, 3, 2, 1)[..., :GROUP]
    pool = stream.LstmStreamPool(arch, nch, 1, ch_mode)
    with torch.no_grad():
        cold, s0 = arch.forward_stream(x, None)
        warm, s1 = arch.forward_stream(x, pool._call_state(pool._new_state(dev), x.shape[0]))
    same = torch.equal(cold, warm)
    for key, idx in pool._TENSORS[pool.kind]:
        same = same and torch.equal(pool._get(s0, key, idx), pool._get(s1, key, idx))
    for k, blk in enumerate(pool._blocks()):
        n = x.shape[0] * 16 * _lib.load().fnssl_lstm_cell_group_floats(blk.narr_hidden_size)
        same = same and torch.equal(s0["ws"][k][:n], s1["ws"][k][:n])
    print("first group, %s: zero state under carry %s the bits of state=None (max |diff| of the prediction %.3g)"
          % (name, "gives" if same else "does NOT give", float((cold - warm).abs().max())))
    assert same


# ---- 5. the in-place path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fnssl", "ipdnet"])
def test_full_in_order_set_runs_in_place(dev, name):
    from fnssl import stream
    arch, mode, nch, ch_mode, SL = model_of(dev, name)
    sigs = [signal(dev, 9340 + s, 3584 + 3 * 3072, nch) for s in range(3)]

    def run(in_place):
        pool = stream.LstmStreamPool(arch, nch, 3, ch_mode)
        pool.in_place = in_place
        slots = [pool.open() for _ in range(3)]
        outs, counts = [], []
        for lo, hi in ((0, 3584), (3584, 6656), (6656, 9728), (9728, 12800)):
            res = pool.push({s: sigs[s][lo:hi] for s in slots})
            assert sorted(res) == slots
            outs.append(torch.stack([res[s][0] for s in slots]))
            counts.append((pool.gathers, pool.scatters))
        return torch.cat(outs, dim=2), counts

    with torch.no_grad():
        got, counts = run(True)
        assert counts == [(1, 1)] * 4                                                    # the fresh set, then carried in order: in place
        forced, counts2 = run(False)
        assert counts2 == [(1, 1), (2, 2), (3, 3), (4, 4)]
        assert got.shape[:3] == (3, 1, 4) and torch.equal(got, forced)
        for s in range(3):
            assert torch.equal(got[s], replay(arch, sigs[s], mode, ch_mode, SL))


# ---- 6. DOA ----------------------------------------------------------------------------------------------------------
def same_tree(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_tree(x, y) for x, y in zip(a, b))
    return torch.equal(a, b)


@pytest.mark.parametrize("name", ["fnssl", "ipdnet"])
def test_doa_of_every_slot_equals_localize_on_its_replay(dev, name):
    """``localize`` = each model's documented prediction -> DOA entry: ``get_metric.predgt2DOA(...)[0]``
    for FN-SSL (a dict), ``get_metric._localize`` for IPDnet ((DOA, VAD), here on the 4-microphone net)."""
    from fnssl import stream
    if name == "fnssl":
        model, mode, nch, ch_mode, SL = fnssl_module(dev), "pair", 2, "M", 298
        entry = lambda p: model.get_metric.predgt2DOA(pred_batch=p)[0]                  # noqa: E731
    else:
        model, mode, nch, ch_mode, SL = ipdnet_module(dev, wide=True), "array", 4, "M", 280
        entry = model.get_metric._localize
    pool = model.open_stream_pool(nch, 3, localize=True)
    assert isinstance(pool, stream.LstmStreamPool)
    feeds = [Feed(signal(dev, 9351, 10000, nch), [3584, 3072, 3072], 0), Feed(signal(dev, 9352, 10000, nch), [6656, None, 3072], 1),
             Feed(signal(dev, 9353, 4000, nch), [3584], 2)]
    with torch.no_grad():
        for push in range(4):
            res, feeds_of = drive_one(pool, feeds, push)
            for s, (pred, doa) in res.items():
                assert len(doa) == pred.shape[1]
                feeds_of[s].got.extend((pred[:, k:k + 1], doa[k]) for k in range(pred.shape[1]))
        for f in feeds:
            want = replay(model.arch, f.sig[:f.lo], mode, ch_mode, SL)
            assert len(f.got) == frames_due(f.lo) // GROUP >= 1
            for k, (pred, doa) in enumerate(f.got):
                assert torch.equal(pred, want[:, k:k + 1])
                assert same_tree(doa, entry(want[:, k:k + 1])), "slot %d group %d" % (f.slot, k)
        if name == "ipdnet":
            assert tuple(feeds[0].got[0][1][0].shape) == (1, 1, 2, 2) and tuple(feeds[0].got[0][1][1].shape) == (1, 1, 2)
        else:
            assert tuple(feeds[0].got[0][1]["doa"].shape) == (1, 1, 2, 1)


# ---- 7. validation at the ABI ---------------------------------------------------------------------------------------
def test_invalid_descriptors_are_refused_before_any_launch(dev):
    from fnssl import _lib, stream
    lib, S, nch, ns = _lib.load(), 4, 2, 3584
    sig = torch.from_numpy(rs_randn(9360, (S, ns, nch), 0.1)).to(dev)
    nbytes = lib.fnssl_stream_frontend_state_bytes(S, nch, 1, 0, 12)
    state = (torch.arange(nbytes // 4, dtype=torch.float32, device=dev) + 7.0)
    x = torch.full((2, GROUP, 256, 2 * nch), -3.0, dtype=torch.float32, device=dev)
    state0, x0 = state.clone(), x.clone()
    ca, cb = stream._stream_coefs(280, True, dev)

    def call(*descs, state_bytes=nbytes, mode=1, out_frames=GROUP):
        arr = (_lib.StreamPoolDesc * len(descs))(*[_lib.StreamPoolDesc(**d) for d in descs])
        return lib.fnssl_stream_frontend_pool(
            sig.data_ptr(), S, nch, nch, 1, mode, 0, arr, len(descs), ca.data_ptr(), cb.data_ptr(), 280, 1e-6, state.data_ptr(),
            state_bytes, x.data_ptr(), 2, out_frames, torch.cuda.current_stream().cuda_stream)

    def desc(slot, out_row, **kw):
        d = dict(slot=slot, frame0=0, nframes=GROUP, out_row=out_row, fresh=1, ns=ns, sample0=0, total=-1,
                 sig_offset=slot * ns * nch)
        d.update(kw)
        return d

    bad = {
        "12 frames need 3328 samples, the window has 3327": (desc(0, 0), desc(1, 1, ns=3327)),     # a window too short
        "slot 4 of 4": (desc(0, 0), desc(4, 1)),
        "slot -1 of 4": (desc(0, 0), desc(-1, 1)),
        "slot 1 appears twice": (desc(1, 0), desc(1, 1)),
        "output row 0 appears twice": (desc(0, 0), desc(1, 0)),
        "output row 2 of 2": (desc(0, 0), desc(1, 2)),
        "13 frames in rows of 12": (desc(0, 0), desc(1, 1, nframes=13)),
        "0 frames in rows of 12": (desc(0, 0), desc(1, 1, nframes=0)),
        "the window starts at sample 255, frame 1 starts at 256": (desc(0, 0), desc(1, 1, frame0=1, sample0=255)),
        "the window starts at sample 0, frame 12 starts at 3072": (desc(0, 0), desc(1, 1, frame0=12)),
        "total length 0": (desc(0, 0), desc(1, 1, total=0)),
        "total length 5000": (desc(0, 0), desc(1, 1, total=5000)),
    }
    for message, descs in bad.items():
        assert call(*descs) == -1, message                                               # FNSSL_E_INVALID
        err = lib.fnssl_last_error().decode()
        assert message in err and "descriptor 1" in err, err
    assert call(desc(0, 0), desc(1, 1), state_bytes=nbytes - 1) == -1                    # a state that is too small
    assert "state of %d bytes, fnssl_stream_frontend_state_bytes asks for %d" % (nbytes - 1, nbytes) in lib.fnssl_last_error().decode()
    assert call(desc(0, 0), desc(1, 1), mode=2) == -1 and "mode 2" in lib.fnssl_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(state, state0) and torch.equal(x, x0)                             # nothing was launched
    assert call(desc(0, 0), desc(1, 1)) == 0                                             # the same call, valid
    want = stream.StreamFrontEnd("array", nch).push(sig[:2])
    assert torch.equal(x, want)
    assert torch.equal(state[2:], state0[2:]) and not torch.equal(state[:2], state0[:2])  # mu of slots 0 and 1 only


# ---- 8. the drop-ins ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fnssl", "ipdnet"])
def test_open_stream_pool_drop_in(dev, name):
    from fnssl import stream
    model = fnssl_module(dev) if name == "fnssl" else ipdnet_module(dev)
    arch, mode, nch, ch_mode, SL = model_of(dev, name)
    sig = signal(dev, 9370, 3584, nch)
    with torch.no_grad():
        want = replay(arch, sig, mode, ch_mode, SL)
        pool = model.open_stream_pool(nch, 2)
        assert isinstance(pool, stream.LstmStreamPool) and pool.model is model.arch and pool.frontend.sample_length == SL
        s = pool.open()
        assert pool.push({s: sig[:3000]}) == {}                                          # no group yet
        (pred, doa), = pool.push({s: sig[3000:]}).values()
        assert doa is None and torch.equal(pred, want)
        pool = model.open_stream_pool(nch, 2, localize=True)
        (pred, doa), = pool.push({pool.open(): sig}).values()
        assert torch.equal(pred, want) and len(doa) == 1
    # the single-stream drop-in gives the same prediction
    single, _ = model.predict_stream(sig.t()[None])
    assert torch.equal(single if name == "fnssl" else single[None], want if name == "fnssl" else want[0][None])


def test_train_mode_and_bf16_are_refused(dev):
    """``forward_stream``'s own errors, at construction."""
    import predict_step as ps
    from IPDnet.FixedAarryIPDnet import IPDnet
    from IPDnet.train_step import MyModel
    with pytest.raises(RuntimeError, match=r"call \.eval\(\) first"):
        ps.MyModel(device="cuda:0").to(dev).train().open_stream_pool(2, 2)
    bf = ps.MyModel(device="cuda:0")
    bf.arch = bf.arch.bfloat16()
    with pytest.raises(RuntimeError, match="fp32 model only"):
        bf.to(dev).eval().open_stream_pool(2, 2)
    mics = torch.from_numpy(MICS4[:2])
    with pytest.raises(RuntimeError, match=r"call \.eval\(\) first"):
        MyModel(arch=IPDnet(), mic_pos=mics, device="cuda:0").to(dev).train().open_stream_pool(2, 2)
    with pytest.raises(RuntimeError, match="online fp32 model only"):
        MyModel(arch=IPDnet().bfloat16(), mic_pos=mics, device="cuda:0").to(dev).eval().open_stream_pool(2, 2)
    with pytest.raises(RuntimeError, match="online fp32 model only"):
        MyModel(arch=IPDnet(4, 128, 2, False), mic_pos=mics, device="cuda:0").to(dev).eval().open_stream_pool(2, 2)
