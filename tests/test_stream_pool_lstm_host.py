"""Host-side tests of the hop-256 stream pool (fnssl/stream.py: hop_pool_plan_push, HopPoolFrontEnd / LstmStreamPool
bookkeeping): pure arithmetic, no device.  The round planner is held to a brute force that knows only the definition of the
hop-256 transform — frame t is complete once sample 256 t + 511 has arrived, the tail starts with the first sample of the
next frame to emit — and that emits ONE group at a time."""
import ctypes as C
import random

import pytest

torch = pytest.importorskip("torch")

from fnssl import _lib, stream  # noqa: E402

GROUP = 12
SIZES = [0, 1, 255, 256, 257, 511, 512, 3071, 3072, 3073, 3583, 3584, 7000, 10000]


class BruteStream:
    """One stream, from the definitions: samples arrive, groups leave one at a time."""

    def __init__(self):
        self.arrived, self.frames = 0, 0

    def push(self, n):
        """-> [(frame0, sample0, ns, total, fresh)] in emission order."""
        self.arrived += n
        out = []
        while self.arrived >= 256 * (self.frames + GROUP - 1) + 512:      # the group's last frame is complete
            out.append((self.frames, 256 * self.frames, self.arrived - 256 * self.frames, -1, self.frames == 0))
            self.frames += GROUP
        return out

    @property
    def tail(self):
        return self.arrived - 256 * self.frames


@pytest.mark.parametrize("seed", range(6))
def test_round_planner_equals_brute_force(seed):
    """6 slots, staggered opens, random chunk sizes from 0 to 10 000 samples (some drawn freely, some from the edges of a
    frame and of a group), slots closed and reopened; planner vs brute force and vs ``plan_push`` at every push."""
    rng = random.Random(9200 + seed)
    nslots = 6
    streams, brute = {}, {}
    free = list(range(nslots))
    reopened, seen, deepest = 0, set(), 0
    for push in range(80):
        if free and (push % 2 == 0 or not streams):                       # staggered opens, the lowest free slot first
            s = min(free)
            free.remove(s)
            streams[s], brute[s] = (0, 0), BruteStream()
            reopened += s in seen
            seen.add(s)
        active = [s for s in streams if rng.random() < 0.8]
        new = {s: rng.choice(SIZES) if rng.random() < 0.6 else rng.randint(0, 10000) for s in active}
        per_slot = {s: stream.plan_push(streams[s][1], new[s], GROUP) for s in active}
        rounds, after = stream.hop_pool_plan_push(dict(streams), new, GROUP)
        want = {s: brute[s].push(new[s]) for s in active}
        depth = max([len(w) for w in want.values()], default=0)
        deepest = max(deepest, depth)
        assert len(rounds) == depth
        for r, groups in enumerate(rounds):
            assert all(isinstance(g, stream.PoolGroup) for g in groups)
            assert [g.slot for g in groups] == sorted(s for s in active if len(want[s]) > r)     # ONE group per slot, in slot order
            for g in groups:
                assert (g.frame0, g.sample0, g.ns, g.total, g.fresh) == want[g.slot][r]
                assert g.ns >= (GROUP - 1) * 256 + 512                    # what fnssl_stream_frontend_pool asks of a window
        assert set(after) == set(active)
        for s in active:
            emit, keep = per_slot[s]
            assert after[s] == (streams[s][0] + emit, keep) == (brute[s].frames, brute[s].tail)
            assert keep < stream.tail_bound(GROUP)
            streams[s] = after[s]
        for s in [s for s in streams if streams[s][0] >= 5 * GROUP]:      # long enough: close, the slot is free again
            del streams[s], brute[s]
            free.append(s)
    assert reopened >= 2 and deepest >= 3


def test_catch_up_push_takes_one_round_per_group():
    rounds, after = stream.hop_pool_plan_push({0: (0, 0), 1: (0, 0), 2: (12, 100)}, {0: 7000, 1: 3584, 2: 3483})
    assert [[g.slot for g in r] for r in rounds] == [[0, 1, 2], [0]]
    assert rounds[1][0] == stream.PoolGroup(0, 12, 3072, 3928, -1, False)
    assert rounds[0][2] == stream.PoolGroup(2, 12, 3072, 3583, -1, False)
    assert after == {0: (24, 856), 1: (12, 512), 2: (24, 511)}
    assert stream.hop_pool_plan_push({0: (0, 0)}, {}) == ([], {})
    assert stream.hop_pool_plan_push({0: (0, 3327)}, {0: 0}) == ([], {0: (0, 3327)})     # one sample short of 12 frames
    assert [len(r) for r in stream.hop_pool_plan_push({0: (0, 3327)}, {0: 1})[0]] == [1]
    # an unknown slot raises before anything is planned
    with pytest.raises(KeyError, match="not an open stream"):
        stream.hop_pool_plan_push({0: (0, 0)}, {0: 4000, 1: 10})


def test_state_seg_layout():
    """fnssl_state_seg (include/fnssl.h): two pointers and a 64-bit count, 24 bytes; eight of them and the slot list of a
    launch stay below the kernel-argument segment."""
    S = _lib.StateSeg
    assert C.sizeof(S) == 24 and [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("pool", 0), ("compact", 8), ("row_floats", 16)]
    assert _lib.STATE_ROWS_MAX_SEGS == 8 and 8 * 24 + 64 * 5 + 8 < 4096
    lib = _lib.load()
    # one 16-sequence group's cell record: 16 * hidden floats, 0 where nothing streams
    assert [lib.fnssl_lstm_cell_group_floats(h) for h in (16, 32, 64, 128, 256)] == [256, 512, 1024, 2048, 4096]
    assert [lib.fnssl_lstm_cell_group_floats(h) for h in (0, -16, 48, 100, 512)] == [0] * 5
    # ... which is what the workspace grows by per group (the sizer counts the same record)
    for h in (64, 128, 256):
        grow = lib.fnssl_lstm_workspace_bytes_ex(16 * 40, h, 1, 0) - lib.fnssl_lstm_workspace_bytes_ex(16 * 39, h, 1, 0)
        per_group = 4 * lib.fnssl_lstm_cell_group_floats(h)
        # fp32 H = 256 keeps a snapshot of the cell region as well; every fp32 cluster shape adds one tag word per member
        assert grow == per_group * (2 if h == 256 else 1) + (4 * (h // 16) if h >= 128 else 0), (h, grow)


def test_frontend_errors_and_bookkeeping():
    with pytest.raises(ValueError, match="mode must be 'pair' or 'array'"):
        stream.HopPoolFrontEnd("centred", 4, 2)
    with pytest.raises(ValueError, match="ch_mode must be 'M' or 'MM'"):
        stream.HopPoolFrontEnd("pair", 4, 2, ch_mode="X")
    with pytest.raises(ValueError, match="0 slots"):
        stream.HopPoolFrontEnd("array", 4, 0)
    with pytest.raises(ValueError, match="1 channels"):
        stream.HopPoolFrontEnd("pair", 1, 2)
    with pytest.raises(ValueError, match="segment_frames 0"):
        stream.HopPoolFrontEnd("array", 4, 2, segment_frames=0)
    fe = stream.HopPoolFrontEnd("pair", 4, 3)
    assert (fe.nrows, fe.width, fe.sample_length, fe.group) == (6, 4, 298, 12)
    assert (stream.HopPoolFrontEnd("pair", 4, 3, ch_mode="M").nrows, stream.HopPoolFrontEnd("array", 4, 3).sample_length) == (3, 280)
    arr = stream.HopPoolFrontEnd("array", 8, 3)
    assert (arr.nrows, arr.width, arr.ch_mode) == (1, 16, "M")
    assert [fe.open() for _ in range(3)] == [0, 1, 2]                     # the lowest free slot first
    with pytest.raises(RuntimeError, match="all 3 slots"):
        fe.open()
    fe.close(1)
    with pytest.raises(KeyError, match="not open"):
        fe.close(1)
    with pytest.raises(KeyError, match="not open"):
        fe.frames(1)
    with pytest.raises(KeyError, match="not open"):                       # a closed slot, before the chunk is looked at
        fe.push({1: torch.zeros((10, 4))})
    assert fe.open() == 1 and (fe.frames(1), fe.tail_samples(1), fe.samples(1)) == (0, 0, 0)
    with pytest.raises(RuntimeError, match=r"expected a chunk \[n, 4\]"):
        fe.push({0: torch.zeros((10, 3))})
    with pytest.raises(RuntimeError, match="expected a ROCm device tensor"):     # there is no CPU implementation
        fe.push({0: torch.zeros((10, 4))})
    assert fe.push({}) == [] and fe.finish(0) == [] and fe.launches == 0
    fe.reset()
    with pytest.raises(KeyError, match="not open"):
        fe.frames(0)
    assert fe.open() == 0


def test_pool_errors_and_bookkeeping():
    import Model
    from IPDnet.FixedAarryIPDnet import IPDnet
    pool = stream.LstmStreamPool(Model.FN_SSL().eval(), nch=4, slots=2)
    assert (pool.kind, pool.np, pool.nslots) == ("pair", 6, 2) and (pool.gathers, pool.scatters, pool.in_place) == (0, 0, True)
    a, b = pool.open(), pool.open()
    assert (a, b) == (0, 1)
    with pytest.raises(RuntimeError, match="all 2 slots"):
        pool.open()
    with pytest.raises(KeyError, match="not open"):
        pool.push({2: torch.zeros((10, 4))})
    pool.close(a)
    with pytest.raises(KeyError, match="not open"):
        pool.push({a: torch.zeros((10, 4))})
    assert pool.open() == a                                               # the freed slot is the next one opened
    with pytest.raises(RuntimeError, match=r"expected a chunk \[n, 4\]"):
        pool.push({b: torch.zeros((10, 5))})
    assert pool.push({}) == {}
    pool.reset()
    assert pool.open() == 0
    ipool = stream.LstmStreamPool(IPDnet(8, 256, 2, True).eval(), nch=4, slots=3)
    assert (ipool.kind, ipool.np, ipool.frontend.sample_length) == ("array", 1, 280)
    # the feature width must be the network's: FN-SSL takes the 4 features of a pair, IPDnet 2 per microphone
    with pytest.raises(ValueError, match="front end emits 8 feature channels, the network takes 4"):
        stream.LstmStreamPool(IPDnet().eval(), nch=4, slots=2)
    with pytest.raises(ValueError, match="front end emits 4 feature channels, the network takes 8"):
        stream.LstmStreamPool(Model.FN_SSL(input_size=8).eval(), nch=4, slots=2)
    # forward_stream's own errors, at construction
    with pytest.raises(RuntimeError, match=r"call \.eval\(\) first"):
        stream.LstmStreamPool(Model.FN_SSL().train(), nch=2, slots=2)
    with pytest.raises(RuntimeError, match="only the online model"):
        stream.LstmStreamPool(Model.FN_SSL(is_online=False).eval(), nch=2, slots=2)
    with pytest.raises(RuntimeError, match="online fp32 model only"):
        stream.LstmStreamPool(IPDnet(8, 256, 2, False).eval(), nch=4, slots=2)
    with pytest.raises(ValueError, match="must be an FN_SSL or a fixed-array IPDnet"):
        stream.LstmStreamPool(torch.nn.Linear(2, 2), nch=2, slots=2)
