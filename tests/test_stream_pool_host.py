"""Host-side tests of the stream pool (fnssl/stream.py: pool_plan_push, pool_pack_descriptors, PoolFrontEnd / StreamPool
bookkeeping): pure arithmetic, no device.  The round planner is held to a brute force that knows only the definition of the
centred hop-320 transform — frame t >= 1 is complete once sample 320 t + 255 has arrived, frame 0 once sample 256 has, a
signal of ``total`` samples has total // 320 + 1 frames, the tail starts one sample before the next frame to emit — and
that emits ONE group at a time."""
import ctypes as C
import random

import pytest

torch = pytest.importorskip("torch")

from fnssl import _lib, stream  # noqa: E402

GROUP = 5
SIZES = [0, 1, 255, 256, 257, 319, 320, 1599, 1600, 1601, 3300]


class BruteStream:
    """One stream, from the definitions: samples arrive, groups leave one at a time."""

    def __init__(self):
        self.arrived, self.frames = 0, 0

    def _frame_complete(self, t):
        return self.arrived >= (257 if t == 0 else 320 * t + 256)

    def _tail_start(self):
        return max(0, 320 * self.frames - 256 - 1)

    def push(self, n, last):
        """-> [(frame0, sample0, ns, total, fresh)] in emission order."""
        self.arrived += n
        out = []
        while self._frame_complete(self.frames + GROUP - 1):
            out.append((self.frames, self._tail_start(), self.arrived - self._tail_start(), -1, self.frames == 0))
            self.frames += GROUP
        if last:
            total = self.arrived
            while self.frames + GROUP - 1 <= total // 320:                # the frames of the signal: 0 .. total // 320
                out.append((self.frames, self._tail_start(), total - self._tail_start(), total, self.frames == 0))
                self.frames += GROUP
        return out

    @property
    def tail(self):
        return self.arrived - self._tail_start()


def run_schedule(seed, ends):
    """6 slots, staggered opens, random chunk sizes, each stream ending at one of ``ends`` samples (the last chunk is cut to
    land there), slots closed after their end and reopened; planner vs brute force at every push."""
    rng = random.Random(seed)
    nslots = 6
    streams, brute, target, opened_at = {}, {}, {}, {}
    free = list(range(nslots))
    fresh_seen = {}
    reopened = 0
    for push in range(60):
        if free and (push % 2 == 0 or not streams):                       # staggered opens, the lowest free slot first
            s = min(free)
            free.remove(s)
            streams[s], brute[s], target[s] = (0, 0), BruteStream(), rng.choice(ends)
            fresh_seen[s] = 0
            reopened += s in opened_at
            opened_at[s] = push
        active = [s for s in streams if rng.random() < 0.8]
        new, last = {}, []
        for s in active:
            n = min(rng.choice(SIZES), target[s] - brute[s].arrived)
            new[s] = n
            if brute[s].arrived + n == target[s]:
                last.append(s)
        rounds, after = stream.pool_plan_push(dict(streams), new, last, GROUP)
        want = {s: brute[s].push(new[s], s in last) for s in active}
        depth = max([len(w) for w in want.values()], default=0)
        assert len(rounds) == depth
        for r, groups in enumerate(rounds):
            assert all(isinstance(g, stream.PoolGroup) for g in groups)
            assert [g.slot for g in groups] == sorted(s for s in active if len(want[s]) > r)     # the active set, in slot order
            for g in groups:
                assert (g.frame0, g.sample0, g.ns, g.total, g.fresh) == want[g.slot][r]
                fresh_seen[g.slot] += g.fresh
                assert g.fresh == (g.frame0 == 0)
        for s in active:
            frames, keep = after[s]
            assert frames == brute[s].frames
            assert keep == (0 if s in last else brute[s].tail)
            assert keep < stream.centred_tail_bound(GROUP)
        assert set(after) == set(active)
        for s in active:
            streams[s] = after[s]
        for s in last:                                                     # ended: close, the slot is free again
            assert fresh_seen[s] == (1 if brute[s].frames else 0)
            del streams[s], brute[s]
            free.append(s)
    assert reopened >= 2


@pytest.mark.parametrize("seed", range(6))
def test_round_planner_equals_brute_force(seed):
    t = 7 + seed
    ends = [320 * t, 320 * t - 1, 320 * t + 1, 320 * t + 255, 320 * t + 256, 320 * (t + 9) + 3]
    run_schedule(8200 + seed, ends)


def test_catch_up_push_takes_one_round_per_group():
    rounds, after = stream.pool_plan_push({0: (0, 0), 1: (0, 0), 2: (5, 100)}, {0: 3300, 1: 1600, 2: 1601}, last=(1,))
    assert [[g.slot for g in r] for r in rounds] == [[0, 1], [0]]
    assert rounds[1][0] == stream.PoolGroup(0, 5, 1343, 1957, -1, False)
    assert after == {0: (10, 3300 - stream.centred_tail_start(10)), 1: (5, 0), 2: (5, 1701)}
    # a slot that is pushed nothing and ends: only what the known end completes
    rounds, after = stream.pool_plan_push({3: (20, 7683 - stream.centred_tail_start(20))}, {}, last=(3,))
    assert [(g.frame0, g.total, g.fresh) for r in rounds for g in r] == [(20, 7683, False)] and after == {3: (25, 0)}


def test_descriptor_packing():
    groups = [stream.PoolGroup(slot=i, frame0=5 * i, sample0=stream.centred_tail_start(5 * i), ns=1700 + i,
                               total=-1 if i % 3 else 10 ** 10 + i, fresh=i == 0) for i in range(65)]
    descs, launches = stream.pool_pack_descriptors(groups, GROUP, lambda g: 10 ** 10 + 7 * g.slot)
    assert launches == [64, 1] and len(descs) == 65 and _lib.STREAM_POOL_MAX_DESC == 64
    d = descs[64]
    assert (d.slot, d.frame0, d.nframes, d.out_row, d.fresh, d.ns) == (64, 320, 5, 64, 0, 1764)
    assert (d.sample0, d.total, d.sig_offset) == (320 * 320 - 257, -1, 10 ** 10 + 7 * 64)
    assert descs[0].fresh == 1 and descs[0].total == 10 ** 10 and [descs[i].out_row for i in range(65)] == list(range(65))
    # the layout of fnssl_stream_pool_desc (include/fnssl.h): six ints, then three 64-bit fields, 48 bytes
    D = _lib.StreamPoolDesc
    assert C.sizeof(D) == 48 and C.sizeof(D) * _lib.STREAM_POOL_MAX_DESC < 4096
    assert [(n, getattr(D, n).offset) for n, _ in D._fields_] == [
        ("slot", 0), ("frame0", 4), ("nframes", 8), ("out_row", 12), ("fresh", 16), ("ns", 20), ("sample0", 24), ("total", 32),
        ("sig_offset", 40)]
    raw = bytes(descs)[64 * 48:]
    assert int.from_bytes(raw[0:4], "little") == 64 and int.from_bytes(raw[40:48], "little") == 10 ** 10 + 7 * 64


def small_net():
    from IPDnet2.IPDnet2 import OnlineSpatialNet
    return OnlineSpatialNet(dim_input=10, dim_output=16, num_layers=1, dim_hidden=96, num_heads=4, kernel_size=(5, 3),
                            conv_groups=(8, 8), norms=["LN", "LN", "GN", "LN", "LN", "LN"], dim_squeeze=8, num_freqs=256,
                            attention='mamba(16,4)', rope=False, time_compression_layer=0, fre_compression_ratio=16,
                            time_compression_ratio=5).eval()


def test_pool_errors():
    pool = stream.StreamPool(small_net(), nch=5, slots=2)
    a, b = pool.open(), pool.open()
    assert (a, b) == (0, 1)
    with pytest.raises(RuntimeError, match="all 2 slots"):                # a full pool
        pool.open()
    with pytest.raises(KeyError, match="not open"):                       # an unknown slot
        pool.push({2: torch.zeros((10, 5))})
    pool.close(a)
    with pytest.raises(KeyError, match="not open"):                       # a closed slot
        pool.push({a: torch.zeros((10, 5))})
    with pytest.raises(KeyError, match="not open"):
        pool.close(a)
    assert pool.open() == a                                               # the freed slot is the next one opened
    with pytest.raises(RuntimeError, match=r"expected a chunk \[n, 5\]"):    # a wrong channel count
        pool.push({b: torch.zeros((10, 4))})
    with pytest.raises(RuntimeError, match="too short for reflect padding of 256"):     # a finish with total <= 256
        pool.finish(b)
    assert not pool.frontend.finished(b)                                  # the refused finish left the stream open
    with pytest.raises(RuntimeError, match="too short for reflect padding"):
        stream.pool_plan_push({0: (0, 100)}, {0: 156}, last=(0,))
    assert stream.pool_plan_push({0: (0, 100)}, {0: 157}, last=(0,)) == ([], {0: (0, 0)})     # 257 samples: one frame, no group
    # a push after finish: the planner only knows open, unfinished streams, and the pool says which it is
    with pytest.raises(KeyError, match="not an open, unfinished stream"):
        stream.pool_plan_push({0: (0, 0)}, {1: 10})
    # No device here, so no stream can really finish: the flag is set by hand to what a finish leaves behind.  The real
    # sequence (push ... last, then a refused push) is in tests/test_gpu_stream_pool.py::test_pool_equals_per_stream_replay.
    pool.frontend._slots[b].finished = True
    with pytest.raises(RuntimeError, match="has been finished"):
        pool.push({b: torch.zeros((10, 5))})
    pool.reset()
    assert pool.open() == 0
    with pytest.raises(ValueError, match="front end emits 8 feature channels, the network takes 10"):
        stream.StreamPool(small_net(), nch=4, slots=2)
    with pytest.raises(RuntimeError, match=r"call \.eval\(\) first"):
        stream.StreamPool(small_net().train(), nch=5, slots=2)
