"""CPU tests of the label stage's host side: the window count and the window times against brute force, every
refusal of fnssl.scene.segment_batch / Segmenting_SRPDNN / trajectory_doa before anything touches the device, and the
descriptors a batch of 25 scenes hands the library (device routes stubbed, as in tests/test_scene_batch_host.py)."""
import ctypes as C
import types

import numpy as np
import pytest

import labels_ref as R

torch = pytest.importorskip("torch")


# ------------------------------------------------------------------------------------------------------------------------
# N_w and tw
# ------------------------------------------------------------------------------------------------------------------------
GRID = [(L, K, step) for L in (1, 2, 7, 64, 100, 999, 1000, 1087, 6400, 72000)
        for K in (1, 2, 3, 7, 37, 64, 100, 257, 300, 1000, 3328, 72000) for step in (1, 2, 3, 7, 37, 64, 129, 350, 1000, 3072, 72000)
        if K <= L and step <= L]


def test_window_count_and_times_against_brute_force():
    from fnssl import scene
    kinds = set()
    for L, K, step in GRID:
        brute = sum(1 for w in range(L) if w * step + K <= L)                     # windows that fit
        nw = scene.num_windows(L, K, step)
        assert nw == int(np.floor(L / step - K / step + 1).astype(int)) == R.num_windows(L, K, step)      # the reference's line
        assert nw >= 1 and (nw - 1) * step + K <= L                                # no window reads past the signal
        divides = (L - K) % step == 0
        assert nw == brute or (divides and nw == brute - 1), (L, K, step, nw, brute)   # the two rounded quotients
        tw = scene.window_times(L, K, step, 16000.0)
        starts = [w * step for w in range(L) if w * step < L - K]
        assert np.array_equal(tw, np.asarray(starts) / 16000.0) and tw.dtype == np.float64
        assert len(tw) == (brute - 1 if divides else brute)                        # the quirk: one short where step | L - K
        kinds |= {"step>K"} if step > K else set()
        kinds |= {"divides"} if divides and L > K else set()
        kinds |= {"nw=1"} if nw == 1 else set()
        kinds |= {"K=L"} if K == L else set()
    assert kinds == {"step>K", "divides", "nw=1", "K=L"}
    assert scene.num_windows(72000, 3328, 3072) == 23 and scene.num_windows(6400, 3328, 3072) == 2


# ------------------------------------------------------------------------------------------------------------------------
# refusals, with CPU-only inputs
# ------------------------------------------------------------------------------------------------------------------------
def make(L=600, m=2, nsrc=2, fs=16000.0, lv=None, **over):
    lv = L if lv is None else lv
    sc = types.SimpleNamespace(DOA=np.zeros((L, 2, nsrc)), mic_vad_sources=np.zeros((lv, nsrc), dtype=bool), mic_vad=np.zeros(lv, dtype=bool),
                               dp_mic_signals_sources=np.zeros((L, m, nsrc), dtype=np.float32), fs=fs,
                               traj_pts=np.ones((3, 3, nsrc)), timestamps=np.arange(3) * 0.01, t=np.arange(L) / fs)
    for k, v in over.items():
        setattr(sc, k, v)
    return sc, np.zeros((L, m), dtype=np.float32)


@pytest.fixture
def no_device(monkeypatch):
    """Every way from the label functions of fnssl.scene to the device fails the test."""
    from fnssl import ops, scene

    def touched(*a, **k):
        raise AssertionError("the device was touched before the refusal")

    for name in ("scene_doa_batch", "scene_segment_batch", "scene_pack_batch"):
        monkeypatch.setattr(ops, name, touched)
    monkeypatch.setattr(scene, "_up", touched)
    monkeypatch.setattr(scene, "_vad_u8", touched)


REFUSALS = [
    ("sources", dict(nsrc=3), dict(max_source=2), ValueError, r"scene 2: 3 sources \(1 \.\. max_source = 2\)"),
    ("L", dict(L=700), {}, ValueError, r"scene 2: 700 samples, scene 0 has 600"),
    ("M", dict(m=3), {}, ValueError, r"scene 2: 3 microphones, scene 0 has 2"),
    ("fs", dict(fs=8000.0), {}, ValueError, r"scene 2: 8000 Hz, scene 0 has 16000"),
    ("long VAD", dict(lv=601), {}, ValueError, r"scene 2: a VAD of 601 samples for a signal of 600"),
    ("CPU tensor", dict(DOA=torch.zeros(600, 2, 2, dtype=torch.float64)), {}, RuntimeError, r"scene 2: .*ROCm device tensor or a numpy array"),
    ("no DOA", dict(DOA=None), {}, ValueError, r"scene 2: DOA None .*pass array_pos"),
    ("short DOA", dict(DOA=np.zeros((500, 2, 2))), {}, ValueError, r"scene 2: DOA \(500, 2, 2\) for \[>= 564, 2, 2\]"),
    ("dp", dict(dp_mic_signals_sources=np.zeros((600, 2, 1), dtype=np.float32)), {}, ValueError, r"scene 2: dp_mic_signals_sources \(600, 2, 1\)"),
    ("timestamps", dict(timestamps=np.array([0.0, 0.02, 0.01])), dict(array_pos=[[1.0, 1.0, 1.0]] * 3), ValueError,
     r"scene 2: timestamps must be \[P\] finite and increasing"),
    ("array_pos", {}, dict(array_pos=[[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, np.nan, 1.0]]), ValueError, r"scene 2: array_pos"),
]


@pytest.mark.parametrize("what,over,kw,exc,match", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_segment_batch_refuses_before_the_device(no_device, what, over, kw, exc, match):
    from fnssl import scene
    pairs = [make(), make(), make(**over)]
    with pytest.raises(exc, match=match):
        scene.segment_batch([p[1] for p in pairs], [p[0] for p in pairs], 100, 58, **kw)


def test_segment_batch_refuses_windows_longer_than_the_signal(no_device):
    from fnssl import scene
    pairs = [make(), make()]
    mics, scenes = [p[1] for p in pairs], [p[0] for p in pairs]
    with pytest.raises(ValueError, match=r"scene 0: the window size 601 is larger than the signal length 600"):
        scene.segment_batch(mics, scenes, 601, 10)
    with pytest.raises(ValueError, match=r"scene 0: the window step 601 is larger than the signal length 600"):
        scene.segment_batch(mics, scenes, 10, 601)
    with pytest.raises(ValueError, match="no scene"):
        scene.segment_batch([], [], 10, 10)
    with pytest.raises(ValueError, match="1 signals for 2 scenes"):
        scene.segment_batch(mics[:1], scenes, 10, 10)
    with pytest.raises(ValueError, match=r"max_source = 5 \(1 \.\. 4\)"):
        scene.segment_batch(mics, scenes, 10, 10, max_source=5)


def test_transform_has_the_references_checks(no_device):
    from fnssl import scene
    with pytest.raises(Exception, match="window must be a NumPy window function"):
        scene.Segmenting_SRPDNN(8, 4, window=np.ones(7))
    with pytest.raises(Exception, match="window must be a NumPy window function"):
        scene.Segmenting_SRPDNN(8, 4, window=lambda k: 1 / 0)
    t = scene.Segmenting_SRPDNN(8, 4, window=np.hanning)
    assert t.K == 8 and t.step == 4 and np.array_equal(t.w, np.hanning(8))
    assert np.array_equal(scene.Segmenting_SRPDNN(8, 4).w, np.ones(8))
    sc, x = make()
    with pytest.raises(Exception, match=r"The window size can not be larger than the signal length \(600\)"):
        scene.Segmenting_SRPDNN(601, 10)(x, sc)
    with pytest.raises(Exception, match=r"The window step can not be larger than the signal length \(600\)"):
        scene.Segmenting_SRPDNN(10, 601)(x, sc)
    sc, x = make(lv=601)
    with pytest.raises(ValueError, match="mic_vad_sources has 601 samples, the signal 600"):
        scene.Segmenting_SRPDNN(100, 58)(x, sc)
    sc, x = make(DOA=torch.zeros(600, 2, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="ROCm device tensor or a numpy array"):
        scene.Segmenting_SRPDNN(100, 58)(x, sc)


def test_trajectory_doa_refuses_before_the_device(no_device):
    from fnssl import scene
    pts, ts = np.ones((3, 3, 2)), np.arange(3) * 0.01
    with pytest.raises(ValueError, match="timestamps must be"):
        scene.trajectory_doa(pts, ts[::-1], 100, 16000.0, [0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match=r"traj_pts is \[P, 3, S\]"):
        scene.trajectory_doa(np.ones((3, 2, 2)), ts, 100, 16000.0, [0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match=r"5 sources \(1 \.\. 4\)"):
        scene.trajectory_doa(np.ones((3, 3, 5)), ts, 100, 16000.0, [0.0, 0.0, 0.0])
    with pytest.raises(RuntimeError, match="ROCm device tensor or a numpy array"):
        scene.trajectory_doa(torch.ones(3, 3, 2), ts, 100, 16000.0, [0.0, 0.0, 0.0])
    # timestamps held in a tensor are checked too (a small copy to the host)
    with pytest.raises(ValueError, match="timestamps must be"):
        scene._host_timestamps(torch.tensor([0.0, 0.02, 0.01], dtype=torch.float64), "t")
    with pytest.raises(ValueError, match="timestamps must be"):
        scene._host_timestamps(torch.tensor([0.0, float("nan")], dtype=torch.float64), "t")
    good = torch.tensor([0.0, 0.01], dtype=torch.float64)
    assert scene._host_timestamps(good, "t") is good


# ------------------------------------------------------------------------------------------------------------------------
# 25 scenes reach the library as 25 records, in order.  The library cuts them into blocks of 24 in csrc/labels.hip; that cut
# is covered on the device (tests/test_gpu_labels.py, 25 scenes), not here
# ------------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_25_hands_over_every_record_in_order(monkeypatch):
    from fnssl import _lib, ops
    seen = {}

    class FakeLib:
        @staticmethod
        def fnssl_scene_segment_batch(descs, nb, length, K, step, nw, smax, doaw, vsw, vw, count, stream):
            seen["seg"] = ([(descs[b].doa, descs[b].vad_sources, descs[b].vad, descs[b].ns, descs[b].doa_len, descs[b].vad_len)
                            for b in range(nb)], (length, K, step, nw, smax))
            return 0

        @staticmethod
        def fnssl_scene_pack_batch(descs, nb, n, m, smax, out, stream):
            seen["pack"] = [(descs[b].dp[0], descs[b].dp[1], descs[b].stride_t, descs[b].stride_c, descs[b].ns) for b in range(nb)]
            return 0

    class FakeCuda(torch.Tensor):
        is_cuda = True

    real_empty = torch.empty
    monkeypatch.setattr(_lib, "load", lambda: FakeLib)
    monkeypatch.setattr(ops, "_need_dev", lambda *a: None)
    monkeypatch.setattr(ops, "_stream", lambda: C.c_void_p(0))
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **k: real_empty(*a, **k))
    nb, L, K, step = 25, 40, 8, 5
    items, dps = [], []
    for b in range(nb):
        ns = 1 + b % 2
        items.append({"ns": ns, "doa": torch.zeros(L, 2, ns, dtype=torch.float64).as_subclass(FakeCuda),
                      "vad_sources": torch.zeros(L - b, ns, dtype=torch.uint8).as_subclass(FakeCuda),
                      "vad": torch.zeros(L - b, dtype=torch.bool).as_subclass(FakeCuda)})
        dps.append(torch.zeros(L, 2, ns).as_subclass(FakeCuda))
    with pytest.raises(RuntimeError, match="scene 3: no DOA"):
        ops.scene_segment_batch.__wrapped__(items[:3] + [dict(items[3], doa=None)], L, K, step, 7, 2)
    out = ops.scene_segment_batch.__wrapped__(items, L, K, step, 7, 2)
    recs, scalars = seen["seg"]
    assert scalars == (L, K, step, 7, 2) and len(recs) == nb
    assert [r[3:] for r in recs] == [(1 + b % 2, L, L - b) for b in range(nb)]
    assert [r[0] for r in recs] == [it["doa"].data_ptr() for it in items]
    assert tuple(out["doa"].shape) == (nb, 7, 2, 2) and tuple(out["vad_sources"].shape) == (nb, 7, K, 2) and out["vad_count"].dtype == torch.int32
    packed = ops.scene_pack_batch.__wrapped__(dps, L, 2, 2)
    assert tuple(packed.shape) == (nb, L, 2, 2)
    for b, (p0, p1, st_t, st_c, ns) in enumerate(seen["pack"]):
        assert (p0, st_t, st_c, ns) == (dps[b].data_ptr(), 2 * ns, ns, 1 + b % 2)   # the stacked signals are read in place
        assert p1 == (dps[b].data_ptr() + 4 if ns == 2 else None)
