"""CPU tests of the batched scene stage: the plan of a batch of RIR jobs (fnssl_rir_batch_plan, host only), every
refusal of fnssl.scene.simulate_batch before anything touches the device, the order in which it consumes numpy's random
stream, and the grouping of more than 16 mixings."""
import ctypes as C
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

CUS = 256


def random_jobs(rs, count):
    jobs = []
    for _ in range(count):
        nb = [int(v) for v in rs.randint(1, 40, 3)] if rs.rand() < 0.8 else [1, 1, 1]
        jobs.append(dict(m_src=int(rs.randint(1, 60)), m_rcv=int(rs.randint(1, 9)), room_sz=[4.0, 5.0, 3.0], nb_img=nb,
                         nism=2 * int(rs.randint(1, 4097))))
    return jobs


def plan_fields(p):
    return {k: v for k, v in p.items() if k != "workspace_offset"}


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_job_is_planned_as_if_alone(seed):
    from fnssl import ops
    rs = np.random.RandomState(seed)
    jobs = random_jobs(rs, 40)                                              # more than one block of FNSSL_RIR_BATCH_JOBS
    plans, total = ops.rir_batch_plan(jobs, CUS)
    assert len(plans) == len(jobs)
    spans = []
    for j, p in zip(jobs, plans):
        alone = ops.rir_plan(j["m_src"], j["m_rcv"], j["nb_img"], j["nism"], CUS)
        assert plan_fields(p) == alone
        if p["nchunks"] == 1:
            assert p["workspace_bytes"] == 0                                # one chunk: straight into the RIR
        else:
            assert p["workspace_bytes"] == 4 * p["nchunks"] * j["m_src"] * j["m_rcv"] * j["nism"]
            spans.append((p["workspace_offset"], p["workspace_offset"] + p["workspace_bytes"]))
    assert len(spans) >= 5 and any(p["nchunks"] == 1 for p in plans)
    spans.sort()
    assert spans[0][0] >= 0 and spans[-1][1] <= total
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))              # disjoint
    assert total == sum(p["workspace_bytes"] for p in plans)

    # added, removed, reordered: a job's plan is its own
    by_id = {id(j): plan_fields(p) for j, p in zip(jobs, plans)}
    order = rs.permutation(len(jobs))
    for sub in ([jobs[i] for i in order], jobs[5:17], jobs[::3] + random_jobs(rs, 7), jobs[:1]):
        for j, p in zip(sub, ops.rir_batch_plan(sub, CUS)[0]):
            if id(j) in by_id:
                assert plan_fields(p) == by_id[id(j)]
    # another device, another plan: the CU count is the one thing outside the job that enters
    assert any(plan_fields(a) != plan_fields(b) for a, b in zip(plans, ops.rir_batch_plan(jobs, 64)[0]))


def test_a_refused_job_is_named_by_the_plan():
    from fnssl import ops
    jobs = random_jobs(np.random.RandomState(3), 4)
    jobs[2] = dict(jobs[2], nism=8194)
    with pytest.raises(RuntimeError, match=r"job 2: nISM = 8194 .*8192"):
        ops.rir_batch_plan(jobs, CUS)
    jobs[2] = dict(jobs[2], nism=100, nb_img=[1, 2000, 1])
    with pytest.raises(RuntimeError, match=r"job 2: nb_img\[1\] = 2000"):
        ops.rir_batch_plan(jobs, CUS)


# ------------------------------------------------------------------------------------------------------------------------
# simulate_batch: refusals and draws, with CPU-only inputs
# ------------------------------------------------------------------------------------------------------------------------
def make(m=2, n=600, nsrc=2, fs=16000.0, vad=True, **over):
    sc = types.SimpleNamespace(
        room_sz=[4.0, 5.0, 3.0], T60=0.3, beta=np.full(6, 0.7), SNR=10.0, fs=fs, noise_signal=np.zeros((n, m)),
        source_signal=np.zeros((n, nsrc)), array_setup=types.SimpleNamespace(mic_orV=None, mic_pattern="omni"),
        mic_pos=np.ones((m, 3)), timestamps=np.arange(3) * n / fs / 3, traj_pts=np.ones((3, 3, nsrc)) * 1.5, t=np.arange(n) / fs)
    if vad:
        sc.source_vad = np.zeros((n, nsrc))
    for k, v in over.items():
        setattr(sc, k, v)
    return sc


@pytest.fixture
def no_device(monkeypatch):
    """Every way from fnssl.scene / fnssl.rir to the device fails the test."""
    from fnssl import ops, rir, scene

    def touched(*a, **k):
        raise AssertionError("the device was touched before the refusal")

    for name in ("rir_ism_batch", "rir_tail_batch", "rir_trajectory_batch", "scene_mix_batch", "rir_ism", "rir_tail"):
        monkeypatch.setattr(ops, name, touched)
    monkeypatch.setattr(rir, "_upload_packed", touched)
    monkeypatch.setattr(scene, "_up", touched)


REFUSALS = [
    ("M", dict(m=4), ValueError, r"scene 2: 4 microphones, scene 0 has 2"),
    ("fs", dict(fs=8000.0), ValueError, r"scene 2: 8000 Hz, scene 0 has 16000"),
    ("len(t)", dict(n=700), ValueError, r"scene 2: 700 samples \(len\(t\)\), scene 0 has 600"),
    ("VAD", dict(vad=False), ValueError, r"scene 2: source_vad is absent, in scene 0 it is present"),
    ("5 sources", dict(nsrc=5), ValueError, r"scene 2: 5 sources \(1 \.\. 4\)"),
    ("0 sources", dict(nsrc=0), ValueError, r"scene 2: 0 sources \(1 \.\. 4\)"),
    ("pattern", dict(array_setup=types.SimpleNamespace(mic_orV=None, mic_pattern="card")), NotImplementedError,
     r"scene 2: mic_pattern 'card' is not built"),
    ("CPU tensor", dict(source_signal=torch.zeros(600, 2)), RuntimeError, r"scene 2: .*ROCm device tensor or a numpy array"),
    ("noise", dict(noise_signal=np.zeros((599, 2))), ValueError, r"scene 2: noise_signal \(599, 2\) for \[>= 600, 2\]"),
    ("receiver", dict(mic_pos=np.array([[1.0, 1.0, 1.0], [1.0, 5.5, 1.0]])), ValueError, r"scene 2: .*receiver position must lie strictly inside"),
]


@pytest.mark.parametrize("what,over,exc,match", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_simulate_batch_refuses_before_the_device(no_device, what, over, exc, match):
    from fnssl import scene
    with pytest.raises(exc, match=match):
        scene.simulate_batch([make(), make(), make(**over)], seeds=[1, 2, 3])


def test_simulate_batch_refuses_short_scenes_and_bad_seeds(no_device):
    from fnssl import scene
    with pytest.raises(ValueError, match=r"scene 0: 511 samples \(acoustic_power needs one window of 512\)"):
        scene.simulate_batch([make(n=511), make(n=511)])
    with pytest.raises(ValueError, match="2 seeds for 3 scenes"):
        scene.simulate_batch([make(), make(), make()], seeds=[1, 2])
    with pytest.raises(ValueError, match="no scene"):
        scene.simulate_batch([])


def test_seeds_and_noise_are_drawn_as_sequential_calls_would(monkeypatch):
    """seeds=None: per scene first the seed, then its noise if None.  The device calls are stubbed: the RIR batch records
    the seeds it was given and stops the call."""
    from fnssl import rir, scene

    class Stop(Exception):
        pass

    seen = {}

    def stub(jobs, **kw):
        seen["seeds"] = [j["seed"] for j in jobs if "seed" in j]
        raise Stop

    monkeypatch.setattr(rir, "simulateRIRBatch", stub)
    n, m = 600, 2
    scenes = [make(nsrc=1), make(noise_signal=None), make(nsrc=3, noise_signal=None), make()]
    np.random.seed(123)
    with pytest.raises(Stop):
        scene.simulate_batch(scenes)
    after = np.random.get_state()[1].copy()
    np.random.seed(123)
    want = []
    for sc in scenes:                                                       # what B calls of simulate() consume, in order
        seed = int(np.random.randint(0, 2 ** 31 - 1))
        want += [seed + s for s in range(sc.traj_pts.shape[-1])]
        if sc.noise_signal is None:
            np.random.standard_normal((n, m))
    assert seen["seeds"] == want
    assert np.array_equal(np.random.get_state()[1], after)
    # explicit seeds leave the stream alone unless a noise is drawn
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    with pytest.raises(Stop):
        scene.simulate_batch([make(), make()], seeds=[9, 10])
    assert seen["seeds"] == [9, 10, 10, 11] and np.array_equal(np.random.get_state()[1], before)


def test_more_than_sixteen_mixings_go_in_groups_in_order(monkeypatch):
    """ops.rir_trajectory_batch hands fnssl_rir_trajectory at most FNSSL_RIR_TRAJ_MAX_BATCH items a call, in order; the
    library call and the device checks are stubbed (the tensors live on the CPU here)."""
    from fnssl import _lib, ops
    calls = []

    class FakeLib:
        @staticmethod
        def fnssl_rir_trajectory(items, count, stream):
            calls.append([(items[k].x, items[k].ns, items[k].len, items[k].npts, items[k].m) for k in range(count)])
            return 0

    monkeypatch.setattr(_lib, "load", lambda: FakeLib)
    monkeypatch.setattr(ops, "_need_dev", lambda *a: None)
    monkeypatch.setattr(ops, "_stream", lambda: C.c_void_p(0))

    class FakeCuda(torch.Tensor):
        is_cuda = True

    n = 37
    xs = [torch.zeros(10 + k).as_subclass(FakeCuda) for k in range(n)]
    rs = [torch.zeros(1 + k % 3, 2, 5 + k).as_subclass(FakeCuda) for k in range(n)]
    ws = [torch.zeros(2 + k % 3, dtype=torch.int32).as_subclass(FakeCuda) for k in range(n)]
    ys = ops.rir_trajectory_batch.__wrapped__(xs, rs, ws)
    assert [len(c) for c in calls] == [16, 16, 5] and _lib.RIR_TRAJ_MAX_BATCH == 16
    flat = [item for c in calls for item in c]
    assert flat == [(xs[k].data_ptr(), 10 + k, 5 + k, 1 + k % 3, 2) for k in range(n)]
    assert [tuple(y.shape) for y in ys] == [(10 + k + 5 + k - 1, 2) for k in range(n)]
