"""GPU tests of the batched scene stage: fnssl_rir_ism_batch / fnssl_rir_tail_batch, fnssl_scene_power_batch /
fnssl_scene_finish_batch, and fnssl.rir.simulateRIRBatch, fnssl.scene.simulate_batch / get_batch over them.

The reference for equality is the single-call route (ops.rir_ism, ops.rir_tail, ops.scene_power, ops.scene_finish,
scene.simulate), which tests/test_gpu_rir.py and tests/test_gpu_scene.py hold to float64: every comparison here is bit for
bit.  The shapes are the smallest at which the batch machinery can go wrong: jobs of one and of several chunks in one launch,
tiles from 2 to 8192 samples under one LDS size, jobs with and without a tail, scenes of 1 to 4 sources and ragged noise.
Run with -m gpu on an MI355X."""
import types

import numpy as np
import pytest

import scene_ref as R
from conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOM = [3.2, 4.1, 2.6]
BETA = [0.8, 0.7, 0.75, 0.85, 0.6, 0.9]
SENTINEL = 7.0
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


def up(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def positions(count, seed, room=ROOM):
    rs = np.random.RandomState(seed)
    return (rs.uniform(0.15, 0.85, (count, 3)) * np.asarray(room)).astype(np.float32)


# (nb_img, nism, nsamples, m_src, m_rcv): one image, a few, and several chunks; tiles of 2, 130, 1600 and 8192 samples;
# nsamples == nism and nsamples > nism
ISM_JOBS = [
    ([1, 1, 1], 2, 2, 1, 1),
    ([3, 2, 2], 130, 130, 5, 2),
    ([9, 7, 11], 1600, 2400, 3, 2),                                        # the job of several chunks (asserted below)
    ([3, 2, 2], 8192, 8192, 1, 3),
    ([1, 1, 1], 1600, 1600, 5, 3),
    ([5, 5, 3], 130, 400, 1, 1),
    ([12, 9, 7], 1600, 1600, 1, 1),
]
CHUNKED = 2


def ism_jobs(dev, which=ISM_JOBS, room=ROOM):
    return [dict(pos_src=up(positions(ms, 10 + k, room), dev), pos_rcv=up(positions(mr, 50 + k, room), dev), room_sz=room, beta=BETA,
                 nb_img=nb, nism=nism, nsamples=ns, fs=R.FS, c=343.0, seed=100 + k)
            for k, (nb, nism, ns, ms, mr) in enumerate(which)]


def sentinel_outputs(jobs, dev):
    """Every job's RIRs as views of one buffer filled with the sentinel, GUARD floats between them."""
    sizes = [j["pos_src"].shape[0] * j["pos_rcv"].shape[0] * j["nsamples"] for j in jobs]
    flat = torch.full((sum(sizes) + GUARD * (len(jobs) + 1),), SENTINEL, dtype=torch.float32, device=dev)
    outs, mask, off = [], torch.ones_like(flat, dtype=torch.bool), GUARD
    for j, size in zip(jobs, sizes):
        outs.append(flat[off:off + size].view(j["pos_src"].shape[0], j["pos_rcv"].shape[0], j["nsamples"]))
        mask[off:off + size] = False
        off += size + GUARD
    return flat, outs, mask


def single_ism(j):
    from fnssl import ops
    return ops.rir_ism(j["pos_src"], j["pos_rcv"], j["room_sz"], j["beta"], j["nb_img"], j["nism"], j["nsamples"], j["fs"], j["c"])


# ------------------------------------------------------------------------------------------------------------------------
# RIR jobs
# ------------------------------------------------------------------------------------------------------------------------
def test_ism_jobs_equal_the_single_calls_whatever_the_batch(dev):
    from fnssl import ops
    jobs = ism_jobs(dev)
    nb, nism, _, ms, mr = ISM_JOBS[CHUNKED]
    plan = ops.rir_plan(ms, mr, nb, nism)
    print("plan of the chunked job alone:", plan)
    assert plan["nchunks"] >= 3 and plan["last_chunk_images"] < plan["chunk_images"]
    assert ops.rir_plan(*ISM_JOBS[1][3:5], ISM_JOBS[1][0], ISM_JOBS[1][1])["nchunks"] == 1     # both store paths share the launch
    alone = [single_ism(j) for j in jobs]

    flat, outs, guard = sentinel_outputs(jobs, dev)
    got = ops.rir_ism_batch(jobs, outs)
    for k, (j, a, g) in enumerate(zip(jobs, alone, got)):
        assert g.data_ptr() == outs[k].data_ptr()
        assert torch.equal(g[:, :, :j["nism"]], a[:, :, :j["nism"]]), k
        assert bool((g[:, :, j["nism"]:] == SENTINEL).all()), k                # [nism, nsamples) is left alone
    assert bool((flat[guard] == SENTINEL).all())                            # nothing outside a job's own RIRs changes

    # reversed, and each job alone in a batch of one: the same bits
    rev = ops.rir_ism_batch(jobs[::-1])[::-1]
    for k, (j, a, r) in enumerate(zip(jobs, alone, rev)):
        assert torch.equal(r, a), k                                         # without `outs` the rest is zero, as rir_ism's
        assert torch.equal(ops.rir_ism_batch([j])[0], a), k


# (nism, nsamples, m_src, m_rcv, seed): the direct sound arrives after 0.5 .. 4 m, 23 .. 190 samples; a segment is 128
TAIL_JOBS = [
    (130, 1000, 2, 2, 5),                                                  # no whole segment: the mean square of the ISM part
    (300, 2000, 1, 3, 6),                                                  # one or two segments: Sabine's slope
    (1600, 1600, 2, 1, 7),                                                 # no tail, in the middle of the batch
    (1600, 9000, 3, 2, 8),                                                 # >= 3 segments: the fitted line; three tiles of 4096
    (1600, 9000, 3, 2, 8),                                                 # the same seed and geometry: the same tail
    (1600, 9000, 3, 2, 9),                                                 # another seed
]


def test_tail_jobs_equal_the_single_calls(dev):
    from fnssl import ops
    jobs = []
    for k, (nism, ns, ms, mr, seed) in enumerate(TAIL_JOBS):
        geo = 30 + min(k, 3)                                                # jobs 3, 4, 5 share their geometry
        jobs.append(dict(pos_src=up(positions(ms, geo), dev), pos_rcv=up(positions(mr, 70 + geo), dev), room_sz=ROOM, beta=BETA,
                         nb_img=[3, 3, 3], nism=nism, nsamples=ns, fs=R.FS, c=343.0, seed=seed))
    alone = []
    for j in jobs:
        r = single_ism(j)
        if j["nsamples"] > j["nism"]:
            ops.rir_tail(r, j["pos_src"], j["pos_rcv"], j["room_sz"], j["beta"], j["nism"], j["fs"], j["c"], j["seed"])
        alone.append(r)
    # the segments the fit sees: none, one or two, three or more
    for k, want in ((0, (0, 0)), (1, (1, 2)), (3, (3, 99))):
        j = jobs[k]
        d = (j["pos_src"][:, None, :] - j["pos_rcv"][None, :, :]).norm(dim=2).cpu().numpy()
        nseg = (j["nism"] - np.minimum(np.floor(d * R.FS / 343.0).astype(int), j["nism"])) // 128
        print("tail job %d: whole segments per RIR %s" % (k, nseg.reshape(-1).tolist()))
        assert want[0] <= nseg.min() and nseg.max() <= want[1], (k, nseg)
    flat, outs, guard = sentinel_outputs(jobs, dev)
    got = ops.rir_tail_batch(jobs, ops.rir_ism_batch(jobs, outs))
    for k, (a, g) in enumerate(zip(alone, got)):
        assert torch.equal(g, a), k
    assert bool((flat[guard] == SENTINEL).all())
    assert torch.equal(got[3], got[4]) and torch.equal(got[3][:, :, :1600], got[5][:, :, :1600])
    assert not torch.equal(got[3][:, :, 1600:], got[5][:, :, 1600:]) and float(got[3][:, :, 1600:].abs().max()) > 0
    # a batch of one, and the gpuRIR-named surface on the same jobs
    for k, j in enumerate(jobs):
        assert torch.equal(ops.rir_tail_batch([j], ops.rir_ism_batch([j]))[0], alone[k]), k


def test_simulate_rir_batch_equals_simulate_rir(dev):
    import fnssl.rir as gpuRIR
    src, rcv = positions(3, 1), positions(2, 2)
    jobs = [dict(room_sz=ROOM, beta=BETA, pos_src=src, pos_rcv=rcv, nb_img=[5, 4, 6], Tmax=0.2, fs=R.FS, Tdiff=0.05, seed=3),
            (ROOM, BETA, src[:1], rcv, [1, 1, 1], 0.1, R.FS),
            dict(room_sz=[6.0, 5.0, 3.0], beta=[0.9] * 6, pos_src=rcv, pos_rcv=src, nb_img=[4, 4, 4], Tmax=0.3, fs=R.FS, Tdiff=0.04, seed=4)]
    got = gpuRIR.simulateRIRBatch(jobs)
    for k, job in enumerate(jobs):
        want = gpuRIR.simulateRIR(**job) if isinstance(job, dict) else gpuRIR.simulateRIR(*job)
        assert isinstance(got[k], np.ndarray) and np.array_equal(got[k].view(np.uint32), want.view(np.uint32)), k
    on_dev = gpuRIR.simulateRIRBatch([dict(jobs[0], pos_src=up(src, dev), pos_rcv=up(rcv, dev))])
    assert on_dev[0].is_cuda and np.array_equal(on_dev[0].cpu().numpy(), got[0])


def test_a_refused_job_is_named_and_nothing_is_enqueued(dev):
    from fnssl import ops
    import fnssl.rir as gpuRIR
    which = [ISM_JOBS[1], ISM_JOBS[5], ([3, 2, 2], 8194, 8194, 1, 1), ISM_JOBS[0]]
    jobs = ism_jobs(dev, which)
    flat, outs, _ = sentinel_outputs(jobs, dev)
    ops.timing_enable(True)
    try:
        ops.timing_collect()
        with pytest.raises(RuntimeError, match=r"job 2: nISM = 8194 .*8192"):
            ops.rir_ism_batch(jobs, outs)
        with pytest.raises(RuntimeError, match=r"job 2: nISM = 8194 .*8192"):
            ops.rir_tail_batch(jobs, outs)
        # a receiver outside its room: the host check of the gpuRIR-named surface, before anything is uploaded
        inside = [dict(room_sz=ROOM, beta=BETA, pos_src=positions(ms, 1), pos_rcv=positions(mr, 2), nb_img=nb, Tmax=ns / R.FS, fs=R.FS,
                       Tdiff=nism / R.FS) for nb, nism, ns, ms, mr in which]
        inside[2] = dict(inside[0], pos_rcv=np.array([[1.0, 1.0, 1.0], [1.0, 4.2, 1.0]], dtype=np.float32))
        with pytest.raises(ValueError, match=r"job 2: .*receiver position must lie strictly inside the room"):
            gpuRIR.simulateRIRBatch(inside, out=[outs[0], outs[1], outs[0], outs[3]])
        torch.cuda.synchronize()
        assert ops.timing_collect() == {}                                   # no launch was recorded
    finally:
        ops.timing_enable(False)
    assert bool((flat == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------
# power and finish
# ------------------------------------------------------------------------------------------------------------------------
def mix_scene(n, nsrc, noise_len, with_vad, seed, m=3):
    rs = np.random.RandomState(seed)
    tot = n + 40
    env = (np.sin(np.arange(tot) / 37.0 + seed) > -0.3).astype(np.float64)[:, None]
    sig = [rs.standard_normal((tot, m)) * env * 0.1 for _ in range(nsrc)]
    dp = [0.6 * a + 0.01 * rs.standard_normal((tot, m)) * env for a in sig]
    vads = [np.abs(rs.standard_normal((tot, m))) * (np.sin(np.arange(tot) / (23.0 + 9 * s)) > 0.2)[:, None] for s in range(nsrc)]
    return dict(sig=sig, dp=dp, noise=rs.standard_normal((noise_len, m)), snr_db=[-5.0, 12.0, 30.0][seed % 3], vads=vads if with_vad else None)


@pytest.mark.parametrize("with_vad", [False, True])
@pytest.mark.parametrize("n", [512, 767, 5000])
def test_power_and_finish_of_a_batch_equal_the_single_calls(dev, n, with_vad):
    from fnssl import ops
    host = [mix_scene(n, 1, n, with_vad, 1), mix_scene(n, 2, n + 300, with_vad, 2), mix_scene(n, 4, n, with_vad, 3)]
    d = lambda seq: None if seq is None else [up(a, dev) for a in seq]
    scenes = [dict(sig=d(h["sig"]), dp=d(h["dp"]), noise=up(h["noise"], dev), snr_db=h["snr_db"], vads=d(h["vads"])) for h in host]
    got = ops.scene_mix_batch(scenes, n)
    assert got["mic"].shape == (3, n, 3) and got["g"].shape == (3,)
    for b, sc in enumerate(scenes):
        p = ops.scene_power(sc["dp"], n)
        pn = ops.scene_power([sc["noise"]])                                 # over the WHOLE noise, n + 300 for scene 1
        fin = ops.scene_finish(sc["sig"], sc["noise"], p, pn, sc["snr_db"], n, sc["vads"])
        assert torch.equal(got["power"][b], p) and torch.equal(got["power_noise"][b], pn), b
        assert torch.equal(got["g"][b:b + 1], fin["g"]) and torch.equal(got["mic"][b], fin["mic"]), b
        if with_vad:
            assert torch.equal(got["vmax"][b], fin["vmax"]) and torch.equal(got["vad_sources"][b], fin["vad_sources"]), b
            assert torch.equal(got["vad"][b], fin["vad"]) and 0 < int(fin["vad"].sum()) < n, b
        else:
            assert got["vmax"][b] is None and got["vad_sources"][b] is None
    with pytest.raises(RuntimeError, match=r"scene 1: 5 (summands|sources) \(1 \.\. 4\)"):
        five = dict(scenes[1], sig=scenes[2]["sig"] + scenes[0]["sig"], dp=scenes[2]["dp"] + scenes[0]["dp"], vads=None)
        ops.scene_mix_batch([scenes[0] | {"vads": None}, five], n)


# ------------------------------------------------------------------------------------------------------------------------
# whole scenes
# ------------------------------------------------------------------------------------------------------------------------
N = 6000
# (T60, sources, trajectory points, room, noise rows beyond n or None for a drawn noise)
MAKEUP = [(0.0, 1, 1, [3.2, 4.1, 2.6], 0), (0.1, 2, 3, [3.2, 4.1, 2.6], 448), (0.3, 3, 7, [5.0, 6.0, 3.0], 0),
          (0.6, 1, 3, [8.0, 9.0, 5.0], 100), (0.3, 2, 1, [4.0, 3.5, 2.8], 0)]


def make_scene(k, m, conv=lambda a: a, with_vad=True, no_noise=False, makeup=MAKEUP, n=N):
    t60, nsrc, npts, room, extra = makeup[k]
    rs = np.random.RandomState(900 + 10 * k + m)
    env = (np.sin(np.arange(n) / (250.0 + 30 * k)) > -0.5).astype(np.float64)
    pts = rs.uniform(0.2, 0.8, (npts, 3, nsrc)) * np.asarray(room)[None, :, None]
    centre = np.asarray(room) * [0.5, 0.45, 0.4]
    mic_pos = centre[None, :] + np.stack([[0.04 * (i - (m - 1) / 2), 0.0, 0.0] for i in range(m)])
    ts = np.sort(np.r_[0.0, rs.uniform(0.01, n / R.FS * 0.9, npts - 1)])
    sc = types.SimpleNamespace(
        room_sz=room, T60=t60, beta=np.asarray(R.rir_beta(room, t60) if t60 else [0.0] * 6), SNR=float([5, 12, 20, 30, -3][k % 5]), fs=R.FS,
        noise_signal=None if no_noise else conv(rs.standard_normal((n + extra, m)).astype(np.float32)),
        source_signal=conv((rs.standard_normal((n, nsrc)) * env[:, None] * 0.3).astype(np.float32)),
        array_setup=types.SimpleNamespace(mic_orV=None, mic_pattern="omni"), mic_pos=conv(mic_pos.astype(np.float32)),
        timestamps=ts, traj_pts=conv(pts.astype(np.float32)), t=np.arange(n) / R.FS, c=343.0)
    if with_vad:
        sc.source_vad = conv(np.stack([(np.sin(np.arange(n) / (200.0 + 25 * s)) > -0.2) for s in range(nsrc)], axis=1).astype(np.float32))
    return sc


def same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)


def compare_scene(b, mic_b, part_b, sc_b, mic_1, part_1, sc_1, with_vad=True):
    assert same(mic_b, mic_1), b
    for name in ("dp_mic_signals_sources",) + (("mic_vad_sources", "mic_vad") if with_vad else ()):
        assert same(getattr(sc_b, name), getattr(sc_1, name)), (b, name)
    assert part_b["seed"] == part_1["seed"]
    for name in ("g", "power", "power_noise", "noise"):
        assert torch.equal(part_b[name], part_1[name]), (b, name)
    for name in ("rirs", "dp_rirs", "mic_signals_sources", "dp_mic_signals_sources") + (("vad_signals",) if with_vad else ()):
        assert len(part_b[name]) == len(part_1[name])
        for s, (x, y) in enumerate(zip(part_b[name], part_1[name])):
            assert torch.equal(x, y), (b, name, s)


@pytest.mark.parametrize("m", [2, 4])
def test_scene_batch_equals_simulate_per_scene(dev, m):
    from fnssl import scene
    conv = (lambda a: a) if m == 2 else (lambda a: up(a, dev))                 # numpy scenes, and scenes of device tensors
    seeds = [41, 7, 2 ** 31 - 5, 0, 123456]
    batch = [make_scene(k, m, conv) for k in range(5)]
    mic, parts = scene.simulate_batch(batch, seeds=seeds, keep=True)
    assert tuple(mic.shape) == (5, N, m) and (isinstance(mic, np.ndarray) if m == 2 else mic.is_cuda)
    for b in range(5):
        one = make_scene(b, m, conv)
        mic_1, part_1 = scene.simulate(one, seed=seeds[b], keep=True)
        compare_scene(b, mic[b], parts[b], batch[b], mic_1, part_1, one)
        assert batch[b].mic_vad_sources.shape == (N, MAKEUP[b][1]) and batch[b].dp_mic_signals_sources.shape == (N, m, MAKEUP[b][1])
    assert float(parts[2]["rirs"][0][:, :, -1].abs().max()) > 0              # the tails were written

    # seeds=None: per scene first the seed, then its noise when it is None
    drawn = (1, 3)
    batch = [make_scene(k, m, conv, no_noise=k in drawn) for k in range(5)]
    np.random.seed(7)
    mic, parts = scene.simulate_batch(batch, keep=True)
    state = np.random.get_state()[1].copy()
    np.random.seed(7)
    for b in range(5):
        one = make_scene(b, m, conv, no_noise=b in drawn)
        mic_1, part_1 = scene.simulate(one, keep=True)
        compare_scene(b, mic[b], parts[b], batch[b], mic_1, part_1, one)
        if b in drawn:
            assert same(batch[b].noise_signal, one.noise_signal) and tuple(one.noise_signal.shape) == (N, m)
    assert np.array_equal(np.random.get_state()[1], state)                  # both routes consumed the same stream


def golden_scene(t60):
    g = load_golden("g23_scene")
    key = "b_%g" % t60
    t60_, snr, fs, seed, n = g[key + "_scalars"]
    sc = types.SimpleNamespace(
        room_sz=g[key + "_room_sz"].tolist(), T60=float(t60_), beta=g[key + "_beta"].astype(np.float64), SNR=float(snr), fs=float(fs),
        noise_signal=g[key + "_noise_signal"], source_signal=g[key + "_source_signal"],
        array_setup=types.SimpleNamespace(mic_orV=None, mic_pattern="omni"), mic_pos=g[key + "_mic_pos"],
        timestamps=g[key + "_timestamps"], traj_pts=g[key + "_traj_pts"], t=np.arange(int(n)) / float(fs), c=343.0,
        source_vad=g[key + "_source_vad"].astype(np.float32))
    return sc, int(seed), g[key + "_mic_signals"]


def test_the_golden_scenes_as_one_batch(dev):
    """Golden G23(b), AcousticScene.simulate of the reference at T60 = 0 and 0.2, run as one batch of two and held by the
    gate tests/test_gpu_scene.py holds the single calls to: scene_ref.GATE's keys, its factor of 8."""
    from fnssl import scene
    cases = [golden_scene(t60) for t60 in (0, 0.2)]
    mic = scene.simulate_batch([c[0] for c in cases], seeds=[c[1] for c in cases])
    assert isinstance(mic, np.ndarray) and mic.dtype == np.float32 and mic.shape == (2, R.SCENE_N, 2)
    for b, t60 in enumerate((0, 0.2)):
        dist = float(np.abs(mic[b].astype(np.float64) - cases[b][2]).max())
        bound = R.GATE_FACTOR * R.GATE["simulate/%g" % t60]
        print("simulate_batch T60 = %g: device %.3e from the golden, float32 restatement %.3e, bound %.3e" % (t60, dist, R.GATE["simulate/%g" % t60], bound))
        assert dist <= bound
        sc = cases[b][0]
        assert sc.mic_vad_sources.shape == (R.SCENE_N, 2) and sc.mic_vad_sources.dtype == bool and sc.mic_vad.shape == (R.SCENE_N,)


def test_one_launch_set_whatever_the_batch(dev):
    """A batch of 2 and a batch of 8 scenes of the same makeup issue the same launches under every kernel name.  The makeup
    is one source without VAD: two RIR jobs and two mixings per scene, so that the 8 scenes fill one block of the smallest
    descriptor, the 16 pairs of fnssl_rir_trajectory (the RIR jobs take 32 per launch, the scenes 24)."""
    from fnssl import ops, scene
    makeup = [(0.3, 1, 3, [5.0, 6.0, 3.0], 0)] * 8
    counts = []
    ops.timing_enable(True)
    try:
        for nb in (2, 8):
            batch = [make_scene(k, 2, with_vad=False, makeup=makeup, n=2048) for k in range(nb)]
            ops.timing_collect()
            scene.simulate_batch(batch, seeds=list(range(nb)))
            torch.cuda.synchronize()
            counts.append({name: v["count"] for name, v in ops.timing_collect().items()})
            print("B = %d: %s" % (nb, counts[-1]))
    finally:
        ops.timing_enable(False)
    assert counts[0] == counts[1]
    assert counts[0] == {"rir_ism_batch": 1, "rir_sum_batch": 1, "rir_tail_batch": 1, "rir_trajectory": 1, "scene_power_batch": 1,
                         "scene_finish_batch": 1}


def test_get_batch_on_a_stub_dataset(dev):
    from fnssl import scene

    def tag(mic, sc):
        sc.tagged = mic.shape
        return mic * 2.0, sc

    made = []

    class Stub:
        transforms = [tag]

        def getRandomScene(self, idx):
            made.append(idx)
            return make_scene(idx % 5, 2, no_noise=idx == 3)

    np.random.seed(11)
    sigs, scenes = scene.get_batch(Stub(), 1, 4)
    assert made == [1, 2, 3] and isinstance(sigs, np.ndarray) and sigs.shape == (3, N, 2) and len(scenes) == 3
    np.random.seed(11)
    for b, idx in enumerate((1, 2, 3)):
        one = make_scene(idx, 2, no_noise=idx == 3)
        want = scene.simulate(one)
        assert np.array_equal(sigs[b], want * 2.0), idx
        assert scenes[b].tagged == (N, 2) and scenes[b].dp_mic_signals_sources.shape == (N, 2, MAKEUP[idx][1])
        assert same(scenes[b].mic_vad, one.mic_vad) and same(scenes[b].mic_vad_sources, one.mic_vad_sources)
    Stub.transforms = None
    assert scene.get_batch(Stub(), 0, 2)[0].shape == (2, N, 2)
