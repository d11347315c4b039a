"""GPU tests of the room simulation (csrc/rir.hip: fnssl_rir_ism, fnssl_rir_tail, fnssl_rir_trajectory; fnssl/rir.py, the
gpuRIR-named surface) against the float64 restatements of tests/rir_ref.py.

Gates: per case the device may be at most 8 x as far from float64 (max abs over the output) as the float32
restatement of rir_ref is; those distances are the table ``rir_ref.GATE``, measured on a CPU and re-measured by
tests/test_rir_ref_host.py.  The tail is restated from the image-source part the DEVICE stored, with the same generator.
The trajectory kernel is held exactly (integer-valued inputs whose partial sums are exact in fp32), one random leg at its
gate.  Every figure is printed before it is asserted.  Run with -m gpu on an MI355X."""
import functools

import numpy as np
import pytest

import rir_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def ism_f64(name):
    return R.ism_case(name)


def device_rir(name, tmax=None, tdiff=None, seed=0):
    import fnssl.rir as gpuRIR
    src, rcv, nb, td, c = R.ISM_CASES[name]
    td = td if tdiff is None else tdiff
    return gpuRIR.simulateRIR(R.ROOM, R.BETA, np.array(src), np.array(rcv), nb, td if tmax is None else tmax, R.FS, Tdiff=td,
                              c=c, seed=seed)


def held(what, got, want, gate_key):
    dist = float(np.abs(got.astype(np.float64) - want).max())
    bound = R.GATE_FACTOR * R.GATE[gate_key]
    print("%s: device %.3e from float64, float32 restatement %.3e, bound %.3e, peak %.3e"
          % (what, dist, R.GATE[gate_key], bound, float(np.abs(want).max())))
    assert dist <= bound, (what, dist, bound)


# ------------------------------------------------------------------------------------------------------------------------
# image-source part
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.ISM_CASES))
def test_ism_is_held_to_float64(dev, name):
    from fnssl import ops
    src, rcv, nb, tdiff, c = R.ISM_CASES[name]
    nism, _ = R.sample_counts(tdiff, tdiff, R.FS)
    got = device_rir(name)
    assert got.dtype == np.float32 and got.shape == (len(src), len(rcv), nism)
    plan = ops.rir_plan(len(src), len(rcv), nb, nism)
    print("plan", name, plan)
    if name == "chunks":        # the image set of one RIR is split, with a ragged last chunk, and summed through the workspace
        assert plan["nchunks"] >= 2 and 0 < plan["last_chunk_images"] < plan["chunk_images"] and plan["workspace_bytes"] > 0
    if name == "direct":
        assert plan["nchunks"] == 1 and plan["workspace_bytes"] == 0
    if name == "odd_count":
        assert nism == 802
    want = ism_f64(name)
    if name == "past_nism":     # some images of the case arrive past nISM (otherwise it does not test the skip)
        assert 0.5 * np.hypot(np.hypot(9 * 3.2, 8 * 4.1), 7 * 2.6) * R.FS / 343.0 > nism + 64
    if name == "near":
        assert np.abs(want[0, 0, :3]).max() > 0.1          # the direct path's window starts before t = 0
    held("ism/" + name, got, want, "ism/" + name)
    again = device_rir(name)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "two runs differ"


def test_ism_too_long_for_the_tile_is_refused(dev):
    import fnssl.rir as gpuRIR
    with pytest.raises(RuntimeError, match="8192"):
        gpuRIR.simulateRIR(R.ROOM, R.BETA, np.array(R.SRC[:1]), np.array(R.RCV[:1]), [3, 3, 3], 0.6, R.FS)
    out = gpuRIR.simulateRIR(R.ROOM, R.BETA, np.array(R.SRC[:1]), np.array(R.RCV[:1]), [3, 3, 3], 0.6, R.FS, Tdiff=0.512)
    assert out.shape == (1, 1, 9600) and np.isfinite(out).all()


# ------------------------------------------------------------------------------------------------------------------------
# diffuse tail
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.TAIL_CASES))
def test_tail_is_held_to_float64_from_the_stored_ism_part(dev, name):
    case, tdiff, tmax, seed, branch = R.TAIL_CASES[name]
    src, rcv, nb, _, c = R.ISM_CASES[case]
    nism, ns = R.sample_counts(tdiff, tmax, R.FS)
    got = device_rir(case, tmax, tdiff, seed)
    assert got.shape == (len(src), len(rcv), ns)
    want, lines = R.tail(got[:, :, :nism], R.ROOM, R.BETA, src, rcv, ns, R.FS, c, seed)
    branches = {ln[2] for row in lines for ln in row}
    print("tail", name, "branches", branches, "line of RIR (0, 0)", lines[0][0])
    assert branches == {branch}
    held("tail/" + name, got[:, :, nism:], want, "tail/" + name)
    # the same seed: the same bits; another seed: another tail, the same image-source part
    again = device_rir(case, tmax, tdiff, seed)
    other = device_rir(case, tmax, tdiff, seed + 1)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    assert np.array_equal(got[:, :, :nism].view(np.uint32), other[:, :, :nism].view(np.uint32))
    assert np.abs(got[:, :, nism:] - other[:, :, nism:]).max() > 0.1 * np.abs(got[:, :, nism:]).max()
    # the image-source part is what the call without a tail gives
    assert np.array_equal(got[:, :, :nism].view(np.uint32), device_rir(case, None, tdiff).view(np.uint32))
    # normalised by its own envelope the tail is unit-variance noise (bounds: rir_ref.noise_bounds, checked for these seeds
    # on the CPU by tests/test_rir_ref_host.py)
    t = np.arange(nism, ns)
    mb, vb = R.noise_bounds(ns - nism)
    for s in range(len(src)):
        for r in range(len(rcv)):
            a, b, _ = lines[s][r]
            xi = got[s, r, nism:].astype(np.float64) / np.exp(0.5 * (a + b * t))
            assert abs(xi.mean()) <= mb and abs(xi.var() - 1) <= vb, (s, r, xi.mean(), xi.var())


# ------------------------------------------------------------------------------------------------------------------------
# moving-source mixing
# ------------------------------------------------------------------------------------------------------------------------
TS = {1: [0.0], 3: [0.0, 0.011, 0.0431], 7: [0.0, 0.004, 0.0101, 0.0101, 0.027, 0.04, 0.0555]}     # ragged, one repeated


def int_case(npts, length, m, seed):
    rs = np.random.RandomState(seed)
    return (rs.randint(-3, 4, 1001).astype(np.float32), rs.randint(-3, 4, (npts, m, length)).astype(np.float32))


@pytest.mark.parametrize("npts", [1, 3, 7])
@pytest.mark.parametrize("length", [1, 17, 300])
@pytest.mark.parametrize("m", [1, 5])
def test_trajectory_is_exact_on_integer_inputs(dev, npts, length, m):
    import fnssl.rir as gpuRIR
    x, rirs = int_case(npts, length, m, 100 * npts + length + m)
    want = R.trajectory(x, rirs, TS[npts], R.FS)
    got = gpuRIR.simulateTrajectory(x, rirs, timestamps=np.array(TS[npts]), fs=R.FS)
    assert got.shape == (1001 + length - 1, m) and got.dtype == np.float32
    assert np.abs(want).max() < 2 ** 24 and np.array_equal(got.astype(np.float64), want)
    if npts == 7:
        want = R.trajectory(x, rirs)
        assert np.array_equal(gpuRIR.simulateTrajectory(x, rirs).astype(np.float64), want)      # timestamps=None


def test_trajectory_batch_equals_one_by_one(dev):
    import fnssl.rir as gpuRIR
    cases = [(7, 300, 5), (3, 17, 5), (7, 300, 1), (1, 1, 2), (3, 300, 2), (7, 17, 4)]
    xs, rs, ts = [], [], []
    for i, (npts, length, m) in enumerate(cases):
        x, r = int_case(npts, length, m, 900 + i)
        xs.append(torch.from_numpy(x[:1001 - 20 * i].copy()).to(dev))
        rs.append(torch.from_numpy(r).to(dev))
        ts.append(np.array(TS[npts]))
    batch = gpuRIR.simulateTrajectoryBatch(xs, rs, ts, R.FS)
    assert len(batch) == len(cases)
    for x, r, t, y in zip(xs, rs, ts, batch):
        one = gpuRIR.simulateTrajectory(x, r, t, R.FS)
        assert y.is_cuda and torch.equal(y, one)
        assert np.array_equal(y.cpu().numpy().astype(np.float64), R.trajectory(x.cpu().numpy(), r.cpu().numpy(), t, R.FS))


def test_trajectory_random_leg_at_its_gate(dev):
    import fnssl.rir as gpuRIR
    x, rirs, ts = R.traj_random_case()
    x, rirs = x.astype(np.float32), rirs.astype(np.float32)
    got = gpuRIR.simulateTrajectory(x, rirs, ts, R.FS)
    held("traj/random", got, R.trajectory(x, rirs, ts, R.FS), "traj/random")
    assert np.array_equal(got, gpuRIR.simulateTrajectory(x, rirs, ts, R.FS))


# ------------------------------------------------------------------------------------------------------------------------
# the calls AcousticScene.simulate() makes
# ------------------------------------------------------------------------------------------------------------------------
def scene(gpuRIR, to):
    """Two moving sources: full and direct-path RIRs along each trajectory, the mixing of each, the VAD trajectory call."""
    rs = np.random.RandomState(77)
    npts, nsamp = 3, 1001
    mic = to(np.array(R.RCV[:2]))
    beta = gpuRIR.beta_SabineEstimation(R.ROOM, 0.35)
    tdiff = gpuRIR.att2t_SabineEstimator(12, 0.35)
    nb_img = gpuRIR.t2n(0.02, R.ROOM)
    timestamps = np.arange(npts) * nsamp / R.FS / npts
    out = {"mix": 0, "dp": 0}
    for k in range(2):
        traj = to(np.linspace(R.SRC[k], R.SRC[k + 1], npts))
        sig = to(rs.standard_normal(nsamp).astype(np.float32))
        vad = to((rs.rand(nsamp) > 0.4).astype(np.float32))
        rirs = gpuRIR.simulateRIR(R.ROOM, beta, traj, mic, nb_img, 0.06, R.FS, Tdiff=min(tdiff, 0.03), seed=3 + k)
        dp_rirs = gpuRIR.simulateRIR(R.ROOM, beta, traj, mic, [1, 1, 1], 0.03, R.FS)
        out["mix"] = out["mix"] + gpuRIR.simulateTrajectory(sig, rirs, timestamps=timestamps, fs=R.FS)
        out["dp"] = out["dp"] + gpuRIR.simulateTrajectory(sig, dp_rirs, timestamps=timestamps, fs=R.FS)
        out["vad%d" % k] = gpuRIR.simulateTrajectory(vad, dp_rirs, timestamps=timestamps, fs=R.FS)
        out["rirs%d" % k] = rirs
    return out


def test_scene_calls_numpy_and_device_tensors_agree(dev):
    import fnssl.rir as gpuRIR
    host = scene(gpuRIR, lambda a: a)
    on_dev = scene(gpuRIR, lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev))
    assert host["mix"].shape == (1001 + 960 - 1, 2) and host["dp"].shape == (1001 + 480 - 1, 2)
    for k, v in host.items():
        assert isinstance(v, np.ndarray) and isinstance(on_dev[k], torch.Tensor) and on_dev[k].is_cuda, k
        assert np.isfinite(v).all() and np.abs(v).max() > 0
        assert np.array_equal(v, on_dev[k].cpu().numpy()), k
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        gpuRIR.simulateTrajectory(torch.zeros(8), torch.zeros(1, 1, 4))
