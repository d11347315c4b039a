"""GPU tests of the label stage: fnssl_scene_doa_batch, fnssl_scene_segment_batch, fnssl_scene_pack_batch and
fnssl.scene.trajectory_doa / Segmenting_SRPDNN / segment_batch / training_batch over them.

The truth is tests/labels_ref.py in ``np.longdouble``; a device angle may lie ``labels_ref.GATE`` (8) times as far from it as
the float64 restatement, the reference's own arithmetic, does (``labels_ref.D64``, pinned and re-measured by
tests/test_labels_ref_host.py, which also asserts that no wrap decision of these cases can flip under rounding, so azimuths
are compared directly).  VADs, counts and the padded signals are exact.  Run with -m gpu on an MI355X."""
import types

import numpy as np
import pytest

import labels_ref as R
from conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


def up(a, dev, dtype=None):
    a = np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a).to(dev)


def gate(name, got, truth, what):
    d = R.dist(got, truth)
    bound = R.GATE * R.D64[name]
    print("CHECK %-34s %-10s device %.3e from longdouble, float64 %.3e, bound %.3e" % (name, what, d, R.D64[name], bound))
    assert d <= bound, (name, what, d, bound)
    return d


# ------------------------------------------------------------------------------------------------------------------------
# trajectory_doa
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.TRAJ_CASES))
def test_trajectory_doa_against_longdouble(dev, name):
    from fnssl import scene
    pts, ts, n, fs, pos = R.traj_case(name)
    want_t, want_d = R.trajectory_doa(pts, ts, n, fs, pos, dtype=R.LD)
    traj, doa = scene.trajectory_doa(pts, ts, n, fs, pos)
    assert isinstance(traj, np.ndarray) and traj.dtype == np.float64 and traj.shape == (n, 3, pts.shape[2])
    assert isinstance(doa, np.ndarray) and doa.dtype == np.float64 and doa.shape == (n, 2, pts.shape[2])
    gate("traj/" + name, traj, want_t, "trajectory")
    gate("doa/" + name, doa, want_d, "DOA")
    # both clamps: the samples before the first and after the last timestamp hold the end points
    t = np.arange(n) / fs
    assert np.array_equal(traj[t < ts[0]], np.broadcast_to(pts[0], ((t < ts[0]).sum(),) + pts[0].shape))
    assert np.array_equal(traj[t > ts[-1]], np.broadcast_to(pts[-1], ((t > ts[-1]).sum(),) + pts[-1].shape))
    # tensors in, tensors out, the same bits
    t2, d2 = scene.trajectory_doa(up(pts, dev), up(ts, dev), n, fs, pos)
    assert t2.is_cuda and d2.dtype == torch.float64 and np.array_equal(t2.cpu().numpy(), traj) and np.array_equal(d2.cpu().numpy(), doa)


# ------------------------------------------------------------------------------------------------------------------------
# segmenting
# ------------------------------------------------------------------------------------------------------------------------
def label_scene(case, dev, m=2, seed=0, conv=None, with_dp=True):
    """A scene of ``segment_batch`` from a labels_ref case (no simulation) and its signal [L, M]."""
    conv = (lambda a: up(a, dev)) if conv is None else conv
    L, _, nsrc = case["DOA"].shape
    rs = np.random.RandomState(500 + seed)
    dp = rs.standard_normal((L, m, nsrc)).astype(np.float32)
    sc = types.SimpleNamespace(DOA=conv(case["DOA"]), mic_vad_sources=conv(case["mic_vad_sources"]), mic_vad=conv(case["mic_vad"]),
                               dp_mic_signals_sources=conv(dp), fs=case["fs"])
    return sc, conv(rs.standard_normal((L, m)).astype(np.float32)), dp


def check_gts_row(name, row, case, shape, smax, dp, doa_truth=None):
    """One scene's rows of ``gts`` (numpy) against the restatement: angles at the gate, the rest exact."""
    L, K, step = shape
    nsrc = case["DOA"].shape[2]
    want = R.transform(L, case, K, step, dtype=R.LD)
    if name is not None:
        gate(name, row["doa"][:, :, :nsrc], want["DOAw"] if doa_truth is None else doa_truth, "DOAw")
    assert row["doa"].dtype == np.float64 and not row["doa"][:, :, nsrc:].any()
    assert row["vad_sources"].dtype == np.uint8 and np.array_equal(row["vad_sources"][:, :, :nsrc], want["mic_vad_sources"])
    assert not row["vad_sources"][:, :, nsrc:].any()
    assert np.array_equal(row["mic_vad"], want["mic_vad"])
    assert row["vad_count"].dtype == np.int32 and np.array_equal(row["vad_count"], row["vad_sources"].sum(axis=1))
    assert row["dp_signal"].dtype == np.float32 and np.array_equal(row["dp_signal"][:, :, :nsrc], dp) and not row["dp_signal"][:, :, nsrc:].any()
    assert row["doa"].shape == (R.num_windows(*shape), 2, smax) and row["vad_sources"].shape == (R.num_windows(*shape), K, smax)


def rows(gts, b):
    return {k: gts[k][b].cpu().numpy() for k in ("doa", "vad_sources", "vad_count", "dp_signal", "mic_vad")}


@pytest.mark.parametrize("shape", R.SEG_SHAPES, ids=R.seg_name)
def test_segmenting_against_longdouble(dev, shape):
    from fnssl import scene
    case = R.seg_case(*shape)
    sc, mic, dp = label_scene(case, dev)
    gts = scene.segment_batch(mic[None], [sc], shape[1], shape[2])
    assert gts["doa"].is_cuda and gts["num_source"].tolist() == [4] and gts["array_setup"] is None
    check_gts_row("seg/" + R.seg_name(shape), rows(gts, 0), case, shape, 4, dp)
    nw = R.num_windows(*shape)
    az = gts["doa"][0, nw // 2, 1].cpu().numpy()
    assert az[0] < 0 < az[1] and az[2] < 0 and abs(az[3] - 0.7) < 1e-12           # fold taken, not taken, negative, static
    if nw > 1:
        assert not gts["vad_count"][0, -1].any().item() and gts["vad_count"][0, 0, 3].item() == shape[1]


# ------------------------------------------------------------------------------------------------------------------------
# padding and batching
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 3])
def test_padding_to_max_source(dev, m):
    """1, 2 and 1 sources padded to 2 and to 4.  L is odd: with M = 3 and max_source 2 a scene is 6522 floats, no multiple of 4,
    and the plain stores run; every other combination takes the float4 stores."""
    from fnssl import scene
    shape = (1087, 257, 129)
    full = R.seg_case(*shape)
    cases = [R.sub_scene(full, src) for src in ((2,), (0, 1), (3,))]
    made = [label_scene(c, dev, m=m, seed=k) for k, c in enumerate(cases)]
    mics = torch.stack([x[1] for x in made])
    for smax in (None, 2, 4):
        gts = scene.segment_batch(mics, [x[0] for x in made], shape[1], shape[2], max_source=smax)
        assert gts["num_source"].tolist() == [1, 2, 1] and tuple(gts["dp_signal"].shape) == (3, 1087, m, smax or 2)
        for b in range(3):
            check_gts_row(None, rows(gts, b), cases[b], shape, smax or 2, made[b][2])
            want = R.segment_doa(cases[b]["DOA"], *shape, dtype=R.LD)
            assert R.dist(gts["doa"][b, :, :, :want.shape[2]].cpu().numpy(), want) <= R.GATE * R.D64["seg/" + R.seg_name(shape)]
    with pytest.raises(ValueError, match=r"scene 1: 2 sources \(1 \.\. max_source = 1\)"):
        scene.segment_batch(mics, [x[0] for x in made], shape[1], shape[2], max_source=1)
    # separate per-source signals pack to the same bits as the stacked tensor
    from fnssl import ops
    lists = [[x[0].dp_mic_signals_sources[:, :, s].contiguous() for s in range(x[0].dp_mic_signals_sources.shape[2])] for x in made]
    assert torch.equal(ops.scene_pack_batch(lists, 1087, m, 4), gts["dp_signal"])


def test_a_second_descriptor_block_and_two_runs(dev):
    """25 tiny scenes (no simulation): the 25th travels in a second launch; every scene equals itself segmented alone, and a
    second run gives the same bits."""
    from fnssl import scene
    L, K, step = 96, 20, 13
    made = []
    for b in range(25):
        nsrc = 1 + b % 3
        rs = np.random.RandomState(b)
        case = {"DOA": np.stack([rs.uniform(0.1, 3.0, (L, nsrc)), rs.uniform(-3.1, 3.1, (L, nsrc))], axis=1),
                "mic_vad_sources": rs.randint(0, 2, (L - b, nsrc)).astype(bool), "fs": R.FS}
        case["mic_vad"] = case["mic_vad_sources"].any(axis=1)
        made.append(label_scene(case, dev, seed=b))
    mics, scenes = torch.stack([x[1] for x in made]), [x[0] for x in made]
    gts = scene.segment_batch(mics, scenes, K, step, max_source=3)
    again = scene.segment_batch(mics, scenes, K, step, max_source=3)
    keys = ("doa", "vad_sources", "vad_count", "dp_signal", "mic_vad", "num_source")
    for k in keys:
        assert torch.equal(gts[k], again[k]), k
    for b in (0, 1, 11, 23, 24):
        alone = scene.segment_batch(mics[b:b + 1], scenes[b:b + 1], K, step, max_source=3)
        for k in keys:
            assert torch.equal(gts[k][b], alone[k][0]), (b, k)
    assert gts["num_source"].tolist() == [1 + b % 3 for b in range(25)]
    want = R.segment_doa(made[24][0].DOA.cpu().numpy(), L, K, step, dtype=R.LD)   # random azimuths: windows that unwrap and fold
    assert R.dist(gts["doa"][24, :, :, :1].cpu().numpy(), want) < 1e-13


def test_array_pos_computes_the_doa_on_the_device(dev):
    """With ``array_pos`` the DOA comes from traj_pts / timestamps and ``scene.DOA`` may be None: the rows equal those of the
    same scenes with ``trajectory_doa``'s DOA uploaded."""
    from fnssl import scene
    made, poss = [], []
    for k, name in enumerate(("p3_s2", "p50_s1", "p50_s2")):
        pts, ts, n, fs, pos = R.traj_case(name)
        _, doa = scene.trajectory_doa(pts, ts, n, fs, pos)
        rs = np.random.RandomState(70 + k)
        case = {"DOA": doa, "mic_vad_sources": rs.randint(0, 2, (n - 7 * k, pts.shape[2])).astype(bool), "fs": fs}
        case["mic_vad"] = case["mic_vad_sources"].any(axis=1)
        sc, mic, _ = label_scene(case, dev, seed=k)
        sc.traj_pts, sc.timestamps, sc.t = up(pts, dev), ts, np.arange(n) / fs
        made.append((sc, mic))
        poss.append(pos + 0.0)
    mics, scenes = torch.stack([x[1] for x in made]), [x[0] for x in made]
    with_doa = scene.segment_batch(mics, scenes, 100, 37)
    for sc in scenes:
        sc.DOA = None
    on_device = scene.segment_batch(mics, scenes, 100, 37, array_pos=poss)
    for k in ("doa", "vad_sources", "vad_count", "dp_signal"):
        assert torch.equal(with_doa[k], on_device[k]), k
    assert with_doa["doa"].abs().max().item() > 3.0                               # a window mean near pi: the path behind the array


# ------------------------------------------------------------------------------------------------------------------------
# G24 on the device
# ------------------------------------------------------------------------------------------------------------------------
def unpack(bits, shape):
    return np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape).astype(np.float64)


@pytest.mark.parametrize("k", range(len(R.GOLDEN_SEG)))
def test_golden_transform_on_the_device(dev, k):
    """Segmenting_SRPDNN.__call__ on a numpy scene and segment_batch on the golden inputs against what the real reference
    recorded: the angles at the gate from the longdouble truth, and (triangle inequality) at GATE + 1 from the record, which is
    the float64 arithmetic; VADs and tw exact, numpy float64 back."""
    from fnssl import scene
    g = load_golden("g24_labels")
    shape, sources = R.GOLDEN_SEG[k]
    name = "seg/" + R.seg_name(shape)
    case = R.sub_scene(R.seg_case(*shape), sources)
    key = "b_%d" % k
    assert np.array_equal(R.digest(case["DOA"], case["mic_vad_sources"], case["mic_vad"]), g[key + "_in"])
    vshape = tuple(g[key + "_vad_shape"])
    sc = types.SimpleNamespace(DOA=case["DOA"].copy(), mic_vad_sources=case["mic_vad_sources"].copy(), mic_vad=case["mic_vad"].copy(), fs=case["fs"])
    x = np.zeros((shape[0], 2), dtype=np.float32)
    x2, sc2 = scene.Segmenting_SRPDNN(shape[1], shape[2])(x, sc)
    assert x2 is x and sc2 is sc
    for a in (sc.DOAw, sc.mic_vad, sc.mic_vad_sources, sc.tw):
        assert isinstance(a, np.ndarray) and a.dtype == np.float64
    truth = R.segment_doa(case["DOA"], *shape, dtype=R.LD)
    gate(name, sc.DOAw, truth, "golden")
    assert sc.DOAw.shape == g[key + "_DOAw"].shape and R.dist(sc.DOAw, g[key + "_DOAw"]) <= (R.GATE + 1) * R.D64[name]
    assert np.array_equal(sc.mic_vad, unpack(g[key + "_mic_vad"], vshape[:2]))
    assert np.array_equal(sc.mic_vad_sources, unpack(g[key + "_mic_vad_sources"], vshape))
    assert np.array_equal(sc.tw, g[key + "_tw"])
    lsc, mic, dp = label_scene(case, dev, conv=lambda a: a)                       # numpy in every scene: numpy out
    gts = scene.segment_batch(mic[None], [lsc], shape[1], shape[2])
    assert isinstance(gts["doa"], np.ndarray) and np.array_equal(gts["doa"][0], sc.DOAw)
    assert np.array_equal(gts["vad_sources"][0].astype(np.float64), sc.mic_vad_sources) and np.array_equal(gts["dp_signal"][0], dp)


# ------------------------------------------------------------------------------------------------------------------------
# drop-in and end to end (simulated scenes)
# ------------------------------------------------------------------------------------------------------------------------
ROOM = [4.0, 5.0, 3.0]
CENTRE = np.asarray(ROOM) * [0.5, 0.45, 0.4]
MICS = np.array([[-0.04, 0.0, 0.0], [0.04, 0.0, 0.0]])


def sim_scene(k, nsrc, n, dev):
    """An anechoic scene of ``simulate_batch`` in device tensors, with the DOA ``getRandomScene`` would give it (numpy)."""
    rs = np.random.RandomState(2400 + k)
    env = (np.sin(np.arange(n) / (250.0 + 30 * k)) > -0.5).astype(np.float64)
    pts = (rs.uniform(0.2, 0.8, (4, 3, nsrc)) * np.asarray(ROOM)[None, :, None]).astype(np.float32)
    ts = np.arange(4) * n / R.FS / 4
    _, doa = R.trajectory_doa(pts.astype(np.float64), ts, n, R.FS, CENTRE)
    return types.SimpleNamespace(
        room_sz=ROOM, T60=0, beta=np.zeros(6), SNR=20.0, fs=R.FS, noise_signal=up(rs.standard_normal((n, 2)).astype(np.float32), dev),
        source_signal=up((rs.standard_normal((n, nsrc)) * env[:, None] * 0.3).astype(np.float32), dev),
        array_setup=types.SimpleNamespace(mic_orV=None, mic_pattern="omni", mic_pos=MICS), mic_pos=up((CENTRE + MICS).astype(np.float32), dev),
        timestamps=ts, traj_pts=up(pts, dev), t=np.arange(n) / R.FS, c=343.0, DOA=doa,
        source_vad=up(np.stack([(np.sin(np.arange(n) / (200.0 + 25 * s)) > -0.2) for s in range(nsrc)], axis=1).astype(np.float32), dev))


class StubDataset:
    """``with_pos``: the scenes carry ``array_pos``, so ``training_batch`` computes their DOA on the device."""

    def __init__(self, dev, n, sources, transforms=None, with_pos=False):
        self.dev, self.n, self.sources, self.transforms, self.with_pos, self.made = dev, n, sources, transforms, with_pos, []

    def getRandomScene(self, idx):
        sc = sim_scene(idx, self.sources[idx], self.n, self.dev)
        if self.with_pos:
            sc.array_pos = CENTRE.copy()
        self.made.append(sc)
        return sc


def test_the_transform_drops_into_get_batch(dev):
    from fnssl import scene
    n, K, step = 1536, 512, 384
    ds = StubDataset(dev, n, [1, 2], transforms=[scene.Segmenting_SRPDNN(K, step)])
    np.random.seed(24)
    mic, scenes = scene.get_batch(ds, 0, 2)
    ref = StubDataset(dev, n, [1, 2])
    np.random.seed(24)
    mic2, plain = scene.get_batch(ref, 0, 2)
    assert torch.equal(mic, mic2)
    gts = scene.segment_batch(mic2, plain, K, step, max_source=2)
    nw = scene.num_windows(n, K, step)
    for b, sc in enumerate(scenes):
        ns = b + 1
        assert sc.DOAw.is_cuda and sc.DOAw.dtype == torch.float64 and torch.equal(sc.DOAw, gts["doa"][b, :, :, :ns])
        assert sc.mic_vad_sources.dtype == torch.uint8 and torch.equal(sc.mic_vad_sources, gts["vad_sources"][b, :, :, :ns])
        assert torch.equal(sc.mic_vad, gts["mic_vad"][b]) and tuple(sc.mic_vad.shape) == (nw, K)
        assert np.array_equal(sc.tw, np.arange(0, n - K, step) / R.FS) and sc.mic_vad_sources.any().item()
        want = R.segment_doa(plain[b].DOA, n, K, step, dtype=R.LD)
        assert R.dist(sc.DOAw.cpu().numpy(), want) < 1e-13
    assert gts["array_setup"].shape == (2, 2, 3) and gts["num_source"].tolist() == [1, 2]


def host_gts(scenes, n, K, step, dev):
    """The gts of the same simulated scenes built on the host by labels_ref in float64, uploaded."""
    seg = [R.transform(n, {"DOA": sc.DOA, "mic_vad_sources": sc.mic_vad_sources.cpu().numpy(), "mic_vad": sc.mic_vad.cpu().numpy(),
                           "fs": sc.fs}, K, step) for sc in scenes]
    g = R.gts(seg, [sc.dp_mic_signals_sources.cpu().numpy() for sc in scenes], 2)
    return {"doa": up(g["doa"], dev), "vad_sources": up(g["vad_sources"], dev), "dp_signal": up(g["dp_signal"], dev, np.float32)}, g


def test_training_batch_feeds_both_training_steps(dev):
    """simulate -> labels -> loss with no host round trip of a signal: ``training_batch`` straight into IPDnet's
    ``training_step`` (finite loss with a grad_fn, every .grad filled, equal at 1e-5 to the step fed host-built float64 labels of
    the same scenes: the difference is ``doa`` after ``.float()``), and into FN-SSL's ``data_preprocess``."""
    import predict_step as ps
    from IPDnet.train_step import MyModel
    from fnssl import ops, scene
    K, step, n = 3328, 3072, 6400
    while scene.num_windows(n, K, step) != ops.num_frames(n) // 12:
        n += 256
    assert n == 6400 and scene.num_windows(n, K, step) == 2
    ds = StubDataset(dev, n, [1, 2], with_pos=True)
    np.random.seed(2424)
    mic, gts = scene.training_batch(ds, 0, 2)
    # the same batch from scenes without array_pos: training_batch uploads their DOA instead; the rest is the same bits
    plain = StubDataset(dev, n, [1, 2])
    np.random.seed(2424)
    mic_up, gts_up = scene.training_batch(plain, 0, 2)
    assert torch.equal(mic, mic_up) and all(torch.equal(gts[k], gts_up[k]) for k in ("vad_sources", "vad_count", "dp_signal", "mic_vad"))
    assert R.dist(gts["doa"].cpu().numpy(), gts_up["doa"].cpu().numpy()) < 1e-12   # the angles lie within rounding of each other
    kept = [sc.DOA for sc in ds.made]
    for sc in ds.made:
        sc.DOA = None                                                              # with array_pos the scene's DOA is not read
    again = scene.segment_batch(mic, ds.made, K, step, 2, array_pos=[sc.array_pos for sc in ds.made])
    assert torch.equal(again["doa"], gts["doa"])
    for sc, doa in zip(ds.made, kept):
        sc.DOA = doa
    assert tuple(mic.shape) == (2, n, 2) and mic.is_cuda and tuple(gts["doa"].shape) == (2, 2, 2, 2)
    assert tuple(gts["dp_signal"].shape) == (2, n, 2, 2) and gts["num_source"].tolist() == [1, 2]
    href, g64 = host_gts(ds.made, n, K, step, dev)
    assert torch.equal(gts["vad_sources"], href["vad_sources"].to(torch.uint8)) and torch.equal(gts["dp_signal"], href["dp_signal"])
    assert np.array_equal(gts["vad_count"].cpu().numpy(), g64["vad_count"]) and gts["vad_count"].sum().item() > 0
    assert R.dist(gts["doa"].cpu().numpy(), g64["doa"]) < 1e-12

    torch.manual_seed(2400)
    model = MyModel(arch=None, train_on_device=True, device="cuda:0").to(dev).train()
    model.arch.utt_offset = 0
    fallbacks = ops.cluster_fallbacks(dev)
    model.arch.force_dropout_base = 77
    loss = model.training_step((mic, gts), 0)["loss"]
    assert loss.grad_fn is not None and loss.shape == () and np.isfinite(loss.item())
    loss.backward()
    for k, p in model.arch.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all().item(), k
    model.arch.force_dropout_base = 77
    want = model.training_step((mic, href), 0)["loss"]
    print("CHECK training_step loss %.9g with device labels, %.9g with host float64 labels" % (loss.item(), want.item()))
    assert abs(loss.item() - want.item()) <= 1e-5 + 1e-5 * abs(want.item())
    assert ops.cluster_fallbacks(dev) == fallbacks

    fn = ps.MyModel(device="cuda:0").to(dev)
    count = gts["vad_count"].cpu().numpy()
    data = fn.data_preprocess(mic, dict(gts))
    out = data[1]
    # its own mean of the windows: the exact sum divided by K in float32 (numpy's division; torch divides a tensor by a
    # scalar through the scalar's reciprocal, which is not the same rounding)
    assert np.array_equal(out["vad_sources"].cpu().numpy(), count.astype(np.float32) / np.float32(K))
    assert out["ipd"].shape[:2] == (2, 2) and torch.isfinite(out["ipd"]).all().item()
