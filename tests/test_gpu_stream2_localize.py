"""GPU tests of online localisation with IPDnet2 (fnssl/stream.py: CentredStreamFrontEnd + OnlineLocalizer;
``IPDnet2.run_step.MyModel.predict_stream``): microphone samples pushed in ragged chunks give, group by group, the bits
``OnlineSpatialNet.forward_stream`` gives on the whole-signal features cut into the same groups (torch.equal: the streamed
front end is bit-identical to ``ops.preprocess_ipdnet2``, tests/test_gpu_stream2_frontend.py), and ``predict_step``'s
whole-signal prediction within the figure tests/test_gpu_ipdnet2.py holds ``forward_stream`` to (rtol 1e-5, atol 1e-5, fp32
and bf16).  The shipped network: 5 microphones, 8 layers, deterministic weights.  Run with -m gpu."""
import numpy as np
import pytest

from conftest import assert_close, rs_randn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NS23 = 320 * 22 + 100                                    # 23 frames: four groups of 5, the last three frames are dropped
NS25 = 320 * 24 + 3                                      # 25 frames: the fifth group holds the end-reflected frame
HEAD = [256, 1, 0, 1400, 3300, 64]                       # groups completed: 0, 0, 0, 1, 2, 0; then the rest completes 1
MICS5 = np.array(((0.0, 0.0, 0.0), (0.04, 0.0, 0.0), (0.0, 0.04, 0.0), (-0.04, 0.0, 0.0), (0.0, -0.04, 0.0)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


def build_model(dev, bf16=False):
    from IPDnet2.run_step import MyModel
    from fnssl import weights as W
    m = MyModel(device="cuda:0")
    m.arch.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in W.make_ipdnet2_state(8100).items()})
    if bf16:
        m.arch = m.arch.bfloat16()
    return m.to(dev).eval()


_models = {}


def model_of(dev, bf16):
    if bf16 not in _models:
        _models[bf16] = build_model(dev, bf16)
    return _models[bf16]


def chunks_of(ns):
    return HEAD + [ns - sum(HEAD)]


class Recorder:
    """Records the frame count of every ``forward_stream`` call of ``arch`` while active."""

    def __init__(self, arch):
        self.arch, self.sizes = arch, []

    def __enter__(self):
        orig = self.arch.forward_stream

        def recording(x, state=None):
            if x.shape[3]:                                # the localizer's zero-frame probe is no group
                self.sizes.append(x.shape[3])
            return orig(x, state)

        self.arch.forward_stream = recording
        return self.sizes

    def __exit__(self, *exc):
        del self.arch.forward_stream


def replay(arch, sig, sizes):
    """``forward_stream`` on the whole-signal features [1, 10, 256, nt], cut into groups of ``sizes`` frames."""
    from fnssl import ops
    feats = ops.preprocess_ipdnet2(sig, frame_major=True)
    st, outs, t0 = None, [], 0
    for n in sizes:
        o, st = arch.forward_stream(feats[..., t0:t0 + n], st)
        outs.append(o)
        t0 += n
    return outs


@pytest.mark.parametrize("ns", [NS23, NS25], ids=["23frames", "25frames"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_predict_stream_equals_forward_stream_and_predict_step(dev, bf16, ns):
    model = model_of(dev, bf16)
    batch = torch.from_numpy(rs_randn(8101, (1, 5, ns), 0.05)).to(dev)
    whole = model.predict_step(batch, 0)                                   # utterance 0: [nt // 5, 512, 4, 2]
    groups = (ns // 320 + 1) // 5
    assert tuple(whole.shape) == (groups, 512, 4, 2)
    sizes_in = chunks_of(ns)
    with Recorder(model.arch) as sizes:
        state, preds, lo = None, [], 0
        for i, n in enumerate(sizes_in):
            pred, state = model.predict_stream(batch[:, :, lo:lo + n], state, last=(i == len(sizes_in) - 1))
            lo += n
            preds.append(pred)
    assert lo == ns and state.frontend.finished and state.frontend.frames == 5 * groups
    assert [p is not None for p in preds] == [False, False, False, True, True, False, True]     # 3 of 7 pushes
    finish_groups = groups - 4                                             # 23 frames: finish completes none; 25: one
    assert sizes == [5, 10, 5] + [5] * finish_groups
    assert [p.shape[0] for p in preds if p is not None] == [1, 2, 1 + finish_groups]
    got = torch.cat([p for p in preds if p is not None], dim=0)
    assert tuple(got.shape) == tuple(whole.shape) and got.dtype == whole.dtype
    want = torch.cat(replay(model.arch, batch.permute(0, 2, 1), sizes), dim=1)[0]
    assert torch.equal(got, want)
    assert_close(got.float().cpu().numpy(), whole.float().cpu().numpy(), 1e-5, 1e-5,
                 "predict_stream vs predict_step (%s)" % ("bf16" if bf16 else "fp32"))


def test_doa_of_the_stream_equals_doa_of_the_replayed_predictions_and_reset(dev):
    """``localize`` = the MSE template search behind ``IPDnet2.Module.PredDOA``: DOA, activity and spectrum of every
    streamed group equal the search applied to the replayed ``forward_stream`` predictions; after ``reset()`` a second
    pass gives the same bits."""
    from IPDnet2.Module import PredDOA
    from fnssl import stream
    model = model_of(dev, False)
    pd = PredDOA(mic_location=MICS5, dev="cuda:0")
    entry = lambda p: pd._search(p[..., :2], 1)                            # noqa: E731
    sig = torch.from_numpy(rs_randn(8101, (1, 5, NS25), 0.05)).to(dev).permute(0, 2, 1)
    loc = stream.OnlineLocalizer(model.arch, stream.CentredStreamFrontEnd(5), localize=entry)

    def one_pass():
        outs, lo = [], 0
        for n in chunks_of(NS25):
            outs.append(loc.push(sig[:, lo:lo + n]))
            lo += n
        outs.append(loc.finish())
        return [o for o in outs if o[0] is not None]

    with torch.no_grad():
        first = one_pass()
        sizes = [5 * pred.shape[1] for pred, _ in first]
        assert sizes == [5, 10, 5, 5]
        want = replay(model.arch, sig, sizes)
        for (pred, doa), w in zip(first, want):
            assert torch.equal(pred, w)
            wdoa = entry(w)
            assert tuple(doa[0].shape) == (2, 1, w.shape[1], 2, 1) and tuple(doa[1].shape) == (2, 1, w.shape[1], 1)
            assert all(torch.equal(a, b) for a, b in zip(doa, wdoa))
        with pytest.raises(RuntimeError, match="has been finished"):
            loc.push(sig[:, :100])
        loc.reset()
        assert loc.state is None and loc.frontend.frames == 0
        for (pred, doa), (pred2, doa2) in zip(first, one_pass()):
            assert torch.equal(pred, pred2) and all(torch.equal(a, b) for a, b in zip(doa, doa2))


def test_train_mode_is_refused(dev):
    model = build_model(dev).train()
    with pytest.raises(RuntimeError, match=r"call \.eval\(\) first"):
        model.predict_stream(torch.zeros((1, 5, 4000), device=dev))
