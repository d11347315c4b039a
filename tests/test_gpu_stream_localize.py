"""GPU tests of online localisation (fnssl/stream.py: OnlineLocalizer; ``predict_stream`` of the two Lightning
drop-ins): microphone samples pushed in ragged chunks give, segment by segment, the bits ``predict_step`` gives on the
whole signal, and the DOA entry of each model applied to the streamed predictions gives what it gives on the
whole-signal prediction.  torch.equal throughout: the streamed front end and ``forward_stream`` are each bit-identical
to their whole-signal counterparts (tests/test_gpu_stream_frontend.py, tests/test_gpu_parity.py).  Run with -m gpu."""
import numpy as np
import pytest

from conftest import rs_randn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FRAMES = 48
NS = 512 + 256 * (FRAMES - 1)
CHUNKS = [300, 100, 0, 3000, 3072, 700, NS - 7172]           # segments completed: 0, 0, 0, 1, 1, 0, 2
MICS4 = np.array(((-0.04, 0.0, 0.0), (0.04, 0.0, 0.0), (0.0, 0.05, 0.01), (0.02, -0.03, 0.0)), dtype=np.float32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


def fnssl_model(dev):
    import predict_step as ps
    from fnssl import weights as W
    model = ps.MyModel(device="cuda:0")
    model.arch.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in W.make_fnssl_state(6100).items()})
    return model.to(dev).eval()


def ipdnet_model(dev):
    from IPDnet.FixedAarryIPDnet import IPDnet
    from IPDnet.train_step import MyModel
    from fnssl import weights as W
    net = IPDnet(8, 256, 2, True)
    net.load_state_dict({k: torch.from_numpy(np.array(v, dtype=np.float32))
                         for k, v in W.make_ipdnet_state(6200, 8, 256, 2, True).items()})
    return MyModel(arch=net, mic_pos=torch.from_numpy(MICS4), device="cuda:0").to(dev).eval()


def push_all(push, batch):
    """batch [nb, nch, NS] through ``push`` in CHUNKS; the outputs that are not None, and how many pushes gave one."""
    outs, lo = [], 0
    for n in CHUNKS:
        outs.append(push(batch[:, :, lo:lo + n]))
        lo += n
    assert lo == NS
    return [o for o in outs if o is not None], sum(o is not None for o in outs)


def test_fnssl_predict_stream_equals_predict_step(dev):
    model = fnssl_model(dev)
    batch = torch.from_numpy(rs_randn(6101, (1, 2, NS), 0.05)).to(dev)
    whole = model.predict_step(batch, 0)                                   # [1, 4, 512]
    assert tuple(whole.shape) == (1, FRAMES // 12, 512)
    state = [None]

    def push(chunk):
        pred, state[0] = model.predict_stream(chunk, state[0])
        return pred

    preds, calls = push_all(push, batch)
    assert calls == 3 and [p.shape[1] for p in preds] == [1, 1, 2]        # of seven pushes
    assert state[0].frontend.frames == FRAMES and state[0].state["frames"] == FRAMES
    assert torch.equal(torch.cat(preds, dim=1), whole)


def test_ipdnet_predict_stream_equals_predict_step(dev):
    model = ipdnet_model(dev)
    batch = torch.from_numpy(rs_randn(6201, (1, 4, NS), 0.05)).to(dev)
    whole = model.predict_step(batch, 0)                                   # utterance 0: [4, 512, 3, 2]
    assert tuple(whole.shape) == (FRAMES // 12, 512, 3, 2)
    state = [None]

    def push(chunk):
        pred, state[0] = model.predict_stream(chunk, state[0])
        return pred

    preds, calls = push_all(push, batch)
    assert calls == 3 and [p.shape[0] for p in preds] == [1, 1, 2]
    assert torch.equal(torch.cat(preds, dim=0), whole)


def test_doa_of_the_stream_equals_doa_of_the_whole_signal(dev):
    """``localize`` = each model's prediction -> DOA entry: the template search behind ``Module.PredDOA`` (FN-SSL) and the
    track localisation of ``IPDnet.Module.PredDOA`` (IPDnet).  Both work frame by frame on the prediction, so the DOAs of
    the streamed segments are those of the whole-signal prediction."""
    from fnssl import stream
    model = fnssl_model(dev)
    batch = torch.from_numpy(rs_randn(6101, (1, 2, NS), 0.05)).to(dev)
    entry = lambda pred: model.get_metric.predgt2DOA(pred_batch=pred)[0]               # noqa: E731
    loc = stream.OnlineLocalizer(model.arch, stream.StreamFrontEnd("pair", 2, model.ch_mode), localize=entry)
    got, _ = push_all(lambda c: loc.push(c.permute(0, 2, 1))[1], batch)
    want = entry(model.predict_step(batch, 0))
    assert tuple(want["doa"].shape) == (1, FRAMES // 12, 2, 1)
    for key in ("doa", "vad_sources", "spatial_spectrum"):
        assert torch.equal(torch.cat([g[key] for g in got], dim=1), want[key]), key

    imodel = ipdnet_model(dev)
    ibatch = torch.from_numpy(rs_randn(6201, (1, 4, NS), 0.05)).to(dev)
    iloc = stream.OnlineLocalizer(imodel.arch, stream.StreamFrontEnd("array", 4), localize=imodel.get_metric._localize)
    igot, _ = push_all(lambda c: iloc.push(c.permute(0, 2, 1))[1], ibatch)
    whole = imodel.forward(imodel.data_preprocess(mic_sig_batch=ibatch.permute(0, 2, 1))[0])     # [1, 4, 512, 3, 2]
    doa, vad = imodel.get_metric._localize(whole)
    assert tuple(doa.shape) == (1, FRAMES // 12, 2, 2) and tuple(vad.shape) == (1, FRAMES // 12, 2)
    assert torch.equal(torch.cat([g[0] for g in igot], dim=1), doa)
    assert torch.equal(torch.cat([g[1] for g in igot], dim=1), vad)
    iloc.reset()                                                                               # and again from sample 0
    again, _ = push_all(lambda c: iloc.push(c.permute(0, 2, 1))[0], ibatch)
    assert torch.equal(torch.cat(again, dim=1), whole)


def test_modules_that_do_not_stream_are_rejected(dev):
    import Model
    import predict_step as ps
    from IPDnet.FixedAarryIPDnet import IPDnet
    from IPDnet.train_step import MyModel
    chunk = torch.zeros((1, 2, 4000), device=dev)
    off = ps.MyModel(device="cuda:0")
    off.arch = Model.FN_SSL(is_online=False)
    with pytest.raises(RuntimeError, match="only the online model"):
        off.to(dev).eval().predict_stream(chunk)
    bf = ps.MyModel(device="cuda:0")
    bf.arch = bf.arch.bfloat16()
    with pytest.raises(RuntimeError, match="fp32 model only"):
        bf.to(dev).eval().predict_stream(chunk)
    chunk4 = torch.zeros((1, 4, 4000), device=dev)
    for arch in (IPDnet(8, 256, 2, False), IPDnet(8, 256, 2, True).bfloat16()):
        m = MyModel(arch=arch, mic_pos=torch.from_numpy(MICS4), device="cuda:0").to(dev).eval()
        with pytest.raises(RuntimeError, match="online fp32 model only"):
            m.predict_stream(chunk4)
