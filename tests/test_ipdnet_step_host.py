"""Host-side checks of the IPDnet training step (no GPU): the three entry points of csrc/ipdnet_step.hip are declared,
exported and validate their arguments before touching the device; the numpy Bessel table; the numpy restatements of the
kernels (tests/ipdnet_step_ref.py) against the real reference's golden batch (tests/golden/g19_ipdnet_step.npz) and
against a brute force; the drop-in module constructs without a device."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

import ipdnet_step_ref as R
from conftest import assert_close, load_golden, rs_randn
from fnssl import _lib, ipdnet_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fnssl_pit_mse_workspace_bytes", "fnssl_pit_mse_loss", "fnssl_dp_vad", "fnssl_ipdnet_targets")


def test_step_symbols_declared_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fnssl.h")).read()
    declared = set(re.findall(r"\b(fnssl_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.fnssl_abi_version() == 19


def _pit(lib, pred=64, strides=(64, 32, 4, 2, 1), gt=64, shape=(2, 2, 8, 2, 2), n_total=0, dpred=64, loss=64, ws=64,
         ws_bytes=1 << 20):
    """Every pointer is the never-dereferenced address 64: each call must fail validation before any launch."""
    p = lambda v: C.c_void_p(v) if v else None                                       # noqa: E731
    st = (C.c_longlong * 5)(*strides) if strides is not None else None
    nb, nt2, nf2, nm1, nsrc = shape
    rc = lib.fnssl_pit_mse_loss(p(pred), st, p(gt), nb, nt2, nf2, nm1, nsrc, n_total or nb * nt2 * nf2 * nm1 * nsrc, p(dpred),
                                p(loss), 0, None, p(ws), ws_bytes, None)
    return rc, lib.fnssl_last_error().decode()


def test_pit_mse_validates_before_launch():
    lib = _lib.load()
    assert lib.fnssl_pit_mse_workspace_bytes(1600) >= 1600 * 4 and lib.fnssl_pit_mse_workspace_bytes(0) == 0
    for kw, word in (({"pred": 0}, "null"), ({"gt": 0}, "null"), ({"dpred": 0}, "null"), ({"loss": 0}, "null"),
                     ({"strides": None}, "null"),
                     ({"shape": (2, 2, 8, 2, 0)}, "sources"), ({"shape": (2, 2, 8, 2, 5)}, "sources"),
                     ({"shape": (2, 2, 0, 2, 2)}, "empty"), ({"shape": (2, 2, 8, 0, 2)}, "empty"),
                     ({"shape": (0, 2, 8, 2, 2)}, "empty"),
                     ({"n_total": 100}, "n_total"),
                     ({"ws": 0}, "workspace"), ({"ws_bytes": 12}, "workspace"),
                     ({"strides": (64, 32, 4, 2, 0)}, "strides"),            # two sources on one address
                     ({"strides": (64, 32, 4, 2, 2)}, "strides"),            # source and microphone axes collide
                     ({"strides": (64, 32, 4, -2, 1)}, "strides"),
                     ({"strides": (64, 16, 4, 2, 1)}, "strides")):           # rows overlap
        rc, msg = _pit(lib, **kw)
        assert rc != 0 and word in msg, (kw, rc, msg)


def test_dp_vad_and_targets_validate_before_launch():
    lib = _lib.load()
    p = C.c_void_p(64)
    err = lambda: lib.fnssl_last_error().decode()                                    # noqa: E731
    assert lib.fnssl_dp_vad(None, p, 1, 2, 2, 24, p, None) != 0 and "null" in err()
    assert lib.fnssl_dp_vad(p, None, 1, 2, 2, 24, p, None) != 0
    assert lib.fnssl_dp_vad(p, p, 1, 2, 2, 24, None, None) != 0
    assert lib.fnssl_dp_vad(p, p, 1, 2, 0, 24, p, None) != 0 and "sources" in err()
    assert lib.fnssl_dp_vad(p, p, 1, 2, 2, 11, p, None) != 0 and "frames" in err()  # less than one segment
    t = lambda **kw: lib.fnssl_ipdnet_targets(*[{**dict(doa=p, vad=p, nb=1, nseg=2, nsrc=2, mic=p, nmic=4, ns=p, bin0=1, nf=256,
                                                        nbins=257, fmax=8000.0, speed=340.0, th=0.001, ipd=p, stream=None),
                                                 **kw}[k]
                                                for k in ("doa", "vad", "nb", "nseg", "nsrc", "mic", "nmic", "ns", "bin0", "nf",
                                                          "nbins", "fmax", "speed", "th", "ipd", "stream")])   # noqa: E731
    assert t(doa=None) != 0 and "null" in err()
    assert t(mic=None) != 0 and t(ipd=None) != 0
    assert t(ns=None) != 0 and "null" in err()                       # a VAD gate needs the non-source target
    assert t(nsrc=0) != 0 and "sources" in err()
    assert t(nsrc=5) != 0 and "sources" in err()
    assert t(nmic=1) != 0 and "microphones" in err()
    assert t(nmic=65) != 0 and "microphones" in err()
    assert t(nf=257) != 0 and "bins" in err()
    assert t(speed=0.0) != 0 and t(fmax=-1.0) != 0
    assert t(th=float("nan")) != 0 and "NaN" in err()


def test_non_source_target_matches_the_reference_table():
    g = load_golden("g19_ipdnet_step")
    t = ipdnet_step.non_source_target(g["mic_pos"])
    assert t.dtype == np.float32 and t.shape == (512, 3)
    assert_close(t[:256], g["non_source"][:256], 0, 2e-7, "Bessel half")
    assert (t[256:] == 0).all() and (g["non_source"][256:] == 0).all()
    assert_close(R.non_source_target(g["mic_pos"]), g["non_source"], 0, 2e-7, "test restatement")
    with pytest.raises(RuntimeError):
        ipdnet_step.non_source_target(g["mic_pos"], bins=range(1, 200))


def test_restatements_reproduce_the_golden_batch():
    """tests/ipdnet_step_ref.py applied to the seeded batch gives the real reference's dp_vad and targets."""
    g = load_golden("g19_ipdnet_step")
    mic_sig, dp, doa, mic_pos = R.g19_batch()
    np.testing.assert_array_equal(doa, g["doa"])
    np.testing.assert_array_equal(mic_pos, g["mic_pos"])
    win = torch.hann_window(512)
    stft = lambda s: torch.stack([torch.stft(torch.from_numpy(np.ascontiguousarray(s[:, :, c])), 512, 256, 512, win,   # noqa: E731
                                             center=False, return_complex=True).permute(0, 2, 1)
                                  for c in range(s.shape[2])], dim=1).numpy()       # [nb, nch, nt, 257]
    vad = R.dp_vad(stft(mic_sig), stft(dp[:, :, 0, :]))
    active = g["dp_vad"] > 0
    assert active.sum() == 7 and (vad[~active] == 0).all()
    assert_close(vad, g["dp_vad"], 1e-5, 0, "dp_vad")
    assert_close(R.ipdnet_targets(doa, g["dp_vad"], mic_pos, g["non_source"].astype(np.float32)), g["ipd"], 0, 2e-6, "targets")
    # silent slots hold the non-source table, active ones a unit-modulus IPD
    ipd = g["ipd"]
    for b, s, k in itertools.product(range(2), range(3), range(2)):
        if active[b, s, k]:
            assert_close(ipd[b, s, :256, :, k] ** 2 + ipd[b, s, 256:, :, k] ** 2, np.ones((256, 3), np.float32), 0, 1e-6, "modulus")
        else:
            np.testing.assert_array_equal(ipd[b, s, :, :, k], g["non_source"].astype(np.float32))


def test_restated_pit_equals_brute_force_and_g18():
    for rows, d, nsrc in ((9, 20, 1), (9, 20, 2), (7, 34, 3), (5, 12, 4)):
        gt = rs_randn(10 + nsrc, (rows, d, nsrc)).astype(np.float64)
        rs = np.random.RandomState(20 + nsrc)
        pis = [rs.permutation(nsrc) for _ in range(rows)]
        pred = np.stack([gt[r][:, pis[r]] for r in range(rows)]) + 0.3 * rs_randn(30 + nsrc, (rows, d, nsrc))
        loss, perm, dpred = R.pit_mse(pred, gt)
        perms = R.perm_list(nsrc)
        total = 0.0
        for r in range(rows):
            costs = [sum(((pred[r][:, pm[j]] - gt[r][:, j]) ** 2).sum() for j in range(nsrc)) for pm in perms]
            assert perm[r] == int(np.argmin(costs))
            # pred[:, pi[j]] is the noisy copy of gt[:, j']: the chosen permutation undoes pi
            assert [pis[r][q] for q in perms[perm[r]]] == list(range(nsrc))
            total += min(costs)
        assert abs(loss - total / pred.size) <= 1e-12 * loss
        eps = 1e-4                                                    # central difference: exact for a quadratic
        up, down = pred.copy(), pred.copy()
        up[2, 3, 0] += eps
        down[2, 3, 0] -= eps
        fd = (R.pit_mse(up, gt)[0] - R.pit_mse(down, gt)[0]) / (2 * eps)
        assert abs(fd - dpred[2, 3, 0]) <= 1e-8 * abs(dpred[2, 3, 0]) + 1e-11
    # exact ties keep the identity
    gt = rs_randn(41, (3, 8, 2)).astype(np.float64)
    pred = rs_randn(42, (3, 8, 2)).astype(np.float64)
    pred[0, :, 1] = pred[0, :, 0]
    gt[1, :, 1] = gt[1, :, 0]
    assert list(R.pit_mse(pred, gt)[1][:2]) == [0, 0]
    # the committed torch restatement and the real reference's golden losses
    import ipdnet_train_ref as T
    g = load_golden("g18_ipdnet_train")
    for case in "abc":
        pred, gt = g[case + "_pred"], g[case + "_gt"]
        nb, nt2 = pred.shape[:2]
        loss = R.pit_mse(pred.reshape(nb * nt2, -1, 2), gt.reshape(nb * nt2, -1, 2))[0]
        assert abs(loss - float(g[case + "_loss"])) <= 1e-5 * abs(float(g[case + "_loss"]))
        assert abs(loss - float(T.pit_mse(torch.from_numpy(pred), torch.from_numpy(gt)))) <= 1e-5 * loss


def test_drop_in_module_constructs_without_a_device():
    from IPDnet.FixedAarryIPDnet import IPDnet
    from IPDnet.train_step import MyModel
    m = MyModel()
    assert isinstance(m.arch, IPDnet) and m.arch.input_size == 4 and m.mic_pos.shape == (2, 3) and m.mic_pos.dtype == np.float32
    assert m.tar_useVAD and m.max_source == 2 and m.vad_th == 0.001
    opt = m.configure_optimizers()
    assert isinstance(opt["optimizer"], torch.optim.Adam) and opt["optimizer"].defaults["lr"] == 5e-4
    assert opt["lr_scheduler"]["scheduler"].gamma == 0.975 and opt["lr_scheduler"]["monitor"] == "valid/loss"
    with pytest.raises(ValueError, match="ch_mode"):
        MyModel(ch_mode='MM')
    with pytest.raises(ValueError, match="hop 256"):
        MyModel(win_len=400)
    with pytest.raises(ValueError, match="microphones"):
        MyModel(mic_pos=R.G19_MICS)                                  # four microphones need arch=IPDnet(8, ...)
    m4 = MyModel(mic_pos=torch.from_numpy(R.G19_MICS), arch=IPDnet(8, 256, 2, True), device="cpu")
    assert m4.arch.input_size == 8
    mic_sig, dp, doa, _ = R.g19_batch()
    batch = (torch.from_numpy(mic_sig), {"doa": torch.from_numpy(doa), "dp_signal": torch.from_numpy(dp)})
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        m4.training_step(batch, 0)
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        m4.cal_loss(torch.zeros(2, 3, 512, 3, 2), [None, torch.zeros(6, 512, 3, 2)])
    for fn, args in ((ipdnet_step.pit_mse, (torch.zeros(1, 1, 4, 1, 2), torch.zeros(1, 1, 4, 1, 2))),
                     (ipdnet_step.dp_vad, (torch.zeros(1, 2, 12, 257, 2), torch.zeros(1, 2, 12, 257, 2))),
                     (ipdnet_step.ipdnet_targets, (torch.zeros(1, 1, 2, 2), None, torch.zeros(2, 3), torch.zeros(512, 1)))):
        with pytest.raises(RuntimeError, match="ROCm device tensor"):
            fn(*args)
