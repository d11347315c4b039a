"""CPU tests of the host side of the room simulation (fnssl/rir.py, ops.rir_plan / fnssl_rir_plan): the Sabine helpers,
argument checks, the chunk planner's arithmetic and the sample-count rounding.  No device."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fnssl.rir as gpuRIR  # noqa: E402
from fnssl import _lib, ops  # noqa: E402

ROOM = [3.2, 4.1, 2.6]


def wall_areas(room):
    return np.array([room[1] * room[2]] * 2 + [room[0] * room[2]] * 2 + [room[0] * room[1]] * 2)


def test_att2t_and_t2n():
    assert gpuRIR.att2t_SabineEstimator(60, 0.7) == pytest.approx(0.7) and gpuRIR.att2t_SabineEstimator(12, 1.3) == pytest.approx(0.26)
    assert gpuRIR.att2t_SabineEstimator(40.0, 0.3) == pytest.approx(0.2)
    n = gpuRIR.t2n(0.26, [8, 7, 4])
    assert n == [23, 26, 45] and all(type(v) is int for v in n)
    assert gpuRIR.t2n(0.1, [3.43, 6.86, 70.0]) == [20, 10, 1] and gpuRIR.t2n(0.1, [4.0, 4.0, 4.0], c=320.0) == [16, 16, 16]


@pytest.mark.parametrize("weights", [[1] * 6, [0.6, 0.9, 0.5, 0.6, 1.0, 0.8], [1, 1, 1, 1, 0, 0.5], [2, 2, 2, 2, 2, 4]])
@pytest.mark.parametrize("t60", [0.2, 0.8, 1.3])
def test_beta_sabine_solves_sabines_equation(weights, t60):
    room = [8.0, 7.0, 4.0]
    beta = gpuRIR.beta_SabineEstimation(room, t60, abs_weights=weights)
    assert beta.shape == (6,) and (beta >= 0).all() and (beta <= 1).all()
    w = np.array(weights, dtype=float) / max(weights)
    alpha = 1 - beta ** 2
    assert alpha == pytest.approx(alpha.max() / w.max() * w)                     # absorptions in the ratios of the weights
    reachable = 0.161 * np.prod(room) / (wall_areas(room) * w).sum() <= t60       # the T60 of x = 1, the most these weights absorb
    if reachable:
        assert 0.161 * np.prod(room) / (wall_areas(room) * alpha).sum() == pytest.approx(t60, rel=1e-12)
    else:
        assert beta == pytest.approx(np.sqrt(1 - w))                              # clamped to x = 1
    try:                                                                          # where scipy imports: the bounded minimiser
        from scipy import optimize as opt
    except ImportError:
        return

    def err(x):                                                                   # the error gpuRIR minimises, on [0, 1]
        return abs(t60 - 0.161 * np.prod(room) / (wall_areas(room) * x * w).sum())

    res = opt.minimize_scalar(err, bounds=(0.0, 1.0), method="bounded", options={"xatol": 1e-12})
    assert np.sqrt(np.maximum(0, 1 - res.x * w)) == pytest.approx(beta, abs=2e-3)


def test_beta_sabine_clamps():
    assert np.array_equal(gpuRIR.beta_SabineEstimation(ROOM, 0), np.zeros(6))             # T60 = 0: x = 1
    assert np.array_equal(gpuRIR.beta_SabineEstimation(ROOM, 1e-3), np.zeros(6))          # unreachable: clamped to x = 1
    b = gpuRIR.beta_SabineEstimation(ROOM, 0, abs_weights=[1, 0.5, 1, 1, 1, 0])
    assert b == pytest.approx(np.sqrt([0, 0.5, 0, 0, 0, 1]))
    assert (gpuRIR.beta_SabineEstimation(ROOM, 1e9) > 1 - 1e-9).all()
    with pytest.raises(ValueError):
        gpuRIR.beta_SabineEstimation(ROOM, 0.5, abs_weights=[0] * 6)
    with pytest.raises(ValueError):
        gpuRIR.beta_SabineEstimation(ROOM[:2], 0.5)


def test_sample_counts_are_made_even():
    assert gpuRIR.sample_counts(0.05, 0.125, 16000) == (800, 2000)
    assert gpuRIR.sample_counts(0.0500625, 0.125, 16000) == (802, 2000)                   # ceil = 801, odd
    assert gpuRIR.sample_counts(None, 0.1, 16000) == (1600, 1600)
    assert gpuRIR.sample_counts(0.2, 0.1, 16000) == (1600, 1600)                          # Tdiff beyond Tmax
    assert gpuRIR.sample_counts(0.26, 0.8667, 16000) == (4160, 13868)
    assert gpuRIR.sample_counts(0.00301, 0.02, 16000) == (50, 320)                        # ceil(48.16) = 49


def test_argument_checks_come_before_any_device_work():
    src, rcv = np.array([[1.0, 1.0, 1.0]]), np.array([[2.0, 2.0, 1.0]])
    beta = [0.8] * 6
    for kw in ({"spkr_pattern": "card"}, {"mic_pattern": "hypcard"}):
        with pytest.raises(NotImplementedError, match=list(kw.values())[0]):
            gpuRIR.simulateRIR(ROOM, beta, src, rcv, [3, 3, 3], 0.1, 16000, **kw)
    for bad in ([[3.2, 1.0, 1.0]], [[1.0, 0.0, 1.0]], [[1.0, 1.0, 2.7]], [[-0.1, 1.0, 1.0]]):
        with pytest.raises(ValueError, match="inside the room"):
            gpuRIR.simulateRIR(ROOM, beta, np.array(bad), rcv, [3, 3, 3], 0.1, 16000)
        with pytest.raises(ValueError, match="inside the room"):
            gpuRIR.simulateRIR(ROOM, beta, src, np.array(bad), [3, 3, 3], 0.1, 16000)
    with pytest.raises(ValueError, match="beta"):
        gpuRIR.simulateRIR(ROOM, [0.8] * 5 + [1.2], src, rcv, [3, 3, 3], 0.1, 16000)
    with pytest.raises(ValueError, match="nb_img"):
        gpuRIR.simulateRIR(ROOM, beta, src, rcv, [3, 0, 3], 0.1, 16000)
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        gpuRIR.simulateRIR(ROOM, beta, torch.tensor(src), rcv, [3, 3, 3], 0.1, 16000)
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        gpuRIR.simulateTrajectory(torch.zeros(16), np.zeros((1, 1, 4)))
    with pytest.raises(ValueError, match="timestamps"):
        gpuRIR._w_ini(3, 100, [0.0, 0.1], 16000)
    with pytest.raises(ValueError, match="fs"):
        gpuRIR._w_ini(3, 100, [0.0, 0.1, 0.2], None)


def test_w_ini():
    assert gpuRIR._w_ini(3, 1001, None, None).tolist() == [0, 333, 667, 1001]             # int(p * 1001 / 3)
    assert gpuRIR._w_ini(4, 1001, [0.0, 0.0101, 0.0101, 0.04], 16000).tolist() == [0, 161, 161, 640, 1001]
    assert gpuRIR._w_ini(2, 100, [0.0, 1.0], 16000).tolist() == [0, 100, 100]             # past the end: an empty segment
    assert gpuRIR._w_ini(3, 1001, None, None).dtype == np.int32


def expected_plan(m_src, m_rcv, nb, nism, cus):
    total = nb[0] * nb[1] * nb[2]
    nrir = m_src * m_rcv
    want = max(1, min(-(-cus * 8 // nrir), -(-total // 256)))
    chunk = -(--(-total // want) // 64) * 64
    nchunks = -(-total // chunk)
    return {"images": total, "chunk_images": chunk, "nchunks": nchunks, "last_chunk_images": total - (nchunks - 1) * chunk,
            "grid_x": nchunks, "grid_y": nrir, "threads": 64, "lds_bytes": 4 * (nism + 2 * sum(nb)),
            "workspace_bytes": 4 * nchunks * nrir * nism if nchunks > 1 else 0}


@pytest.mark.parametrize("m_src,m_rcv,nb,nism", [(1, 1, [1, 1, 1], 800), (1, 2, [11, 9, 8], 800), (3, 5, [9, 8, 7], 800),
                                                 (50, 15, [23, 26, 45], 4160), (50, 2, [23, 26, 45], 4160),
                                                 (1, 1, [16, 16, 1], 2), (200, 15, [70, 60, 110], 8192)])
def test_rir_plan_arithmetic(m_src, m_rcv, nb, nism):
    plan = ops.rir_plan(m_src, m_rcv, nb, nism, cus=256)
    assert plan == expected_plan(m_src, m_rcv, nb, nism, 256)
    assert plan["chunk_images"] % 64 == 0 and 0 < plan["last_chunk_images"] <= plan["chunk_images"]
    assert (plan["nchunks"] - 1) * plan["chunk_images"] < plan["images"] <= plan["nchunks"] * plan["chunk_images"]
    nbc = (C.c_int * 3)(*nb)
    assert _lib.load().fnssl_rir_workspace_bytes(m_src, m_rcv, C.byref(nbc), nism, 256) == plan["workspace_bytes"]
    assert ops.rir_plan(m_src, m_rcv, nb, nism, cus=64)["nchunks"] <= plan["nchunks"]


def test_rir_plan_paths_and_limits():
    assert ops.rir_plan(1, 1, [1, 1, 1], 800, 256)["nchunks"] == 1                        # written straight to the RIR
    p = ops.rir_plan(1, 2, [11, 9, 8], 800, 256)
    assert (p["nchunks"], p["chunk_images"], p["last_chunk_images"]) == (4, 256, 24)      # ragged last chunk, summed via the workspace
    assert ops.rir_plan(50, 15, [23, 26, 45], 4160, 256)["nchunks"] == 3                  # the reference's scene, 15 microphones
    # an image-source part too long for the LDS tile is refused, and the message names the limit
    assert _lib.RIR_MAX_ISM_SAMPLES == 8192 and _lib.RIR_MAX_IMAGES_AXIS == 1024 and _lib.RIR_TRAJ_MAX_BATCH == 16
    for args, word in (((1, 1, [3, 3, 3], 8194), "8192"), ((1, 1, [3, 3, 3], 801), "even"), ((1, 1, [1025, 1, 1], 800), "1024"),
                       ((0, 1, [3, 3, 3], 800), "sources"), ((300, 300, [3, 3, 3], 800), "65535")):
        with pytest.raises(RuntimeError, match=word):
            ops.rir_plan(*args, cus=256)
    nbc = (C.c_int * 3)(3, 3, 3)
    assert _lib.load().fnssl_rir_workspace_bytes(1, 1, C.byref(nbc), 8194, 256) == 0
    assert C.sizeof(_lib.RirTrajItem) == 48 and 16 * 48 <= 4096 and C.sizeof(_lib.RirPlanInfo) == 40
