"""CPU tests that pin the label reference of tests/labels_ref.py (the yardstick of tests/test_gpu_labels.py): its float64 form
against golden G24 recorded from the real Dataset.py (bit for bit) and against ``np.interp``, the input conditions the device
gates rest on, the gate table re-measured, and mutants of the transform that must each fail against G24."""
import numpy as np
import pytest

import labels_ref as R
from conftest import load_golden


def unpack(bits, shape):
    return np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------
# G24
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.TRAJ_CASES))
def test_interpolation_is_numpys_and_cart2sph_is_the_references(name):
    g = load_golden("g24_labels")
    pts, ts, n, fs, pos = R.traj_case(name)
    traj, doa = R.trajectory_doa(pts, ts, n, fs, pos)
    t = np.arange(n) / fs
    assert (t < ts[0]).sum() >= 50 and (t > ts[-1]).sum() >= 50                  # both clamps are hit
    for s in range(pts.shape[2]):
        want = np.array([np.interp(t, ts, pts[:, i, s]) for i in range(3)]).transpose()
        assert np.array_equal(traj[:, :, s], want)
        cart = traj[:, :, s] - pos
        assert np.array_equal(R.digest(cart), g["a_%s_%d_in" % (name, s)])
        assert np.array_equal(R.cart2sph(cart)[::4], g["a_%s_%d_sph" % (name, s)])
        assert np.array_equal(doa[::4, :, s], g["a_%s_%d_sph" % (name, s)][:, 1:3])


def test_trajectory_cases_cover_the_crossing_and_the_pole():
    az_jump, el_min = [], []
    for name in R.TRAJ_CASES:
        _, doa = R.trajectory_doa(*R.traj_case(name))
        az_jump.append(np.abs(np.diff(doa[:, 1], axis=0)).max())
        el_min.append(doa[:, 0].min())
    assert max(az_jump) > 6.0 and min(el_min) < 0.01                              # +-pi is crossed; the elevation nears 0
    assert az_jump[0] > 6.0 and el_min[2] < 0.01                                  # by a one-source case each


def golden_seg(g, k):
    shape, sources = R.GOLDEN_SEG[k]
    case = R.sub_scene(R.seg_case(*shape), sources)
    key = "b_%d" % k
    assert np.array_equal(R.digest(case["DOA"], case["mic_vad_sources"], case["mic_vad"]), g[key + "_in"])
    vshape = tuple(g[key + "_vad_shape"])
    want = {"DOAw": g[key + "_DOAw"], "mic_vad": unpack(g[key + "_mic_vad"], vshape[:2]),
            "mic_vad_sources": unpack(g[key + "_mic_vad_sources"], vshape), "tw": g[key + "_tw"]}
    return shape, case, want


def same(got, want):
    return all(got[k].shape == want[k].shape and got[k].dtype == np.float64 and np.array_equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize("k", range(len(R.GOLDEN_SEG)))
def test_transform_equals_the_real_reference_bit_for_bit(k):
    shape, case, want = golden_seg(load_golden("g24_labels"), k)
    got = R.transform(shape[0], case, shape[1], shape[2])
    assert want["DOAw"].shape == (R.num_windows(*shape), 2, 2)
    assert same(got, want)


def test_gts_restatement_pads_with_zeros():
    """``labels_ref.gts`` is a RESTATEMENT of the padding in ``FixTrajectoryDataset.__getitem__`` (no golden record: the reference
    hard-codes its training shapes there and reads its scenes from files).  Checked against its definition: every scene's
    rows in the first S_b sources, zeros behind them, counts = the ones of every window."""
    shape = R.GOLDEN_SEG[0][0]
    full = R.seg_case(*shape)
    rs = np.random.RandomState(24)
    subsets = ((2,), (0, 1), (3,))
    segs = [R.transform(shape[0], R.sub_scene(full, src), shape[1], shape[2]) for src in subsets]
    dps = [rs.standard_normal((shape[0], 2, len(src))).astype(np.float32) for src in subsets]
    for smax in (2, 4):
        got = R.gts(segs, dps, smax)
        assert got["num_source"].tolist() == [1, 2, 1] and got["doa"].shape == (3, R.num_windows(*shape), 2, smax)
        for b, src in enumerate(subsets):
            ns = len(src)
            assert np.array_equal(got["doa"][b, :, :, :ns], segs[b]["DOAw"]) and not got["doa"][b, :, :, ns:].any()
            assert np.array_equal(got["vad_sources"][b, :, :, :ns], segs[b]["mic_vad_sources"]) and not got["vad_sources"][b, :, :, ns:].any()
            assert np.array_equal(got["dp_signal"][b, :, :, :ns], dps[b]) and not got["dp_signal"][b, :, :, ns:].any()
            assert np.array_equal(got["vad_count"][b], got["vad_sources"][b].sum(axis=1)) and got["vad_count"].dtype == np.int32


MUTANTS = ["no_plus_2pi", "no_fold", "fold_elevation", "no_vad_extension", "tw_nw"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_of_the_transform_fail_against_the_golden(mutant):
    g = load_golden("g24_labels")
    failed = 0
    for k in range(len(R.GOLDEN_SEG)):
        shape, case, want = golden_seg(g, k)
        failed += not same(R.transform(shape[0], case, shape[1], shape[2], mutant=mutant), want)
    assert failed >= 1


# ------------------------------------------------------------------------------------------------------------------------
# the conditions the device gates rest on
# ------------------------------------------------------------------------------------------------------------------------
def seg_scenes():
    """Every scene the GPU tests segment: the four-source scene of every shape and the golden subsets."""
    for shape in R.SEG_SHAPES:
        yield shape, R.seg_case(*shape)
    for shape, sources in R.GOLDEN_SEG:
        yield shape, R.sub_scene(R.seg_case(*shape), sources)


def test_no_wrap_decision_can_flip_under_rounding():
    for (L, K, step), case in seg_scenes():
        nw = R.num_windows(L, K, step)
        for s in range(case["DOA"].shape[2]):
            az = case["DOA"][:, 1, s]
            for w in range(nw):
                win = az[w * step:w * step + K].copy()
                jump = np.abs(np.diff(win)).max() if K > 1 else 0.0
                assert jump < 1.0 or jump > 5.0, (L, K, step, s, w, jump)
                if jump > np.pi:
                    win[win < 0] += 2 * np.pi
                mean = win.mean()
                assert abs(abs(mean) - np.pi) > 1e-6, (L, K, step, s, w, mean)    # before the fold
                if mean > np.pi:
                    mean -= 2 * np.pi
                assert abs(abs(mean) - np.pi) > 1e-6, (L, K, step, s, w, mean)    # and after it


@pytest.mark.parametrize("shape", R.SEG_SHAPES, ids=R.seg_name)
def test_every_shape_has_the_four_kinds_of_source(shape):
    L, K, step = shape
    case = R.seg_case(*shape)
    nw = R.num_windows(*shape)
    assert (nw - 1) * step + K <= L
    w = nw // 2
    win = case["DOA"][w * step:w * step + K, 1, :]
    jumps = np.abs(np.diff(win, axis=0)).max(axis=0)
    assert jumps[0] > 5 and jumps[1] > 5 and jumps[2] < 1 and jumps[3] == 0
    unwrapped = np.where(win < 0, win + 2 * np.pi, win).mean(axis=0)
    assert unwrapped[0] > np.pi + 1e-6 and unwrapped[1] < np.pi - 1e-6           # the fold is taken / is not
    assert (case["DOA"][:, 1, 2] < 0).all()
    out = R.transform(L, case, K, step)
    assert out["DOAw"][w, 1, 0] < 0 < out["DOAw"][w, 1, 1]
    lv = case["mic_vad"].shape[0]
    assert lv < L
    if nw > 1:
        assert lv <= (nw - 1) * step and not out["mic_vad_sources"][-1].any()    # a window wholly in the zero extension
        assert out["mic_vad_sources"][:-1].any()


def test_gate_table_is_what_this_host_measures():
    names = ["%s/%s" % (kind, c) for c in R.TRAJ_CASES for kind in ("traj", "doa")] + ["seg/" + R.seg_name(s) for s in R.SEG_SHAPES]
    assert sorted(names) == sorted(R.D64)
    for name in names:
        d = R.measure_d64(name)
        print("d64 %-28s measured %.3e pinned %.3e" % (name, d, R.D64[name]))
        assert d > 0                                                              # every case has a moving source
        assert R.D64[name] / 2 <= d <= R.D64[name] * 2                            # the pinned figure, whatever the libm's last bit
