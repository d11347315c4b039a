"""CPU tests that pin the room-simulation reference of tests/rir_ref.py (the yardstick of tests/test_gpu_rir.py) to forms
written out independently: one windowed sinc in closed form, a 1-D room with its image positions by hand, the trajectory
formula against segment / np.convolve / overlap-add, the Philox known answer, the noise statistics of the seeds the GPU
tests use, and the gate table re-measured.  Mutants of the reference (swapped wall exponents, an inclusive index range, a
window one sample too wide) must be told apart."""
import numpy as np
import pytest

import rir_ref as R


def test_direct_path_is_one_windowed_sinc():
    src, rcv = R.SRC[0], R.RCV[0]
    d = np.sqrt(((np.array(src) - np.array(rcv)) ** 2).sum())
    got = R.ism(R.ROOM, R.BETA, [src], [rcv], [1, 1, 1], 800, R.FS)[0, 0]
    want = R.single_windowed_sinc(d, 800, R.FS)
    assert np.abs(want).max() > 0.05 and np.abs(got - want).max() < 1e-15
    # c = 320, 1.0 m: tau = 50 exactly, the peak is the amplitude itself and every other tap sits on a zero of the sinc
    got = R.ism(R.ROOM, R.BETA, [[0.5, 2.0, 1.0]], [[1.5, 2.0, 1.0]], [1, 1, 1], 800, R.FS, 320.0)[0, 0]
    assert abs(got[50] - 1 / (4 * np.pi)) < 1e-16 and np.abs(np.delete(got, 50)).max() < 1e-16


def test_one_dimensional_room_against_images_by_hand():
    """beta = 0 on the y and z walls: only the x images survive.  L = 3.2, source at 1.1, receiver at 1.55, same y and z.
    Five images n = -2 .. 2 at -5.3, -1.1, 1.1, 5.3, 7.5 with (wall 0, wall L) reflections (1, 1), (1, 0), (0, 0), (0, 1), (1, 1)."""
    b0, b1 = 0.7, 0.9
    beta = [b0, b1, 0, 0, 0, 0]
    got = R.ism(R.ROOM, beta, [[1.1, 2.0, 1.0]], [[1.55, 2.0, 1.0]], [5, 3, 3], 800, R.FS)[0, 0]
    want = np.zeros(800)
    for x, amp in ((-5.3, b0 * b1), (-1.1, b0), (1.1, 1.0), (5.3, b1), (7.5, b0 * b1)):
        want += amp * R.single_windowed_sinc(abs(x - 1.55), 800, R.FS)
    assert np.abs(got - want).max() < 1e-15 and np.abs(want).max() > 0.1
    # an even count: n = -2 .. 1
    got = R.ism(R.ROOM, beta, [[1.1, 2.0, 1.0]], [[1.55, 2.0, 1.0]], [4, 1, 1], 800, R.FS)[0, 0]
    want -= b0 * b1 * R.single_windowed_sinc(7.5 - 1.55, 800, R.FS)
    assert np.abs(got - want).max() < 1e-15


@pytest.mark.parametrize("mutant", ["swapped_walls", "inclusive_range", "window_plus_one"])
def test_mutants_of_the_reference_are_told_apart(mutant):
    """A reference with swapped wall exponents, with the index range -N/2 .. N/2 inclusive or with a window one sample too
    wide fails the pins above by eight orders of magnitude more than their tolerance, and a device that computed it would
    miss the gate of at least one GPU case (the window mutant: the direct path, the near source and the chunked case; it is
    5.2e-6 from the reference elsewhere, inside 8 x 7.5e-7)."""
    b0, b1 = 0.7, 0.9
    images = ((-5.3, b0 * b1), (-1.1, b0), (1.1, 1.0), (5.3, b1), (7.5, b0 * b1))
    broken = 0.0
    for nb, imgs in (([5, 3, 3], images), ([4, 1, 1], images[:4])):              # (an odd count has the inclusive range anyway)
        bad = R.ism(R.ROOM, [b0, b1, 0, 0, 0, 0], [[1.1, 2.0, 1.0]], [[1.55, 2.0, 1.0]], nb, 800, R.FS, mutant=mutant)[0, 0]
        want = sum(amp * R.single_windowed_sinc(abs(x - 1.55), 800, R.FS) for x, amp in imgs)
        broken = max(broken, np.abs(bad - want).max())
    assert broken > 1e-7
    caught = []
    for name in ("direct", "even_odd", "near", "chunks"):
        src, rcv, nb, tdiff, c = R.ISM_CASES[name]
        dist = np.abs(R.ism(R.ROOM, R.BETA, src, rcv, nb, 800, R.FS, c, mutant=mutant) - R.ism_case(name)).max()
        print(mutant, name, dist, R.GATE_FACTOR * R.GATE["ism/" + name])
        caught.append(dist > R.GATE_FACTOR * R.GATE["ism/" + name])
    assert sum(caught) >= 3


@pytest.mark.parametrize("npts,ts", [(1, [0.0]), (3, [0.0, 0.011, 0.0431]), (7, [0.0, 0.004, 0.0101, 0.0101, 0.027, 0.04, 0.0555]),
                                     (7, None)])
def test_trajectory_formula_is_segment_convolve_overlap_add(npts, ts):
    rs = np.random.RandomState(5 + npts)
    x, rirs = rs.standard_normal(1001), rs.standard_normal((npts, 2, 33))
    a = R.trajectory(x, rirs, ts, R.FS if ts is not None else None)
    b = R.trajectory_overlap_add(x, rirs, ts, R.FS if ts is not None else None)
    assert a.shape == (1033, 2) and np.abs(a - b).max() < 1e-12
    # the gather form of the same sum, one output at a time
    w = R.w_ini(npts, 1001, ts, R.FS if ts is not None else None)
    point = np.searchsorted(w, np.arange(1001), side="right") - 1
    for t in (0, 17, 500, 1000, 1032):
        want = sum(rirs[point[t - k], :, k] * x[t - k] for k in range(33) if 0 <= t - k < 1001)
        assert np.abs(a[t] - want).max() < 1e-12


def test_philox_known_answers_and_uniforms():
    """Philox4x32-10 known answers (Random123's kat_vectors: zero, all ones, the digits of pi)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in R.philox4x32_10(ctr, key).reshape(4)) == want
    u = R.uniforms(7, 1, 2, np.arange(800, 2000))
    assert u.min() > 0 and u.max() < 1 and np.array_equal(u, u.astype(np.float32)) and np.array_equal(1 - u, (1 - u).astype(np.float32))
    assert not np.array_equal(u, R.uniforms(8, 1, 2, np.arange(800, 2000)))
    assert np.array_equal(u[100:104], R.uniforms(7, 1, 2, np.arange(900, 904)))        # a function of t alone


def test_noise_bounds_hold_for_the_seeds_of_the_gpu_tests():
    for name, (case, tdiff, tmax, seed, _) in R.TAIL_CASES.items():
        src, rcv = R.ISM_CASES[case][:2]
        nism, ns = R.sample_counts(tdiff, tmax, R.FS)
        mb, vb = R.noise_bounds(ns - nism)
        for s in range(len(src)):
            for r in range(len(rcv)):
                u = R.uniforms(seed, s, r, np.arange(nism, ns))
                xi = np.sqrt(3) / np.pi * np.log(u / (1 - u))
                assert abs(xi.mean()) <= mb and abs(xi.var() - 1) <= vb, (name, s, r, xi.mean(), xi.var())


def test_tail_branches_and_line():
    """A synthetic exponential decay is recovered by the fit; the branches are taken as stated."""
    t = np.arange(800)
    h = np.exp(-0.004 * t) * np.where(t >= 40, 1.0, 0.0) * np.cos(0.9 * t)
    a, b, branch = R.tail_line(h, R.ROOM, R.BETA, [1.0, 1.0, 1.0], [1.0 + 40 * 343.0 / R.FS + 1e-6, 1.0, 1.0], R.FS)
    assert branch == "fit" and abs(b + 0.008) < 2e-4                     # the energy decays twice as fast as the amplitude
    _, b2, branch = R.tail_line(h[:300], R.ROOM, R.BETA, [1.0, 1.0, 1.0], [1.8575, 1.0, 1.0], R.FS)
    assert branch == "sabine_last" and b2 == R.sabine_slope(R.ROOM, R.BETA, R.FS) < 0
    _, _, branch = R.tail_line(h[:100], R.ROOM, R.BETA, [1.0, 1.0, 1.0], [1.8575, 1.0, 1.0], R.FS)
    assert branch == "sabine_mean"
    assert R.sabine_slope(R.ROOM, [1.0] * 6, R.FS) == 0.0
    # Sabine: 60 dB of energy decay in T60 = 0.161 V / A
    t60 = -np.log(1e6) / R.sabine_slope(R.ROOM, R.BETA, R.FS) / R.FS
    area = [4.1 * 2.6, 4.1 * 2.6, 3.2 * 2.6, 3.2 * 2.6, 3.2 * 4.1, 3.2 * 4.1]
    assert abs(t60 - 0.161 * 3.2 * 4.1 * 2.6 / sum(s * (1 - bb * bb) for s, bb in zip(area, R.BETA))) < 1e-12


def test_gate_table_is_what_the_float32_restatement_measures():
    """The table is measured with this numpy's float32 kernels; another build may round a sine differently, so the stored
    figures may differ from a re-measurement by a quarter, not more."""
    measured = R.measure_gates()
    assert set(measured) == set(R.GATE)
    for k, v in measured.items():
        print(k, "%.3e" % v, "%.3e" % R.GATE[k])
        assert 0.8 * R.GATE[k] <= v <= 1.25 * R.GATE[k], (k, v, R.GATE[k])
