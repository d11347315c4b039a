"""Pin tests/lstm_bf16_f64_ref.py (the step-consistent float64 reference the bf16 LSTM kernels are held to in
test_gpu_lstm_bf16_f64.py).  CPU only: the reference against ``O.lstm_dir(..., bf16=True)``; the mutants the method
claims, restated in numpy, against both checkers; the input builders; and the committed table of oracle distances,
re-measured."""
import numpy as np
import pytest
import torch

import lstm_bf16_f64_ref as R
from conftest import rs_randn
from fnssl import weights as W
from oracle import fnssl_oracle as O

F32 = np.float32


def _state(I, H, seed, scale=1.0):
    return W.make_state([("L." + n, s) for n, s in W.lstm_param_shapes(I, H, False)], seed=seed, scale=scale)


def _args(sd):
    return sd["L.weight_ih_l0"], sd["L.weight_hh_l0"], sd["L.bias_ih_l0"], sd["L.bias_hh_l0"]


def bf16_trunc(a):
    return (np.ascontiguousarray(a, dtype=F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def bf16_half_away(a):
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x8000)) & np.uint64(0xFFFF0000)).astype(np.uint32).view(F32)


def lstm_dir_variant(x, w_ih, w_hh, b_ih, b_hh, reverse=False, x_conv=O.bf16_round, operand=O.bf16_round, bias=None,
                     store=lambda h: h):
    """O.lstm_dir(..., bf16=True) with its conversions as parameters: x_conv (x -> MFMA operand), operand (stored h ->
    recurrent operand), bias (fp32 bias -> what the kernel adds), store (fp32 h -> what is stored, and fed on)."""
    x = np.asarray(x, dtype=F32)
    N, T, _ = x.shape
    H = w_hh.shape[1]
    b = (b_ih + b_hh).astype(F32)
    b = b if bias is None else bias(b)
    xw = ((x_conv(x).reshape(N * T, -1) @ O.bf16_round(w_ih).T).reshape(N, T, 4 * H) + b).astype(F32)
    whhT = np.ascontiguousarray(O.bf16_round(w_hh).T)
    h, c = np.zeros((N, H), dtype=F32), np.zeros((N, H), dtype=F32)
    out = np.empty((N, T, H), dtype=F32)
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        g = (xw[:, t] + operand(h) @ whhT).astype(F32)
        i, f, o = O._sigmoid(g[:, 0:H]), O._sigmoid(g[:, H:2 * H]), O._sigmoid(g[:, 3 * H:4 * H])
        c = (f * c + i * np.tanh(g[:, 2 * H:3 * H], dtype=F32)).astype(F32)
        h = store((o * np.tanh(c, dtype=F32)).astype(F32))
        out[:, t] = h
    return out


# The four shapes of the oracle's measured distances, reduced.  The bound is fp32 rounding, not a
# measured figure: a gate pre-activation is an fp32 sum of I + H <= 528 products with sum |terms| ~ 10 (~ 100 with weights x 4
# and inputs x 3), so it carries a few 2^-24 * sum |terms| = 6e-7 (6e-6); sigmoid' <= 1/4 and tanh' <= 1 bring a gate to
# ~2e-7 (2e-6), and the cell state's own recurrence (c = f c + i g, f < 1) multiplies what is left by 1 / (1 - f), a few:
# 1e-6 and 1e-5.  The claimed mutants sit at 2e-4 and more.
@pytest.mark.parametrize("H,I,n,T,wscale,xscale,bound", [
    (256, 272, 6, 40, 1.0, 0.7, 1e-6),
    (128, 272, 6, 40, 1.0, 0.7, 1e-6),
    (128, 16, 8, 40, 1.0, 0.7, 1e-6),
    (256, 272, 6, 40, 4.0, 3.0, 1e-5),
])
@pytest.mark.parametrize("reverse", [False, True])
def test_reference_pins_the_bf16_oracle(H, I, n, T, wscale, xscale, bound, reverse):
    sd = _state(I, H, 9100 + H + I, wscale)
    x = R.fp32_block(9101, (n, T, I), xscale)
    want = O.lstm_dir(x, *_args(sd), reverse=reverse, bf16=True)
    ref = R.step_consistent(x, *_args(sd), want, reverse)
    assert ref.dtype == np.float64 and np.isfinite(ref).all()
    d = np.abs(want - ref).max()
    print("H %d I %d reverse %s: oracle vs step-consistent %.3g" % (H, I, reverse, d))
    assert d <= bound, d
    # the variant restates the oracle exactly (the mutants below differ from it in one conversion only)
    assert np.array_equal(lstm_dir_variant(x, *_args(sd), reverse=reverse), want)


@pytest.fixture(scope="module")
def mutant_case():
    """H = 256, I = 272, 40 sequences x 60 steps: where the claimed mutants were measured."""
    sd = _state(272, 256, 9200)
    x = np.concatenate([O.bf16_round(rs_randn(9201, (40, 60, 256), 0.7)), R.fp32_block(9202, (40, 60, 16), 0.7)], axis=-1)
    return sd, x


DELTA_MUT = R.DELTA["wide_narrow256"]     # the gate of the shape the mutants are built at (at real step count: not tighter)


# kw: the mutant where h is stored as fp32 (lstm_bf16.h).  kwb: where it is stored as bf16 (the wide kernels): there the
# stored row IS the operand, one conversion serves both, so "the operand truncated" is that conversion truncating.
@pytest.mark.parametrize("name,kw,kwb,least", [
    # (measured here: 5.6e-4 and 2.2e-4; asserted a decade lower, still a decade above the gate)
    ("h operand truncated to bf16", dict(operand=bf16_trunc), dict(store=bf16_trunc), 5e-5),
    ("bias cut to its first bf16 term", dict(bias=O.bf16_round), dict(bias=O.bf16_round, store=O.bf16_round), 2e-5),
])
@pytest.mark.parametrize("reverse", [False, True])
def test_claimed_mutants_fail_both_checkers(mutant_case, name, kw, kwb, least, reverse):
    sd, x = mutant_case
    good = lstm_dir_variant(x, *_args(sd), reverse=reverse)
    R.check_f32(good, R.step_consistent(x, *_args(sd), good, reverse), DELTA_MUT, "correct oracle")
    # bf16 output: the stored (rounded) row is what the next step reads
    gb = lstm_dir_variant(x, *_args(sd), reverse=reverse, store=O.bf16_round)
    R.check_bf16(gb, R.step_consistent(x, *_args(sd), gb, reverse), DELTA_MUT, "correct oracle, bf16 output")

    bad = lstm_dir_variant(x, *_args(sd), reverse=reverse, **kw)
    ref = R.step_consistent(x, *_args(sd), bad, reverse)
    s = R.f32_stats(bad, ref)
    print("%s, reverse %s: step-consistent max %.3g (delta %.3g)" % (name, reverse, s["max"], DELTA_MUT))
    assert s["max"] >= least
    with pytest.raises(AssertionError, match="max .got - ref"):
        R.check_f32(bad, ref, DELTA_MUT, name)
    badb = lstm_dir_variant(x, *_args(sd), reverse=reverse, **kwb)
    refb = R.step_consistent(x, *_args(sd), badb, reverse)
    sb = R.bf16_stats(badb, refb)
    print("%s, bf16 output: over half a spacing by %.3g, bias %.4f" % (name, sb["excess"], sb["bias"]))
    assert sb["excess"] >= least
    with pytest.raises(AssertionError, match="half-spacing"):
        R.check_bf16(badb, refb, DELTA_MUT, name)


@pytest.mark.parametrize("reverse", [False, True])
def test_truncating_store_fails_both_conditions_of_check_bf16(mutant_case, reverse):
    sd, x = mutant_case
    bad = lstm_dir_variant(x, *_args(sd), reverse=reverse, store=bf16_trunc)
    ref = R.step_consistent(x, *_args(sd), bad, reverse)
    s = R.bf16_stats(bad, ref)
    print("truncating store: over half a spacing by %.3g, bias %.4f over %d" % (s["excess"], s["bias"], s["n"]))
    assert s["n"] >= R.BIAS_MIN_N
    assert s["excess"] > 1e-4 > DELTA_MUT                  # (up to half a spacing of 2^-8; measured 9.8e-4)
    assert s["bias"] < -0.4                                # truncation: -0.5 of a spacing towards zero
    with pytest.raises(AssertionError, match="half-spacing"):
        R.check_bf16(bad, ref, DELTA_MUT)
    with pytest.raises(AssertionError, match="rounding bias"):
        R.check_bf16(bad, ref, 1.0)                        # the second condition alone (the first one switched off)
    # a correct rounding passes the second condition with the margin derived for it
    good = lstm_dir_variant(x, *_args(sd), reverse=reverse, store=O.bf16_round)
    sg = R.bf16_stats(good, R.step_consistent(x, *_args(sd), good, reverse))
    assert abs(sg["bias"]) < 0.003 and sg["excess"] <= 1e-6, sg


def test_spacing_and_checker_edges():
    assert R.spacing_bf16(np.array([1.0, 0.75, 0.5, 1.0 - 2.0 ** -20, 2.0 ** -6, 0.0])).tolist() == \
        [2.0 ** -7, 2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -13, 2.0 ** -133]
    ref = np.linspace(-1, 1, 200001)
    got = O.bf16_round(ref.astype(F32))
    assert R.check_bf16(got, ref, 1e-7)["excess"] <= 1e-7       # (fp32 rounding of ref before the bf16 one)
    with pytest.raises(AssertionError, match="only"):
        R.check_bf16(got[:1000], ref[:1000], 1e-7)
    with pytest.raises(AssertionError, match="non-finite"):
        R.check_f32(np.array([np.nan]), np.array([0.0]), 1.0)
    # one element off by a spacing is enough: nothing is left out
    bad = got.copy()
    bad[12345] += 2.0 ** -8
    with pytest.raises(AssertionError, match="half-spacing"):
        R.check_bf16(bad, ref, 1e-7)


def test_tie_inputs_tell_nearest_even_from_half_away():
    x = R.fp32_block(9300, (7, 33, 16), 0.7)
    bits = x.reshape(-1).view(np.uint32)
    low = bits & 0xFFFF
    assert (low != 0).all(), "a bf16-representable value: the in-kernel conversion would have nothing to round"
    tie = low == 0x8000
    per_group = tie.reshape(-1, 8).sum(axis=1)
    assert (per_group >= 1).all() and (per_group == 1).mean() > 0.999, "one forced tie in every eight elements"
    odd = ((bits >> 16) & 1).astype(bool)
    n = int(tie.sum())
    assert abs(int(odd[tie].sum()) * 2 - n) <= 4 * np.sqrt(n), "even and odd kept mantissas in equal numbers (4 sigma)"
    # every one of the 16 channels (every lane position of the in-kernel conversion) meets ties of both parities
    ch = np.arange(bits.size) % 16
    for c in range(16):
        assert (tie & odd & (ch == c)).sum() >= 5 and (tie & ~odd & (ch == c)).sum() >= 5, c
    ne, ha = O.bf16_round(x).reshape(-1), bf16_half_away(x).reshape(-1)
    assert np.array_equal(ne[~tie], ha[~tie])
    assert np.array_equal(ne[tie & odd], ha[tie & odd]) and (ne[tie & ~odd] != ha[tie & ~odd]).all()
    assert np.array_equal(ne[tie & ~odd], bf16_trunc(x).reshape(-1)[tie & ~odd])          # half to even: down
    assert np.isfinite(x).all() and abs(float(x.std()) - 0.7) < 0.02
    # through the recurrence (block 1's shape: all 16 channels are converted in the kernel): half-away fails the gate
    sd = _state(16, 128, 9301)
    x = R.fp32_block(9302, (24, 40, 16), 0.7)
    bad = lstm_dir_variant(x, *_args(sd), x_conv=bf16_half_away)
    s = R.f32_stats(bad, R.step_consistent(x, *_args(sd), bad))
    print("x rounded half away from zero: step-consistent max %.3g" % s["max"])
    assert s["max"] > 100 * R.DELTA["wide_block1"]


def test_counter_block_is_a_function_of_sequence_step_channel():
    seqs = torch.tensor([0, 5, 8198, 31])
    a = R.counter_block(torch, seqs, 256, 16, 77, 0.7, True)
    b = R.counter_block(torch, torch.tensor([5]), 256, 16, 77, 0.7, True)
    assert a.dtype == torch.float32 and a.shape == (4, 256, 16) and torch.equal(a[1:2], b)
    assert not torch.equal(a[0], a[1]) and not torch.equal(a, R.counter_block(torch, seqs, 256, 16, 78, 0.7, True))
    bits = a.numpy().view(np.uint32)
    tie = (bits & 0xFFFF) == 0x8000
    assert ((bits & 0xFFFF) != 0).all() and (tie.reshape(-1, 8).sum(axis=1) >= 1).all() and abs(tie.mean() - 0.125) < 1e-3
    kept = ((bits >> 16) & 1).astype(bool)
    for c in range(16):      # both parities on every channel
        assert (tie & kept)[..., c].sum() >= 20 and (tie & ~kept)[..., c].sum() >= 20, c
    # the same function of the flat index as the numpy builder's
    idx = ((seqs.numpy()[:, None, None] * 256 + np.arange(256)[None, :, None]) * 16 + np.arange(16)[None, None, :])
    plain = R.force_ties(np.full(idx.shape, 0x3F801234, dtype=np.int64), idx)
    assert np.array_equal(plain, R.force_ties(torch.full(idx.shape, 0x3F801234, dtype=torch.int64), torch.from_numpy(idx)).numpy())
    forced = (plain & 0xFFFF) == 0x8000
    assert forced.reshape(-1, 8).sum(axis=1).tolist() == [1] * (forced.size // 8) and tie[forced].all()
    big = R.counter_block(torch, torch.arange(64), 256, 256, 79, 0.7, False)
    assert torch.equal(big, big.bfloat16().float()), "the bf16 block is representable by construction"
    v = big.numpy().astype(np.float64)
    assert abs(v.mean()) < 5e-3 and abs(v.std() - 0.7) < 5e-3 and np.abs(v).max() > 2.0


def test_samples_cover_what_the_gpu_legs_promise():
    assert R.full_band_clusters(R.FULL_BIG_NSEQ, R.MI355X_CUS, False) == (13, 20)       # waves 0-3 three parts, 4-7 two;
    assert R.full_band_clusters(R.FULL_BIG_NSEQ, R.MI355X_CUS, True) == (11, 24)        # the last cluster 17 tiles either way
    assert R.full_band_clusters(64 * 300 * 1, R.MI355X_CUS, False) == (30, 20)          # (config 3, as the kernel's comments say)
    assert (R.FULL_BIG_NSEQ + 63) // 64 * 2 > R.MI355X_CUS >= (R.FULL_BIG_NSEQ - 7 + 63) // 64 * 2 - 1
    assert R.cluster_sample(R.FULL_BIG_NSEQ, 20) == [0, 19, 240, 256] and R.cluster_sample(R.FULL_BIG_NSEQ, 24) == [0, 23, 240, 256]
    # narrow-band, H = 256 (forward_bf16c: cl = ceil(tiles / 16), tpc = ceil(tiles / cl)): 600 sequences are 10 + 9 tiles
    assert R.narrow_clusters(512) == (1, 16) and R.narrow_clusters(600) == (2, 10) and R.narrow_clusters(999) == (2, 16)
    assert R.narrow_clusters(2313) == (5, 15) and R.narrow_clusters(16640) == (33, 16)       # (the sizes of the parity test)
    assert R.cluster_sample(600, 10) == [0, 9, 10, 18] and R.cluster_sample(999, 16) == [0, 15, 16, 31]
    assert R.leg_sample("wide_full128", R.FULL_BIG_NSEQ, (20, 24)) == R.tiles_to_seqs([0, 19, 23, 240, 256], R.FULL_BIG_NSEQ)
    for row, r in R.ROWS.items():
        s = R.row_sample(row)
        assert len(s) >= 64 and len(set(s)) == len(s), row
        for nseq in ((r["nseq"],) if r["gen"] == "normal" else (40, 200)):
            leg = R.leg_sample(row, nseq)
            assert set(leg) <= set(s) and set(range(min(32, nseq))) <= set(leg) and nseq - 1 in leg, (row, nseq)
            assert len(leg) >= min(64, nseq)
    assert set(R.DELTA) == set(R.ORACLE) == set(R.ROWS)


@pytest.mark.parametrize("row", sorted(R.ROWS))
def test_committed_oracle_distance_is_what_the_oracle_measures(row):
    """DELTA = 8 x ORACLE is only a derived gate while ORACLE is what the fp32 oracle really sits at on the row's inputs."""
    s = R.measure_oracle(row, torch)
    print("%s: oracle vs step-consistent max %.3g mean %.3g; |h| > 0.99: %.3f %%; committed %.3g"
          % (row, s["max"], s["mean"], 100 * s["sat"], R.ORACLE[row]))
    assert s["finite"]
    assert 0.5 * R.ORACLE[row] <= s["max"] <= 2.0 * R.ORACLE[row], (s["max"], R.ORACLE[row])
    assert R.DELTA[row] == R.MARGIN * R.ORACLE[row] and R.MARGIN == 8
    if row.endswith("_sat"):
        assert 0.0005 <= s["sat"] <= 0.05, s["sat"]
