"""Pin tests/lstm_f32_f64_ref.py (the step-consistent float64 reference the fp32 LSTM forward kernels are held to in
test_gpu_lstm_f32_f64.py).  CPU only: the committed table of oracle distances, re-measured, with the conditions on every row's
inputs; the reference against torch.nn.LSTM in float64; the restated cuts of the launches and the samples built on them; and
the mutants the method claims, restated in numpy — each asserted separable (margin printed) or listed as not separable."""
import ctypes as C

import numpy as np
import pytest
import torch

import lstm_bf16_f64_ref as B
import lstm_f32_f64_ref as R
from oracle import fnssl_oracle as O

F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("row", sorted(R.ROWS))
def test_committed_oracle_distance_and_input_conditions(row):
    """DELTA = 8 x ORACLE is only a derived gate while ORACLE is what the fp32 oracle really sits at on the row's inputs."""
    r = R.ROWS[row]
    s = R.measure_oracle(row, torch)
    print("%s: %d sequences x %d steps, oracle vs step-consistent max %.3g mean %.3g; largest |pre-activation| %.3g; |h| > 0.99: "
          "%.4f %%; committed %.3g" % (row, s["nseq"], R.row_steps(row), s["max"], s["mean"], s["pre"], 100 * s["sat"], R.ORACLE[row]))
    assert s["finite"] and s["oracle_finite"]
    assert s["nseq"] >= min(64, min(R.LEGS[n]["nseq"] for n in R.LEGS if R.leg_row(n) == row))
    assert 0.5 * R.ORACLE[row] <= s["max"] <= 2.0 * R.ORACLE[row], (s["max"], R.ORACLE[row])
    assert R.DELTA[row] == R.MARGIN * R.ORACLE[row] and R.MARGIN == 8 == B.MARGIN
    R.check_conditions(r["kind"], s["pre"], s["sat"], row)
    if r["kind"] == "plain":
        assert R.DELTA[row] <= 8e-6, "a plain row's gate is a few 1e-6, not the old 1e-5 + 1e-4 |h|"


def test_table_covers_every_row_and_every_fp32_forward_family():
    assert set(R.DELTA) == set(R.ORACLE) == set(R.ROWS)
    assert {leg["family"] for leg in R.LEGS.values()} == {"generic", "static", "static3", "static4", "split", "split_static",
                                                          "f32_cluster", "train"}
    for n in R.LEGS:
        assert R.leg_row(n) in R.ROWS, n
    # the first steps: one and two, for every family, the bidirectional rows among them (reverse: the first step is the last row)
    firsts = [n for n in R.LEGS if n.startswith("first")]
    assert {R.LEGS[n]["family"] for n in firsts} == {leg["family"] for leg in R.LEGS.values()}
    assert {R.LEGS[n]["extras"]["use"] for n in firsts} == {1, 2}
    for fam in ("generic", "static", "split_static", "train", "f32_cluster"):
        assert any(R.ROWS[R.LEGS[n]["row"]]["bidir"] for n in firsts if R.LEGS[n]["family"] == fam), fam


@pytest.mark.parametrize("H,I,bidir,T", [(256, 260, False, 40), (128, 256, True, 33), (16, 4, True, 57)])
def test_reference_is_a_float64_lstm(H, I, bidir, T):
    """Free-running, the reference's arithmetic is torch.nn.LSTM's in float64 (the bias as the packer forms it: one float32
    sum); driven by the float32 rows of such a run it returns that run's unrounded h — at 1e-12."""
    from fnssl import weights as W
    sd = W.make_state([("L." + n, s) for n, s in W.lstm_param_shapes(I, H, bidir)], seed=9400 + H)
    x = R.counter_block(torch, torch.arange(5), T, I, 9401, 1.0, True).numpy()
    free = R.free_running(x, sd, bidir)
    m = torch.nn.LSTM(I, H, 1, batch_first=True, bidirectional=bidir).double()
    with torch.no_grad():
        for s in R.SFX[:2 if bidir else 1]:
            getattr(m, "weight_ih_l0" + s).copy_(torch.from_numpy(sd["L.weight_ih_l0" + s]).double())
            getattr(m, "weight_hh_l0" + s).copy_(torch.from_numpy(sd["L.weight_hh_l0" + s]).double())
            getattr(m, "bias_ih_l0" + s).copy_(torch.from_numpy(R.packed_bias(sd["L.bias_ih_l0" + s], sd["L.bias_hh_l0" + s])).double())
            getattr(m, "bias_hh_l0" + s).zero_()
        want = m(torch.from_numpy(x).double())[0].numpy()
    assert np.abs(free - want).max() <= 1e-12, np.abs(free - want).max()
    stored = R.free_running(x, sd, bidir, store=lambda h: h.astype(F32).astype(F64))       # h fed on as the float32 row
    ref = R.step_consistent_layer(x, sd, stored.astype(F32), bidir)
    assert ref.dtype == F64 and np.abs(ref - stored).max() <= 1e-12, np.abs(ref - stored).max()
    assert np.abs(stored - free).max() > 1e-9        # (the two runs are not the same thing: the stored row matters)


def test_generalised_step_consistent_keeps_the_bf16_reference():
    """The rounding argument's default is the bf16 module's behaviour, bit for bit: restated here from its parts."""
    from fnssl import weights as W
    sd = W.make_state([("L." + n, s) for n, s in W.lstm_param_shapes(32, 32, False)], seed=9410)
    a = [sd["L." + n] for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    x = B.fp32_block(9411, (3, 9, 32), 0.7)
    h = O.lstm_dir(x, *a, bf16=True)
    for rev in (False, True):
        got = B.step_consistent(x, *a, h, rev)
        xb, wi, wh, hb = (O.bf16_round(v).astype(F64) for v in (x, a[0], a[1], h))
        hp = np.zeros_like(hb)
        if rev:
            hp[:, :-1] = hb[:, 1:]
        else:
            hp[:, 1:] = hb[:, :-1]
        g = (xb.reshape(27, 32) @ wi.T + hp.reshape(27, 32) @ wh.T + (a[2].astype(F64) + a[3].astype(F64))).reshape(3, 9, 128)
        c = np.zeros((3, 32))
        want = np.empty((3, 9, 32))
        for t in (range(8, -1, -1) if rev else range(9)):
            c = B._sig(g[:, t, 32:64]) * c + B._sig(g[:, t, :32]) * np.tanh(g[:, t, 64:96])
            want[:, t] = B._sig(g[:, t, 96:]) * np.tanh(c)
        assert np.array_equal(got, want)
        assert not np.array_equal(got, R.step_consistent(x, *a, h, rev))


def test_cuts_and_samples():
    from fnssl import _lib
    lib = _lib.load()
    buf = (C.c_int * 16)()
    # the rounds the library plans on 256 CUs: one round each, of 12- and of 8-wave workgroups
    assert lib.fnssl_lstm_plan_rounds(256, R.BIG_NSEQ, 1, R.MI355X_CUS, buf, 16) == 1 and buf[0] == R.ROUND_WAVES_H256 == 12
    assert lib.fnssl_lstm_plan_rounds(128, R.BIG128_NSEQ, 2, R.MI355X_CUS, buf, 16) == 1 and buf[0] == R.BIG128_WAVES == 8
    assert R.groups_of(R.BIG_NSEQ) == 3071 and R.BIG_NSEQ - 16 * 3070 == 5
    assert R.round_cut(R.BIG_NSEQ, 12) == [12, 3060] and R.round_cut(R.BIG128_NSEQ, 8) == [8, 512] and R.round_cut(100, 12) == []
    # forward_f32c: clusters of H / 16 CUs; groups per cluster = ceil(groups / clusters per direction)
    assert R.f32c_cut(1536, 256, 1) == (16, 6) and R.f32c_cut(256, 256, 1) == (16, 1) and R.f32c_cut(750, 256, 1) == (16, 3)
    assert R.f32c_cut(2750, 256, 1) == (16, 11) and R.f32c_cut(10240, 256, 1) == (16, 40)
    assert R.f32c_cut(249, 128, 2) == (16, 1) and R.f32c_cut(240, 128, 2) == (16, 1) and R.f32c_cut(24576, 128, 2) == (16, 96)
    assert R.cluster_cut(1536, 256, 1) == [6, 90] and R.cluster_cut(750, 256, 1) == [3, 45] and R.cluster_cut(10240, 256, 1) == [40, 600]
    assert R.cluster_cut(2750, 256, 1) == [11, 165] and R.cluster_cut(16, 256, 1) == []
    seqs = lambda gs, n: [s for g in gs for s in range(16 * g, min(16 * g + 16, n))]  # noqa: E731
    assert R.sample(256) == list(range(256)) and R.sample(37) == list(range(37))
    assert R.sample(R.BIG_NSEQ, [12, 3060]) == seqs([0, 11, 12, 3059, 3060, 3070], R.BIG_NSEQ)
    assert R.sample(1536, [6, 90]) == seqs([0, 5, 6, 89, 90, 95], 1536)
    assert R.sample(750, [3, 45]) == seqs([0, 2, 3, 44, 45, 46], 750)
    assert R.sample(1000) == seqs([0, 21, 31, 42, 62], 1000)        # no boundary: first, last and evenly spaced groups up to 64
    for n, leg in R.LEGS.items():
        s = R.leg_sample(n)
        nseq = leg["nseq"]
        assert len(s) == len(set(s)) >= min(64, nseq) and (nseq > 256 or len(s) == nseq), n
        assert set(range(min(16, nseq))) <= set(s) and set(range(16 * (R.groups_of(nseq) - 1), nseq)) <= set(s), n
        assert set(s) <= set(R.row_sample(R.leg_row(n))), n
        if leg["cut"] and nseq > 256:
            assert R.leg_cut(n), n
            for b in R.leg_cut(n):
                assert {16 * (b - 1), 16 * b} <= set(s), (n, b)


def test_counter_rows_are_the_same_on_any_batch():
    a = R.row_inputs("n128x1", [0, 5, 4000], torch)
    b = R.row_inputs("n128x1", [5], torch)
    assert a[2] is None and a[1] is not None and torch.equal(a[0][1:2], b[0]) and torch.equal(a[1][1:2], b[1])
    assert not torch.equal(a[0], a[1])
    x = R.row_x("n128x1", [0, 5, 4000], torch)
    assert np.array_equal(x, (a[0].numpy() + a[1].numpy()).astype(F32)) and abs(float(x.std()) - 1.0) < 0.02
    x0, _, x2 = R.row_inputs("big260", [7], torch)
    assert x0.shape == (1, R.SUM_STEPS, 256) and x2.shape == (1, R.SUM_STEPS, 4)
    assert np.array_equal(R.row_x("big260_s2", [7], torch), np.concatenate([x0.numpy(), x2.numpy()], -1)[:, :2])


# --------------------------------------------------------------------------- mutants of the oracle
L2E2 = F32(2.8853900817779268)       # 2 log2(e), lstm_kernel.h tanh2: exp(2x) = exp2(x * 2 log2e)


def oracle_variant(x, w_ih, w_hh, b_ih, b_hh, tanh_mult=None, nan_form=False, drop_bhh=None, stale=None, zero_c_at=None,
                   swap_if=None):
    """O.lstm_dir in float32 (forward direction) with one fault at a time.  tanh_mult: tanh as 1 - 2 / (exp2(x * m) + 1) with
    this multiplier (the exact one restates the kernel's form); nan_form: (e - 1) / (e + 1) instead; drop_bhh, swap_if: a
    slice of hidden units whose gate rows lose b_hh / whose i and f rows are exchanged; stale: a slice of units whose h
    operand comes from step t - 2; zero_c_at: the step in front of which the cell state is zeroed."""
    x = np.asarray(x, dtype=F32)
    N, T, _ = x.shape
    H = w_hh.shape[1]
    b = (b_ih + b_hh).astype(F32).copy()
    if drop_bhh is not None:
        for q in range(4):
            b[q * H:(q + 1) * H][drop_bhh] = b_ih[q * H:(q + 1) * H][drop_bhh]
    xw = ((x.reshape(N * T, -1) @ w_ih.T.astype(F32)).reshape(N, T, 4 * H) + b).astype(F32)
    whhT = np.ascontiguousarray(w_hh.T.astype(F32))

    def tanh(v):
        if tanh_mult is None and not nan_form:
            return np.tanh(v, dtype=F32)
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp2((v * F32(L2E2 if tanh_mult is None else tanh_mult)).astype(F32), dtype=F32)
            if nan_form:
                return ((e - F32(1)) / (e + F32(1))).astype(F32)
            return (F32(1) - F32(2) / (e + F32(1))).astype(F32)

    h = np.zeros((N, H), dtype=F32)
    h2 = h.copy()
    c = np.zeros((N, H), dtype=F32)
    out = np.empty((N, T, H), dtype=F32)
    for t in range(T):
        hop = h
        if stale is not None:
            hop = h.copy()
            hop[:, stale] = h2[:, stale]
        with np.errstate(over="ignore"):
            g = (xw[:, t] + hop @ whhT).astype(F32)
            gi, gf = g[:, 0:H].copy(), g[:, H:2 * H].copy()
            if swap_if is not None:
                gi[:, swap_if], gf[:, swap_if] = g[:, H:2 * H][:, swap_if], g[:, 0:H][:, swap_if]
            i, f, o = O._sigmoid(gi), O._sigmoid(gf), O._sigmoid(g[:, 3 * H:4 * H])
        if zero_c_at == t:
            c = np.zeros_like(c)
        c = (f * c + i * tanh(g[:, 2 * H:3 * H])).astype(F32)
        h2, h = h, (o * tanh(c)).astype(F32)
        out[:, t] = h
    return out


def _case(row, nseq, nsteps):
    r = R.ROWS[row]
    sd = R.row_state(row)
    x0, x1, x2 = (None if t is None else t.numpy()[:, :nsteps] for t in R.row_inputs(row, list(range(nseq)), torch))
    a = [sd["L." + n] for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    assert not r["bidir"]
    return a, x0, x1, x2


TILE, QUAD = slice(16, 32), slice(4, 8)
# name, row, keyword of oracle_variant, separable at the row's gate?  The reason of each "no" is in DESIGN section 7.
MUTANTS = [
    ("tanh multiplier 2.886390 (4th digit)", "n256", dict(tanh_mult=F32(2.886390)), True),
    ("tanh multiplier 2.885490 (5th digit)", "n256", dict(tanh_mult=F32(2.885490)), True),
    # 3e-6 relative: |x| sech^2(x) <= 0.45 makes it at most 1.5e-6 on tanh, under a gate of 8 x the oracle's 3.8e-7
    ("tanh multiplier 2.885400 (6th digit)", "n256", dict(tanh_mult=F32(2.885400)), False),
    ("b_hh dropped on one 16-row tile", "n256", dict(drop_bhh=TILE), True),
    ("h operand of one quad from step t - 2", "n256", dict(stale=QUAD), True),
    ("cell state zeroed in front of step 12", "n256", dict(zero_c_at=12), True),
    ("i and f exchanged in one tile", "n256", dict(swap_if=TILE), True),
    ("x1 dropped", "n128x1", dict(), True),
    ("(e - 1) / (e + 1) tanh form", "n256_ovf", dict(nan_form=True), True),
]


@pytest.mark.parametrize("name,row,kw,separable", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutants_of_the_oracle(name, row, kw, separable):
    a, x0, x1, x2 = _case(row, 32, 40)
    x = R.kernel_x(x0, x1, x2)
    delta = R.DELTA[row]          # the gate of the row at its real step count: not tighter than that of these 40 steps
    with np.errstate(over="ignore"):
        good = oracle_variant(x, *a, tanh_mult=L2E2 if "tanh_mult" in kw else None)
        assert "tanh_mult" in kw or np.array_equal(good, O.lstm_dir(x, *a))
    R.check_f32(good, R.step_consistent(x, *a, good), delta, "the unmutated oracle")
    bad = oracle_variant(x0 if name == "x1 dropped" else x, *a, **kw)
    if kw.get("nan_form"):
        assert np.isnan(bad).any() and np.isfinite(good).all()
        with pytest.raises(AssertionError, match="non-finite"):
            R.check_f32(bad, R.step_consistent(x, *a, np.nan_to_num(bad)), delta, name)
        print("%s: NaN where exp2 overflows; 1 - 2 / (e + 1) stays finite" % name)
        return
    s = R.f32_stats(bad, R.step_consistent(x, *a, bad))
    print("%s: step-consistent max %.3g = %.3g x delta (%.3g)" % (name, s["max"], s["max"] / delta, delta))
    if separable:
        assert s["max"] > delta, "claimed separable"
        with pytest.raises(AssertionError, match="max .got - ref"):
            R.check_f32(bad, R.step_consistent(x, *a, bad), delta, name)
    else:
        assert s["max"] <= delta, "listed as not separable, but the gate catches it: move it"
