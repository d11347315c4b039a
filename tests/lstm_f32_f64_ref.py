"""Step-consistent float64 reference of the fp32 LSTM forward kernels (csrc/lstm_kernel.h, lstm_static*.h, lstm_split*.h,
lstm_f32c.h, lstm_train.h, with the cell update of lstm_wave.h), the seeded inputs, the sampling of the big launches and the
table of gates.  numpy (+ torch integer ops for the generator that gives the same bits on the host and on the device);
imported by tests/test_lstm_f32_f64_ref_host.py and tests/test_gpu_lstm_f32_f64.py.

The method is that of tests/lstm_bf16_f64_ref.py with the operand rounding taken out: the gates of step t are formed in
float64 from the operands exactly as the kernel receives them — x_t in float32 (the float32 sum x0 + x1 where the call
passes x1, the concatenated x2 channels appended), the float32 weights, the bias as fnssl_lstm_pack forms it,
float32(b_ih + b_hh), and h^dev_{t-1}, the row the kernel stored one step earlier — and only the reference's own float64
cell state is carried.  A kernel that is right at every step agrees at every step to fp32 gate-math error; one that is
wrong at step t disagrees at step t, and the recurrence's contraction cannot hide it.
"""
import numpy as np

import lstm_bf16_f64_ref as B
from oracle import fnssl_oracle as O

F32, F64 = np.float32, np.float64
MARGIN = B.MARGIN
check_f32, f32_stats, counter_block = B.check_f32, B.f32_stats, B.counter_block
SFX = ("", "_reverse")


def _same(a):
    return np.asarray(a, dtype=F32)


def packed_bias(b_ih, b_hh):
    """fnssl_lstm_pack (csrc/lstm.hip): one float32 addition per gate row."""
    return (np.asarray(b_ih, dtype=F32) + np.asarray(b_hh, dtype=F32)).astype(F32)


def step_consistent(x, w_ih, w_hh, b_ih, b_hh, h_dev, reverse=False, info=None):
    """x [N, T, I] float32 as the kernel forms it, h_dev [N, T, H] what the kernel stored -> float64 [N, T, H]."""
    return B.step_consistent(x, w_ih, w_hh, b_ih, b_hh, h_dev, reverse, rnd=_same, bias=packed_bias(b_ih, b_hh), info=info)


def step_consistent_layer(x, sd, h_dev, bidir, prefix="L.", info=None):
    """nn.LSTM layer: the forward direction on the first H output columns, the reverse one on the last H."""
    p = lambda n: sd[prefix + n]  # noqa: E731
    H = p("weight_hh_l0").shape[1]
    refs = []
    for k, s in enumerate(SFX[:2 if bidir else 1]):
        refs.append(step_consistent(x, p("weight_ih_l0" + s), p("weight_hh_l0" + s), p("bias_ih_l0" + s), p("bias_hh_l0" + s),
                                    h_dev[..., k * H:(k + 1) * H], reverse=k == 1, info=info))
    return np.concatenate(refs, axis=-1)


def free_running(x, sd, bidir, prefix="L.", store=lambda h: h):
    """The same arithmetic fed by its OWN h (through `store`: what the next step reads of it); with the identity that is what
    torch.nn.LSTM computes in float64 (host test).  Returns the h before `store`."""
    p = lambda n: sd[prefix + n]  # noqa: E731
    x = np.asarray(x, dtype=F32).astype(F64)
    N, T, _ = x.shape
    outs = []
    for k, s in enumerate(SFX[:2 if bidir else 1]):
        wih, whh = p("weight_ih_l0" + s).astype(F64), p("weight_hh_l0" + s).astype(F64)
        bias = packed_bias(p("bias_ih_l0" + s), p("bias_hh_l0" + s)).astype(F64)
        H = whh.shape[1]
        h, c = np.zeros((N, H)), np.zeros((N, H))
        out = np.empty((N, T, H))
        for t in (range(T - 1, -1, -1) if k else range(T)):
            g = x[:, t] @ wih.T + h @ whh.T + bias
            c = B._sig(g[:, H:2 * H]) * c + B._sig(g[:, :H]) * np.tanh(g[:, 2 * H:3 * H])
            out[:, t] = B._sig(g[:, 3 * H:]) * np.tanh(c)
            h = store(out[:, t])
        outs.append(out)
    return np.concatenate(outs, axis=-1)


# --------------------------------------------------------------------------- the cuts of a launch, restated
MI355X_CUS = 256
ROUND_WAVES_H256 = 12      # the full-chip narrow-band round: one workgroup of 12 waves per CU (Fp32Call::launch_round_interleaved_h256)
BIG128_WAVES = 8           # fnssl_lstm_plan_rounds(128, 8193, 2, 256): one round of 8-wave workgroups (both pinned in the host test)


def groups_of(nseq):
    return (nseq + 15) // 16


def round_cut(nseq, waves):
    """Group numbers at which a round of `waves`-wave workgroups changes workgroup (lstm_wave.h: task = wg * NW + wave): the
    first boundary (last wave of workgroup 0 | first of workgroup 1) and the last."""
    wgs = (groups_of(nseq) + waves - 1) // waves
    return sorted({waves, (wgs - 1) * waves}) if wgs > 1 else []


def f32c_cut(nseq, H, ndir, ncu=MI355X_CUS):
    """(clusters per direction, groups per cluster) of forward_f32c (csrc/lstm_f32c.hip): clusters of H / 16 CUs, the groups
    dealt out in consecutive blocks (lstm_f32c.h: g0 = cluster * groups_per_cluster)."""
    cpd = (ncu // (H // 16)) // ndir
    return cpd, (groups_of(nseq) + cpd - 1) // cpd


def cluster_cut(nseq, H, ndir, ncu=MI355X_CUS):
    """Group numbers at which the cluster changes: behind the first cluster and in front of the last one."""
    gpc = f32c_cut(nseq, H, ndir, ncu)[1]
    ncl = (groups_of(nseq) + gpc - 1) // gpc
    return sorted({gpc, (ncl - 1) * gpc}) if ncl > 1 else []


def sample(nseq, cut=()):
    """Sequence numbers a leg checks (all steps of each): everything up to 256 sequences; else the whole first group, the ragged
    last one, the groups on either side of every boundary in `cut`, and evenly spaced groups until there are 64 sequences."""
    if nseq <= 256:
        return list(range(nseq))
    n = groups_of(nseq)
    g = {0, n - 1}
    for b in cut:
        if 0 < b < n:
            g |= {b - 1, b}
    k = 2
    while sum(min(16, nseq - 16 * t) for t in g) < 64:
        g |= {(n * j) // k for j in range(1, k)}
        k += 1
    return sorted({s for t in g for s in range(16 * t, min(16 * t + 16, nseq))})


# --------------------------------------------------------------------------- rows: one seeded input set each
# Sequence s of a row has the same values whatever the batch (counter_block), so legs of one shape at several sizes share a
# row.  x1: the call passes a second summed input.  kind: "plain" (largest |pre-activation| of the reference >= 2), "sat"
# (weights x 4, inputs x 3: 0.05 % - 5 % of reference |h| > 0.99), "ovf" (weights x 16, inputs x 8: |pre-activation| > 89, so
# exp(-x) and exp(2x) overflow float32 in some units).  use: only the first `use` steps (rows of their own: the oracle is
# closer there, and so is the gate).
NARROW_STEPS, FULL_STEPS, FULL_STEPS_STFT = 300, 256, 257
BIG_STEPS = 40
BIG_NSEQ = 49125           # 3071 groups, 5 sequences in the last: the smallest ragged size that selects the full-chip rounds
BIG128_NSEQ, BIG128_STEPS = 8193, 64
SUM_STEPS = 20             # a leg with skip / out_sum holds four tensors of this size: 20 steps keep it under 4 GB


def _row(H, bidir, c0, c2, nsteps, seed, xscale=1.0, wscale=1.0, x1=False, kind="plain"):
    return dict(H=H, bidir=bidir, c0=c0, c2=c2, nsteps=nsteps, seed=seed, xscale=xscale, wscale=wscale, x1=x1, kind=kind, use=None)


ROWS = {
    "big256": _row(256, False, 256, 0, BIG_STEPS, 8400),
    "big256_sum": _row(256, False, 256, 0, SUM_STEPS, 8405),
    "big260": _row(256, False, 256, 4, SUM_STEPS, 8410),      # (lstm_static3.h / lstm_static4.h take [256 | 4] with out_sum only)
    "big256_sat": _row(256, False, 256, 0, BIG_STEPS, 8420, xscale=3.0, wscale=4.0, kind="sat"),
    "big128": _row(128, True, 256, 4, BIG128_STEPS, 8430),
    "g16": _row(16, True, 4, 0, FULL_STEPS_STFT, 8440, xscale=3.0),
    "g32": _row(32, False, 32, 4, NARROW_STEPS, 8450, xscale=3.0),
    "g64": _row(64, False, 48, 20, FULL_STEPS_STFT, 8460, xscale=3.0),
    "g64bi": _row(64, True, 48, 20, FULL_STEPS, 8465, xscale=3.0),
    "n256": _row(256, False, 256, 0, NARROW_STEPS, 8470),
    "n260": _row(256, False, 256, 4, NARROW_STEPS, 8480),
    "n256_120": _row(256, False, 256, 0, 120, 8490),
    "n256bi": _row(256, True, 256, 0, NARROW_STEPS, 8500),
    "f128": _row(128, True, 256, 0, FULL_STEPS, 8510),
    "f128_257": _row(128, True, 256, 0, FULL_STEPS_STFT, 8515),
    "n128x1": _row(128, False, 256, 0, NARROW_STEPS, 8520, x1=True),
    "t128": _row(128, True, 256, 4, FULL_STEPS_STFT, 8530),
    "n256_sat": _row(256, False, 256, 0, NARROW_STEPS, 8540, xscale=3.0, wscale=4.0, kind="sat"),
    "n256_ovf": _row(256, False, 256, 0, BIG_STEPS, 8550, xscale=8.0, wscale=16.0, kind="ovf"),
}


# --------------------------------------------------------------------------- legs
# name -> row, sequences, layout ("narrow": sequences are the bins, steps the frames), the family fnssl_lstm_plan must answer,
# tuning knobs (on top of an all-default Tuning), cut ("round": workgroups of `waves` waves; "cluster"; None), extras:
# variant, sum (skip / out_sum), reserve (training forward), carry (25 calls of 12 frames), use (first steps only).
def _leg(row, nseq, mode, family, knobs=None, cut=None, waves=ROUND_WAVES_H256, **extras):
    return dict(row=row, nseq=nseq, mode=mode, family=family, knobs=knobs or {}, cut=cut, waves=waves, extras=extras)


BIG = dict(no_f32_small=1)
LEGS = {
    # full-chip narrow-band rounds, H = 256
    "static4_256": _leg("big256", BIG_NSEQ, "narrow", "static4", BIG, "round"),
    "static4_256_sum": _leg("big256_sum", BIG_NSEQ, "narrow", "static4", BIG, "round", sum=True),
    "static_256": _leg("big256", BIG_NSEQ, "narrow", "static", dict(BIG, no_static3=1), "round"),
    "static4_260": _leg("big260", BIG_NSEQ, "narrow", "static4", BIG, "round", sum=True),
    "static3_260": _leg("big260", BIG_NSEQ, "narrow", "static3", dict(BIG, no_static4=1), "round", sum=True),
    "static4_256_sat": _leg("big256_sat", BIG_NSEQ, "narrow", "static4", BIG, "round"),
    # H = 128 full-chip rounds ([256 | 4] is no cluster shape), both directions, fused residual
    "static_128": _leg("big128", BIG128_NSEQ, "narrow", "static", {}, "round", waves=BIG128_WAVES, sum=True),
    # families that few sequences select, at real step counts
    "generic_16": _leg("g16", 37, "full", "generic"),
    "generic_32": _leg("g32", 37, "narrow", "generic"),
    "generic_64": _leg("g64", 37, "full", "generic"),
    "split_static_256": _leg("n256bi", 37, "narrow", "split_static"),
    "split_128_x1": _leg("n128x1", 37, "narrow", "split"),
    "train_128": _leg("t128", 37, "full", "train", reserve=True),
    # the cluster-resident kernel in each form (lstm_f32c.hip: forward_f32c)
    "cluster_256_6": _leg("n256", 6 * 256, "narrow", "f32_cluster", cut="cluster", sum=True),           # 6 groups per cluster: row held
    "cluster_260_6": _leg("n260", 6 * 256, "narrow", "f32_cluster", cut="cluster", sum=True),
    "cluster_260_1": _leg("n260", 256, "narrow", "f32_cluster", cut="cluster"),                         # one per cluster: gate split
    "cluster_256_ragged": _leg("n256", 750, "narrow", "f32_cluster", cut="cluster"),                    # 46 groups + 14 sequences
    "cluster_260_11": _leg("n260", 11 * 250, "narrow", "f32_cluster", cut="cluster", sum=True),         # 11 per cluster: streamed row
    "cluster_256_40": _leg("n256_120", 40 * 256, "narrow", "f32_cluster", cut="cluster"),               # 40 per cluster: groups change hands
    "cluster_128_16": _leg("f128", 249, "full", "f32_cluster", cut="cluster", sum=True),                # 16 groups per direction
    "cluster_128_15": _leg("f128_257", 240, "full", "f32_cluster", cut="cluster"),                      # 15: fewer than clusters
    "cluster_256_6_split4": _leg("n256", 6 * 256, "narrow", "f32_cluster", dict(f32c_gate_split=4), "cluster"),
    "cluster_260_1_split1": _leg("n260", 256, "narrow", "f32_cluster", dict(f32c_gate_split=1), "cluster"),
    "cluster_128_16_split1": _leg("f128", 249, "full", "f32_cluster", dict(f32c_gate_split=1), "cluster"),
    "cluster_128_15_split4": _leg("f128_257", 240, "full", "f32_cluster", dict(f32c_gate_split=4), "cluster"),
    "cluster_256_carried": _leg("n256", 256, "narrow", "f32_cluster", cut="cluster", carry=12),
    # saturated gates and float32 overflow of both exponentials
    "cluster_256_sat": _leg("n256_sat", 6 * 256, "narrow", "f32_cluster", cut="cluster"),
    "generic_256_sat": _leg("n256_sat", 37, "narrow", "generic", variant=4),
    "cluster_256_ovf": _leg("n256_ovf", 6 * 256, "narrow", "f32_cluster", cut="cluster"),
    "generic_256_ovf": _leg("n256_ovf", 37, "narrow", "generic", variant=4),
}
for _v in range(1, 9):       # every launch geometry of the generic kernel (kVariants)
    LEGS["generic_256_v%d" % _v] = _leg("n256", 37, "narrow", "generic", variant=_v)
    LEGS["generic_128_v%d" % _v] = _leg("f128", 37, "full", "generic", variant=_v)
# first steps: h_{-1} = 0 alone, then the first recurrent operand; one leg per family, the bidirectional ones cover the
# reverse direction, whose first step is the LAST row
LEGS["generic_64bi"] = _leg("g64bi", 37, "full", "generic")
FIRST_OF = {"static4": "static4_260", "static3": "static3_260", "static_256": "static_256", "static_128": "static_128",
            "generic_16": "generic_16", "generic_64": "generic_64bi", "split_static": "split_static_256", "split": "split_128_x1",
            "train": "train_128", "f32_cluster_128": "cluster_128_16", "f32_cluster_256": "cluster_260_6"}
for _f, _l in sorted(FIRST_OF.items()):
    for _k in (1, 2):
        LEGS["first%d_%s" % (_k, _f)] = dict(LEGS[_l], extras=dict(LEGS[_l]["extras"], use=_k))


def leg_row(name):
    """The row whose gate a leg is held to: its input row, or that row cut to the leg's first steps."""
    leg = LEGS[name]
    use = leg["extras"].get("use")
    return leg["row"] if use is None else "%s_s%d" % (leg["row"], use)


for _n in list(LEGS):
    if leg_row(_n) not in ROWS:
        ROWS[leg_row(_n)] = dict(ROWS[LEGS[_n]["row"]], use=LEGS[_n]["extras"]["use"])

def leg_cut(name, ncu=MI355X_CUS):
    leg = LEGS[name]
    r = ROWS[leg["row"]]
    if leg["cut"] == "round":
        return round_cut(leg["nseq"], leg["waves"])
    if leg["cut"] == "cluster":
        return cluster_cut(leg["nseq"], r["H"], 2 if r["bidir"] else 1, ncu)
    return []


def leg_sample(name):
    return sample(LEGS[name]["nseq"], leg_cut(name))


def row_sample(row):
    """The sequences ORACLE[row] is measured on: the union of the samples of the row's legs."""
    s = set()
    for n in LEGS:
        if leg_row(n) == row:
            s |= set(leg_sample(n))
    return sorted(s)


def row_steps(row):
    r = ROWS[row]
    return r["use"] or r["nsteps"]


def row_state(row):
    from fnssl import weights as W
    r = ROWS[row]
    shapes = [("L." + n, s) for n, s in W.lstm_param_shapes(r["c0"] + r["c2"], r["H"], r["bidir"])]
    return W.make_state(shapes, seed=r["seed"], scale=r["wscale"])


def row_inputs(row, seqs, torch, device="cpu"):
    """(x0, x1, x2) of the named sequences, float32 [len(seqs), nsteps, C] torch tensors on `device` (x1 / x2: None where the
    row has none).  Every step of the row: a `use` row is cut by the caller."""
    r = ROWS[row]
    seqs = torch.as_tensor(seqs, dtype=torch.int64)
    x1scale = r["xscale"] * (0.5 ** 0.5 if r["x1"] else 1.0)          # (x0 + x1 has the row's scale)
    blk = lambda k, ch: counter_block(torch, seqs, r["nsteps"], ch, r["seed"] + k, x1scale if k < 3 else r["xscale"], True, device)  # noqa: E731
    return blk(1, r["c0"]), (blk(2, r["c0"]) if r["x1"] else None), (blk(3, r["c2"]) if r["c2"] else None)


def row_skip(row, seqs, torch, device="cpu", nsteps=None):
    """The residual a `sum` leg adds (no operand of the recurrence): float32 [len(seqs), nsteps, ndir * H]."""
    r = ROWS[row]
    return counter_block(torch, torch.as_tensor(seqs, dtype=torch.int64), nsteps or r["nsteps"], (2 if r["bidir"] else 1) * r["H"],
                         r["seed"] + 4, 0.5, True, device)


def kernel_x(x0, x1, x2):
    """The layer input as the kernel forms it: float32(x0 + x1), the x2 channels appended (numpy)."""
    x = x0 if x1 is None else (x0.astype(F32) + x1.astype(F32)).astype(F32)
    return x if x2 is None else np.concatenate([x, x2], axis=-1)


def row_x(row, seqs, torch):
    x0, x1, x2 = (None if t is None else t.numpy() for t in row_inputs(row, seqs, torch))
    return np.ascontiguousarray(kernel_x(x0, x1, x2)[:, :row_steps(row)])


def measure_oracle(row, torch):
    """max / mean |float32 oracle - step-consistent reference driven by the oracle's own output| on the row's sample, and the
    input conditions, taken on the reference."""
    r = ROWS[row]
    x = row_x(row, row_sample(row), torch)
    sd = row_state(row)
    with np.errstate(over="ignore"):
        want = O.lstm(x, sd, "L.", r["bidir"])
    info = {}
    ref = step_consistent_layer(x, sd, want, r["bidir"], info=info)
    s = f32_stats(want, ref)
    s.update(sat=float((np.abs(ref) > 0.99).mean()), finite=bool(np.isfinite(ref).all()), oracle_finite=bool(np.isfinite(want).all()),
             pre=info["pre"], nseq=x.shape[0])
    return s


def check_conditions(kind, pre, sat, what=""):
    """The conditions on a row's inputs, on the float64 reference (never on the kernel)."""
    if kind == "plain":
        assert pre >= 2.0, "%s: largest |pre-activation| %.3g < 2: the gate functions are only evaluated near 0" % (what, pre)
    elif kind == "sat":
        assert 0.0005 <= sat <= 0.05, "%s: %.4f %% of |h| > 0.99 is not a saturated-gate input" % (what, 100 * sat)
    else:
        assert pre > 89.0, "%s: largest |pre-activation| %.3g does not overflow exp(-x) / exp(2x) in float32" % (what, pre)


# --------------------------------------------------------------------------- the gates
# ORACLE[row]: max over the row's sample and all its steps of |O.lstm(...) - step_consistent(driven by that output)|, measured
# on the CPU on the row's own seeded inputs (tests/test_lstm_f32_f64_ref_host.py re-measures each and fails when a figure is
# more than 2 x off).  DELTA[row] = MARGIN * ORACLE[row]; DESIGN section 7 carries a copy.  Never taken from a kernel.
ORACLE = {
    "big256_sum": 3.54e-07, "big256": 4.69e-07, "big260": 3.23e-07, "big256_sat": 6.23e-06, "big128": 6.75e-07, "g16": 1.81e-07,
    "g32": 6.03e-07, "g64": 8.09e-07, "g64bi": 8.59e-07, "n256": 4.87e-07, "n260": 5.58e-07,
    "n256_120": 4.30e-07, "n256bi": 4.62e-07, "f128": 7.99e-07, "f128_257": 8.10e-07, "n128x1": 5.83e-07,
    "t128": 7.06e-07, "n256_sat": 9.26e-06, "n256_ovf": 5.07e-05, "f128_s1": 3.82e-07,
    "f128_s2": 5.09e-07, "n260_s1": 2.50e-07, "n260_s2": 2.78e-07, "g16_s1": 8.78e-08, "g16_s2": 8.88e-08,
    "g64bi_s1": 4.83e-07, "g64bi_s2": 6.61e-07, "n128x1_s1": 2.26e-07, "n128x1_s2": 3.86e-07, "n256bi_s1": 2.19e-07,
    "n256bi_s2": 2.81e-07, "big260_s1": 2.20e-07, "big260_s2": 3.23e-07, "big128_s1": 3.53e-07, "big128_s2": 4.25e-07,
    "big256_s1": 2.59e-07, "big256_s2": 2.59e-07, "t128_s1": 3.77e-07, "t128_s2": 4.08e-07,
}
DELTA = {k: MARGIN * v for k, v in ORACLE.items()}
