"""Step-consistent float64 reference of the bf16-MFMA LSTM kernels (csrc/lstm_bf16.h, lstm_bf16w.h, lstm_bf16p.h,
lstm_bf16c.h), its two checkers, the input builders and the table of gates.  numpy (+ torch integer ops for the one
generator that must give the same bits on the host and on the device); imported by the host test and the GPU test.

A free-running comparison of two bf16 recurrences has to absorb rounding flips: an h_{t-1} within an fp32 error of a
bf16 midpoint is rounded one way by the kernel and the other way by the reference, and the 2^-9 relative difference
travels on.  Here the reference is DRIVEN by the kernel's own stored output: the gates of step t are formed in
float64 from bf16(x_t), the bf16-rounded weights, the bias and bf16(h^dev_{t-1}) — the row the kernel stored one step
earlier, which is the operand it used (lstm_bf16w.h gate(): `hb4` is stored and staged; lstm_bf16.h stores `hn` and
feeds convert(hn)) — and only the reference's own float64 cell state is carried.  A kernel that is right at every
step agrees at every step to fp32 gate-math error; one that is wrong at step t disagrees at step t.
"""
import numpy as np

from oracle import fnssl_oracle as O

F32, F64 = np.float32, np.float64


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def step_consistent(x, w_ih, w_hh, b_ih, b_hh, h_dev, reverse=False, rnd=O.bf16_round, bias=None, info=None):
    """x [N, T, I] fp32, h_dev [N, T, H] (what the kernel stored, fp32 or bf16 values) -> float64 [N, T, H].
    The matrix products of all steps are one float64 product (no step depends on the reference's previous h); only
    c_t = f c + i g and h_t = o tanh(c_t) run sequentially.
    rnd: what the kernel does to x, the weights and the stored h where they enter the product (the bf16 kernels: nearest-even
    bf16; the fp32 kernels of tests/lstm_f32_f64_ref.py: nothing).  bias: the [4H] bias as the kernel adds it, when that is not
    the exact b_ih + b_hh.  info: a dict that receives "pre", the largest |gate pre-activation|."""
    x = np.asarray(x, dtype=F32)
    h_dev = np.asarray(h_dev, dtype=F32)
    N, T, I = x.shape
    H = w_hh.shape[1]
    assert h_dev.shape == (N, T, H), (h_dev.shape, (N, T, H))
    xb = rnd(x).astype(F64)
    wih, whh = rnd(w_ih).astype(F64), rnd(w_hh).astype(F64)
    if bias is None:
        bias = np.asarray(b_ih, dtype=F64) + np.asarray(b_hh, dtype=F64)
    bias = np.asarray(bias, dtype=F64)
    hp = np.zeros((N, T, H), dtype=F64)                       # the operand h_{t-1}: zero at the first step
    hb = rnd(h_dev).astype(F64)
    if reverse:
        hp[:, :-1] = hb[:, 1:]
    else:
        hp[:, 1:] = hb[:, :-1]
    g = (xb.reshape(N * T, I) @ wih.T + hp.reshape(N * T, H) @ whh.T + bias).reshape(N, T, 4 * H)
    if info is not None:
        info["pre"] = max(float(np.abs(g).max()), info.get("pre", 0.0))
    ig, fg = _sig(g[..., 0:H]), _sig(g[..., H:2 * H])
    gg, og = np.tanh(g[..., 2 * H:3 * H]), _sig(g[..., 3 * H:4 * H])
    c = np.zeros((N, H), dtype=F64)
    out = np.empty((N, T, H), dtype=F64)
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        c = fg[:, t] * c + ig[:, t] * gg[:, t]
        out[:, t] = og[:, t] * np.tanh(c)
    return out


def step_consistent_layer(x, sd, h_dev, bidir, prefix="L."):
    """nn.LSTM layer: the forward direction on the first H output columns, the reverse one on the last H."""
    p = lambda n: sd[prefix + n]  # noqa: E731
    H = p("weight_hh_l0").shape[1]
    refs = [step_consistent(x, p("weight_ih_l0"), p("weight_hh_l0"), p("bias_ih_l0"), p("bias_hh_l0"), h_dev[..., :H])]
    if bidir:
        refs.append(step_consistent(x, p("weight_ih_l0_reverse"), p("weight_hh_l0_reverse"), p("bias_ih_l0_reverse"),
                                    p("bias_hh_l0_reverse"), h_dev[..., H:], reverse=True))
    return np.concatenate(refs, axis=-1)


# --------------------------------------------------------------------------- checkers
def spacing_bf16(ref):
    """Distance between neighbouring bf16 values in the binade of |ref| (8 significant bits), floored at the smallest
    normal spacing.  A value that rounds UP to the next power of two still errs by at most half of this."""
    a = np.abs(np.asarray(ref, dtype=F64))
    _, e = np.frexp(a)                                        # |ref| in [2^(e-1), 2^e); frexp(0) = (0, 0)
    return np.ldexp(1.0, np.maximum(np.where(a == 0, -125, e), -125) - 8)


def f32_stats(got, ref):
    d = np.abs(np.asarray(got, dtype=F64) - ref)
    return {"max": float(d.max()), "mean": float(d.mean())}


def check_f32(got, ref, delta, what=""):
    """fp32 output (h observed before any rounding): max |got - ref| <= delta, over every element."""
    assert np.isfinite(got).all(), "%s: non-finite output" % what
    s = f32_stats(got, ref)
    assert s["max"] <= delta, "%s: max |got - ref| = %.3g > delta %.3g (mean %.3g)" % (what, s["max"], delta, s["mean"])
    return s


BIAS_MIN_REF = 2.0 ** -6
BIAS_TOL = 0.01
BIAS_MIN_N = 100000


def bf16_stats(got, ref):
    """excess: max over every element of |got - ref| - spacing/2 (what delta has to cover).
    bias: mean of (|got| - |ref|) / spacing over the elements with |ref| >= 2^-6 (n of them): 0 for round-to-nearest
    (standard error 0.29 / sqrt(n)), -0.5 for truncation."""
    got = np.asarray(got, dtype=F64)
    sp = spacing_bf16(ref)
    big = np.abs(ref) >= BIAS_MIN_REF
    n = int(big.sum())
    bias = float(((np.abs(got[big]) - np.abs(ref[big])) / sp[big]).mean()) if n else 0.0
    return {"excess": float((np.abs(got - ref) - 0.5 * sp).max()), "bias": bias, "n": n,
            "max": float(np.abs(got - ref).max())}


def check_bf16(got, ref, delta, what=""):
    """bf16 output.  (1) every element within half a bf16 spacing of the reference, plus delta; (2) the rounding is
    unbiased: |bias| <= 0.01 over at least 1e5 elements (10 sigma of a correct rounding; truncation gives -0.5)."""
    assert np.isfinite(got).all(), "%s: non-finite output" % what
    s = bf16_stats(got, ref)
    assert s["excess"] <= delta, "%s: half-spacing bound exceeded by %.3g > delta %.3g" % (what, s["excess"], delta)
    assert s["n"] >= BIAS_MIN_N, "%s: only %d elements with |ref| >= 2^-6; the bias bound is derived for 1e5" % (what, s["n"])
    assert abs(s["bias"]) <= BIAS_TOL, "%s: rounding bias %.4f spacings (n = %d) outside +-%.2f" % (what, s["bias"], s["n"], BIAS_TOL)
    return s


# --------------------------------------------------------------------------- inputs
def force_ties(bits, flat_index):
    """uint32 patterns of fp32 values -> patterns that are NOT bf16-representable, exactly one element of every eight
    consecutive ones on an exact tie: low 16 bits 0x8000, the kept mantissa's last bit 0 or 1, so nearest-even rounds
    half of them down and half up while round-half-away rounds all of them away from zero.  Which of the eight, and
    which parity, is a hash of the group's number: every channel (every lane position of the in-kernel conversion)
    meets ties of both parities.  Works on numpy arrays and on torch int64 tensors alike (integer operations only;
    products are masked to 32 bits, so int64 wrap-around does not matter)."""
    M = 0xFFFFFFFF
    low = bits & 0xFFFF
    bits = bits | (1 - ((low + 0xFFFF) >> 16))                # a representable value (low half 0) moves one fp32 ulp
    h = (((flat_index >> 3) & M) * 0x9E3779B1) & M
    h = ((h ^ (h >> 15)) * 0x85EBCA6B) & M
    h = h ^ (h >> 13)
    tie = 1 - ((((flat_index ^ h) & 7) + 7) >> 3)             # 1 at position (h & 7) of the group of eight
    odd = (h >> 3) & 1
    tied = (bits & 0xFFFE0000) | (odd << 16) | 0x8000
    return tie * tied + (1 - tie) * bits


def fp32_block(seed, shape, scale=1.0):
    """Input builder for the blocks the kernels convert themselves (kW_F0 / kW_F2, and all of lstm_bf16.h's x):
    seeded normals * scale, passed through force_ties."""
    a = (np.random.RandomState(int(seed)).standard_normal(size=tuple(shape)) * scale).astype(F32)
    bits = a.reshape(-1).view(np.uint32).astype(np.int64)
    idx = np.arange(bits.size, dtype=np.int64)
    return force_ties(bits, idx).astype(np.uint32).view(F32).reshape(shape)


def counter_block(torch, seqs, nsteps, ch, seed, scale, ties, device="cpu"):
    """Counter-based generator for the batches that are built ON THE DEVICE (tens of thousands of sequences, of which the
    host needs a sample): element (sequence s, step t, channel c) is a function of (seed, s, t, c) alone, computed
    with integer operations and one exactly-rounded fp32 multiplication, so the device tensor and the host's rows
    carry the same bits.  Sum of four 16-bit uniforms (variance-matched to a normal; 2.6e5 levels), * scale.
    seqs: 1-D int64 tensor of sequence numbers -> float32 [len(seqs), nsteps, ch]; ties: force_ties, else the values
    are rounded to bf16 (the bf16 block is representable by construction)."""
    M = 0xFFFFFFFF
    s = seqs.to(device=device, dtype=torch.int64).view(-1, 1, 1)
    t = torch.arange(nsteps, device=device, dtype=torch.int64).view(1, -1, 1)
    c = torch.arange(ch, device=device, dtype=torch.int64).view(1, 1, -1)
    idx = (s * nsteps + t) * ch + c

    def mix(z):
        z = z & M
        z = ((z ^ (z >> 16)) * 0x85EBCA6B) & M
        z = ((z ^ (z >> 13)) * 0xC2B2AE35) & M
        return z ^ (z >> 16)

    z1 = mix(idx * 0x9E3779B1 + int(seed))
    z2 = mix(z1 + 0x7F4A7C15 + (idx >> 32))
    u = (z1 & 0xFFFF) + (z1 >> 16) + (z2 & 0xFFFF) + (z2 >> 16) - 131070
    x = u.to(torch.float32) * float(np.float32(scale / 37837.2))          # |u| < 2^24: exact; one rounding
    if not ties:
        return x.bfloat16().float()
    bits = x.view(torch.int32).to(torch.int64) & M
    bits = force_ties(bits, idx)
    return (bits - ((bits >> 31) << 32)).to(torch.int32).view(torch.float32)


# --------------------------------------------------------------------------- the rows: shapes, seeds, samples
# A row is one seeded input set (shape, weights, x) and the sequences on which the fp32 oracle's step-consistent distance
# was measured for it.  gen "normal": numpy normals through fp32_block (the whole x is fp32: lstm_bf16.h converts all of
# it).  gen "counter": counter_block — [c0 bf16-representable | c2 fp32 with ties], or c0 fp32 with ties when c2 = 0
# (block 1); sequence s has the same values whatever the batch, so the 40-, 200-, 600-, 999- and 8199-sequence legs of a shape
# are prefixes of one another and share the row.
def _row(gen, mode, H, bidir, c0, c2, nsteps, seed, wscale=1.0, xscale=0.7, nseq=None, use=None):
    return dict(gen=gen, mode=mode, H=H, bidir=bidir, c0=c0, c2=c2, nsteps=nsteps, seed=seed, wscale=wscale, xscale=xscale,
                nseq=nseq, use=use)


NARROW_STEPS, FULL_STEPS, FULL_STEPS_BF16 = 300, 256, 257     # 300 frames; IPDnet's 256 bins; the 257 bins of a 512-point STFT
BF16_NSEQ = 16 * 4 + 7                                        # lstm_bf16.h: 16-sequence groups, the last one ragged
# the shapes of test_lstm_bf16_layer_matches_bf16_oracle (tests/test_gpu_parity.py)
BF16_SHAPES = [("narrow", 256, False, 256, 16), ("full", 128, True, 256, 16), ("full", 128, True, 16, 0),
               ("narrow", 128, False, 128, 16), ("full", 64, True, 128, 16), ("full", 64, True, 16, 0),
               ("narrow", 128, True, 256, 16)]
ROWS = {}
for _i, (_m, _H, _b, _c0, _c2) in enumerate(BF16_SHAPES):
    ROWS["bf16_%d" % _i] = _row("normal", _m, _H, _b, _c0, _c2, NARROW_STEPS if _m == "narrow" else FULL_STEPS_BF16,
                                8100 + 10 * _i, nseq=BF16_NSEQ)
    for _k in (1, 2):      # the same inputs cut to their first one / two steps: rows of their own, the oracle is closer there
        ROWS["bf16_%d_s%d" % (_i, _k)] = dict(ROWS["bf16_%d" % _i], use=_k)
ROWS["bf16_sat"] = _row("normal", "narrow", 256, False, 256, 16, NARROW_STEPS, 8180, wscale=4.0, xscale=3.0, nseq=BF16_NSEQ)
# the three shapes the wide path is built for (lstm_bf16w.hip: TRYW / TRYP; lstm_bf16c.hip)
ROWS["wide_narrow256"] = _row("counter", "narrow", 256, False, 256, 16, NARROW_STEPS, 8300)
ROWS["wide_full128"] = _row("counter", "full", 128, True, 256, 16, FULL_STEPS, 8310)
ROWS["wide_block1"] = _row("counter", "full", 128, True, 16, 0, FULL_STEPS, 8320)
ROWS["wide_narrow256_sat"] = _row("counter", "narrow", 256, False, 256, 16, NARROW_STEPS, 8330, wscale=4.0, xscale=3.0)


def tiles_to_seqs(tiles, nseq, group=32):
    """Every live sequence of the named 32-sequence groups."""
    return sorted({s for t in tiles for s in range(t * group, min((t + 1) * group, nseq))})


def full_band_clusters(nseq, ncu, full_tiles):
    """(clusters per direction, tiles per cluster) forward_bf16c (csrc/lstm_bf16c.hip) cuts an H = 128 full-band layer
    into: clusters of 4 CUs, 8 waves x 3 parts; unless FNSSL_CLUSTER_FULL_TILES is set, the smallest number of clusters of
    at least 17 tiles that fits one launch and lowers parts(wave 0) + parts(wave 4)."""
    tiles = (nseq + 31) // 32
    cl = (tiles + 23) // 24

    def cost(k):
        tpc = (tiles + k - 1) // k
        parts = lambda w: 0 if tpc <= w else max(2, (tpc - w + 7) // 8)  # noqa: E731
        return parts(0) + parts(4)

    if not full_tiles:
        best = cl
        for k in range(cl + 1, min((ncu // 4) // 2, tiles // 17) + 1):
            if cost(k) < cost(best):
                best = k
        cl = best
    return cl, (tiles + cl - 1) // cl


def narrow_clusters(nseq):
    """(clusters, tiles per cluster) of the H = 256 narrow-band layer (forward_bf16c: 8 waves x 2 parts = at most 16 tiles
    per cluster, the tiles spread evenly over the fewest clusters that hold them)."""
    tiles = (nseq + 31) // 32
    cl = (tiles + 15) // 16
    return cl, (tiles + cl - 1) // cl


def cluster_sample(nseq, tpc):
    """Groups a cluster leg always checks: the first, the last group of the first cluster, the first group of the last
    cluster, the last (ragged) one."""
    tiles = (nseq + 31) // 32
    ncl = (tiles + tpc - 1) // tpc
    return sorted({0, min(tpc, tiles) - 1, (ncl - 1) * tpc, tiles - 1})


MI355X_CUS = 256
# past one round of pair-split workgroups (bf16c_handles: ceil(nseq / 64) * 2 directions > CUs) — also past
# 2 groups per CU, where the solo kernels switch to four consumer waves (forward_bf16w_plain) — with a ragged last group
FULL_BIG_NSEQ = 64 * (MI355X_CUS // 2) + 7
NARROW_CLUSTER_NSEQ = 600      # 19 tiles = two clusters of 10 and 9 tiles (waves 0-1 two parts, waves 2-7 one + a phantom), 24 in the last
NARROW_FULL_CLUSTER_NSEQ = 999  # 32 tiles = two full clusters of 16 (every wave two live parts), 7 sequences in the last tile
LEG_TILES = {                                                  # nseq -> the 32-groups a leg of that size checks
    40: [0, 1],                                                # one full + one ragged group: everything
    200: [0, 3, 6],                                            # 7 groups (odd): first, a middle one, the ragged last
}


def leg_sample(row, nseq, tpc=None):
    """Sequence numbers a leg of `nseq` sequences checks (all steps of each)."""
    if ROWS[row]["gen"] == "normal":
        return list(range(nseq))
    if tpc is None:
        tiles = LEG_TILES[nseq]
    else:                                                      # (several cuts: the boundary groups of each)
        tiles = sorted({t for k in (tpc if isinstance(tpc, tuple) else (tpc,)) for t in cluster_sample(nseq, k)})
    return tiles_to_seqs(tiles, nseq)


def row_sample(row):
    """The sequences ORACLE[row] is measured on: the union of the samples of the row's legs."""
    r = ROWS[row]
    if r["gen"] == "normal":
        return list(range(r["nseq"]))
    s = set(leg_sample(row, 40)) | set(leg_sample(row, 200))
    if r["mode"] == "narrow":
        for n in (NARROW_CLUSTER_NSEQ, NARROW_FULL_CLUSTER_NSEQ):
            s |= set(leg_sample(row, n, narrow_clusters(n)[1]))
    else:
        for ft in (False, True):
            s |= set(leg_sample(row, FULL_BIG_NSEQ, full_band_clusters(FULL_BIG_NSEQ, MI355X_CUS, ft)[1]))
    return sorted(s)


def row_state(row):
    from fnssl import weights as W
    r = ROWS[row]
    shapes = [("L." + n, s) for n, s in W.lstm_param_shapes(r["c0"] + r["c2"], r["H"], r["bidir"])]
    return W.make_state(shapes, seed=r["seed"], scale=r["wscale"])


def row_inputs(row, seqs, torch=None, device="cpu"):
    """x of the named sequences, [len(seqs), nsteps, c0 + c2] float32: a numpy array for gen "normal", a torch tensor on
    `device` for gen "counter"."""
    r = ROWS[row]
    if r["gen"] == "normal":
        x = fp32_block(r["seed"] + 1, (r["nseq"], r["nsteps"], r["c0"] + r["c2"]), r["xscale"])
        return np.ascontiguousarray(x[np.asarray(seqs), :r["use"]])
    seqs = torch.as_tensor(seqs, dtype=torch.int64)
    x0 = counter_block(torch, seqs, r["nsteps"], r["c0"], r["seed"] + 1, r["xscale"], r["c2"] == 0, device)
    if not r["c2"]:
        return x0
    return torch.cat([x0, counter_block(torch, seqs, r["nsteps"], r["c2"], r["seed"] + 2, r["xscale"], True, device)], dim=-1)


def measure_oracle(row, torch=None):
    """max / mean |fp32 oracle - step-consistent reference driven by the oracle's own output| on the row's sample."""
    r = ROWS[row]
    x = row_inputs(row, row_sample(row), torch)
    x = x if isinstance(x, np.ndarray) else x.numpy()
    sd = row_state(row)
    want = O.lstm(x, sd, "L.", r["bidir"], bf16=True)
    ref = step_consistent_layer(x, sd, want, r["bidir"])
    s = f32_stats(want, ref)
    s["sat"] = float((np.abs(ref) > 0.99).mean())
    s["finite"] = bool(np.isfinite(ref).all())
    return s


# --------------------------------------------------------------------------- the gates
MARGIN = 8      # as DESIGN section 7's IPDnet2 table: v_exp_f32 / v_rcp_f32 against numpy's correctly rounded functions,
                # and another MFMA accumulation order

# ORACLE[row]: max over the row's sample and all steps of |O.lstm(..., bf16=True) - step_consistent(driven by that
# output)|, measured on the CPU on the row's own seeded inputs (tests/test_lstm_bf16_f64_ref_host.py re-measures
# each and fails when a figure is more than 2 x off).  DELTA[row] = MARGIN * ORACLE[row]; DESIGN section 7 carries a copy.
ORACLE = {
    "bf16_0": 1.40e-07, "bf16_0_s1": 8.50e-08, "bf16_0_s2": 8.50e-08, "bf16_1": 1.75e-07, "bf16_1_s1": 1.17e-07,
    "bf16_1_s2": 1.28e-07, "bf16_2": 8.58e-08, "bf16_2_s1": 3.12e-08, "bf16_2_s2": 4.27e-08, "bf16_3": 1.39e-07,
    "bf16_3_s1": 6.25e-08, "bf16_3_s2": 6.91e-08, "bf16_4": 1.54e-07, "bf16_4_s1": 9.40e-08, "bf16_4_s2": 1.30e-07,
    "bf16_5": 8.30e-08, "bf16_5_s1": 4.41e-08, "bf16_5_s2": 5.55e-08, "bf16_6": 1.77e-07, "bf16_6_s1": 1.18e-07,
    "bf16_6_s2": 1.18e-07, "bf16_sat": 3.99e-06, "wide_narrow256": 1.58e-07, "wide_full128": 1.86e-07,
    "wide_block1": 7.01e-08, "wide_narrow256_sat": 3.28e-06,
}
DELTA = {k: MARGIN * v for k, v in ORACLE.items()}
