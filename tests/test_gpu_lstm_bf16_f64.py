"""The bf16-MFMA LSTM kernels (csrc/lstm_bf16.h, lstm_bf16w.h, lstm_bf16p.h, lstm_bf16c.h) against the step-consistent
float64 reference of tests/lstm_bf16_f64_ref.py, one step at a time, at real step counts (narrow-band 300 frames,
full-band 256 / 257 bins), with inputs the kernels have to round themselves (exact ties included) and at saturated gates.

Gate of a leg: DELTA[row] = 8 x the fp32 oracle's own step-consistent distance on the row's seeded inputs, measured on
the CPU (lstm_bf16_f64_ref.ORACLE; re-measured by test_lstm_bf16_f64_ref_host.py; DESIGN section 7 has the table and the
kernels' measured distances).  fp32 outputs (family bf16) go through check_f32, bf16 outputs (the wide families) through
check_bf16: within half a bf16 spacing + delta everywhere, and an unbiased rounding.  Every leg asserts the family the
library plans, so no leg can silently test another kernel; every step of every sampled sequence is checked.
"""
import functools

import numpy as np
import pytest

import lstm_bf16_f64_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KNOBS = ("FNSSL_NO_CLUSTER", "FNSSL_NO_CLUSTER_H128", "FNSSL_NO_CLUSTER_B1", "FNSSL_CLUSTER_FULL_TILES", "FNSSL_CLUSTER_SPREAD",
         "FNSSL_BF16W_SOLO", "FNSSL_BF16P_DRAIN")
SFX = ("", "_reverse")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    yield torch.device("cuda:0")
    _device_inputs.cache_clear()
    _packed.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _state(row):
    return R.row_state(row)


@functools.lru_cache(maxsize=None)
def _packed(row, wide, dev):
    from fnssl import ops
    r, sd = R.ROWS[row], _state(row)
    pack = ops.pack_lstm_bf16w if wide else ops.pack_lstm_bf16
    return [pack(sd["L.weight_ih_l0" + s], sd["L.weight_hh_l0" + s], sd["L.bias_ih_l0" + s], sd["L.bias_hh_l0" + s],
                 r["c0"], r["c2"], dev) for s in SFX[:2 if r["bidir"] else 1]]


def _to4d(t, mode):
    """[nseq, nsteps, C] -> the layer's logical [nb = 1, nt, nf, C] tensor (narrow: sequences are the bins, steps the frames)."""
    return t.unsqueeze(0) if mode == "full" else t.permute(1, 0, 2).contiguous().unsqueeze(0)


def _rows_of(out4d, mode, seqs):
    """the sampled sequences of a [1, nt, nf, C] tensor, as a host [len(seqs), nsteps, C] float32 array"""
    idx = torch.as_tensor(list(seqs), device=out4d.device)
    rows = out4d[0].index_select(0, idx) if mode == "full" else out4d[0].index_select(1, idx).permute(1, 0, 2)
    return rows.float().cpu().numpy()


def _saturated(ref, what):
    """The condition of a saturated leg, on the float64 reference (not on the kernel)."""
    assert np.isfinite(ref).all(), what
    frac = float((np.abs(ref) > 0.99).mean())
    assert 0.0005 <= frac <= 0.05, "%s: %.4f %% of |h| > 0.99 is not a saturated-gate input" % (what, 100 * frac)
    return frac


# --------------------------------------------------------------------------- family bf16 (lstm_bf16.h): fp32 tensors
def _run_bf16(dev, row, saturated=False):
    from fnssl import ops
    r, sd = R.ROWS[row], _state(row)
    nseq, H, c0, c2, mode = r["nseq"], r["H"], r["c0"], r["c2"], r["mode"]
    x = R.row_inputs(row, list(range(nseq)))                          # fp32, nothing bf16-representable, one tie in eight
    xd = _to4d(torch.from_numpy(x).to(dev), mode)
    x0, x2 = xd[..., :c0].contiguous(), (xd[..., c0:].contiguous() if c2 else None)
    w = _packed(row, False, dev)
    ndir = len(w)
    out = torch.full(tuple(xd.shape[:3]) + (ndir * H,), float("nan"), device=dev)
    fam = ops.lstm_plan(mode, x0, None, x2, w, H, out, bf16=True)[0]
    assert fam == "bf16", fam
    ops.lstm_layer(mode, x0, None, x2, w, H, out, bf16=True)
    got = _rows_of(out, mode, range(nseq))
    ref = R.step_consistent_layer(x, sd, got, r["bidir"])
    what = "%s (%s H %d <- %d + %d, %d sequences x %d steps)" % (row, mode, H, c0, c2, nseq, x.shape[1])
    if saturated:
        print("%s: %.3f %% of |h| > 0.99" % (what, 100 * _saturated(ref, what)))
    s = R.f32_stats(got, ref)
    print("LEG bf16 %s: kernel vs step-consistent max %.3g mean %.3g (delta %.3g)" % (what, s["max"], s["mean"], R.DELTA[row]))
    R.check_f32(got, ref, R.DELTA[row], what)


BF16_ROWS = ["bf16_%d" % i for i in range(len(R.BF16_SHAPES))]


@pytest.mark.parametrize("row", BF16_ROWS)
def test_bf16_family_at_real_step_counts(dev, row):
    """The shapes of test_lstm_bf16_layer_matches_bf16_oracle, both modes and directions, 300 frames / 257 bins, 16 k + 7
    sequences (a ragged last group); h is observed as fp32, before any rounding."""
    _run_bf16(dev, row)


@pytest.mark.parametrize("nsteps", [1, 2])
@pytest.mark.parametrize("row", BF16_ROWS)
def test_bf16_family_first_steps(dev, row, nsteps):
    """One step (h_{-1} = 0 only) and two (the first recurrent operand), each direction of every shape; the gate is that of
    the oracle on these one / two steps (rows of their own), not the looser one of the whole length."""
    _run_bf16(dev, "%s_s%d" % (row, nsteps))


def test_bf16_family_saturated_gates(dev):
    _run_bf16(dev, "bf16_sat", saturated=True)


# --------------------------------------------------------------------------- wide families: bf16 output
@functools.lru_cache(maxsize=None)
def _device_inputs(row, nseq, dev):
    """(x0, x2) of sequences 0 .. nseq - 1 as the layer's 4-D tensors, generated on the device."""
    r = R.ROWS[row]
    c0, c2 = r["c0"], r["c2"]
    x0 = torch.empty((nseq, r["nsteps"], c0), device=dev, dtype=torch.bfloat16 if c2 else torch.float32)
    x2 = torch.empty((nseq, r["nsteps"], c2), device=dev) if c2 else None
    for a in range(0, nseq, 512):
        b = min(a + 512, nseq)
        x = R.row_inputs(row, torch.arange(a, b), torch, dev)
        x0[a:b] = x[..., :c0]                                   # (the bf16 block is representable: the cast is exact)
        if c2:
            x2[a:b] = x[..., c0:]
    return _to4d(x0, r["mode"]), (_to4d(x2, r["mode"]) if c2 else None)


def _force(monkeypatch, family, full_tiles=False):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if family in ("bf16_pair", "bf16_solo"):
        for k in ("FNSSL_NO_CLUSTER", "FNSSL_NO_CLUSTER_H128", "FNSSL_NO_CLUSTER_B1"):
            monkeypatch.setenv(k, "1")
    if family == "bf16_solo":
        monkeypatch.setenv("FNSSL_BF16W_SOLO", "1")
    if full_tiles:
        monkeypatch.setenv("FNSSL_CLUSTER_FULL_TILES", "1")


def _solo_waves(nseq, ndir, H, ncu):
    """forward_bf16w_plain (csrc/lstm_bf16w.hip): two consumer waves + two loader waves while the launch leaves SIMDs idle
    (and always at H = 256, where four h staging areas do not fit the LDS), else four consumers."""
    return 2 if ((nseq + 31) // 32) * ndir <= 2 * ncu or H >= 256 else 4


def _run_wide(dev, monkeypatch, row, nseq, family, full_tiles=False, tpc=None, saturated=False, tag=""):
    from fnssl import ops
    r, sd = R.ROWS[row], _state(row)
    H, c0, c2, mode = r["H"], r["c0"], r["c2"], r["mode"]
    w = _packed(row, True, dev)
    ndir = len(w)
    x0, x2 = _device_inputs(row, nseq, dev)
    out = torch.full(tuple(x0.shape[:3]) + (ndir * H,), float("nan"), device=dev, dtype=torch.bfloat16)
    _force(monkeypatch, family, full_tiles)
    fam, rounds = ops.lstm_plan(mode, x0, None, x2, w, H, out, bf16=True, wide=True)
    assert fam == family, "planned %s, the leg is for %s" % (fam, family)
    assert rounds == 1      # (all the plan says of a wide launch: the cut into clusters / waves is restated in lstm_bf16_f64_ref)
    ops.lstm_layer(mode, x0, None, x2, w, H, out, bf16=True, wide=True)
    if family == "bf16_cluster":
        with torch.cuda.device(dev):
            assert ops.lstm_cluster_status(nseq, H, ndir, dev) == 0, "a bounded wait ran out: the guarded fallback computed this"
    assert not torch.isnan(out).any(), "a row of the output was not written"
    seqs = R.leg_sample(row, nseq, tpc)
    assert len(seqs) >= min(64, nseq)
    got = _rows_of(out, mode, seqs)
    # the sampled rows as the host builds them are the rows the kernel read
    x = R.row_inputs(row, seqs, torch).numpy()
    assert np.array_equal(x[..., :c0], _rows_of(x0, mode, seqs)) and (not c2 or np.array_equal(x[..., c0:], _rows_of(x2, mode, seqs)))
    ref = R.step_consistent_layer(x, sd, got, r["bidir"])
    what = "%s %s%s (%s H %d <- %d + %d, %d of %d sequences x %d steps)" % (family, row, tag, mode, H, c0, c2, len(seqs), nseq,
                                                                            r["nsteps"])
    if saturated:
        print("%s: %.3f %% of |h| > 0.99" % (what, 100 * _saturated(ref, what)))
    s = R.bf16_stats(got, ref)
    print("LEG %s: kernel over half a bf16 spacing by %.3g (delta %.3g), rounding bias %.4f over %d, max |got - ref| %.3g"
          % (what, s["excess"], R.DELTA[row], s["bias"], s["n"], s["max"]))
    R.check_bf16(got, ref, R.DELTA[row], what)


WIDE_ROWS = ["wide_narrow256", "wide_full128", "wide_block1"]


@pytest.mark.parametrize("nseq", [40, 200])      # one full + one ragged group; 7 groups (odd) over several workgroups
@pytest.mark.parametrize("row", WIDE_ROWS)
def test_pair_split_kernels(dev, monkeypatch, row, nseq):
    """lstm_bf16p.h on the three built shapes; the fp32 blocks (kW_F2: the 16 skip channels; kW_F0: block 1's 16 feature
    channels) carry values the kernel has to round, one in eight on an exact tie."""
    _run_wide(dev, monkeypatch, row, nseq, "bf16_pair")


@pytest.mark.parametrize("nseq", [40, 200])
@pytest.mark.parametrize("row", WIDE_ROWS)
def test_solo_kernels_with_loader_waves(dev, monkeypatch, row, nseq):
    """lstm_bf16w.h, NW = 2: two consumer waves + two loader waves."""
    r = R.ROWS[row]
    assert _solo_waves(nseq, 2 if r["bidir"] else 1, r["H"], torch.cuda.get_device_properties(dev).multi_processor_count) == 2
    _run_wide(dev, monkeypatch, row, nseq, "bf16_solo", tag=" NW 2")


def _big_nseq(dev):
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    assert ncu == R.MI355X_CUS, "the committed sample and gate of the full-band legs are those of %d CUs, not %d" % (R.MI355X_CUS, ncu)
    return R.FULL_BIG_NSEQ, ncu


@pytest.mark.parametrize("row", ["wide_full128", "wide_block1"])
def test_solo_kernels_with_four_consumer_waves(dev, monkeypatch, row):
    """lstm_bf16w.h, NW = 4 (H = 128 only): the smallest batch past two groups per CU."""
    nseq, ncu = _big_nseq(dev)
    assert _solo_waves(nseq, 2, 128, ncu) == 4 and _solo_waves(nseq - 7, 2, 128, ncu) == 2
    _run_wide(dev, monkeypatch, row, nseq, "bf16_solo", tpc=(20, 24), tag=" NW 4")     # (the cluster legs' groups)


@pytest.mark.parametrize("nseq,cut", [(R.NARROW_CLUSTER_NSEQ, (2, 10)), (R.NARROW_FULL_CLUSTER_NSEQ, (2, 16))])
def test_cluster_kernel_narrow_band(dev, monkeypatch, nseq, cut):
    """lstm_bf16c.h, H = 256, 300 frames.  600 sequences: forward_bf16c spreads the 19 tiles over two clusters of 10 and 9
    (waves 0-1 two live parts, the others one and a phantom; 24 sequences in the last tile) — groups 0, 9 | 10, 18 are checked.
    999: two full clusters of 16 tiles (two live parts in every wave), 7 sequences in the last — groups 0, 15 | 16, 31."""
    assert R.narrow_clusters(nseq) == cut
    _run_wide(dev, monkeypatch, "wide_narrow256", nseq, "bf16_cluster", tpc=cut[1])


@pytest.mark.parametrize("full_tiles", [False, True])
@pytest.mark.parametrize("row", ["wide_full128", "wide_block1"])
def test_cluster_kernel_full_band(dev, monkeypatch, row, full_tiles):
    """lstm_bf16c.h, H = 128, both built shapes, at the smallest batch the cluster kernel takes (bf16c_handles: more
    pair-split workgroups than CUs): 257 tiles per direction, cut into 13 clusters of 20 tiles (waves 0-3 three parts, waves
    4-7 two; the last cluster 17 tiles) or, with FNSSL_CLUSTER_FULL_TILES=1, 11 of 24 (the last one 17)."""
    nseq, ncu = _big_nseq(dev)
    cl, tpc = R.full_band_clusters(nseq, ncu, full_tiles)
    assert (cl, tpc) == ((11, 24) if full_tiles else (13, 20)) and 257 - (cl - 1) * tpc == 17
    # (the boundary groups of BOTH cuts are checked in either leg: tiles 0, 19 | 23, 240, 256)
    _run_wide(dev, monkeypatch, row, nseq, "bf16_cluster", full_tiles=full_tiles, tpc=(20, 24),
              tag=" full tiles" if full_tiles else " default tiling")


@pytest.mark.parametrize("family,nseq,tpc", [("bf16_pair", 40, None), ("bf16_solo", 40, None),
                                             ("bf16_cluster", R.NARROW_CLUSTER_NSEQ, R.narrow_clusters(R.NARROW_CLUSTER_NSEQ)[1])])
def test_wide_families_saturated_gates(dev, monkeypatch, family, nseq, tpc):
    """Weights x 4, inputs of scale 3: about 0.1 % of |h| beyond 0.99 (asserted on the reference)."""
    _run_wide(dev, monkeypatch, "wide_narrow256_sat", nseq, family, tpc=tpc, saturated=True)
