"""The fp32 LSTM forward kernels (lstm_kernel.h, lstm_static.h, lstm_static3.h, lstm_static4.h, lstm_split*.h, lstm_f32c.h,
lstm_train.h) against the step-consistent float64 reference of tests/lstm_f32_f64_ref.py, one step at a time: the full-chip
rounds at 49 125 sequences x 40 steps, the few-sequence families at real step counts (narrow-band 300 frames, full-band
256 / 257 bins), the streaming form as 25 carried calls, the first one and two steps of every family, saturated gates and
inputs that overflow both float32 exponentials.

Gate of a leg: DELTA[row] = 8 x the float32 oracle's own step-consistent distance on the row's seeded inputs, measured on the
CPU (lstm_f32_f64_ref.ORACLE; re-measured by test_lstm_f32_f64_ref_host.py; DESIGN section 7 has the table and the kernels'
measured distances).  Every leg asserts the family the library plans, so no leg can silently test another kernel; every
hidden unit of every step of every sampled sequence is checked; the rows behind the last sequence must stay untouched.
"""
import ctypes as C

import numpy as np
import pytest

import lstm_f32_f64_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SPARE = 27                       # rows behind the last sequence of every output buffer: NaN before, NaN after
CACHE_BYTES = 2200 << 20         # device inputs kept between legs: one full-chip row, or all the small ones
_inputs, _weights = {}, {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib, ops
    _lib.load()
    d = torch.device("cuda:0")
    ncu = torch.cuda.get_device_properties(d).multi_processor_count
    assert ncu == R.MI355X_CUS, "the committed samples and families are those of %d CUs, not %d" % (R.MI355X_CUS, ncu)
    yield d
    _inputs.clear()
    _weights.clear()
    ops.release_workspaces()
    torch.cuda.empty_cache()


def _packed(base, dev):
    from fnssl import ops
    if base not in _weights:
        r, sd = R.ROWS[base], R.row_state(base)
        _weights[base] = (sd, [ops.pack_lstm(sd["L.weight_ih_l0" + s], sd["L.weight_hh_l0" + s], sd["L.bias_ih_l0" + s],
                                             sd["L.bias_hh_l0" + s], r["c0"], r["c2"], dev) for s in R.SFX[:2 if r["bidir"] else 1]])
    return _weights[base]


def _store(chunks, nseq, nsteps, mode, dev):
    """Logical [1, nt, nf, C] tensor of `nseq` sequences x `nsteps` steps, contiguous in that order, filled chunk by chunk from
    a generator of ([a, b), [b - a, nsteps, C] tensor)."""
    t = None
    for a, b, x in chunks:
        if t is None:
            t = torch.empty((1, nseq, nsteps, x.shape[-1]) if mode == "full" else (1, nsteps, nseq, x.shape[-1]), device=dev)
        if mode == "full":
            t[0, a:b] = x
        else:
            t[0, :, a:b] = x.permute(1, 0, 2)
    # fnssl_lstm_forward bounds (batch stride + 16 sequences + all steps) of a tensor by 4 GB, whatever the batch: a
    # step-major tensor of 2 GB with its ONE batch index at stride 0 says the same thing and stays inside it
    return t.as_strided(t.shape, (0,) + t.stride()[1:]) if t.numel() * 8 >= 3.9e9 else t


def _cached(key, nbytes, make):
    """Device inputs kept between legs, the oldest dropped BEFORE a new one is generated (no leg holds two full-chip rows)."""
    if key not in _inputs:
        while _inputs and sum(v[0] for v in _inputs.values()) + nbytes > CACHE_BYTES:
            _inputs.pop(next(iter(_inputs)))
        _inputs[key] = (nbytes, make())
    return _inputs[key][1]


def _device_inputs(base, nseq, mode, skip_steps, dev):
    """(x0, x1, x2, skip) of sequences 0 .. nseq - 1 as the layer's 4-D tensors, generated on the device, 512 sequences at a
    time.  skip (the residual of a `sum` leg, `skip_steps` steps of it) is no operand of the recurrence: cached on its own."""
    r = R.ROWS[base]
    spans = [(a, min(a + 512, nseq)) for a in range(0, nseq, 512)]
    gen = lambda k: ((a, b, R.row_inputs(base, torch.arange(a, b), torch, dev)[k]) for a, b in spans)  # noqa: E731
    x = _cached((base, nseq, mode), nseq * r["nsteps"] * (r["c0"] * (2 if r["x1"] else 1) + r["c2"]) * 4, lambda: (
        _store(gen(0), nseq, r["nsteps"], mode, dev), _store(gen(1), nseq, r["nsteps"], mode, dev) if r["x1"] else None,
        _store(gen(2), nseq, r["nsteps"], mode, dev) if r["c2"] else None))
    skip = None
    if skip_steps:
        ch = (2 if r["bidir"] else 1) * r["H"]
        skip = _cached((base, nseq, mode, skip_steps), nseq * skip_steps * ch * 4, lambda: _store(
            ((a, b, R.row_skip(base, torch.arange(a, b), torch, dev, skip_steps)) for a, b in spans), nseq, skip_steps, mode, dev))
    return x + (skip,)


def _steps(t, mode, a, b):
    """steps [a, b) of a logical [1, nt, nf, C] tensor"""
    return None if t is None else (t[:, :, a:b] if mode == "full" else t[:, a:b])


def _rows_of(t, mode, seqs):
    """the sampled sequences of a logical [1, nt, nf, C] tensor, as a host [len(seqs), nsteps, C] float32 array"""
    idx = torch.as_tensor(list(seqs), device=t.device)
    rows = t[0].index_select(0, idx) if mode == "full" else t[0].index_select(1, idx).permute(1, 0, 2)
    return rows.float().cpu().numpy()


def _out_buffer(nseq, nsteps, C, mode, dev, lead=0):
    """NaN-filled storage [1, nseq + SPARE, lead + nsteps, C] (sequence-major, as the network keeps a narrow-band layer's output)
    and the logical [1, nt, nf, C] view of its first nseq sequences, steps lead .. lead + nsteps - 1."""
    buf = torch.full((1, nseq + SPARE, lead + nsteps, C), float("nan"), device=dev)
    v = buf[:, :nseq, lead:]
    return buf, (v if mode == "full" else v.permute(0, 2, 1, 3))


def _run(dev, name):
    from fnssl import _lib, ops
    leg = R.LEGS[name]
    row, base, ex = R.leg_row(name), leg["row"], leg["extras"]
    r = R.ROWS[base]
    nseq, mode, H, c0, c2 = leg["nseq"], leg["mode"], r["H"], r["c0"], r["c2"]
    ndir = 2 if r["bidir"] else 1
    nsteps = R.row_steps(row)
    sd, w = _packed(base, dev)
    x0, x1, x2, skip = (_steps(t, mode, 0, nsteps) for t in _device_inputs(base, nseq, mode, nsteps if ex.get("sum") else 0, dev))
    tuning = _lib.make_tuning(base=_lib.Tuning(), **leg["knobs"])       # the leg's knobs and no others, whatever the environment says
    kw = dict(variant=ex.get("variant", 0), tuning=tuning)
    chunk = ex.get("carry")
    buf, out = _out_buffer(nseq, nsteps, ndir * H, mode, dev, lead=1 if chunk else 0)
    bsum = osum = None
    if skip is not None:
        bsum, osum = _out_buffer(nseq, nsteps, ndir * H, mode, dev)
        kw.update(skip=skip, out_sum=osum)
    if ex.get("reserve"):
        kw.update(reserve=torch.empty(ops.lstm_reserve_floats(nseq, H, ndir, nsteps), device=dev))
    ops.cluster_fallbacks(dev, reset=True)

    def status(ws):
        if ws is None:      # (the binding's own workspace)
            with torch.cuda.device(dev):
                return ops.lstm_cluster_status(nseq, H, ndir, dev)
        word = C.c_uint(0xffffffff)
        ops.check(_lib.load().fnssl_lstm_cluster_status(ws.data_ptr(), ws.numel() * 4, nseq, H, ndir,
                                                        torch.cuda.current_stream(dev).cuda_stream, C.byref(word)), "lstm_cluster_status")
        return int(word.value)

    def call(a, b, **more):
        args = (mode, _steps(x0, mode, a, b), _steps(x1, mode, a, b), _steps(x2, mode, a, b), w, H,
                _steps(out, mode, a, b))
        k = dict(kw, **more)
        fam = ops.lstm_plan(*args, **k)[0]
        assert fam == leg["family"], "planned %s, the leg is for %s" % (fam, leg["family"])
        ops.lstm_layer(*args, **k)
        if fam == "f32_cluster":
            assert status(more.get("carry_workspace")) == 0, "a bounded wait ran out: the guarded fallback computed this"

    if chunk:      # the protocol of test_lstm_carry_state_continues_a_sequence: one buffer, the row before `out` is h_{-1}
        assert nsteps % chunk == 0
        ws = ops.lstm_state_workspace(nseq, H, dev)
        for a in range(0, nsteps, chunk):
            call(a, a + chunk, carry_workspace=ws, carry=a > 0)
    else:
        call(0, nsteps)
    assert ops.cluster_fallbacks(dev) == 0, "a cluster launch fell back"
    assert torch.isnan(buf[:, nseq:]).all(), "%s wrote behind the last sequence" % leg["family"]
    assert not chunk or torch.isnan(buf[:, :nseq, 0]).all()
    assert not torch.isnan(out).any(), "a row of the output was not written"
    if osum is not None:
        assert torch.isnan(bsum[:, nseq:]).all(), "%s wrote the residual output behind the last sequence" % leg["family"]
        assert torch.equal(osum, out + skip), "out_sum is not h + skip"
    seqs = R.leg_sample(name)
    assert len(seqs) >= min(64, nseq) and (nseq > 256 or len(seqs) == nseq)
    got = _rows_of(out, mode, seqs)
    # the sampled rows as the host builds them are the rows the kernel read
    h0, h1, h2 = (None if t is None else t.numpy()[:, :nsteps] for t in R.row_inputs(base, seqs, torch))
    assert np.array_equal(h0, _rows_of(x0, mode, seqs)) and (h1 is None or np.array_equal(h1, _rows_of(x1, mode, seqs))) and \
        (h2 is None or np.array_equal(h2, _rows_of(x2, mode, seqs)))
    info = {}
    ref = R.step_consistent_layer(R.kernel_x(h0, h1, h2), sd, got, r["bidir"], info=info)
    what = "%s %s (%s H %d <- %d%s + %d, %d of %d sequences x %d steps%s)" % (
        name, row, mode, H, c0, " + x1" if r["x1"] else "", c2, len(seqs), nseq, nsteps, ", %s" % leg["knobs"] if leg["knobs"] else "")
    assert np.isfinite(ref).all(), what
    R.check_conditions(r["kind"], info["pre"], float((np.abs(ref) > 0.99).mean()), what)
    s = R.f32_stats(got, ref)
    print("LEG %s %s: kernel max %.3g mean %.3g (delta %.3g, oracle %.3g); largest |pre-activation| %.3g, |h| > 0.99: %.3f %%"
          % (leg["family"], what, s["max"], s["mean"], R.DELTA[row], R.ORACLE[row], info["pre"], 100 * float((np.abs(ref) > 0.99).mean())))
    R.check_f32(got, ref, R.DELTA[row], what)


def _legs(pred):
    return sorted((n for n in R.LEGS if pred(n)), key=lambda n: (R.LEGS[n]["row"], n))


# ordered so that the legs of one full-chip row follow one another (its 2 GB input is generated once)
@pytest.mark.parametrize("name", _legs(lambda n: R.LEGS[n]["row"].startswith("big")))
def test_full_chip_rounds(dev, name):
    """static4 / static3 / static at 49 125 sequences (3 071 groups, 5 sequences in the last) x 40 steps — many wraps of the
    two-slot weight ring and of the operand ring — on [256], [256 | 4], with skip / out_sum and at saturated gates; the H = 128
    rounds of 8 193 sequences x 2 directions on [256 | 4] with out_sum; and the first one and two steps of each."""
    _run(dev, name)


@pytest.mark.parametrize("name", _legs(lambda n: not R.LEGS[n]["row"].startswith("big") and R.LEGS[n]["family"] != "f32_cluster"))
def test_few_sequence_families(dev, name):
    """generic (H 16, 32, 64; every launch geometry at H 256 and H 128), split_static, split (with x1), train (with a reserve;
    h only) at 300 frames / 256 / 257 bins, their first steps, saturated gates and the overflow row on the generic kernel."""
    _run(dev, name)


@pytest.mark.parametrize("name", _legs(lambda n: R.LEGS[n]["family"] == "f32_cluster"))
def test_cluster_resident_kernel(dev, name):
    """lstm_f32c.h in each form: one, 6, 11 and 40 groups per cluster, ragged, [256 | 4], H = 128 at 16 and 15 groups per
    direction, the gate-split forms under their knob, the streaming form as 25 carried calls of 12 frames against the
    whole-sequence reference, saturated gates, the overflow row, first steps — status word 0 and no fallback counted."""
    _run(dev, name)
