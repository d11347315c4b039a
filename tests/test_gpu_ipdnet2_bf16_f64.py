"""The bf16 IPDnet2 kernels (csrc/spatialnet.hip, ``BF = true``: v_mfma_f32_16x16x32_bf16) against the float64
reference of tests/ipdnet2_bf16_f64_ref.py, ONE PRODUCT AT A TIME: every product is restated from what the kernel itself
stored (the encoder's input; xz, dbl and y in the Mamba workspace, read back after each call), so no rounding flip is left
to absorb, and where the operand is an in-kernel intermediate (a LayerNorm output, SiLU(conv + b), the squeezed row) the
reference carries a per-element flip bound.  Every element must satisfy |got - ref| <= delta + bound; the elements with
bound <= delta (the tight ones: at least a third and at least 10 000 of every leg, in every output channel and at every
position of a 16-point tile — asserted from the reference before anything is compared) are held to delta alone.

delta = 8 x the float32 oracle's distance from the same reference on the same inputs, eps likewise (R.ORACLE, measured on
the host and re-measured by test_ipdnet2_bf16_f64_ref_host.py).  None is chosen from what the kernels give.  Every weight
tensor of every product carries exact bf16 ties of both parities, one element in eight (identity / one-hot probe tensors
excepted: they are exact by construction), so a truncating or half-away weight image shows without any bound.  Every call
goes through fnssl.spatialnet with precision = BF16, and every call of every bf16 leg also asserts that its output is NOT
bit-equal to the FP32 call's (carried calls: the FP32 twin starts from a copy of the same state).  Figures are printed before they are asserted."""
import numpy as np
import pytest

import ipdnet2_bf16_f64_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _id(leg):
    return leg if isinstance(leg, str) else R.full_name(*leg)


# ================================================================================================================== #
# Encoder: x is the direct operand (fp32 values that are not bf16-representable, with ties): bound 0 everywhere.
# ================================================================================================================== #
def device_encoder(name, dev, cus):
    from fnssl import spatialnet as sn
    cin, nb, nf, nt, chunks = R.enc_spec(name, cus)
    x, w, b = R.enc_case(cin, nb, nf, nt)
    xd, wT, bd = to_dev(x, dev), to_dev(w, dev).permute(1, 2, 0).contiguous(), to_dev(b, dev)
    out, st, t0 = [], None, 0
    for n in (chunks or (nt,)):
        so = torch.empty((nb, cin, nf, 4), dtype=torch.float32, device=dev) if chunks else None
        o = sn.encoder(xd[..., t0:t0 + n], wT, bd, state_in=st, state_out=so, precision=sn.BF16)
        o32 = sn.encoder(xd[..., t0:t0 + n], wT, bd, state_in=st, precision=sn.FP32)
        assert not torch.equal(o, o32), "%s: the BF16 call returned the FP32 kernel's bits" % name
        out.append((o.cpu().numpy(), None if so is None else so.cpu().numpy()))
        st, t0 = so, t0 + n
    whole = sn.encoder(xd, wT, bd, precision=sn.BF16) if chunks else None
    return out, whole


@pytest.mark.parametrize("name", list(R.ENC_LEGS))
def test_encoder_product_vs_float64(dev, cus, name):
    """K = cin * 5 = 50 (padded to 80), 80 (exact), 85 and 150 (to 160), 160 at 16 bins x 23 frames; the non-pipelined
    kernel (3 frames); chunks 9 + 1 + 13 with carried frames, each held to the reference and together EQUAL to the
    whole-signal call bit for bit (the pipelined and the carried kernel start the accumulator at the bias, pack the same
    K / 4 values with the same pack8_bf16 and issue the same MFMAs in the same k-step order against the same weight image);
    the smallest size with a partial second pass of the persistent grid."""
    stored, whole = device_encoder(name, dev, cus)
    R.check_leg(name, stored, cus)
    if whole is not None:
        chunks = np.concatenate([o for o, _ in stored], axis=2)
        print("%s: chunks vs whole signal, max abs %.3e" % (name, float(np.abs(chunks - whole.cpu().numpy()).max())))
        assert np.array_equal(chunks, whole.cpu().numpy()), "%s: the carried chunks are not the whole-signal call's bits" % name


# ================================================================================================================== #
# Mamba block, phase by phase: the workspace (xz | dbl | y) is read back after every call.
# ================================================================================================================== #
def device_mamba(name, dev, cus):
    from fnssl import ops
    from fnssl import spatialnet as sn
    sd, x, seqs, (nb, nf, nt, tp, chunks) = R.mamba_case(name, cus)
    w, keep = sn.pack_mamba(sd, R.P_NORM, R.P_MAMBA, dev)
    xd = to_dev(x.reshape(nb, nf, nt, 96), dev)
    idx = torch.as_tensor(seqs, device=dev)
    st = sn.mamba_state(nb, nf, dev)
    if name == "m_wide_carry":
        st = tuple(to_dev(a, dev) for a in R.wide_carry_state(nb * nf))
    recs, t0 = [], 0
    for n in (chunks or (nt,)):
        carry = t0 > 0 or name == "m_wide_carry"
        st_in = tuple(a[idx].cpu().numpy() for a in st) if carry else None
        st32 = tuple(a.clone() for a in st)                    # the state this call starts from, for the FP32 twin below
        out = sn.mamba(xd[:, :, t0:t0 + n], w, residual=True, time_pool=tp, state=st, carry=carry, precision=sn.BF16)
        npts = nb * nf * n
        lay, total = R.mamba_ws_layout(npts)
        ws = ops._workspace(total, dev, "sn_mamba")[:total].view(torch.float32)
        reg = {k: ws[o:o + npts * wd].view(nb * nf, n, wd)[idx].cpu().numpy() for k, (o, wd) in lay.items()}
        recs.append(dict(reg, x=np.ascontiguousarray(x[seqs][:, t0:t0 + n]), seqs=seqs, state_in=st_in, carry=carry,
                         time_pool=tp, residual=True, out=out.reshape(nb * nf, n // tp, 96)[idx].cpu().numpy(),
                         ssm=st[1][idx].cpu().numpy()))
        # the FP32 twin of this very call, on a copy of the state it started from (the workspace has been read: the twin
        # may reuse it): the fused path and the carried one (conv + xproj, scan with have_u) each have their own routing
        o32 = sn.mamba(xd[:, :, t0:t0 + n], w, residual=True, time_pool=tp, state=st32, carry=carry, precision=sn.FP32)
        assert not torch.equal(out, o32), "%s: call at frame %d: BF16 returned the FP32 kernels' bits" % (name, t0)
        t0 += n
    del keep
    return recs


@pytest.mark.parametrize("name", R.MAMBA_ALL)
def test_mamba_block_phase_by_phase_vs_float64(dev, cus, name):
    """in_proj: xz^dev against in_proj(bf16(LN(x))), flip bound from the LN output.  x_proj: dbl^dev against
    x_proj(bf16(SiLU(conv4(xz^dev) + b))), taps from the device's own xz (and carried taps), flip bound from SiLU(conv) —
    the fused conv + x_proj kernel on whole sequences (35 = 2 * 13 + 9 frames, 9 < 13, 250 = 19 * 13 + 3; the 17 x 16 x 250
    leg runs whole and compares 48 of its 272 sequences: utterances 0, 8 and 16), conv + xproj on
    the carried path (4 + 1 + 30).  scan: y^dev (gated, as stored) and the final state against the float64 scan driven by
    xz^dev and dbl^dev: all fp32, the fp32 file's rule (8 x the oracle's max / rms).  out_proj: out against
    out_proj(bf16(pool_T(y^dev))) + pool_T(x); the kernel's fp32 pooling is RESTATED EXACTLY (R.pool32: frames added in
    order from 0.f, one multiplication by float32(1 / tp)), so the operand is exact and the bound 0 at pools 1, 3 (the
    run-time trip count) and 5.  m_wide / m_wide_carry: one partial second pass of every phase kernel's grid."""
    R.check_leg(name, device_mamba(name, dev, cus), cus)


# ================================================================================================================== #
# fconv: flip bound from the LN output, through PReLU, the residual and the F-pooling.
# ================================================================================================================== #
@pytest.mark.parametrize("name", R.FCONV_ALL)
def test_fconv_product_vs_float64(dev, cus, name):
    """256 bins pool 2, 128 bins pool 8, 16 and 32 bins pool 1 at 5 frames; 37 frames at 16 bins (a partial last
    workgroup); cus * 16 + 5 frames (a partial second pass).  fc16_planted: the k >= 60 padding lanes read live LDS (the
    first four channels of each group in the row of bin f - 2) against weights that must be zero: those channels hold 1e30 (LayerNorm
    bias; their true weights are zero), so a non-zero padded weight shows as 1e28."""
    # (poff = 0 in sn_fconv_mfma_kernel: the padding lanes of bin f read channels 12 g .. 12 g + 3 of the image row of bin
    # f - 2; for f < 2 that is the zero 'same'-padding row, so those two bins of a frame read zeros there)
    from fnssl import spatialnet as sn
    sd, x, pool = R.fconv_case(name, cus)
    w, keep = sn.pack_fconv(sd, R.FCONV_P, dev)
    xd = to_dev(x, dev)
    out = sn.fconv(xd, w, residual=True, pool=pool, precision=sn.BF16)
    assert not torch.equal(out, sn.fconv(xd, w, residual=True, pool=pool, precision=sn.FP32)), "BF16 returned the FP32 bits"
    got = out.cpu().numpy()
    fr = R.leg_frames(name, cus)
    R.check_leg(name, got if fr is None else got[:, :, fr], cus)
    del keep


# ================================================================================================================== #
# full: three chained products; probes S / F / U give each stage generic weights once.
# ================================================================================================================== #
@pytest.mark.parametrize("leg", R.FULL_ALL, ids=_id)
def test_full_branch_probes_vs_float64(dev, cus, leg):
    """The three bf16 sizes (16, 64, 128 bins), probes S / F / U of the same kernel (R.full_state_dict), bounds
    propagated through the chain.  full16G keeps generic weights in all three stages: it asserts delta + bound only and is
    EXEMPT from the tight-share condition (a three-product chain leaves about a tenth of it tight).  full16S_multi: a
    partial second pass."""
    from fnssl import spatialnet as sn
    nf, probe, multi = leg
    sd, x = R.full_case(nf, probe, cus, multi)
    w, keep, _ = sn.pack_full(sd, R.FULL_P, dev)
    xd = to_dev(x, dev)
    out = sn.full(xd, w, residual=True, precision=sn.BF16)
    assert not torch.equal(out, sn.full(xd, w, residual=True, precision=sn.FP32)), "BF16 returned the FP32 bits"
    got = out.cpu().numpy()
    fr = R.leg_frames(leg, cus)
    R.check_leg(leg, got if fr is None else got[:, :, fr], cus)
    del keep


# ================================================================================================================== #
# Precision routing, bit for bit: the shapes without a bf16 kernel run the fp32 kernels under BF16.
# ================================================================================================================== #
def test_fconv_below_16_bins_runs_the_fp32_kernel_under_bf16(dev):
    from fnssl import spatialnet as sn
    sd = R.fconv_state_dict(R.FCONV_SEED)
    w, keep = sn.pack_fconv(sd, R.FCONV_P, dev)
    xd = to_dev(R.fp32_block(R.FCONV_SEED + 99, (2, 8, 5, 96), 1.0), dev)
    assert torch.equal(sn.fconv(xd, w, precision=sn.BF16), sn.fconv(xd, w, precision=sn.FP32))
    del keep


@pytest.mark.parametrize("nf", [8, 32, 256])
def test_full_outside_16_64_128_bins_runs_the_fp32_kernel_under_bf16(dev, nf):
    from fnssl import spatialnet as sn
    sd = R.full_state_dict(R.FULL_SEED + nf, nf, "G")
    w, keep, _ = sn.pack_full(sd, R.FULL_P, dev)
    xd = to_dev(R.fp32_block(R.FULL_SEED + 98 + nf, (1, nf, 3, 96), 1.0), dev)
    assert torch.equal(sn.full(xd, w, precision=sn.BF16), sn.full(xd, w, precision=sn.FP32))
    del keep
