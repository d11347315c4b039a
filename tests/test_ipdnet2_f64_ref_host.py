"""Pin tests/ipdnet2_f64_ref.py (the float64 restatement the fp32 IPDnet2 kernels are held to in
test_gpu_ipdnet2_f64.py).  CPU only.  Three independent anchors: the float32 oracle ``oracle/ipdnet2_oracle.py`` at
float32 rounding, tests/golden/g14_ipdnet2.npz (outputs of the reference's own torch classes) at the goldens' own
tolerance (test_oracle_ipdnet2.py: 2e-5 for the pieces, rtol 1e-4 / atol 5e-5 for layers and networks), and the O(T^2)
parallel float64 Mamba ``mamba_parallel_f64`` at 1e-10."""
import numpy as np

import ipdnet2_f64_ref as R8
from conftest import assert_close, load_golden, rs_randn
from fnssl import weights as W
from oracle import ipdnet2_oracle as O2

# "float32 rounding": an O(1) float32 result of a few hundred float32 operations is ~sqrt(n) * 2^-24 * |x| ~ 1e-6 from its
# exact value.  Measured on these shapes (float32 oracle against this module, max abs): 7.4e-8 (_full, outputs up to 0.39)
# .. 1.0e-6 (LayerNorm, outputs up to 4.5); layer 6.0e-7 and network 9.2e-7 (outputs up to 4.9 / 1.4), which get
# rtol = atol = 1e-5 below.
F32 = dict(rtol=1e-5, atol=5e-6)
GOLD = dict(rtol=2e-5, atol=2e-5)
GOLD_NET = dict(rtol=1e-4, atol=5e-5)


def test_pieces_agree_with_float32_oracle_and_reference_goldens():
    g = load_golden("g14_ipdnet2")
    x = rs_randn(3, (3, 96, 7))
    got = R8.layer_norm(x.transpose(0, 2, 1), g["ln_w"], g["ln_b"]).transpose(0, 2, 1)
    assert got.dtype == np.float64
    assert_close(got, g["ln_out"], what="LayerNorm vs golden", **GOLD)
    assert_close(got, O2.layer_norm(x.transpose(0, 2, 1), g["ln_w"], g["ln_b"]).transpose(0, 2, 1), what="LayerNorm", **F32)
    xc = rs_randn(6, (4, 10, 23))
    y, st = R8.causal_conv1d(xc, g["cc_w"], g["cc_b"])
    assert_close(y, g["cc_out"], what="CausalConv1d vs golden", **GOLD)
    assert_close(y, O2.causal_conv1d(xc, g["cc_w"], g["cc_b"])[0], what="CausalConv1d", **F32)
    assert st.shape == (4, 10, 4) and np.array_equal(st, xc[..., -4:].astype(np.float64))
    sd = W.make_ipdnet2_state(2100)
    x0 = rs_randn(2101, (2, 32, 6, 96))
    f1 = R8.fconv(sd, "layers.0.fconv1", x0)
    assert_close(f1, g["fconv1_out"], what="_fconv vs golden", **GOLD)
    assert_close(f1, O2.fconv(sd, "layers.0.fconv1", x0), what="_fconv", **F32)
    for pool, key in ((2, "pool2_out"), (8, "pool8_out")):
        assert_close(R8.avgpool_f(x0, pool), g[key], what="F-pool vs golden", rtol=1e-6, atol=1e-6)
        assert_close(R8.fconv(sd, "layers.0.fconv1", x0, residual=True, pool=pool), O2.avgpool_f(x0 + g["fconv1_out"], pool),
                     what="fconv + residual + pool %d" % pool, **GOLD)
    x128 = rs_randn(2102, (1, 128, 3, 96))
    assert_close(R8.full(sd, "layers.0.", x128), g["full128_out"], what="_full 128 vs golden", **GOLD)
    assert_close(R8.full(sd, "layers.0.", x128), O2.full(sd, "layers.0.", x128), what="_full 128", **F32)
    x16 = rs_randn(2103, (2, 16, 5, 96))
    assert_close(R8.full(sd, "layers.1.", x16), g["full16_out"], what="_full 16 vs golden", **GOLD)
    assert_close(R8.full(sd, "layers.1.", x16, residual=True), x16 + O2.full(sd, "layers.1.", x16), what="_full 16 + residual",
                 **F32)
    assert_close(R8.fconv(sd, "layers.1.fconv2", x16), g["fconv2_l1_out"], what="_fconv l1 vs golden", **GOLD)
    xt = rs_randn(2104, (6, 13, 96))
    assert_close(R8.avgpool_t(xt[None], 5)[0], g["tpool_out"], what="T-pool (floor) vs golden", rtol=1e-6, atol=1e-6)
    # FreqInverse + tanh alone is the head with an identity decoder, read back through the output re-ordering
    xh = rs_randn(2105, (2, 96, 4, 16))                                    # the golden's [B, H, T, Fc]
    sdi = dict(sd)
    sdi["decoder.weight"], sdi["decoder.bias"] = np.eye(16, dtype=np.float32), np.zeros(16, np.float32)
    hd = R8.head(sdi, xh.transpose(0, 3, 2, 1))                            # [B, T, 2F, 4, 2]
    B, T, F = 2, 4, 256
    dec = hd.reshape(B, T, F, 2, 4, 2).transpose(0, 2, 1, 5, 3, 4).reshape(B, F, T, 16)     # [.., a, g, m] -> a*8+g*4+m
    assert_close(dec.transpose(0, 3, 2, 1), g["finv_out"], what="FreqInverse vs golden", **GOLD)


def test_layers_and_networks_agree_with_oracle_and_goldens():
    g = load_golden("g14_ipdnet2")
    sd = W.make_ipdnet2_state(2100)
    x1 = rs_randn(2106, (1, 16, 10, 96))
    y, st = R8.layer_forward(sd, "layers.1.", x1, False)
    assert_close(y, g["layer1_out"], what="layer 1 vs golden", **GOLD_NET)
    assert_close(y, O2.layer_forward(sd, "layers.1.", x1, False)[0], what="layer 1", rtol=1e-5, atol=1e-5)
    x0 = rs_randn(2107, (1, 256, 10, 96), 0.5)
    y, _ = R8.layer_forward(sd, "layers.0.", x0, True)
    assert y.shape == (1, 16, 10, 96)
    assert_close(y, g["layer0_out"], what="layer 0 vs golden", **GOLD_NET)
    xn = rs_randn(2110, (2, 10, 256, 20))
    out = R8.forward(sd, xn)
    assert out.shape == (2, 4, 512, 4, 2) and out.dtype == np.float64
    assert_close(out, g["net_out"], what="network vs golden", **GOLD_NET)
    assert_close(out, O2.forward(sd, xn), what="network", rtol=1e-5, atol=1e-5)
    sd3 = W.make_ipdnet2_state(2200, dim_input=30, num_layers=3)
    assert_close(R8.forward(sd3, rs_randn(2210, (1, 30, 256, 15))), g["net30_out"], what="15-mic network vs golden", **GOLD_NET)
    ym, _ = R8.mamba(sd, "layers.1.mhsa.", rs_randn(2108, (3, 17, 96)))
    assert_close(ym, g["mamba_out"], what="mamba vs the goldens' torch twin", rtol=1e-4, atol=2e-5)


def test_recurrent_float64_mamba_equals_parallel_form():
    sd = W.make_ipdnet2_state(2500, num_layers=2)
    p = "layers.1.mhsa."
    x = rs_randn(2501, (3, 40, 96))
    got, _ = R8.mamba(sd, p, x)
    assert_close(got, O2.mamba_parallel_f64(sd, p, x), what="recurrent vs parallel float64", rtol=1e-10, atol=1e-10)
    # and on the probe, whose dt spans e^-25 .. 25 and whose decay underflows: the two forms share no scan code
    ps = R8.probe_state(sd, p, 0, "spread")
    got, _ = R8.mamba(ps, p, x)
    want = O2.mamba_parallel_f64(ps, p, x)
    err, scale = R8.channel_rel_err(got, want)
    assert err.max() <= 1e-10, err.max()


def test_chunked_with_state_equals_whole():
    sd = W.make_ipdnet2_state(2510, num_layers=2)
    x = rs_randn(2511, (1, 4, 23, 96))
    whole, stw = R8.mamba_block(sd, "layers.1.norm_mhsa", "layers.1.mhsa", x, residual=True)
    st, parts, t0 = None, [], 0
    for n in (4, 1, 2, 16):                                                # chunks shorter than the conv's 3 carried taps
        y, st = R8.mamba_block(sd, "layers.1.norm_mhsa", "layers.1.mhsa", x[:, :, t0:t0 + n], st, residual=True)
        parts.append(y)
        t0 += n
    assert_close(np.concatenate(parts, 2), whole, what="Mamba chunked", rtol=1e-12, atol=1e-12)
    assert_close(st[0], stw[0], what="conv taps", rtol=0, atol=0)
    assert_close(st[1], stw[1], what="SSM state", rtol=1e-12, atol=1e-14)
    # the float32 oracle's state layout is the same
    _, sto = O2.mamba_block(sd, "layers.1.norm_mhsa", "layers.1.mhsa", x)
    assert_close(stw[0], sto[0], what="conv taps vs oracle", **F32)
    assert_close(stw[1], sto[1], what="SSM state vs oracle", **F32)
    xc = rs_randn(6, (2, 10, 8, 23))
    w, b = rs_randn(7, (96, 10, 5), 0.1), rs_randn(8, (96,), 0.1)
    ye, se = R8.encoder(w, b, xc)
    y0, s0 = R8.encoder(w, b, xc[..., :9])
    y1, s1 = R8.encoder(w, b, xc[..., 9:11], s0)
    y2, s2 = R8.encoder(w, b, xc[..., 11:], s1)
    assert_close(np.concatenate([y0, y1, y2], 2), ye, what="encoder chunked", rtol=1e-13, atol=1e-13)
    assert np.array_equal(s2, se) and se.shape == (2, 10, 8, 4)
    sdn = W.make_ipdnet2_state(2300, num_layers=2)
    xn = rs_randn(2301, (1, 10, 256, 20))
    wn = R8.forward(sdn, xn)
    st, outs = {}, []
    for t0, t1 in ((0, 5), (5, 15), (15, 20)):
        y, st = R8.forward(sdn, xn[..., t0:t1], state=st)
        outs.append(y)
    assert_close(np.concatenate(outs, 1), wn, what="network chunked", rtol=1e-11, atol=1e-12)


def test_probe_is_self_consistent():
    sd = W.make_ipdnet2_state(2600, num_layers=2)
    p = "layers.1.mhsa."
    x = rs_randn(2601, (3, 30, 96))
    for half in (0, 1):
        for kind in ("spread", "exact", "silu"):
            ps = R8.probe_state(sd, p, half, kind)
            assert all(v.dtype == np.float32 for v in ps.values())
            wo = ps[p + "out_proj.weight"]
            assert wo.shape == (96, 192) and set(np.unique(wo)) == {0.0, 1.0} and (wo.sum(1) == 1).all()
            assert np.array_equal(np.nonzero(wo)[1], 96 * half + np.arange(96))
            assert not ps[p + "D"].any()
            a = np.exp(ps[p + "A_log"].astype(np.float64))
            assert 1e-2 <= a.min() and a.max() <= 64.0
            # the one-hot out_proj returns exactly the selected inner channels: evaluate the block with a 192 x 192
            # identity out_proj and compare bit for bit
            full_ = dict(ps)
            full_[p + "out_proj.weight"] = np.eye(192, dtype=np.float32)
            inner, _ = R8.mamba(full_, p, x)
            got, _ = R8.mamba(ps, p, x)
            assert np.array_equal(got, inner[..., 96 * half:96 * half + 96])
    b = R8.probe_state(sd, p, 0, "spread")[p + "dt_proj.bias"]
    assert b.min() == -25.0 and b.max() == 25.0 and len(np.unique(b)) == 192
    be = R8.probe_state(sd, p, 0, "exact")
    assert not be[p + "dt_proj.weight"].any()
    b = be[p + "dt_proj.bias"]
    assert b.min() == -60.0 and b.max() == 60.0
    one = np.float32(1.0)
    last = b[(one + np.exp(b.astype(np.float32)) > one)].min()            # the last value with 1 + e^x > 1 in float32
    assert np.float32(20.0) in b and np.nextafter(np.float32(20), np.float32(21)) in b
    assert np.nextafter(np.float32(20), np.float32(19)) in b
    # ... its float32 neighbours on both sides are there too, so the threshold itself is bracketed to one step
    assert np.nextafter(last, np.float32(-100)) in b and np.nextafter(last, np.float32(0)) in b
    assert abs(float(last) - R8.LAST_LT1) < 4e-6
    assert (R8.probe_state(sd, p, 0, "silu")[p + "in_proj.weight"] == 4 * sd[p + "in_proj.weight"]).all()
