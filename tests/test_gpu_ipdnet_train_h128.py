"""GPU tests of IPDnet training at the reference's default width, hidden_size = 128 (``IPDnet()``: two microphones,
full-band BiLSTM H = 64, narrow-band LSTM H = 128 online or BiLSTM H = 64 offline): the H = 64 instantiations of the
reserve-saving forward and of BPTT (csrc/lstm_train_h64.hip), the train graph at either width (fnssl/ipdnet_train.py),
``IPDnet.forward_train`` and ``MyModel(train_on_device=True)``.  Layer by layer against float64 references
(tests/fp64_ref.py) at geometries that take every branch of the launch planner, the whole network against the PyTorch
CPU restatement (tests/ipdnet_train_ref.py) with the same dropout masks and against the real reference's golden step
(tests/golden/g22_ipdnet_train_h128.npz).  Tolerances: those of tests/test_gpu_ipdnet_train.py for the same
arithmetic at twice the dot-product length."""
import numpy as np
import pytest

from conftest import assert_close, load_golden, rs_randn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import fp64_ref as F64  # noqa: E402
import ipdnet_step_ref as S  # noqa: E402
import ipdnet_train_ref as R  # noqa: E402
from test_gpu_ipdnet_train import _free, _sampled_sequences, _shape, fails_without, rel_close, rel_err  # noqa: E402

HIDDEN = 128


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; none visible (the HIP path has no CPU fallback)")
    from fnssl import _lib
    _lib.load()
    return torch.device("cuda:0")


def _nets(dev, sd, nc, online, hidden=HIDDEN):
    from IPDnet.FixedAarryIPDnet import IPDnet
    net = IPDnet(nc, hidden, 2, online)
    net.load_state_dict(R.state_tensors(sd))
    net = net.to(dev).train()
    ref = R.RefIPDnet(nc, hidden, 2, online)
    ref.load_state_dict(R.state_tensors(sd))
    return net, ref


# ----------------------------------------------------------------------------------------------------------------
# layer legs against float64
# ----------------------------------------------------------------------------------------------------------------
# (mode, hidden, ndir, c0, c2, c0g) of a hidden-128 train-graph LSTM -> (forward family with a reserve, BPTT family), at
# every geometry: H = 64 has no cluster kernel (f32c_handles / bwdc_handles decline it) and its BPTT never splits (one
# or three 64-channel output slices); the online narrow-band layer's [D | x] input keeps its forward off the H = 128
# cluster kernel, its BPTT (co_pad = 256: four members) is cluster-resident
LSTM_FAMILIES = {
    ("full", 64, 2, 4, 0, 0): ("train", "bwd"),                      # block 1 full band
    ("full", 64, 2, 128, 4, 128): ("train", "bwd"),                  # block 2 full band
    ("narrow", 128, 1, 128, 4, 128): ("train", "bwd_cluster"),       # online narrow band (blocks 1 and 2)
    ("narrow", 64, 2, 128, 4, 128): ("train", "bwd"),                # offline narrow band (blocks 1 and 2)
}
# layer -> (online model?, index in IPDnetTrainGraph.lstms): one of each distinct shape above
LAYERS = {"full1": (True, 0), "narrow_online": (True, 1), "full2": (True, 2), "narrow_offline": (False, 1)}
# the branches of the training forward's launch plan (csrc/lstm_train.hip plan_rounds) a layer leg runs at
BRANCHES = {"full1": ("split4", "split4w8", "split2", "rounds"), "full2": ("split4", "split4w8", "split2", "rounds"),
            "narrow_offline": ("split4", "split4w8", "split2", "rounds"), "narrow_online": ("split4", "rounds")}
LEGS = [(layer, br) for layer in sorted(LAYERS) for br in BRANCHES[layer]]


def forward_branch(nseq, ndir, cus):
    """plan_rounds of the reserve-saving forward at H = 64 / 128, restated: with total = 16-sequence groups x directions,
    four waves per group while total <= 2 CUs (8-wave workgroups of two groups once total > CUs), two waves per group
    while 2 total <= 12 CUs, else one wave per group in rounds of <= 12 waves per CU."""
    total = (nseq + 15) // 16 * ndir
    if total <= 2 * cus:
        return "split4w8" if total > cus else "split4"
    return "split2" if 2 * total <= 12 * cus else "rounds"


def leg_geometry(mode, ndir, branch, cus):
    """(nb, nf, nt) with 20 - 24 steps whose sequence count puts the forward in ``branch`` on a device of ``cus`` CUs: no
    multiple of 16 sequences, sequences per utterance no multiple of 16 (a group straddles two utterances)."""
    steps = 22 if mode == "full" else 24
    if branch == "split4":
        nb, q = 2, (36 if mode == "full" else 20)
    else:
        q = 301 if mode == "full" else 250
        # groups x directions in the middle of the branch's window: (CUs, 2 CUs], (2 CUs, 6 CUs], (6 CUs, ...)
        total = {"split4w8": 1.5, "split2": 2.6, "rounds": 6.25}[branch] * cus
        nb = max(2, int(round(total / ndir * 16 / q)))
        while (nb * q) % 16 == 0:
            nb += 1
    return (nb, steps, q) if mode == "full" else (nb, q, steps)


def _train_graph(dev, online, wseed):
    from fnssl import ipdnet_train
    from fnssl import weights as W
    sd = W.make_ipdnet_state(wseed, 4, HIDDEN, 2, online)
    net, _ = _nets(dev, sd, 4, online)
    return ipdnet_train.IPDnetTrainGraph(net)


def assert_lstm_families(g, nb, nf, nt, dev):
    """Every LSTM call of the train graph takes the family LSTM_FAMILIES names, with the operands in the graph's
    natural layouts (plan queries: nothing is launched)."""
    from fnssl import ops
    fw, bw, _, _ = g.streams(dev)
    got, want = [], []
    for L in g.lstms:
        nseq, nsteps = (nb * nt, nf) if L.mode == "full" else (nb * nf, nt)
        x0 = L.natural(nb, nt, nf, L.c0, dev)
        x2 = L.natural(nb, nt, nf, L.c2, dev) if L.c2 else None
        res = torch.empty(ops.lstm_reserve_floats(nseq, L.hidden, L.ndir, nsteps), device=dev)
        out = L.natural(nb, nt, nf, L.ndir * L.hidden, dev)
        da = L.natural(nb, nt, nf, L.ndir * 4 * L.hidden, dev)
        dx = L.natural(nb, nt, nf, L.ndir * L.c0g, dev) if L.c0g else None
        got.append((L.name, ops.lstm_plan(L.mode, x0, None, x2, fw[L.name], L.hidden, out, reserve=res)[0],
                    ops.lstm_backward(L.mode, res, out, da, dx, bw[L.name], L.hidden, L.c0g, plan_only=True)))
        want.append((L.name,) + LSTM_FAMILIES[_shape(L)])
        del x0, x2, res, out, da, dx
    _free()
    assert got == want, got


def test_leg_geometries_cover_every_forward_branch(dev):
    """The geometries of the layer legs fall one in each branch of the forward's launch plan on this device — the H = 64
    shapes in all four (split 4 in 4- and 8-wave workgroups, split 2, per-wave rounds), the H = 128 narrow shape in a
    small and a rounds-sized one — with a partial last group and a group that straddles two utterances."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for layer, branch in LEGS:
        g_mode, ndir = ("full", 2) if layer.startswith("full") else ("narrow", 1 if layer == "narrow_online" else 2)
        nb, nf, nt = leg_geometry(g_mode, ndir, branch, cus)
        nseq, q, steps = (nb * nt, nt, nf) if g_mode == "full" else (nb * nf, nf, nt)
        assert forward_branch(nseq, ndir, cus) == branch, (layer, branch, nseq, cus)
        assert nseq % 16 and q % 16 and nb >= 2 and 20 <= steps <= 24, (layer, branch, nb, nf, nt)
    # the issue's own figures on 256 CUs
    assert [forward_branch(n, 2, 256) for n in (72, 4515, 12500)] == ["split4", "split2", "rounds"]
    assert [forward_branch(n, 2, 256) for n in (40, 5000, 12500)] == ["split4", "split2", "rounds"]


@pytest.mark.parametrize("layer,branch", LEGS)
def test_lstm_layer_vs_float64(dev, layer, branch):
    """One hidden-128 IPDnet LSTM layer, operands in the train graph's natural layouts ([D | x] with the 4 skip channels
    concatenated), at a geometry of the named forward branch: exact kernel families; the reserve-saving forward equals
    the plain one bit for bit; h, dA (gate order i, f, g, o) and dx of the first, a middle, the last and the
    utterance-boundary 16-sequence groups against a float64 step loop; the weight gradients over ALL rows against
    float64 products of the kernel's own dA, inputs and shifted h, with a tolerance that one missing 16-row stage or
    the last slab of the split-K sum would exceed."""
    from fnssl import _lib, ops
    online, idx = LAYERS[layer]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    g = _train_graph(dev, online, 2800)
    L = g.lstms[idx]
    mode, H, ndir, c0, c2, c0g = _shape(L)
    nb, nf, nt = leg_geometry(mode, ndir, branch, cus)
    geom = "%s (%d x %d x %d)" % (branch, nb, nf, nt)
    nseq, nsteps = (nb * nt, nf) if mode == "full" else (nb * nf, nt)
    assert forward_branch(nseq, ndir, cus) == branch and nseq % 16 and (nt if mode == "full" else nf) % 16
    fw, bw, _, _ = g.streams(dev)
    gen = torch.Generator(device=dev).manual_seed(2801 + idx)
    x0 = L.natural(nb, nt, nf, c0, dev).normal_(0, 0.5, generator=gen)
    x2 = L.natural(nb, nt, nf, c2, dev).normal_(0, 0.5, generator=gen) if c2 else None
    res = torch.empty(ops.lstm_reserve_floats(nseq, H, ndir, nsteps), device=dev)
    out = L.natural(nb, nt, nf, ndir * H, dev)
    dh = L.natural(nb, nt, nf, ndir * H, dev).normal_(0, 1, generator=gen)
    da = L.natural(nb, nt, nf, ndir * 4 * H, dev)
    dx = L.natural(nb, nt, nf, ndir * c0g, dev) if c0g else None
    fams = (ops.lstm_plan(mode, x0, None, x2, fw[L.name], H, out, reserve=res)[0],
            ops.lstm_backward(mode, res, dh, da, dx, bw[L.name], H, c0g, plan_only=True))
    assert fams == LSTM_FAMILIES[_shape(L)], fams
    fallbacks = ops.cluster_fallbacks(dev)
    ops.lstm_layer(mode, x0, None, x2, fw[L.name], H, out, reserve=res)
    plain = L.natural(nb, nt, nf, ndir * H, dev)
    ops.lstm_layer(mode, x0, None, x2, fw[L.name], H, plain)
    assert torch.equal(out, plain), "the reserve-saving forward computes the same h"
    del plain
    ops.lstm_backward(mode, res, dh, da, dx, bw[L.name], H, c0g)
    assert ops.cluster_fallbacks(dev) == fallbacks
    del res
    # ---- sampled sequences against a float64 step loop (CPU)
    seqs = torch.tensor(_sampled_sequences(mode, nb, nf, nt), device=dev)
    q = nt if mode == "full" else nf
    bi, qi = seqs // q, seqs % q

    def sample(t):                  # logical [nb, nt, nf, C] -> [S, nsteps, C] of the sampled sequences
        return (t if mode == "full" else t.permute(0, 2, 1, 3))[bi, qi].double().cpu()

    params = [[p.detach().double().cpu() for p in L.params(n)]
              for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    h64, da64, dx64 = F64.lstm_bptt(torch.cat([sample(x0)] + ([sample(x2)] if c2 else []), -1), list(zip(*params)),
                                    sample(dh))
    got_h = sample(out)
    print("CHECK %-58s %.3g of the tolerance (rtol 1e-4, atol 1e-5)" % (
        "%s %s h" % (layer, geom), float(((got_h - h64).abs() / (1e-5 + 1e-4 * h64.abs())).max())))
    assert_close(got_h.numpy(), h64.numpy(), 1e-4, 1e-5, "%s %s: h of the sampled sequences" % (layer, geom))
    rel_err(sample(da), da64, 2e-4, "%s %s dA (sampled)" % (layer, geom))
    if c0g:
        assert dx.shape[-1] == ndir * c0g                # the 4 concatenated skip channels get no gradient
        rel_err(sample(dx), dx64[..., :c0g].reshape(dx64.shape[0], nsteps, ndir * c0g), 2e-4,
                "%s %s dx (sampled)" % (layer, geom))
    # ---- weight gradients over all rows against float64 products (on the device)
    init = 0.5
    gw = {k: [torch.full(s, init, device=dev) for _ in range(ndir)]
          for k, s in (("wih", (4 * H, c0 + c2)), ("whh", (4 * H, H)), ("bih", (4 * H,)), ("bhh", (4 * H,)))}
    ops.lstm_weight_grads(L.rows(da), L.rows(x0), L.rows(x2) if c2 else None, L.rows(out), H, ndir, nsteps,
                          gw["wih"], gw["whh"], gw["bih"], gw["bhh"])
    rows = nseq * nsteps
    xs = [L.rows(x0)] + ([L.rows(x2)] if c2 else [])
    part = lambda r0, r1: F64.lstm_weight_grads(L.rows(da), xs, L.rows(out), H, ndir, nsteps, r0, r1)  # noqa: E731
    want = part(0, rows)
    # the split-K plan of this launch (csrc/wgrad.hip): slab count from the workspace size, rows per slab restated
    M, ncat = ndir * 4 * H, c0 + c2 + H
    slabs = (_lib.load().fnssl_lstm_weight_grads_workspace_bytes(rows, H, ndir, c0, c2) - 256) // (4 * M * (ncat + 1))
    ntiles = ((0 if c0 == 4 else (c0 + 127) // 128) + (0 if c2 == 4 and c0 != 4 else (c2 + 127) // 128)
              + (H + 127) // 128)
    plan, rps = F64.slab_plan(rows, M // 256 * ntiles, cus, 4, 512)
    assert plan == slabs >= 2, (plan, slabs)
    stage, last = part(rps - 16, rps), part((slabs - 1) * rps, rows)
    for d in range(ndir):
        for k, name in (("wih", "dW_ih"), ("whh", "dW_hh"), ("bih", "db_ih"), ("bhh", "db_hh")):
            w = want["b" if k[0] == "b" else k][d]
            what = "%s %s %s[%d] (%d slabs)" % (layer, geom, name, d, slabs)
            rel_err(gw[k][d].double() - init, w, 2e-5, what)
            fails_without(w, {"one 16-row stage": stage["b" if k[0] == "b" else k][d],
                              "the last slab": last["b" if k[0] == "b" else k][d]}, 2e-5, what)
    del x0, x2, out, dh, da, dx, gw, want, stage, last
    _free()


# ----------------------------------------------------------------------------------------------------------------
# whole network against the CPU restatement and the reference's golden step
# ----------------------------------------------------------------------------------------------------------------
# G22's cases: (input_size, online, nb, nf, nt, weight seed)
CASES = {"a": (4, True, 2, 24, 36, 2700), "b": (4, False, 2, 20, 24, 2710), "c": (8, True, 2, 16, 36, 2720)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_train_step_matches_cpu_restatement(dev, case):
    from fnssl import ops
    from fnssl import weights as W
    nc, online, nb, nf, nt, wseed = CASES[case]
    base, b0 = 1234, 0
    sd = W.make_ipdnet_state(wseed, nc, HIDDEN, 2, online)
    net, ref = _nets(dev, sd, nc, online)
    net.force_dropout_base = base
    net.utt_offset = b0
    x = rs_randn(wseed + 1, (nb, nc, nf, nt))
    gt = rs_randn(wseed + 2, (nb, nt // 12, 2 * nf, nc // 2 - 1, 2), 0.5)
    fallbacks = ops.cluster_fallbacks(dev)
    pred = net.forward_train(torch.from_numpy(x).to(dev))
    assert pred.grad_fn is not None
    loss = R.pit_mse(pred, torch.from_numpy(gt).to(dev))
    loss.backward()
    pref = ref(torch.from_numpy(x), R.site_masks(base, nb, nt, nf, b0, c=HIDDEN))
    lref = R.pit_mse(pref, torch.from_numpy(gt))
    lref.backward()
    np.testing.assert_allclose(pred.detach().cpu().numpy(), pref.detach().numpy(), rtol=1e-4, atol=1e-5)
    assert abs(loss.item() - lref.item()) <= 1e-5 * abs(lref.item())
    rp = dict(ref.named_parameters())
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        rel_close(p.grad.cpu().numpy(), rp[k].grad.numpy(), 5e-4, "grad " + k)
    assert ops.cluster_fallbacks(dev) == fallbacks
    # one Adam step on both; eval() then sees the stepped weights
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    opt_r = torch.optim.Adam(ref.parameters(), lr=5e-4)
    opt.step()
    opt_r.step()
    for k, p in net.named_parameters():
        g = rp[k].grad.abs().numpy()
        sel = g > 1e-3 * g.max()
        np.testing.assert_allclose(p.detach().cpu().numpy()[sel], rp[k].detach().numpy()[sel], rtol=0, atol=2e-5)
    net.eval()
    with torch.no_grad():
        ye = net(torch.from_numpy(x).to(dev)).cpu().numpy()
        ref.eval()
        yr = ref(torch.from_numpy(x), [None] * 4).numpy()
    np.testing.assert_allclose(ye, yr, rtol=1e-4, atol=1e-5)


def test_train_step_matches_reference_golden(dev):
    """G22: the real reference (FixedAarryIPDnet.IPDnet(nc, 128, ...) in train() mode, dropout as the keep-scale masks,
    PIT-MSE, autograd, torch.optim.Adam(lr=5e-4)) on cases (a)-(c); G18's bars."""
    from fnssl import weights as W
    g = load_golden("g22_ipdnet_train_h128")
    for case in ("a", "b", "c"):
        nc, online, nb, nf, nt = (int(v) for v in g[case + "_cfg"])
        assert (nc, bool(online), nb, nf, nt) == CASES[case][:5]
        sd = W.make_ipdnet_state(int(g[case + "_wseed"]), nc, HIDDEN, 2, bool(online))
        net, _ = _nets(dev, sd, nc, bool(online))
        net.force_dropout_base = int(g[case + "_base"])
        net.utt_offset = 0
        pred = net.forward_train(torch.from_numpy(g[case + "_x"]).to(dev))
        np.testing.assert_allclose(pred.detach().cpu().numpy(), g[case + "_pred"], rtol=1e-4, atol=1e-5)
        loss = R.pit_mse(pred, torch.from_numpy(g[case + "_gt"]).to(dev))
        assert abs(loss.item() - float(g[case + "_loss"])) <= 1e-5 * abs(float(g[case + "_loss"]))
        loss.backward()
        names = [k for k, _ in net.named_parameters()]
        for i, (k, p) in enumerate(net.named_parameters()):
            gd = p.grad.cpu().numpy().astype(np.float64)
            norm = float(g[case + "_gnorm"][i])
            assert abs(np.sqrt((gd * gd).sum()) - norm) <= 5e-4 * norm + 1e-12, k
            head = g[case + "_ghead"][i]
            n = min(16, gd.size)
            np.testing.assert_allclose(gd.reshape(-1)[:n], head[:n], rtol=0, atol=5e-4 * np.abs(gd).max() + 1e-12,
                                       err_msg=k)
        torch.optim.Adam(net.parameters(), lr=5e-4).step()
        for i, k in enumerate(names):
            p = dict(net.named_parameters())[k].detach().cpu().numpy().reshape(-1)[:16]
            np.testing.assert_allclose(p, g[case + "_phead"][i][:p.size], rtol=0, atol=2e-5, err_msg=k)


def test_batch_sharding_equals_one_batch(dev):
    """Utterances [0:4) with utt_offset 0 plus [4:8) with utt_offset 4 give the gradients of one 8-utterance call: the
    dropout masks follow the global utterance index of the logical [nb, nt, nf, 128] activation."""
    from fnssl import weights as W
    from IPDnet.FixedAarryIPDnet import IPDnet
    sd = W.make_ipdnet_state(2900, 4, HIDDEN, 2, True)
    nb, nf, nt = 8, 16, 24
    x = torch.from_numpy(rs_randn(2901, (nb, 4, nf, nt))).to(dev)
    gt = torch.from_numpy(rs_randn(2902, (nb, nt // 12, 2 * nf, 1, 2), 0.5)).to(dev)

    def grads(parts):
        net = IPDnet(4, HIDDEN, 2, True)
        net.load_state_dict(R.state_tensors(sd))
        net = net.to(dev).train()
        net.force_dropout_base = 99
        for lo, hi in parts:
            net.utt_offset = lo
            # the sum of per-row MSE means: the shards' losses add up to the whole batch's (times nb)
            (R.pit_mse(net.forward_train(x[lo:hi]), gt[lo:hi]) * (hi - lo)).backward()
        return {k: p.grad.clone() for k, p in net.named_parameters()}

    one = grads([(0, nb)])
    two = grads([(0, 4), (4, nb)])
    for k in one:
        rel_close(two[k].cpu().numpy(), one[k].cpu().numpy(), 1e-5, "sharded grad " + k)


def test_forward_train_at_hidden256_is_the_train_mode_forward(dev):
    """At hidden 256 ``forward_train`` is today's train-mode ``forward``: the same bits under a pinned dropout base, and
    the same dropout counters / bases without one."""
    from fnssl import weights as W
    sd = W.make_ipdnet_state(3000, 16, 256, 2, True)
    x = torch.from_numpy(rs_randn(3001, (2, 16, 16, 24))).to(dev)
    outs, grads = [], []
    for entry in ("forward", "forward_train"):
        net, _ = _nets(dev, sd, 16, True, hidden=256)
        net.force_dropout_base = 7
        net.utt_offset = 3
        y = getattr(net, entry)(x)
        (y * y).sum().backward()
        outs.append(y.detach())
        grads.append({k: p.grad for k, p in net.named_parameters()})
        assert net.dropout_calls == 1 and net.last_dropout_base == 7
    assert torch.equal(outs[0], outs[1])
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
    bases = []
    for entry in ("forward", "forward_train"):
        net, _ = _nets(dev, sd, 16, True, hidden=256)
        net.dropout_seed = 11
        a = getattr(net, entry)(x).detach()
        b = getattr(net, entry)(x).detach()
        assert net.dropout_calls == 2 and not torch.equal(a, b)
        bases.append((net.last_dropout_base, a, b))
    assert bases[0][0] == bases[1][0] and torch.equal(bases[0][1], bases[1][1]) and torch.equal(bases[0][2], bases[1][2])


def _two_mic_batch(dev):
    """G19's synthetic batch (tests/ipdnet_step_ref.py), its first two microphones: [2, ns, 2] mixtures of 36 frames."""
    mic_sig, dp, doa, _ = S.g19_batch()
    return (torch.from_numpy(np.ascontiguousarray(mic_sig[:, :, :2])).to(dev),
            {"doa": torch.from_numpy(doa).to(dev), "dp_signal": torch.from_numpy(np.ascontiguousarray(dp[:, :, :2])).to(dev)})


def test_training_step_of_the_default_model_on_device(dev):
    """``MyModel(arch=None, train_on_device=True)``, the reference's own construction: ``training_step`` gives a loss
    with a ``grad_fn`` whose backward fills every ``.grad`` with finite numbers; the loss is ``cal_loss`` of the CPU
    restatement's prediction on ``data_preprocess``'s features (1e-5 relative); an Adam step changes it."""
    from IPDnet.train_step import MyModel
    from fnssl import ops
    from fnssl import weights as W
    torch.manual_seed(3100)
    model = MyModel(arch=None, train_on_device=True, device="cuda:0")
    sd = W.make_ipdnet_state(3101, 4, HIDDEN, 2, True)
    model.arch.load_state_dict(R.state_tensors(sd))
    model = model.to(dev).train()
    base = 4321
    model.arch.force_dropout_base = base
    model.arch.utt_offset = 0
    batch = _two_mic_batch(dev)
    fallbacks = ops.cluster_fallbacks(dev)
    loss = model.training_step(batch, 0)["loss"]
    assert loss.grad_fn is not None and loss.shape == () and np.isfinite(loss.item())
    loss.backward()
    for k, p in model.arch.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all().item() and float(p.grad.abs().max()) > 0, k
    assert ops.cluster_fallbacks(dev) == fallbacks
    data = model.data_preprocess(*batch)
    nb, nc, nf, nt = data[0].shape
    assert (nb, nc, nf, nt) == (2, 4, 256, 36)
    ref = R.RefIPDnet(4, HIDDEN, 2, True)
    ref.load_state_dict(R.state_tensors(sd))
    ref.train()
    with torch.no_grad():
        pref = ref(data[0].cpu(), R.site_masks(base, nb, nt, nf, 0, c=HIDDEN))
        lref = model.cal_loss(pred_batch=pref.to(dev).contiguous(), gt_batch=data[1:])
    print("CHECK training_step loss %.9g, cal_loss of the restatement's prediction %.9g" % (loss.item(), lref.item()))
    assert abs(loss.item() - lref.item()) <= 1e-5 * abs(lref.item())
    torch.optim.Adam(model.arch.parameters(), lr=5e-4).step()
    after = model.training_step(batch, 0)["loss"]
    assert np.isfinite(after.item()) and after.item() != loss.item()
    # without gradients (validation inside a train() module) the opt-in takes no autograd route
    with torch.no_grad(), pytest.raises(RuntimeError, match="call .eval\\(\\) first"):
        model(data[0])


def test_default_module_still_raises_in_train_mode(dev):
    """``train_on_device`` defaults to False: ``MyModel(arch=None)`` keeps the forward-only error in ``train()``."""
    from IPDnet.train_step import MyModel
    model = MyModel(arch=None, device="cuda:0").to(dev).train()
    assert model.train_on_device is False
    with pytest.raises(RuntimeError, match="call .eval\\(\\) first"):
        model.training_step(_two_mic_batch(dev), 0)
    with pytest.raises(RuntimeError, match="call .eval\\(\\) first"):
        model.arch(torch.zeros(1, 4, 16, 24, device=dev))


def test_reference_training_size(dev):
    """One call at the reference's training size, 16 utterances x 2 microphones x 256 bins x 280 frames: finite
    gradients, the LSTM calls' kernel families, no cluster fallback."""
    from fnssl import ops
    from fnssl import weights as W
    from IPDnet.FixedAarryIPDnet import IPDnet
    net = IPDnet()
    net.load_state_dict(R.state_tensors(W.make_ipdnet_state(3200, 4, HIDDEN, 2, True)))
    net = net.to(dev).train()
    net.force_dropout_base = 5
    nb, nf, nt = 16, 256, 280
    x = torch.from_numpy(rs_randn(3201, (nb, 4, nf, nt), 0.5)).to(dev)
    ops.cluster_fallbacks(dev, reset=True)
    pred = net.forward_train(x)
    assert tuple(pred.shape) == (nb, nt // 12, 2 * nf, 1, 2)
    (pred * pred).mean().backward()
    torch.cuda.synchronize()
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all().item(), k
    assert ops.cluster_fallbacks(dev) == 0
    del pred, x
    _free()
    assert_lstm_families(net._train_graph, nb, nf, nt, dev)
