"""Float64 references for the config-3 tests of IPDnet training (tests/test_gpu_ipdnet_train.py).

* an LSTM step loop whose gate pre-activations keep their gradient (the BPTT kernel's dA);
* the weight-gradient products of one LSTM layer and of one causal 3x3 conv, over any range of rows;
* the per-op backward of the conv head;
* a restatement of the split-K slab plans (csrc/wgrad.hip ``plan_slabs``, csrc/conv_train.hip ``wgrad_plan``), so that
  a test can name the rows of one slab and of one 16-row stage.

Plain torch in float64; nothing here calls the library under test."""
import torch
import torch.nn.functional as F

STAGE = 16                   # rows per stage of both split-K kernels (kBK)


def lstm_bptt(x, params, dh):
    """One (bi)LSTM layer over independent sequences, in float64 with autograd.

    x [S, T, I]; params: per direction (w_ih [4H, I], w_hh [4H, H], b_ih, b_hh); dh [S, T, ndir * H], the upstream
    gradient.  Returns h [S, T, ndir * H], dA [S, T, ndir * 4H] (pre-activation gate gradients, PyTorch gate order
    i, f, g, o) and dx [S, T, ndir, I] (the input gradient through each direction separately)."""
    S, T, _ = x.shape
    hs, das, dxs = [], [], []
    for d, (w_ih, w_hh, b_ih, b_hh) in enumerate(params):
        H = w_hh.shape[1]
        xd = x.detach().clone().requires_grad_(True)
        h = x.new_zeros((S, H))
        c = x.new_zeros((S, H))
        out, pre = [None] * T, [None] * T
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            a = xd[:, t] @ w_ih.t() + h @ w_hh.t() + b_ih + b_hh
            a.retain_grad()
            i, f, g, o = a.split(H, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            out[t], pre[t] = h, a
        hd = torch.stack(out, 1)
        (hd * dh[..., d * H:(d + 1) * H]).sum().backward()
        hs.append(hd.detach())
        das.append(torch.stack([a.grad for a in pre], 1))
        dxs.append(xd.grad)
    return torch.cat(hs, -1), torch.cat(das, -1), torch.stack(dxs, 2)


def lstm_weight_grads(da, xs, h, hidden, ndir, nsteps, r0, r1, chunk=1 << 16):
    """dW_ih = dA^T [x0 | x2], dW_hh = dA^T h_prev, db = sum dA over rows [r0, r1) of one layer, in float64.

    da [R, ndir * 4H], xs (list of [R, c] input matrices), h [R, ndir * H]: the layer's row matrices (row = sequence *
    nsteps + step).  h_prev is h one step earlier in the direction's own order, zero at the sequence boundary.
    Returns {"wih", "whh", "b"}: lists over directions."""
    G = 4 * hidden
    cin = sum(x.shape[1] for x in xs)
    dev = da.device
    acc = {k: [torch.zeros(s, dtype=torch.float64, device=dev) for _ in range(ndir)]
           for k, s in (("wih", (G, cin)), ("whh", (G, hidden)), ("b", (G,)))}
    for c0 in range(r0, r1, chunk):
        rr = torch.arange(c0, min(c0 + chunk, r1), device=dev)
        step = rr % nsteps
        x = torch.cat([t[rr] for t in xs], 1).double()
        for d in range(ndir):
            a = da[rr, d * G:(d + 1) * G].double()
            if d == 0:
                ok, src = step > 0, rr - 1
            else:
                ok, src = step < nsteps - 1, rr + 1
            hp = h[src.clamp(0, h.shape[0] - 1), d * hidden:(d + 1) * hidden].double() * ok[:, None]
            acc["wih"][d] += a.t() @ x
            acc["whh"][d] += a.t() @ hp
            acc["b"][d] += a.sum(0)
    return acc


def conv_weight_grads(dz, xs, r0, r1, chunk=1 << 16):
    """dW [cout, cin, 3, 3] of the causal conv (Conv2d padding (1, 2), last two frames cropped) over rows [r0, r1) of
    r = (b * nf + f) * nt + t, in float64: nine tap-shifted products dZ^T X[f + kf - 1, t + kt - 2] (zero outside).
    dz [nb, nf, nt, cout]; xs: list of [nb, nf, nt, c] tensors, concatenated along channels (conv 1's [D3 | x])."""
    nb, nf, nt, cout = dz.shape
    cin = sum(x.shape[3] for x in xs)
    dev = dz.device
    dw = torch.zeros((cout, cin, 3, 3), dtype=torch.float64, device=dev)
    for c0 in range(r0, r1, chunk):
        rr = torch.arange(c0, min(c0 + chunk, r1), device=dev)
        t, f, b = rr % nt, (rr // nt) % nf, rr // (nt * nf)
        a = dz[b, f, t].double()
        for kf in range(3):
            for kt in range(3):
                ff, tt = f + kf - 1, t + kt - 2
                ok = ((ff >= 0) & (ff < nf) & (tt >= 0))[:, None]
                fc, tc = ff.clamp(0, nf - 1), tt.clamp(0, nt - 1)
                xg = torch.cat([x[b, fc, tc] for x in xs], 1).double() * ok
                dw[:, :, kf, kt] += a.t() @ xg
    return dw


def act_pool_backward(y, dp, k, act):
    """Autograd of AvgPool((1, k))(act(Z)) for one utterance: y [nf, nt, C] the saved post-activation output, dp
    [nf, nt // k, C] -> dZ [nf, nt, C].  Z is recovered from y (ReLU: y itself, whose derivative at 0 is 0; tanh:
    atanh(y))."""
    y = y.double().permute(2, 0, 1)[None]
    z = (y if act == "relu" else torch.atanh(y)).detach().requires_grad_(True)
    a = torch.relu(z) if act == "relu" else torch.tanh(z)
    p = F.avg_pool2d(a, (1, k)) if k > 1 else a
    (p * dp.double().permute(2, 0, 1)[None]).sum().backward()
    return z.grad[0].permute(1, 2, 0)


def conv_backward_data(dz, w, cin_g):
    """Input gradient of the causal conv for one utterance: dz [nf, nt, cout] (pre-activation), w [cout, cin, 3, 3]
    -> dX [nf, nt, cin_g], the first cin_g input channels."""
    nf, nt, _ = dz.shape
    g = F.pad(dz.double().permute(2, 0, 1)[None], (0, 2))           # the two cropped frames get no gradient
    dx = torch.nn.grad.conv2d_input((1, w.shape[1], nf, nt), w.double(), g, padding=(1, 2))
    return dx[0, :cin_g].permute(1, 2, 0)


def slab_plan(rows, per_slab, cus, min_stages, cap):
    """(slabs, rows_per_slab) of the split-K planners: about three rounds of two resident workgroups per CU, at least
    ``min_stages`` 16-row stages per slab, at most ``cap`` slabs, rows per slab a multiple of 16."""
    slabs = (3 * 2 * cus + per_slab - 1) // per_slab
    slabs = min(slabs, max(1, (rows + min_stages * STAGE - 1) // (min_stages * STAGE)), cap)
    slabs = max(slabs, 1)
    rps = (rows + slabs - 1) // slabs
    rps = (rps + STAGE - 1) // STAGE * STAGE
    return (rows + rps - 1) // rps, rps
