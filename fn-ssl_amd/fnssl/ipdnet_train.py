"""Training of the fixed-array IPDnet (``IPDnet/FixedAarryIPDnet.py``) on the HIP path: the drop-in ``IPDnet.forward`` in
``train()`` mode returns a tensor with a ``grad_fn``, so the reference's loop runs unchanged
(``pred = self.arch(in_batch); loss = cal_loss(pred, gt); loss.backward(); optimizer.step()``, Adam lr 5e-4).

Trainable (``trainable()``): fp32 modules with ``hidden_size`` 256 (full-band BiLSTM H = 128; narrow-band LSTM H = 256
online or BiLSTM H = 128 offline) or 128, the reference's default (full-band BiLSTM H = 64; narrow-band LSTM H = 128
online or BiLSTM H = 64 offline), ``input_size`` a multiple of 4 up to 16 and an output width
``2 * (input_size // 2 - 1) * max_track`` that is a multiple of 4; ``offline_inference=False``.  ``IPDnet.forward`` routes
here by itself only at hidden 256 (``supported()``); at hidden 128 the train-mode forward is the opt-in
``IPDnet.forward_train`` (``MyModel(..., train_on_device=True)`` in ``IPDnet/train_step.py``), and ``forward`` keeps
raising the forward-only error ("... call .eval() first") — as it does for bf16 modules, ``offline_inference=True`` and
``forward_stream``.

``IPDnetTrainGraph`` runs, over the C-ABI kernels only (no ATen compute; plumbing copies and the weight packing aside):

    forward   full 1 (reserve) -> dropout site 0 -> narrow 1 [D0 | x] -> site 1 -> full 2 [D1 | x] -> site 2
              -> narrow 2 [D2 | x] -> site 3 -> conv head [D3 | x] with saves (conv 1 / 2 post-ReLU outputs, their
              pooled outputs, conv 3's tanh output)
    backward  conv head backward (fnssl_conv3x3_act_pool_backward, fnssl_conv3x3_causal_backward_data into D3's 256
              channels, fnssl_conv3x3_weight_grads) -> site 3 -> narrow-2 BPTT (c0g = 256) -> site 2 -> full-2 BPTT
              (c0g = 256) -> site 1 -> narrow-1 BPTT (c0g = 256) -> site 0 -> full-1 BPTT (c0g = 0), with
              fnssl_lstm_weight_grads per layer (256 = hidden_size; 128 at the default width).  No residual sums: the skips are concatenations, whose x part gets
              no gradient.

Dropout (p = 0.2, every FNblock of the reference): sites 0-3 are block_1.dropout_full, block_1.dropout_narr,
block_2.dropout_full, block_2.dropout_narr.  nn.Dropout's Bernoulli stream cannot be reproduced outside torch's RNG; the
keep mask of site s is the library's keep-scale hash (``fnssl_train_combine``, restated as
``oracle.train_ref.dropout_scale``) with seed ``train.layer_seed(base, s)`` over the LOGICAL [nb, nt, nf, hidden_size]
activation, element index ((u * nt + t) * nf + f) * hidden_size + c with u the GLOBAL utterance index.  ``base`` follows
``FN_SSL``'s rules (``fnssl.autograd``): ``module.dropout_seed`` (default ``torch.initial_seed()``) and
``module.dropout_calls`` (incremented per train-mode forward), or ``module.force_dropout_base`` pinned.  The first
utterance of the call is global utterance ``module.utt_offset`` (default rank * nb under an initialised process group,
else 0), so that N ranks draw the masks of one process on the concatenated batch.

The gradient w.r.t. the input features is not produced (block 1's full-band layer has no input-gradient path,
c0g = 0): ``backward`` returns ``None`` for it and ``in_batch.grad`` stays ``None``.  Parameter gradients are
ACCUMULATED into ``.grad`` under the reference's state_dict names.  The weight streams are packed from the current
parameters and cached on their versions, so the forward after ``optimizer.step()`` (train or eval) sees the new weights.
"""
from __future__ import annotations

import torch

from . import autograd, ops, train

SITES = ("block_1.dropout_full", "block_1.dropout_narr", "block_2.dropout_full", "block_2.dropout_narr")
CH = 256                     # FN-block output channels at hidden_size 256, the width ``IPDnet.forward`` routes by itself
WIDTHS = (128, 256)          # hidden sizes with training kernels: full-band BiLSTM H = 64 / 128


def _param_key(module):
    return tuple((p.data_ptr(), p._version, str(p.device)) for p in module.parameters())


def trainable(model, offline_inference=False) -> bool:
    """Whether the HIP training path (``IPDnet.forward_train``) takes this module and call."""
    if offline_inference or next(model.parameters()).dtype != torch.float32:
        return False
    nc, cout = model.input_size, model.cnn_out_dim
    blocks = (model.block_1, model.block_2)
    return (model.hidden_size in WIDTHS and 4 <= nc <= 16 and nc % 4 == 0 and cout > 0 and cout % 4 == 0 and
            model.conv.cnn_hidden_dim == 128 and all(abs(float(b.dropout) - 0.2) < 1e-12 for b in blocks))


def supported(model, offline_inference=False) -> bool:
    """Whether ``IPDnet.forward`` in train mode routes to the HIP training path by itself: the trainable modules of
    hidden_size 256.  (The default width trains through ``IPDnet.forward_train``: its ``forward`` keeps the
    forward-only error in train mode.)"""
    return model.hidden_size == CH and trainable(model, offline_inference)


def dropout_sites(model):
    """The four dropout modules of the train graph, in site order."""
    return [model.block_1.dropout_full, model.block_1.dropout_narr, model.block_2.dropout_full, model.block_2.dropout_narr]


def site_seeds(base: int):
    return [train.layer_seed(base, s) for s in range(len(SITES))]


class _Lstm:
    """One LSTM of the graph: natural layout ("full": stored [b, t, f, C]; "narrow": [b, f, t, C]), operand widths."""

    def __init__(self, name, mode, module, c0, c2, c0g):
        self.name, self.mode, self.module, self.c0, self.c2, self.c0g = name, mode, module, c0, c2, c0g
        self.hidden, self.ndir = module.hidden_size, 2 if module.bidirectional else 1
        self.sfx = [""] + (["_reverse"] if self.ndir == 2 else [])

    def natural(self, nb, nt, nf, c, dev):
        if self.mode == "full":
            return torch.empty((nb, nt, nf, c), dtype=torch.float32, device=dev)
        return torch.empty((nb, nf, nt, c), dtype=torch.float32, device=dev).permute(0, 2, 1, 3)

    def rows(self, t):
        """[rows = seq * step, C] matrix of a logical [b, t, f, C] tensor stored in the natural layout (a view)."""
        st = t if self.mode == "full" else t.permute(0, 2, 1, 3)
        return st.view(-1, st.shape[-1])

    def params(self, what):
        return [getattr(self.module, "%s_l0%s" % (what, s)) for s in self.sfx]


class IPDnetTrainGraph:
    """Train-mode forward and backward of IPDnet (FixedAarryIPDnet.py:29-40, 61-73, 91-120) over the C-ABI kernels."""

    def __init__(self, model):
        self.model = model
        nc = model.input_size
        b1, b2 = model.block_1, model.block_2
        self.nc, self.cout = nc, model.cnn_out_dim
        ch = self.ch = model.hidden_size                            # FN-block output channels
        self.lf1 = _Lstm("block_1.fullLstm", "full", b1.fullLstm, nc, 0, 0)
        self.ln1 = _Lstm("block_1.narrLstm", "narrow", b1.narrLstm, ch, nc, ch)
        self.lf2 = _Lstm("block_2.fullLstm", "full", b2.fullLstm, ch, nc, ch)
        self.ln2 = _Lstm("block_2.narrLstm", "narrow", b2.narrLstm, ch, nc, ch)
        self.lstms = (self.lf1, self.ln1, self.lf2, self.ln2)
        self._packed, self._packed_key = None, None

    def streams(self, dev):
        """Forward / backward LSTM weight streams and the conv streams, re-packed when a parameter changed."""
        key = (_param_key(self.model), str(dev))
        if self._packed is None or self._packed_key != key:
            fw, bw = {}, {}
            for L in self.lstms:
                fw[L.name], bw[L.name] = [], []
                for s in L.sfx:
                    g = lambda n: getattr(L.module, "%s_l0%s" % (n, s)).detach().float()   # noqa: E731
                    fw[L.name].append(ops.pack_lstm(g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh"), L.c0,
                                                    L.c2, dev))
                    bw[L.name].append(torch.from_numpy(ops.pack_lstm_bwd_host(g("weight_ih"), g("weight_hh"),
                                                                              L.c0g)).to(dev))
            cv = self.model.conv
            conv_fw = (ops.pack_conv3x3(cv.conv1.weight, self.ch, self.nc, dev), ops.pack_conv3x3(cv.conv2.weight, 128, 0, dev),
                       ops.pack_conv3x3(cv.conv3.weight, 128, 0, dev))
            conv_bw = (ops.pack_conv3x3_backward_data(cv.conv1.weight, self.ch, dev),
                       ops.pack_conv3x3_backward_data(cv.conv2.weight, 128, dev),
                       ops.pack_conv3x3_backward_data(cv.conv3.weight, 128, dev))
            self._packed, self._packed_key = (fw, bw, conv_fw, conv_bw), key
        return self._packed

    def forward(self, x, seeds, b0):
        """x [nb, nc, nf, nt] -> (conv 3 output [nb, nf, nt // 12, cout], saved activations for ``backward``)."""
        nb, nc, nf, nt = x.shape
        dev = x.device
        CH = self.ch
        fw, _, cfw, _ = self.streams(dev)
        lf1, ln1, lf2, ln2 = self.lstms
        XF = ops.nchw_to_seq(x)                                        # [b, t, f, nc]
        XN = XF.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)    # same numbers, stored [b, f, t, nc]
        res, D = {}, []

        def lstm(L, src0, src2, masked_out, seed):
            out = L.natural(nb, nt, nf, L.ndir * L.hidden, dev)
            nseq, nsteps = (nb * nt, nf) if L.mode == "full" else (nb * nf, nt)
            res[L.name] = torch.empty((ops.lstm_reserve_floats(nseq, L.hidden, L.ndir, nsteps),), dtype=torch.float32,
                                      device=dev)
            ops.lstm_layer(L.mode, src0, None, src2, fw[L.name], L.hidden, out, reserve=res[L.name])
            train.combine(masked_out, masked=(out,), seed32=seed, b0=b0)          # nn.Dropout (keep-scale hash)
            return out

        D0 = ln1.natural(nb, nt, nf, CH, dev)
        F1 = lstm(lf1, XF, None, D0, seeds[0])                         # full 1 (:31-33), dropout_full
        D1 = lf2.natural(nb, nt, nf, CH, dev)
        N1 = lstm(ln1, D0, XN, D1, seeds[1])                           # narrow 1 on [D0 | x] (:34-37), dropout_narr
        D2 = ln2.natural(nb, nt, nf, CH, dev)
        F2 = lstm(lf2, D1, XF, D2, seeds[2])                           # full 2 on [D1 | x] (cat :38 of block 1)
        D3 = ln2.natural(nb, nt, nf, CH, dev)
        N2 = lstm(ln2, D2, XN, D3, seeds[3])                           # narrow 2 on [D2 | x], dropout_narr
        # conv head on [D3 | x] (:61-73), channels-last [nb, nf, nt, C] views
        xa, xb = D3.permute(0, 2, 1, 3), XN.permute(0, 2, 1, 3)
        Y1 = ops.conv3x3_causal(xa, xb, cfw[0], 128, "relu")
        P1 = ops.avgpool_time(Y1, 3)
        Y2 = ops.conv3x3_causal(P1, None, cfw[1], 128, "relu")
        P2 = ops.avgpool_time(Y2, 4)
        Y3 = ops.conv3x3_causal(P2, None, cfw[2], self.cout, "tanh")
        saved = {"XF": XF, "XN": XN, "res": res, "F1": F1, "N1": N1, "F2": F2, "N2": N2, "D": (D0, D1, D2, D3),
                 "Y1": Y1, "P1": P1, "Y2": Y2, "P2": P2, "Y3": Y3, "shape": (nb, nf, nt)}
        return Y3, saved

    def backward(self, saved, dY3, seeds, b0, grads):
        """Accumulate every parameter gradient given dL/dY3 ([nb, nf, nt // 12, cout]); ``grads``: name -> tensor."""
        nb, nf, nt = saved["shape"]
        dev = dY3.device
        CH = self.ch
        _, bw, _, cbw = self.streams(dev)
        lf1, ln1, lf2, ln2 = self.lstms
        XF, XN, res = saved["XF"], saved["XN"], saved["res"]
        D0, D1, D2, D3 = saved["D"]
        # ---- conv head (new HIP: act / pool backward, anti-causal dgrad, split-K wgrad) ----------------------------
        dZ3 = ops.conv3x3_act_pool_backward(dY3, saved["Y3"], 1, "tanh")
        ops.conv3x3_weight_grads(dZ3, saved["P2"], None, grads["conv.conv3.weight"])
        dP2 = ops.conv3x3_causal_backward_data(dZ3, cbw[2], 128)
        dZ2 = ops.conv3x3_act_pool_backward(dP2, saved["Y2"], 4, "relu")
        ops.conv3x3_weight_grads(dZ2, saved["P1"], None, grads["conv.conv2.weight"])
        dP1 = ops.conv3x3_causal_backward_data(dZ2, cbw[1], 128)
        dZ1 = ops.conv3x3_act_pool_backward(dP1, saved["Y1"], 3, "relu")
        ops.conv3x3_weight_grads(dZ1, D3.permute(0, 2, 1, 3), XN.permute(0, 2, 1, 3), grads["conv.conv1.weight"])
        dY = ops.conv3x3_causal_backward_data(dZ1, cbw[0], CH)          # [nb, nf, nt, CH] = dL/dD3, narrow storage
        del dZ1, dP1, dZ2, dP2, dZ3

        def weight_grads(L, dA, x0, x2, h):
            g = lambda n: [grads["%s.%s_l0%s" % (L.name, n, s)] for s in L.sfx]   # noqa: E731
            nsteps = nf if L.mode == "full" else nt
            ops.lstm_weight_grads(L.rows(dA), L.rows(x0) if x0 is not None else None,
                                  L.rows(x2) if x2 is not None else None, L.rows(h), L.hidden, L.ndir, nsteps,
                                  g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh"))

        def bptt(L, dh, x0, x2, h):
            dA = L.natural(nb, nt, nf, L.ndir * 4 * L.hidden, dev)
            dx = L.natural(nb, nt, nf, L.ndir * L.c0g, dev) if L.c0g else None
            ops.lstm_backward(L.mode, res[L.name], dh, dA, dx, bw[L.name], L.hidden, L.c0g)
            weight_grads(L, dA, x0, x2, h)
            return tuple(dx[..., d * L.c0g:(d + 1) * L.c0g] for d in range(L.ndir)) if dx is not None else ()

        DN2 = ln2.natural(nb, nt, nf, CH, dev)
        train.combine(DN2, masked=(dY.permute(0, 2, 1, 3),), seed32=seeds[3], b0=b0)       # site 3 backward
        del dY
        dv = bptt(ln2, DN2, D2, XN, saved["N2"])                                          # narrow 2, c0g = CH
        DF2 = lf2.natural(nb, nt, nf, CH, dev)
        train.combine(DF2, masked=dv, seed32=seeds[2], b0=b0)                             # site 2 backward
        du = bptt(lf2, DF2, D1, XF, saved["F2"])                                          # full 2, c0g = CH
        DN1 = ln1.natural(nb, nt, nf, CH, dev)
        train.combine(DN1, masked=du, seed32=seeds[1], b0=b0)                             # site 1 backward
        dv = bptt(ln1, DN1, D0, XN, saved["N1"])                                          # narrow 1, c0g = CH
        DF1 = lf1.natural(nb, nt, nf, CH, dev)
        train.combine(DF1, masked=dv, seed32=seeds[0], b0=b0)                             # site 0 backward
        bptt(lf1, DF1, XF, None, saved["F1"])                                             # full 1, c0g = 0


class IPDnetTrainFunction(torch.autograd.Function):
    """Y3 = conv head output of IPDnet(x) in train mode; backward accumulates every parameter gradient."""

    @staticmethod
    def forward(ctx, x, graph, seeds, b0, names, *params):
        with torch.cuda.device(x.device):
            y3, saved = graph.forward(x.detach().float().contiguous(), seeds, b0)
            # act_pool_backward needs tanh's output: keep an alias (another tensor object), not the returned tensor
            # itself (which would close the cycle output -> grad_fn -> ctx -> output)
            saved["Y3"] = y3.detach()
        ctx.graph, ctx.saved, ctx.seeds, ctx.b0, ctx.names = graph, saved, seeds, b0, names
        ctx.set_materialize_grads(False)
        return y3

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy3):
        names = ctx.names
        if ctx.saved is None:
            raise RuntimeError("fnssl.ipdnet_train: backward through the same forward twice (the saved activations were "
                               "released; call forward again)")
        if dy3 is None:
            return (None,) * (5 + len(names))
        shapes = {n: p.shape for n, p in ctx.graph.model.named_parameters()}
        with torch.cuda.device(dy3.device):
            grads = {n: torch.zeros(shapes[n], dtype=torch.float32, device=dy3.device) for n in names}
            ctx.graph.backward(ctx.saved, dy3.float().contiguous(), ctx.seeds, ctx.b0, grads)
        ctx.saved = None
        return (None, None, None, None, None) + tuple(grads[n] if ctx.needs_input_grad[5 + i] else None
                                                      for i, n in enumerate(names))


def train_forward(model, x):
    """``IPDnet.forward`` / ``IPDnet.forward_train`` in train mode (trainable configurations): x [nb, nc, nf, nt] ->
    [nb, nt // 12, 2 nf, nc / 2 - 1, max_track] with a ``grad_fn``."""
    ops._need_dev(x)
    if x.ndim != 4 or x.shape[1] != model.input_size or x.shape[3] < ops.SEG_FRAMES:
        raise RuntimeError("IPDnet.forward (train mode): expected [nb, %d, nf, nt >= 12], got %s"
                           % (model.input_size, tuple(x.shape)))
    graph = getattr(model, "_train_graph", None)
    if graph is None:
        graph = model._train_graph = IPDnetTrainGraph(model)
    base = autograd._next_base(model)
    seeds = site_seeds(base)
    nb, _, nf, nt = x.shape
    b0 = getattr(model, "utt_offset", None)
    b0 = autograd._rank_offset(nb) if b0 is None else int(b0)
    model.last_dropout_base = base
    named = list(model.named_parameters())
    names = tuple(n for n, _ in named)
    y3 = IPDnetTrainFunction.apply(x, graph, seeds, b0, names, *[p for _, p in named])
    nt2 = nt // 12
    c = y3.permute(0, 2, 1, 3)                                          # = conv(x).permute(0,3,2,1)  (:113)
    c = c.reshape(nb, nt2, nf, 2, -1).permute(0, 1, 3, 2, 4)
    return c.reshape(nb, nt2, 2, nf * 2, -1).permute(0, 1, 3, 4, 2)
