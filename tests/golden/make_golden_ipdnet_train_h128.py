#!/usr/bin/env python3
"""Golden vectors for IPDnet training at the reference's default width, hidden_size = 128 (G22): the recipe of
make_golden_ipdnet_train.py (G18) on the REAL reference (IPDnet/FixedAarryIPDnet.py IPDnet in train() mode, autograd
backward, torch.optim.Adam(lr=5e-4) as in runIPDnetOn.py / runIPDnetOff.py), with full-band BiLSTMs of H = 64 and
narrow-band layers of H = 128 (online) or 2 x 64 (offline).  The same two substitutions: each nn.Dropout's forward is a
multiplication with the deterministic keep-scale tensor the HIP path draws (oracle.train_ref.dropout_scale over the
logical [nb, nt, nf, 128] activation, seed fnssl.train.layer_seed(base, site)), and the loss is the reference's cal_loss
with the permutation-invariant MSE restated (tests/ipdnet_train_ref.pit_mse).

Data only: per case the input, target, prediction, loss, and per parameter tensor (state_dict order) the gradient's L2
norm and first 16 entries, and the first 16 entries of the Adam-updated parameter.

usage: make_golden_ipdnet_train_h128.py <the reference checkout's IPDnet directory>"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "fn-ssl_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "FixedAarryIPDnet.py")):
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])
sys.modules.setdefault("soundfile", types.ModuleType("soundfile"))
sys.modules.setdefault("webrtcvad", types.ModuleType("webrtcvad"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import FixedAarryIPDnet as ref  # noqa: E402  (reference)
from fnssl import weights as W  # noqa: E402
from ipdnet_train_ref import pit_mse, site_masks  # noqa: E402

torch.set_num_threads(8)

HIDDEN = 128
# case: (input_size, online, nb, nf, nt, weight seed, dropout base)
CASES = {"a": (4, True, 2, 24, 36, 2700, 5151), "b": (4, False, 2, 20, 24, 2710, 5252),
         "c": (8, True, 2, 16, 36, 2720, 5353)}


def rs_randn(seed, shape, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(size=shape) * scale).astype(np.float32)


def main():
    arrs = {}
    for case, (nc, online, nb, nf, nt, wseed, base) in sorted(CASES.items()):
        sd = W.make_ipdnet_state(wseed, nc, HIDDEN, 2, online)
        net = ref.IPDnet(nc, HIDDEN, 2, online)
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
        net.train()
        masks = site_masks(base, nb, nt, nf, 0, c=HIDDEN)
        blocks = (net.block_1, net.block_2)
        for k, blk in enumerate(blocks):
            mf = masks[2 * k].reshape(nb * nt, nf, -1)
            mn = masks[2 * k + 1].permute(0, 2, 1, 3).reshape(nb * nf, nt, -1)
            blk.dropout_full.forward = (lambda x, m=mf: x * m)
            blk.dropout_narr.forward = (lambda x, m=mn: x * m)
        x = rs_randn(wseed + 1, (nb, nc, nf, nt))
        gt = rs_randn(wseed + 2, (nb, nt // 12, 2 * nf, nc // 2 - 1, 2), 0.5)
        pred = net(torch.from_numpy(x))
        loss = pit_mse(pred, torch.from_numpy(gt))
        loss.backward()
        named = list(net.named_parameters())
        gnorm = np.array([float(p.grad.double().norm()) for _, p in named])
        ghead = np.stack([np.pad(p.grad.reshape(-1)[:16].numpy(), (0, max(0, 16 - p.numel()))) for _, p in named])
        torch.optim.Adam(net.parameters(), lr=5e-4).step()
        phead = np.stack([np.pad(p.detach().reshape(-1)[:16].numpy(), (0, max(0, 16 - p.numel()))) for _, p in named])
        arrs.update({case + "_cfg": np.array([nc, int(online), nb, nf, nt]), case + "_wseed": np.array(wseed),
                     case + "_base": np.array(base), case + "_x": x, case + "_gt": gt,
                     case + "_pred": pred.detach().numpy(), case + "_loss": np.array(loss.item()),
                     case + "_gnorm": gnorm, case + "_ghead": ghead.astype(np.float32),
                     case + "_phead": phead.astype(np.float32)})
        print(case, "loss %.6f" % loss.item(), "pred", tuple(pred.shape))
    np.savez_compressed(os.path.join(HERE, "g22_ipdnet_train_h128.npz"), **arrs)


if __name__ == "__main__":
    main()
