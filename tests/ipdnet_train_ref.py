"""CPU restatement of IPDnet's training forward (IPDnet/FixedAarryIPDnet.py:29-40, 61-73, 91-120) with PyTorch autograd,
for the GPU tests of fnssl/ipdnet_train.py: nn.LSTM / nn.Conv2d under the reference's parameter names, the four dropouts
as explicit keep-scale tensors (oracle.train_ref.dropout_scale), and the PIT-MSE loss of the reference's ``cal_loss``
(for every (utterance, frame) row, the track permutation with the lower MSE, ties to the identity)."""
import itertools

import numpy as np
import torch
import torch.nn as nn

from fnssl import train
from oracle import train_ref


class RefFNblock(nn.Module):
    def __init__(self, input_size, hidden_size, add_skip_dim, is_online, is_first):
        super().__init__()
        fh = hidden_size // 2
        nh = hidden_size if is_online else hidden_size // 2
        self.fullLstm = nn.LSTM(input_size if is_first else input_size + add_skip_dim, fh, batch_first=True,
                                bidirectional=True)
        self.narrLstm = nn.LSTM(2 * fh + add_skip_dim, nh, batch_first=True, bidirectional=not is_online)

    def forward(self, x, fb_skip, nb_skip, m_full, m_narr):
        nb, nt, nf, _ = x.shape
        x, _ = self.fullLstm(x.reshape(nb * nt, nf, -1))
        if m_full is not None:                     # None: eval mode (no dropout)
            x = x * m_full.reshape(nb * nt, nf, -1)
        x = torch.cat((x, fb_skip), dim=-1)
        x = x.view(nb, nt, nf, -1).permute(0, 2, 1, 3).reshape(nb * nf, nt, -1)
        x, _ = self.narrLstm(x)
        x = x.view(nb, nf, nt, -1).permute(0, 2, 1, 3)
        if m_narr is not None:
            x = x * m_narr
        return torch.cat((x, nb_skip.view(nb, nf, nt, -1).permute(0, 2, 1, 3)), dim=-1)


class RefConv(nn.Module):
    def __init__(self, inp, out, hid=128):
        super().__init__()
        self.conv1 = nn.Conv2d(inp, hid, 3, padding=(1, 2), bias=False)
        self.conv2 = nn.Conv2d(hid, hid, 3, padding=(1, 2), bias=False)
        self.conv3 = nn.Conv2d(hid, out, 3, padding=(1, 2), bias=False)

    def forward(self, x, relu_masks=None):
        """``relu_masks`` (optional, bool [nb, hid, nf, nt'] per ReLU): the branch each ReLU takes instead of the sign
        of its own input, so that a float64 run can follow an fp32 run where a pre-activation lies within rounding of 0.
        ``self.mask_flips`` then lists per ReLU (positions where the mask differs from the sign, the largest |input|
        there relative to the largest |input|)."""
        m = relu_masks if relu_masks is not None else (None, None)
        self.mask_flips = []
        y = self._relu(self.conv1(x)[..., :-2], m[0])
        y = nn.functional.avg_pool2d(y, (1, 3))
        y = self._relu(self.conv2(y)[..., :-2], m[1])
        y = nn.functional.avg_pool2d(y, (1, 4))
        return torch.tanh(self.conv3(y)[..., :-2])

    def _relu(self, z, mask):
        if mask is None:
            return torch.relu(z)
        a = z.detach().abs()
        flip = (z.detach() > 0) != mask
        self.mask_flips.append((int(flip.sum()), float(a[flip].max() / a.max()) if flip.any() else 0.0))
        return z * mask


class RefIPDnet(nn.Module):
    def __init__(self, input_size, hidden_size, max_track, is_online):
        super().__init__()
        self.block_1 = RefFNblock(input_size, hidden_size, input_size, is_online, True)
        self.block_2 = RefFNblock(hidden_size, hidden_size, input_size, is_online, False)
        self.conv = RefConv(hidden_size + input_size, 2 * (input_size // 2 - 1) * max_track)

    def forward(self, x, masks, relu_masks=None):
        x = x.permute(0, 3, 2, 1)
        nb, nt, nf, nc = x.shape
        fb = x.reshape(nb * nt, nf, nc)
        nbs = x.permute(0, 2, 1, 3).reshape(nb * nf, nt, nc)
        x = self.block_1(x, fb, nbs, masks[0], masks[1])
        x = self.block_2(x, fb, nbs, masks[2], masks[3])
        nt2 = nt // 12
        x = self.conv(x.permute(0, 3, 2, 1), relu_masks).permute(0, 3, 2, 1)
        x = x.reshape(nb, nt2, nf, 2, -1).permute(0, 1, 3, 2, 4)
        return x.reshape(nb, nt2, 2, nf * 2, -1).permute(0, 1, 3, 4, 2)


def site_masks(base, nb, nt, nf, b0=0, c=256):
    """Keep-scale tensors of the four dropout sites, logical [nb, nt, nf, 256]."""
    return [torch.from_numpy(train_ref.dropout_scale(train.layer_seed(base, s), (nb, nt, nf, c), b0)) for s in range(4)]


def pit_mse(pred, gt):
    """The reference's cal_loss: pred / gt [nb, nt2, 2nf, nmic - 1, nsrc]; per row the best track permutation."""
    nb, nt, _, _, ns = pred.shape
    p = pred.reshape(nb * nt, -1, ns).permute(0, 2, 1)
    g = gt.reshape(nb * nt, -1, ns).permute(0, 2, 1)
    perms = list(itertools.permutations(range(ns)))
    errs = torch.stack([((p[:, list(pm)] - g) ** 2).mean(dim=(1, 2)) for pm in perms], dim=1)
    best = errs.detach().argmin(dim=1)             # argmin returns the first minimum: ties go to the identity
    idx = torch.tensor(perms, device=pred.device)[best]
    p = torch.gather(p, 1, idx.unsqueeze(-1).expand(-1, -1, p.shape[2]))
    return nn.functional.mse_loss(p.contiguous(), g.contiguous())


def state_tensors(sd):
    return {k: torch.from_numpy(np.array(v, dtype=np.float32)) for k, v in sd.items()}
