#!/usr/bin/env python3
"""G19: one batch through the data half of IPDnet's training step, from the REAL reference (build container only:
needs /root/reference and scipy).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ipdnet_step.py

Imports the reference's own ``IPDnet/Module.py`` (``STFT``, ``DPIPD``), ``utils_.forgetting_norm`` and
``scipy.special.jn`` and applies the lines of ``cal_vad`` (IPDnet/runIPDnetOn.py:224-235),
``euclidean_distances_to_bessel`` (:209-221) and ``data_preprocess`` (:237-290) with the calls the reference makes, in
its order (runIPDnetOn.py itself cannot be imported: pytorch_lightning and torchmetrics are absent and it opens datasets
at import).  The inputs come from seeds (tests/ipdnet_step_ref.g19_batch), only the results are stored.  Only data is
written.  The script asserts that the fixture is well-posed: the fp32 ``dp_vad`` agrees with a float64 evaluation to
1e-5 relative and no slot lies in (0, 0.002), so the 0.001 threshold is never decided by rounding.
"""
import os
import sys
import types
from copy import deepcopy

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference/IPDnet")
sys.modules.setdefault("soundfile", types.ModuleType("soundfile"))
sys.modules.setdefault("webrtcvad", types.ModuleType("webrtcvad"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy.special import jn  # noqa: E402

import Module as at_module  # noqa: E402  (reference)
from utils_ import forgetting_norm  # noqa: E402  (reference)

import ipdnet_step_ref as R  # noqa: E402

FRE_RANGE_USED = range(1, 257, 1)                                  # runIPDnetOn.py:127
MAX_SOURCE = 2


def euclidean_distances_to_bessel(data, fre_use, order=0):         # :209-221
    reference = data[0, :]
    distances = np.sqrt(np.sum((data[1:] - reference) ** 2, axis=1))
    frequencies = 2 * np.pi * np.linspace(0, 8000, 257) / 340
    frequencies = frequencies[fre_use]
    bessel_values_extended = []
    for distance in distances:
        bessel_value = jn(order, frequencies * distance)
        zero_vector = np.zeros(256)
        extended_value = np.concatenate((bessel_value, zero_vector))
        bessel_values_extended.append(extended_value)
    return np.array(bessel_values_extended).T


def cal_vad(dostft, dp_mic_sig_batch, stft, dtype=None):           # :224-235 (dtype: the float64 cross-check only)
    nb, nf, nt, nc = stft.shape
    dp_vad = torch.zeros(nb, nt, MAX_SOURCE, dtype=dtype or torch.float32)
    for source_idx in range(MAX_SOURCE):
        dp_temp = dostft(signal=dp_mic_sig_batch[:, :, :, source_idx])
        dp_temp_mag = torch.abs(dp_temp)
        if dtype is not None:
            dp_temp_mag, stft = dp_temp_mag.to(dtype), stft.to(torch.complex128)
        vad_temp = dp_temp_mag[:, :, :, 0] / torch.abs(stft[:, :, :, 0])
        vad_temp = torch.mean(vad_temp, dim=1)
        dp_vad[:, :, source_idx] = vad_temp
    pooling = torch.nn.AvgPool2d(kernel_size=(12, 1))
    return pooling(dp_vad)


def main():
    mic_np, dp_np, doa_np, mic_pos = R.g19_batch()
    mic_sig_batch, dp_signal, doa = torch.from_numpy(mic_np), torch.from_numpy(dp_np), torch.from_numpy(doa_np)
    dostft = at_module.STFT(win_len=512, win_shift_ratio=0.5, nfft=512)
    gerdpipd = at_module.DPIPD(ndoa_candidate=[1, 180], mic_location=mic_pos, nf=257, fre_max=8000.0, ch_mode='M', speed=340)
    eps = 1e-6
    # ---- data_preprocess, :237-290 ----
    stft = dostft(signal=mic_sig_batch)
    nb, nf, nt, nc = stft.shape
    dp_vad = cal_vad(dostft, dp_signal, stft)
    stft_rebatch = stft.permute(0, 3, 1, 2)
    mag = torch.abs(stft_rebatch)
    mean_value = forgetting_norm(mag, sample_length=280)
    stft_rebatch_real = torch.real(stft_rebatch) / (mean_value + eps)
    stft_rebatch_image = torch.imag(stft_rebatch) / (mean_value + eps)
    real_image_batch = torch.cat((stft_rebatch_real, stft_rebatch_image), dim=1)
    features = real_image_batch[:, :, FRE_RANGE_USED, :]
    source_doa = doa.cpu().numpy()
    _, ipd_batch = gerdpipd(source_doa=source_doa)
    non_source_tar = euclidean_distances_to_bessel(mic_pos, fre_use=FRE_RANGE_USED)
    non_source_np = non_source_tar
    non_source_tar = torch.from_numpy(non_source_tar)
    ipd_batch = np.concatenate((ipd_batch.real[:, :, FRE_RANGE_USED, :, :], ipd_batch.imag[:, :, FRE_RANGE_USED, :, :]),
                               axis=2).astype(np.float32)
    ipd_batch = torch.from_numpy(ipd_batch)
    nb, nt2, nf2, nmic, nsrc = ipd_batch.shape
    vad_batch_copy = deepcopy(dp_vad)
    th = 0.001
    vad_batch_copy[vad_batch_copy <= th] = 0
    vad_batch_copy[vad_batch_copy > th] = 1
    vad_batch_expand_ipd = vad_batch_copy[:, :, np.newaxis, np.newaxis, :].expand(nb, nt2, nf2, nmic, nsrc)
    ipd_batch = ipd_batch * vad_batch_expand_ipd
    for i in range(nb):
        for j in range(nt2):
            for k in range(nsrc):
                if (ipd_batch[i, j, :, :, k] == 0).all():
                    ipd_batch[i, j, :, :, k] = non_source_tar.to(ipd_batch)
    # ---- the fixture is well-posed ----
    v32 = dp_vad.numpy()
    v64 = cal_vad(dostft, dp_signal, stft, dtype=torch.float64).numpy()
    rel = np.abs(v32 - v64) / np.maximum(np.abs(v64), 1e-30)
    rel[v64 == 0] = np.abs(v32[v64 == 0])
    assert rel.max() <= 1e-5, rel.max()
    assert not ((v32 > 0) & (v32 < 0.002)).any(), v32
    assert (v32[0, :, 1] == 0).all() and (v32[1, 1:, 0] == 0).all() and (v32 == 0).sum() == 5, v32
    # the closed form the kernel implements (tests/ipdnet_step_ref.ipdnet_targets) against the reference's own output
    closed = R.ipdnet_targets(doa_np, v32, mic_pos, non_source_np.astype(np.float32))
    print("closed form vs reference targets: max abs diff %.3g" % np.abs(closed - ipd_batch.numpy()).max())
    print("numpy J0 vs scipy: max abs diff %.3g" % np.abs(R.non_source_target(mic_pos).astype(np.float64) - non_source_np).max())
    print("dp_vad fp32 vs float64: %.3g relative; active slots %.3g .. %.3g" % (rel.max(), v32[v32 > 0].min(), v32.max()))
    arrs = {"mic_pos": mic_pos, "doa": doa_np, "features": features.numpy().astype(np.float32), "dp_vad": v32,
            "ipd": ipd_batch.numpy().astype(np.float32), "non_source": non_source_np,
            "shape": np.array(R.G19_SHAPE)}
    out = os.path.join(HERE, "g19_ipdnet_step.npz")
    np.savez_compressed(out, **arrs)
    print("wrote", out, os.path.getsize(out), "bytes", {k: v.shape for k, v in arrs.items()})


if __name__ == "__main__":
    main()
