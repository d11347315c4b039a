"""Drop-in for the evaluation half of the reference's ``IPDnet/Module.py``: ``getMetric`` (:70-278) and ``PredDOA``
(:423-600) over the HIP path.  The template search of all tracks is one launch (``fnssl_ipd2doa_tracks``), the metrics
one kernel pair (``fnssl_doa_metrics``); predictions, DOAs, VADs and metrics stay on the device.

Not reproduced: ``max_num_sources`` other than 1 and ``time_pool_size`` (both raise), the ``np.save`` files that
``evaluate`` writes under ``./results/`` when ``idx`` is given (``idx`` is accepted and ignored), and the reference's
reading of the IPD tensor as the VAD when the module was built with ``tar_useVAD=False`` (``gt_batch[-1]``): that raises.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from fnssl import doa as fdoa                                        # noqa: E402
from fnssl import metrics as fmetrics                                # noqa: E402


class getMetric(nn.Module):
    """Reference getMetric (:70-278): ``forward`` returns the LIST [ACC, MAE] ('single') or [ACC, MD, FA, MAE, RMSE]
    ('multiple') of device tensors, unfolded into one-element tensors with ``metric_unfold``.  Of several ``ae_mode``
    entries the reference's if / elif chain evaluates ONE (ele, else azi, else aziele) and 'multiple' repeats it
    ``len(ae_mode)`` times; so does this.  ``last_counts``: the per-utterance K_gt, K_est, K_corr of the last call."""

    def __init__(self, source_mode='multiple', metric_unfold=True, large_number=10000, invalid_source_idx=10):
        super(getMetric, self).__init__()
        if source_mode not in ('single', 'multiple'):
            raise ValueError("source_mode must be 'single' or 'multiple'")
        if 0 <= int(invalid_source_idx) < fmetrics.MAX_SOURCES:
            raise ValueError("invalid_source_idx %r would collide with a source index (0..%d)"
                             % (invalid_source_idx, fmetrics.MAX_SOURCES - 1))
        self.source_mode = source_mode
        self.metric_unfold = metric_unfold
        self.inf = large_number
        self.invlid_sidx = invalid_source_idx
        self.last_counts = None

    def forward(self, doa_gt, vad_gt, doa_est, vad_est, ae_mode, ae_TH=30, useVAD=True, vad_TH=[0.5, 0.5], radians=False):
        """doa_gt, doa_est [nb, nt, 2, ns] in degrees (``radians=True``: radians, converted by the kernel as
        ``PredDOA.evaluate`` does), vad_gt, vad_est [nb, nt, ns]."""
        mode = next((m for m in ('ele', 'azi', 'aziele') if m in ae_mode), None)
        if mode is None:
            raise Exception('Angle error mode unrecognized')
        f = lambda t: None if t is None else t.float()                           # noqa: E731
        m, k_gt, k_est, k_corr = fmetrics.doa_metrics(f(doa_gt), f(vad_gt), f(doa_est), f(vad_est), self.source_mode, [mode],
                                                      ae_TH, useVAD, vad_TH, radians, self.inf, 1e-5)
        self.last_counts = {'K_gt': k_gt, 'K_est': k_est, 'K_corr': k_corr}
        s = fmetrics.AE_SLOT[mode]
        if self.source_mode == 'single':
            metric = [m[fmetrics.SLOT_ACC], m[fmetrics.SLOT_MAE + s:fmetrics.SLOT_MAE + s + 1]]
        else:
            nmode = len(ae_mode)
            metric = [m[fmetrics.SLOT_ACC:fmetrics.SLOT_ACC + 1], m[fmetrics.SLOT_MDR:fmetrics.SLOT_MDR + 1],
                      m[fmetrics.SLOT_FAR:fmetrics.SLOT_FAR + 1],
                      m[fmetrics.SLOT_MAE + s:fmetrics.SLOT_MAE + s + 1].expand(nmode),
                      m[fmetrics.SLOT_RMSE + s:fmetrics.SLOT_RMSE + s + 1].expand(nmode)]
        if self.metric_unfold:
            metric = self.unfold_metric(metric)
        return metric

    def unfold_metric(self, metric):
        metric_unfold = []
        for m in metric:
            if m.numel() != 1:
                for n in range(m.numel()):
                    metric_unfold += [m[n]]
            else:
                metric_unfold += [m]
        return metric_unfold


class PredDOA(nn.Module):
    """Multi-track DP-IPD predictions -> DOA / VAD per track -> ACC, MDR, FAR, MAE, RMSE (reference PredDOA, :423-600).
    The template bank ([cos | sin] of bins 1..256; elevation pi/2, azimuth linspace(0, pi, res_phi); reference-microphone
    pairs; speed 340) is built once per geometry on the host."""

    def __init__(self, source_num_mode='UnkNum', max_num_sources=1, max_track=2, res_the=1, res_phi=180, fs=16000, nfft=512,
                 ch_mode='M', dev='cuda', mic_location=None, is_linear_array=True, is_planar_array=True):
        super(PredDOA, self).__init__()
        if int(max_num_sources) != 1:
            raise ValueError("PredDOA: one source per track (max_num_sources = 1, as the reference's MyModel builds it), got %r"
                             % (max_num_sources,))
        if source_num_mode not in ('KNum', 'UnkNum'):
            raise ValueError("source_num_mode must be 'KNum' or 'UnkNum'")
        if mic_location is None:
            raise ValueError("PredDOA: mic_location [nmic, 3] is required")
        self.nfft = nfft
        self.fre_max = fs / 2
        self.ch_mode = ch_mode
        self.source_num_mode = source_num_mode
        self.max_num_sources = 1
        self.fre_range_used = range(1, int(self.nfft / 2) + 1, 1)
        self.dev = dev
        self.max_track = int(max_track)
        mic = mic_location.detach().cpu().numpy() if isinstance(mic_location, torch.Tensor) else np.asarray(mic_location)
        self.mic_location = mic
        template, cand = fdoa.dpipd_templates(mic.reshape(-1, 3), res_the, res_phi, int(self.nfft / 2) + 1, self.fre_max, ch_mode, 340,
                                              search_space_ele=(np.pi / 2, np.pi / 2), search_space_azi=(0, np.pi))
        k = list(self.fre_range_used)
        bank = np.concatenate((template.real[:, :, k, :], template.imag[:, :, k, :]), axis=2).astype(np.float32)
        self.register_buffer("bank", torch.from_numpy(np.ascontiguousarray(bank)), persistent=False)      # [nele, nazi, 2nf, np]
        self.register_buffer("ele_candidate", torch.from_numpy(cand[0].astype(np.float32)), persistent=False)
        self.register_buffer("azi_candidate", torch.from_numpy(cand[1].astype(np.float32)), persistent=False)
        self.getmetric = getMetric(source_mode='multiple', metric_unfold=True)

    def forward(self, pred_batch, gt_batch, idx=None):
        doa, vad = self._localize(pred_batch)
        return self.evaluate(pred_batch=[doa, vad, None], gt_batch=gt_batch, idx=idx)

    def _localize(self, pred_batch, ntrack=None):
        """pred [nb, nt, 2nf, nmic - 1, nmax] -> (DOA [nb, nt, 2, ntrack], VAD [nb, nt, ntrack]): views of the kernel's
        track-major outputs."""
        pred = pred_batch.detach().to(self.dev)
        if pred.ndim != 5:
            raise RuntimeError("PredDOA: pred_batch must be [nb, nt, 2nf, nmic - 1, ntrack], got %s" % (tuple(pred.shape),))
        ntrack = self.max_track if ntrack is None else ntrack
        if ntrack > pred.shape[-1]:
            raise RuntimeError("PredDOA: max_track = %d but the prediction has %d tracks" % (ntrack, pred.shape[-1]))
        bank = self.bank.to(pred.device)
        idx, vad, _ = fmetrics.localize_tracks(pred.float()[..., :ntrack], bank, 1, self.source_num_mode)
        nazi = bank.shape[1]
        idx = idx[..., 0].long()                                                  # [ntrack, nb, nt]
        doa = torch.stack((self.ele_candidate.to(pred.device)[idx // nazi], self.azi_candidate.to(pred.device)[idx % nazi]), dim=3)
        return doa.permute(1, 2, 3, 0), vad[..., 0].permute(1, 2, 0)

    def pred2DOA(self, pred_batch, gt_batch):
        """:463-484 — returns ([DOA [nb, nt, 2, max_track], VAD [nb, nt, max_track], the re-batched IPD
        [nb * (nmic - 1), nt, 2nf, nmax]], gt_batch)."""
        doa, vad = self._localize(pred_batch)
        nb, nt, ndoa, nmic, nmax = pred_batch.shape
        pred_ipd = pred_batch.detach().permute(0, 3, 1, 2, 4).reshape(nb * nmic, nt, ndoa, nmax)
        return [doa, vad, pred_ipd], self._detach(gt_batch)

    def pred2DOA_track(self, pred_batch=None, gt_batch=None, time_pool_size=None):
        """One track (:487-579): pred [nb * (nmic - 1), nt, 2nf] -> [DOAs [nb, nt, 2, 1], VADs [nb, nt, 1], spatial spectrum
        [nb, nt, nele, nazi]]."""
        if time_pool_size is not None:
            raise NotImplementedError("PredDOA.pred2DOA_track: time_pool_size is not supported")
        out = None
        if pred_batch is not None:
            pred = pred_batch.detach().to(self.dev).float()
            bank = self.bank.to(pred.device)
            nb = pred.shape[0] // bank.shape[-1]
            idx, vad, ss = fdoa.localize(pred, bank, nb, 1, 'kNum' if self.source_num_mode == 'KNum' else 'unkNum')
            nazi = bank.shape[1]
            idx = idx.long()
            doa = torch.stack((self.ele_candidate.to(pred.device)[idx // nazi], self.azi_candidate.to(pred.device)[idx % nazi]), dim=2)
            out = [doa, vad, ss]
        return out, self._detach(gt_batch)

    @staticmethod
    def _detach(gt_batch):
        if gt_batch is not None:
            if type(gt_batch) is list:
                for i in range(len(gt_batch)):
                    gt_batch[i] = gt_batch[i].detach()
            else:
                gt_batch = gt_batch.detach()
        return gt_batch

    def evaluate(self, pred_batch=None, gt_batch=None, vad_TH=[0.001, 0.5], idx=None):
        """:582-600 — pred_batch = pred2DOA's list, gt_batch = [doa [nb, nt, 2, ns] in radians, ..., vad [nb, nt, ns]] ->
        {'ACC', 'MDR', 'FAR', 'MAE', 'RMSE'} of one-element device tensors (azimuth, ae_TH = 10 degrees)."""
        doa_gt, vad_gt = gt_batch[0], gt_batch[-1]
        doa_est, vad_est = pred_batch[0], pred_batch[-2]
        if vad_gt.ndim != 3 or tuple(vad_gt.shape[:2]) != tuple(doa_gt.shape[:2]):
            raise RuntimeError("PredDOA.evaluate: gt_batch[-1] %s is not a VAD [nb, nt, ns]; a module built with tar_useVAD=False "
                               "hands the IPD tensor here (the reference then thresholds the IPDs as if they were VADs)"
                               % (tuple(vad_gt.shape),))
        dev = doa_est.device
        metric = {}
        metric['ACC'], metric['MDR'], metric['FAR'], metric['MAE'], metric['RMSE'] = \
            self.getmetric(doa_gt.to(dev), vad_gt.to(dev), doa_est, vad_est, ae_mode=['azi'], ae_TH=10, useVAD=True,
                           vad_TH=vad_TH, radians=True)
        return metric
