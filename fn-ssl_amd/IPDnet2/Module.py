"""Drop-in for the hot-path class of the reference's ``IPDnet2/Module.py``: ``STFT`` (:28-64) — the IPDnet2 tree's
transform is CENTRED (``torch.stft(..., center=True)``, reflect padding) and its run script uses
``win_shift_ratio = 0.625`` (hop 320; IPDnet2/run_IPDnet2.py:91-93,135-136), unlike FN-SSL's ``Module.STFT``.
The fused front end the network entry uses is ``fnssl.ops.preprocess_ipdnet2`` (STFT kernel + one scan + one pack
kernel = run_IPDnet2.py:277-288); this class keeps code written against the per-stage API working.

The evaluation half of that file runs on device too: ``getMetric`` (:67-278) with IPDnet2's rules (an estimate is active
when its activity, an MSE, is BELOW the threshold; ACC / MDR / FAR divide by K_gt + 1e-6), ``DPIPD2`` (:413-498) with the
near-field ``forward(source_doa, source_distance)`` (``fnssl_ipdnet2_targets``), and ``PredDOA`` (:508-706) with the MSE
template search of all tracks in one launch (``fnssl_ipd2doa_mse_tracks``) and the metrics in one kernel pair
(``fnssl_doa_metrics_ex``).  Predictions, DOAs, activities and metrics stay on the device.

Not reproduced: ``DPIPD2`` with ``ch_mode='MM'`` and ``PredDOA.pred2DOA`` with ``max_num_sources`` other than 1 (the
reference's own slice assignment needs 1), ``time_pool_size`` (unused by the reference) — all three raise —, and the
``np.save`` dumps ``evaluate`` writes when ``idx`` and ``dir_name`` are given (both are accepted and ignored).  ``DPIPD2``
returns device tensors where the reference returns numpy arrays.  Plotting stays out of scope."""
import numpy as np
import torch
import torch.nn as nn

from fnssl import ipdnet_step, ops
from fnssl import metrics as fmetrics


class STFT(nn.Module):
    """signal [nb, ns, nch] -> complex64 [nb, 257, nt = ns // hop + 1, nch]  (Hann-512, centred, reflect-padded)."""

    def __init__(self, win_len, win_shift_ratio, nfft, win='hann'):
        super(STFT, self).__init__()
        if win_len != 512 or nfft != 512 or win != 'hann':
            raise ValueError("STFT: the MI355X path is built for win_len = nfft = 512, hann (run_IPDnet2.py:91-93)")
        self.win_len = win_len
        self.win_shift_ratio = win_shift_ratio
        self.nfft = nfft
        self.win = win

    def forward(self, signal):
        hop = int(self.win_len * self.win_shift_ratio)                 # Module.py:51
        spec, _ = ops.stft(signal, hop=hop, center=True)               # [nb, nch, nt, 257, 2]
        return torch.view_as_complex(spec).permute(0, 3, 2, 1)


class getMetric(nn.Module):
    """Reference getMetric (:67-278): ``forward`` returns the LIST [ACC, MAE] ('single') or [ACC, MD, FA, MAE, RMSE]
    ('multiple') of device tensors, unfolded into one-element tensors with ``metric_unfold``.  'multiple' is IPDnet2's: an
    estimate is active when ``vad_est < vad_TH[1]`` (:167) and the three ratios divide by ``K_gt + 0.000001`` (:208-210);
    'single' keeps ``>`` and the bare ratio (:114-125).  Of several ``ae_mode`` entries the reference's if / elif chain
    evaluates ONE (ele, else azi, else aziele); so does this.  The DOAs are degrees (the reference's conversion is
    commented out, :105-106); ``radians=(gt, est)`` lets the kernel convert either side as ``PredDOA.evaluate`` does.
    ``last_counts``: the per-utterance K_gt, K_est, K_corr of the last call."""

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

    def forward(self, doa_gt, vad_gt, doa_est, vad_est, ae_mode, ae_TH=30, useVAD=True, vad_TH=[0.5, 0.5], radians=(False, False)):
        mode = next((m for m in ('ele', 'azi', 'aziele') if m in ae_mode), None)
        if mode is None:
            raise Exception('Angle error mode unrecognized')
        f = lambda t: None if t is None else t.float()                           # noqa: E731
        multiple = self.source_mode == 'multiple'
        m, k_gt, k_est, k_corr = fmetrics.doa_metrics(f(doa_gt), f(vad_gt), f(doa_est), f(vad_est), self.source_mode, [mode], ae_TH,
                                                      useVAD, vad_TH, tuple(radians), self.inf, 1e-5, est_below=multiple,
                                                      ratio_eps=1e-6 if multiple else 0.0)
        self.last_counts = {'K_gt': k_gt, 'K_est': k_est, 'K_corr': k_corr}
        s = fmetrics.AE_SLOT[mode]
        if not multiple:
            metric = [m[fmetrics.SLOT_ACC], m[fmetrics.SLOT_MAE + s:fmetrics.SLOT_MAE + s + 1]]
        else:
            metric = [m[fmetrics.SLOT_ACC:fmetrics.SLOT_ACC + 1], m[fmetrics.SLOT_MDR:fmetrics.SLOT_MDR + 1],
                      m[fmetrics.SLOT_FAR:fmetrics.SLOT_FAR + 1], m[fmetrics.SLOT_MAE + s:fmetrics.SLOT_MAE + s + 1],
                      m[fmetrics.SLOT_RMSE + s:fmetrics.SLOT_RMSE + s + 1]]
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


def _mic_table(mic_location):
    mic = mic_location.detach().cpu().numpy() if isinstance(mic_location, torch.Tensor) else np.asarray(mic_location)
    return np.ascontiguousarray(mic, dtype=np.float64).reshape(-1, 3)


class DPIPD2(nn.Module):
    """Complex-valued direct-path inter-channel phase difference, near field (reference :413-498).  ``forward()`` returns
    (the far-field template bank complex64 [nele, nazi, nf, nmic - 1] of ``__init__`` (:424-441), the near-field DP-IPD of
    the given sources complex64 [nb, ntime, nf, nmic - 1, nsource] or None), both on ``dev``.  The bank, the float64
    microphone table and the grids are cached per geometry (``fnssl.ipdnet_step.ipdnet2_geometry``)."""

    def __init__(self, ndoa_candidate, mic_location, nf=257, fre_max=8000, ch_mode='M', speed=343.0, dev='cuda'):
        super(DPIPD2, self).__init__()
        if ch_mode != 'M':
            raise ValueError("DPIPD2: the MI355X path forms the reference-microphone pairs (ch_mode 'M'), got %r" % (ch_mode,))
        self.ndoa_candidate = ndoa_candidate
        self.mic_location = _mic_table(mic_location)
        self.nf = int(nf)
        self.fre_max = fre_max
        self.speed = speed
        self.ch_mode = ch_mode
        self.dev = dev

    def geometry(self, device=None):
        return ipdnet_step.ipdnet2_geometry(self.mic_location, torch.device(self.dev if device is None else device),
                                            self.ndoa_candidate[0], self.ndoa_candidate[1], 2 * (self.nf - 1), float(self.fre_max),
                                            float(self.speed))

    @property
    def dpipd_template(self):
        """complex64 [nele, nazi, nf, nmic - 1] on ``dev``; bin 0 is 1 + 0j (its delay-phase is 0)."""
        g = self.geometry()
        bank, n = g["bank"], self.nf - 1
        one = torch.ones(bank.shape[:2] + (1, bank.shape[3]), dtype=torch.float32, device=bank.device)
        return torch.complex(torch.cat((one, bank[:, :, :n]), dim=2), torch.cat((0 * one, bank[:, :, n:]), dim=2))

    def forward(self, source_doa=None, source_distance=None):
        """source_doa [nb, ntimestep, 2, nsource] (elevation, azimuth; radians), source_distance [nb, ntimestep, nsource]:
        numpy arrays or tensors."""
        dpipd = None
        if source_doa is not None and source_distance is not None:
            g = self.geometry()
            dev = g["mic"].device
            doa = torch.as_tensor(source_doa).to(dev).float()
            dist = torch.as_tensor(source_distance).to(dev).float()
            out = ipdnet_step.ipdnet2_targets(doa, dist, None, g["mic"], None, 0, self.nf, self.nf, float(self.fre_max),
                                              float(self.speed))
            dpipd = torch.complex(out[:, :, :self.nf].contiguous(), out[:, :, self.nf:].contiguous())
        return self.dpipd_template, dpipd


class PredDOA(nn.Module):
    """Multi-track DP-IPD predictions -> DOA / activity per track -> ACC, MDR, FAR, MAE, RMSE (reference PredDOA, :508-706):
    the far-field bank of ``DPIPD2`` (elevation pi / 2, azimuth linspace(-pi, pi, res_phi), speed 340), the MSE search, and
    ``evaluate``'s rules — ground truth [azi, azi] in degrees, activities / 0.2919, vad_TH [0.001, 0.4], ae_TH 5."""

    def __init__(self, source_num_mode='UnkNum', max_num_sources=1, max_track=2, res_the=1, res_phi=360, fs=16000, nfft=512,
                 ch_mode='M', dev='cuda', mic_location=None, is_linear_array=False, is_planar_array=True):
        super(PredDOA, self).__init__()
        if source_num_mode not in ('KNum', 'UnkNum'):
            raise ValueError("source_num_mode must be 'KNum' or 'UnkNum'")
        if not 1 <= int(max_num_sources) <= fmetrics.MAX_SOURCES:
            raise ValueError("PredDOA: max_num_sources must be 1..%d, got %r" % (fmetrics.MAX_SOURCES, max_num_sources))
        if mic_location is None:
            raise ValueError("PredDOA: mic_location [nmic, 3] is required")
        self.nfft = nfft
        self.fre_max = fs / 2
        self.ch_mode = ch_mode
        self.source_num_mode = source_num_mode
        self.max_num_sources = int(max_num_sources)
        self.fre_range_used = range(1, int(self.nfft / 2) + 1, 1)
        self.dev = dev
        self.max_track = int(max_track)
        self.gerdpipd = DPIPD2(ndoa_candidate=[res_the, res_phi], mic_location=mic_location, nf=int(self.nfft / 2) + 1,
                               fre_max=self.fre_max, ch_mode=self.ch_mode, speed=340, dev=dev)
        self.getmetric = getMetric(source_mode='multiple', metric_unfold=True)

    def forward(self, pred_batch, gt_batch, idx, gt_batch_ipd=None, pred_batch_ipd=None, dir_name=None):
        pred_batch, _ = self.pred2DOA(pred_batch=pred_batch, gt_batch=gt_batch)
        return self.evaluate(pred_batch=pred_batch, gt_batch=gt_batch, idx=idx, gt_batch_ipd=gt_batch_ipd,
                             pred_batch_ipd=pred_batch_ipd, dir_name=dir_name)

    def _search(self, pred5, ns):
        """pred5 [nb, nt, 2nf, nmic - 1, ntrack] (any strides) -> (DOA [ntrack, nb, nt, 2, ns], activity [ntrack, nb, nt, ns],
        spectrum [ntrack, nb, nt, nele, nazi])."""
        g = self.gerdpipd.geometry(pred5.device)
        idx, vad, ss = fmetrics.localize_tracks_mse(pred5, g["bank"], ns, self.source_num_mode)
        nazi = g["bank"].shape[1]
        idx = idx.long()
        return torch.stack((g["ele"][idx // nazi], g["azi"][idx % nazi]), dim=3), vad, ss

    def pred2DOA(self, pred_batch, gt_batch):
        """:548-570 — returns ([DOA [nb, nt, 2, max_track], activity [nb, nt, max_track], the re-batched IPD
        [nb * (nmic - 1), nt, 2nf, nmax]], gt_batch)."""
        if self.max_num_sources != 1:
            raise ValueError("PredDOA.pred2DOA: one source per track (the reference's slice assignment, :558-559, needs "
                             "max_num_sources = 1), got %d" % self.max_num_sources)
        pred = pred_batch.detach().to(self.dev).float()
        if pred.ndim != 5:
            raise RuntimeError("PredDOA: pred_batch must be [nb, nt, 2nf, nmic - 1, ntrack], got %s" % (tuple(pred.shape),))
        if self.max_track > pred.shape[-1]:
            raise RuntimeError("PredDOA: max_track = %d but the prediction has %d tracks" % (self.max_track, pred.shape[-1]))
        doa, vad, _ = self._search(pred[..., :self.max_track], 1)
        nb, nt, ndoa, nmic, nmax = pred.shape
        pred_ipd = pred.permute(0, 3, 1, 2, 4).reshape(nb * nmic, nt, ndoa, nmax)
        return [doa[..., 0].permute(1, 2, 3, 0), vad[..., 0].permute(1, 2, 0), pred_ipd], self._detach(gt_batch)

    def pred2DOA_track(self, pred_batch=None, gt_batch=None, time_pool_size=None):
        """One track (:573-666): pred [nb * (nmic - 1), nt, 2nf] -> [DOAs [nb, nt, 2, ns], activities [nb, nt, ns], the MSE
        spectrum [nb, nt, nele, nazi]], ns = max_num_sources."""
        if time_pool_size is not None:
            raise NotImplementedError("PredDOA.pred2DOA_track: time_pool_size is not supported (the reference does not use it)")
        out = None
        if pred_batch is not None:
            pred = pred_batch.detach().to(self.dev).float()
            nm1 = self.gerdpipd.mic_location.shape[0] - 1
            if pred.ndim != 3 or pred.shape[0] % nm1:
                raise RuntimeError("PredDOA.pred2DOA_track: pred must be [nb * %d, nt, 2nf], got %s" % (nm1, tuple(pred.shape)))
            nbm, nt, nf2 = pred.shape
            pred5 = pred.unflatten(0, (nbm // nm1, nm1)).permute(0, 2, 3, 1).unsqueeze(-1)     # a view: read in place
            doa, vad, ss = self._search(pred5, self.max_num_sources)
            out = [doa[0], vad[0], ss[0]]
        return out, self._detach(gt_batch)

    @staticmethod
    def _detach(gt_batch):
        if gt_batch is not None:
            if type(gt_batch) is list:
                for i in range(len(gt_batch)):
                    if torch.is_tensor(gt_batch[i]):
                        gt_batch[i] = gt_batch[i].detach()
            else:
                gt_batch = gt_batch.detach()
        return gt_batch

    def evaluate(self, pred_batch=None, gt_batch=None, vad_TH=[0.001, 0.4], idx=None, gt_batch_ipd=None, pred_batch_ipd=None,
                 dir_name=None):
        """:669-706 — pred_batch = pred2DOA's list, gt_batch = [azimuth [nb, nt, ns] in degrees, ..., vad [nb, nt, ns]] ->
        {'ACC', 'MDR', 'FAR', 'MAE', 'RMSE'} of one-element device tensors (azimuth, ae_TH = 5 degrees)."""
        azi_gt, vad_gt = gt_batch[0], gt_batch[-1]
        doa_est = pred_batch[0]
        dev = doa_est.device
        if azi_gt.ndim != 3 or tuple(vad_gt.shape) != tuple(azi_gt.shape):
            raise RuntimeError("PredDOA.evaluate: gt_batch[0] %s must be the azimuths [nb, nt, ns] and gt_batch[-1] %s their VAD"
                               % (tuple(azi_gt.shape), tuple(vad_gt.shape)))
        azi_gt = azi_gt.to(dev).float()
        doa_gt = torch.cat((azi_gt[:, :, np.newaxis, :], azi_gt[:, :, np.newaxis, :]), dim=-2)
        vad_est = pred_batch[-2].to(dev) / 0.2919
        metric = {}
        metric['ACC'], metric['MDR'], metric['FAR'], metric['MAE'], metric['RMSE'] = \
            self.getmetric(doa_gt, vad_gt.to(dev), doa_est, vad_est, ae_mode=['azi'], ae_TH=5, useVAD=True, vad_TH=vad_TH,
                           radians=(False, True))
        return metric
