"""The Lightning module of the reference's IPDnet2 (``MyModel`` of IPDnet2/run_IPDnet2.py:82-339) restated over the HIP
path, evaluation side: a batch ``(mic_sig [nb, ns, nch], azimuth [nb, nt, nsrc] in degrees, vad [nb, nt, nsrc],
array geometry [nb, nmic, 3], distance [nb, nt, nsrc])`` becomes features, near-field DP-IPD targets, the network's
prediction, a frame-level PIT-MSE loss and the ACC / MDR / FAR / MAE / RMSE metrics without leaving the device:

    data_preprocess   :266-328   ``ops.preprocess_ipdnet2`` (STFT hop 320 centred, forgetting norm), ``fnssl_ipdnet2_targets``
                                 (near-field targets gated by the label VAD at threshold 0, Bessel target in silent slots)
    cal_loss          :237-251   ``fnssl_pit_mse_loss``; ``mode='test'`` also returns the targets and the permuted prediction
    validation_step / test_step  :173-221   the loss, then ``IPDnet2.Module.PredDOA(mic_location=gt_batch[-3])``: the MSE
                                 template search of all tracks and the metrics, logged as ``valid/<m>`` / ``test/<m>`` when a
                                 trainer is attached and kept on ``last_metrics``
    predict_step      :225-229   and ``predict_stream``, the same from a stream of samples (fnssl/stream.py)
    configure_optimizers :330-339   AdamW(lr 5e-4) + ExponentialLR(0.975)

Frame-count alignment (:183-189).  When the prediction has more frames than the targets the reference cuts the prediction;
so does this.  Otherwise the reference cuts the targets, slicing the FLATTENED ``nb * nt`` axis of the IPD tensor by the
prediction's frame count (:187) — right only for one utterance, and the following reshape fails for more.  Here each
utterance's targets, azimuths, distances and VAD are cut to the prediction's frames: identical to the reference for
``nb = 1`` and whenever the counts are equal.

``pytorch_lightning`` is optional: with it ``MyModel`` is a ``LightningModule``, without it an ``nn.Module`` whose
methods are called directly.  The constructor is the reference's plus a trailing ``arch``: ``None`` builds the shipped
``OnlineSpatialNet(...)`` of :103-119.  ``compile`` is accepted and ignored (there is nothing to compile).

Training (:159-171) is opt-in: ``MyModel(..., train_on_device=True)`` routes ``forward`` to
``OnlineSpatialNet.forward_train`` while the module is in ``train()`` with gradients enabled, and ``training_step`` then
aligns the frame counts as the evaluation steps do and returns ``{"loss": loss}`` with the PIT-MSE loss of
``fnssl.ipdnet_step.PitMSE``, whose ``backward()`` fills the ``.grad`` of every parameter of ``arch`` on the device (fp32).
With the default ``train_on_device=False`` everything is as before: ``OnlineSpatialNet.forward`` is forward-only, so
``training_step`` raises its forward-only error unless the module is in ``eval()`` mode, and the loss carries no ``grad_fn``.

Out of scope: datasets and the CLI, the ``np.save`` dumps of ``test_step``'s evaluation, ``ch_mode='MM'``, bf16 training.
"""
import itertools
import os
import sys

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from fnssl import ipdnet_step, ops                                  # noqa: E402
from IPDnet2.IPDnet2 import OnlineSpatialNet                        # noqa: E402
from IPDnet2.Module import PredDOA                                  # noqa: E402

try:  # optional, absent in the build image
    from pytorch_lightning import LightningModule as _Base
except Exception:  # pragma: no cover
    _Base = torch.nn.Module


class MyModel(_Base):
    def __init__(self, tar_useVAD: bool = True, ch_mode: str = 'M', res_the: int = 1, res_phi: int = 180, fs: int = 16000,
                 win_len: int = 512, nfft: int = 512, win_shift_ratio: float = 0.625, method_mode: str = 'IDL',
                 cuda_activated: bool = True, return_metric: bool = True, compile: bool = False, exp_name: str = 'exp',
                 device: str = 'cuda', arch=None, train_on_device: bool = False):
        super().__init__()
        self.train_on_device = bool(train_on_device)
        if (win_len, nfft, win_shift_ratio, fs) != (512, 512, 0.625, 16000):
            raise ValueError("the MI355X path is built for fs 16000, win_len = nfft = 512, hop 320 (run_IPDnet2.py:90-93)")
        if ch_mode != 'M':
            raise ValueError("IPDnet2's targets are the reference-microphone pairs (ch_mode 'M'), got %r" % (ch_mode,))
        self.arch = arch if arch is not None else OnlineSpatialNet(
            dim_input=10, dim_output=16, num_layers=8, dim_hidden=96, num_heads=4, kernel_size=(5, 3), conv_groups=(8, 8),
            norms=["LN", "LN", "GN", "LN", "LN", "LN"], dim_squeeze=8, num_freqs=256, attention='mamba(16,4)', rope=False,
            time_compression_layer=0, fre_compression_ratio=16, time_compression_ratio=5)
        self.dev = device
        self.tar_useVAD = tar_useVAD
        self.method_mode = method_mode
        self.cuda_activated = cuda_activated
        self.ch_mode = ch_mode
        self.nfft = nfft
        self.fre_max = fs / 2
        self.return_metric = return_metric
        self.fre_range_used = range(1, int(self.nfft / 2) + 1, 1)
        self.res_the, self.res_phi, self.exp_name = res_the, res_phi, exp_name
        self.speed = 340.0
        self.last_metrics = None

    def forward(self, x):
        if self.train_on_device and self.arch.training and torch.is_grad_enabled():
            return self.arch.forward_train(x)
        return self.arch(x)

    def _log(self, name, value, **kw):
        if hasattr(self, "log") and getattr(self, "_trainer", None) is not None:
            self.log(name, value, **kw)

    def _forward_aligned(self, batch):
        """data_preprocess, forward and the frame-count alignment of :179-189 -> (pred_batch, gt_batch)."""
        data_batch = self.data_preprocess(batch[0], batch[1], batch[3], batch[2], batch[4])
        gt_batch = data_batch[1:]
        pred_batch = self(data_batch[0])
        nb, ntp = pred_batch.shape[:2]
        ntg = gt_batch[0].shape[1]
        if ntp > ntg:
            pred_batch = pred_batch[:, :ntg]
        elif ntp < ntg:                                                              # per utterance, see the module docstring
            gt_batch[0] = gt_batch[0][:, :ntp]
            gt_batch[1] = gt_batch[1].view(nb, ntg, *gt_batch[1].shape[1:])[:, :ntp].reshape(nb * ntp, *gt_batch[1].shape[1:])
            gt_batch[-1] = gt_batch[-1][:, :ntp]
            gt_batch[-2] = gt_batch[-2][:, :ntp]
        return pred_batch, gt_batch

    def _eval_step(self, batch, stage, idx):
        pred_batch, gt_batch = self._forward_aligned(batch)
        if stage == "test":
            loss, gt_batch_ipd, pred_batch_ipd = self.cal_loss(pred_batch=pred_batch, gt_batch=gt_batch, mode='test')
        else:
            loss, gt_batch_ipd, pred_batch_ipd = self.cal_loss(pred_batch=pred_batch, gt_batch=gt_batch), None, None
        self._log(stage + "/loss", loss, sync_dist=True)
        get_metric = PredDOA(mic_location=gt_batch[-3], dev=self.dev)
        with torch.no_grad():
            metric = get_metric(pred_batch=pred_batch, gt_batch=gt_batch, idx=idx, gt_batch_ipd=gt_batch_ipd,
                                pred_batch_ipd=pred_batch_ipd, dir_name=None)
        self.last_metrics = metric
        for m in metric:
            self._log(stage + '/' + m, metric[m], sync_dist=True)
        return loss

    def training_step(self, batch, batch_idx: int = 0):
        """:159-171.  ``train_on_device``: the aligned prediction of ``forward_train`` and the differentiable PIT-MSE loss.
        Otherwise the network is forward-only: in ``train()`` mode ``self(in_batch)`` raises its forward-only error."""
        if self.train_on_device:
            pred_batch, gt_batch = self._forward_aligned(batch)        # cutting the prediction is a view
            loss = self.cal_loss(pred_batch=pred_batch, gt_batch=gt_batch)
            self._log("train/loss", loss, prog_bar=True)
            return {"loss": loss}
        data_batch = self.data_preprocess(batch[0], batch[1], batch[3], batch[2], batch[4])
        pred_batch = self(data_batch[0])
        loss = self.cal_loss(pred_batch=pred_batch, gt_batch=data_batch[1:])
        self._log("train/loss", loss, prog_bar=True)
        return {"loss": loss}

    def validation_step(self, batch, batch_idx: int = 0):
        """The loss and the DOA metrics of :173-196; returns the loss."""
        return self._eval_step(batch, "valid", None)

    def test_step(self, batch, batch_idx: int = 0):
        """:198-221; returns the loss."""
        return self._eval_step(batch, "test", batch_idx)

    @torch.no_grad()
    def predict_step(self, batch, batch_idx: int = 0):
        """batch [nb, nch, ns] -> the first utterance's prediction [nt', 512, nmic - 1, max_track] (:225-229)."""
        data_batch = self.data_preprocess(mic_sig_batch=batch.permute(0, 2, 1))
        return self.forward(data_batch[0])[0]

    @torch.no_grad()
    def predict_stream(self, chunk, state=None, last: bool = False):
        """Online ``predict_step``: chunk [nb, nch, n] = the NEXT n samples (any n) -> (preds, state).  ``preds`` is the
        first utterance's [new frames, 512, nmic - 1, max_track] for the groups of 5 transform frames this chunk completes
        (a frame is complete 256 samples after its centre), or None when it completes none; ``state`` (None for the first
        chunk) is the ``fnssl.stream.OnlineLocalizer`` that carries the sample tail, the normalisation and the network
        state.  ``last=True`` says that the signal ends with this chunk: the groups only the known end completes (the last
        frame reflects at it) are returned with the chunk's own, and the stream is finished."""
        from fnssl import stream
        if state is None:
            state = stream.OnlineLocalizer(self.arch, stream.CentredStreamFrontEnd(
                chunk.shape[1], sample_length=249, eps=1e-6, segment_frames=self.arch.time_compression_ratio))
        preds = [state.push(chunk.permute(0, 2, 1).to(self.dev).float())[0]]
        if last:
            preds.append(state.finish()[0])
        preds = [p[0] for p in preds if p is not None]
        return (None if not preds else preds[0] if len(preds) == 1 else torch.cat(preds, dim=0)), state

    def open_stream_pool(self, nch: int, slots: int, localize: bool = False, mic_location=None):
        """A ``fnssl.stream.StreamPool`` on ``self.arch``: ``slots`` independent streams of ``nch`` microphones, each with
        its own start, chunk sizes and end, served by one set of launches per push (``pool.open()``, ``pool.push({slot:
        chunk [n, nch]}, last=())``, ``pool.close(slot)``).  ``localize=True`` maps every prediction to (DOA, activity,
        spectrum) of its two tracks with the template search of ``PredDOA`` on ``mic_location`` [nmic, 3]."""
        from fnssl import stream
        entry = None
        if localize:
            if mic_location is None:
                raise ValueError("open_stream_pool: localize=True needs mic_location [nmic, 3]")
            pd = PredDOA(mic_location=mic_location, dev=self.dev)
            entry = lambda p: pd._search(p[..., :2], 1)                     # noqa: E731
        return stream.StreamPool(self.arch, nch, slots, localize=entry, sample_length=249, eps=1e-6)

    def cal_loss(self, pred_batch=None, gt_batch=None, mode='train'):
        """Frame-level PIT-MSE (:237-251) in one HIP kernel.  ``mode='train'``: the loss, a 0-d device tensor; otherwise
        (loss, ipd_gt [nb * nt, nsrc, D], the prediction [nb * nt, nsrc, D] with its tracks in the best permutation),
        D = 512 * (nmic - 1).  A ``pred_batch`` that requires a gradient gives, in ``mode='train'``, the same loss with a
        ``grad_fn`` (``ipdnet_step.PitMSE``)."""
        if mode == 'train' and pred_batch.requires_grad and torch.is_grad_enabled():
            return ipdnet_step.PitMSE.apply(pred_batch.to(self.dev).float(), gt_batch[1])
        pred = pred_batch.detach().to(self.dev).float()
        ipd_gt = gt_batch[1]
        want = mode != 'train'
        loss, _dpred, perm = ipdnet_step.pit_mse(pred, ipd_gt, want_perm=want)
        loss = loss.reshape(())
        if not want:
            return loss
        nb, nt, _, _, nsrc = pred.shape
        table = torch.tensor(list(itertools.permutations(range(nsrc))), dtype=torch.long, device=pred.device)
        pm = table[perm.long()]                                                       # [nb * nt, nsrc]: track paired with target j
        flat = pred.reshape(nb * nt, -1, nsrc).permute(0, 2, 1)
        pred_perm = torch.gather(flat, 1, pm[:, :, None].expand(-1, -1, flat.shape[2]))
        return loss, ipd_gt.reshape(nb * nt, -1, nsrc).permute(0, 2, 1), pred_perm

    def data_preprocess(self, mic_sig_batch=None, targets_batch=None, array_gemo_data=None, vad_data_batch=None,
                        distance_batch=None, eps=1e-6):
        """:266-328 on device.  Returns [features [nb, 2 nch, 256, nt], targets_batch, ipd.view(nb * nt, 512, nmic - 1, nsrc),
        mic_loc (numpy float64 [nmic, 3], the first utterance's as in the reference), distance_batch, vad_batch]; without
        ``targets_batch`` just the features (``predict_step``)."""
        sig = mic_sig_batch.to(self.dev).float()
        data = [ops.preprocess_ipdnet2(sig, eps, 249)]
        if targets_batch is None:
            return data
        geo = array_gemo_data.detach().cpu().numpy() if isinstance(array_gemo_data, torch.Tensor) else np.asarray(array_gemo_data)
        mic_loc = np.ascontiguousarray(geo[0], dtype=np.float64).reshape(-1, 3)
        if mic_loc.shape[0] != sig.shape[2]:
            raise RuntimeError("data_preprocess: the geometry has %d microphones, the signals %d channels" % (mic_loc.shape[0], sig.shape[2]))
        azi = targets_batch.to(self.dev).float()
        if azi.ndim != 3 or vad_data_batch is None or distance_batch is None or tuple(vad_data_batch.shape) != tuple(azi.shape) \
                or tuple(distance_batch.shape) != tuple(azi.shape):
            raise RuntimeError("data_preprocess: targets, vad and distance must all be [nb, nt, nsource]")
        azi_ele = torch.cat((torch.full_like(azi, 90.0)[:, :, np.newaxis, :], azi[:, :, np.newaxis, :]), dim=-2)
        doa = azi_ele / 180 * np.pi                                                  # :292, fp32
        g = ipdnet_step.ipdnet2_geometry(mic_loc, doa.device, 1, 360, self.nfft, self.fre_max, self.speed)
        vad_batch = vad_data_batch.to(self.dev)
        gate = vad_batch.float() if self.tar_useVAD else None
        ipd = ipdnet_step.ipdnet2_targets(doa, distance_batch.to(self.dev).float(), gate, g["mic"], g["non_source"], 1,
                                          int(self.nfft / 2), int(self.nfft / 2) + 1, self.fre_max, self.speed, 0.0)
        nb, nt, nf2, nm1, nsrc = ipd.shape
        data += [targets_batch, ipd.view(nb * nt, nf2, nm1, nsrc), mic_loc, distance_batch, vad_batch]
        return data

    def configure_optimizers(self):
        optimizer = torch.optim.AdamW(self.arch.parameters(), lr=0.0005)
        lr_scheduler = torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma=0.975, last_epoch=-1)
        return {'optimizer': optimizer, 'lr_scheduler': {'scheduler': lr_scheduler, 'monitor': 'valid/loss'}}
