"""The Lightning module of the reference's online IPDnet (``MyModel`` of IPDnet/runIPDnetOn.py:80-301) restated over the
HIP path: a batch ``(mic_sig_batch [nb, ns, nch], {'doa' [nb, nseg, 2, nsrc], 'dp_signal' [nb, ns, nch, nsrc]})`` becomes
features, DP-VAD, per-source DP-IPD targets and a frame-level PIT-MSE loss with a ``grad_fn`` without leaving the
device:

    data_preprocess   :237-290   STFT once (features + VAD), ``fnssl_dp_vad``, ``fnssl_ipdnet_targets``
    cal_loss          :196-206   ``fnssl_pit_mse_loss`` (``fnssl.ipdnet_step.PitMSE``)
    training_step     :144-154
    validation_step / test_step :156-180   the loss, then ``get_metric`` (``IPDnet.Module.PredDOA``): the template search of
                                 all tracks and ACC / MDR / FAR / MAE / RMSE on device, logged as ``valid/<m>`` / ``test/<m>``
    configure_optimizers :292-301   Adam(lr 5e-4) + ExponentialLR(0.975)
    predict_step      :182-186   and ``predict_stream``, the same from a stream of samples (fnssl/stream.py)

``pytorch_lightning`` is optional: with it ``MyModel`` is a ``LightningModule``, without it an ``nn.Module`` whose
methods are called directly.  The constructor is the reference's plus two trailing keywords.  ``arch``: ``None`` builds
``IPDnet()`` as the reference does; arrays of more than two microphones pass ``IPDnet(2 * nmic, 256, max_source, True)``
(the reference tells its users to edit that line).  ``train_on_device``: with ``True``, ``forward`` in ``train()`` mode
with gradients enabled calls ``arch.forward_train`` (fnssl/ipdnet_train.py), so ``training_step`` gives a loss whose
``backward()`` fills every ``.grad`` — for the hidden-128 two-microphone default too (full-band H = 64 training kernels,
csrc/lstm_train_h64.hip).  With the default ``False`` nothing changes: ``forward`` is ``arch(x)``, which trains by itself
at hidden 256 and raises the forward-only error in ``train()`` mode at hidden 128.  ``compile`` is accepted and ignored
(there is nothing to compile).

Out of scope: datasets and the CLI, the ``np.save`` dumps of ``test_step``'s evaluation, runIPDnetOff.py's
whole-utterance normalisation, bf16 training.
"""
import os
import sys

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from fnssl import ipdnet_step, ops                                  # noqa: E402
from IPDnet.FixedAarryIPDnet import IPDnet                          # noqa: E402
from IPDnet.Module import PredDOA                                   # noqa: E402

try:  # optional, absent in the build image
    from pytorch_lightning import LightningModule as _Base
except Exception:  # pragma: no cover
    _Base = torch.nn.Module

_DEFAULT_MICS = ((-0.04, 0.0, 0.0), (0.04, 0.0, 0.0))


class MyModel(_Base):
    def __init__(self, tar_useVAD: bool = True, ch_mode: str = 'M', res_the: int = 1, res_phi: int = 180, fs: int = 16000,
                 win_len: int = 512, nfft: int = 512, win_shift_ratio: float = 0.5, max_source: int = 2, device: str = 'cuda',
                 mic_pos=None, compile: bool = False, is_linear_array: bool = True, is_planar_array: bool = True,
                 exp_name: str = 'exp', arch=None, train_on_device: bool = False):
        super().__init__()
        if (win_len, nfft, win_shift_ratio) != (512, 512, 0.5):
            raise ValueError("the MI355X path is built for win_len = nfft = 512, hop 256 (runIPDnetOn.py:34-35)")
        if ch_mode != 'M':
            raise ValueError("IPDnet's targets are the reference-microphone pairs (ch_mode 'M'): DPIPD.forward fills only "
                             "those rows (IPDnet/Module.py:386-387), got %r" % (ch_mode,))
        if not 1 <= int(max_source) <= ipdnet_step.MAX_SOURCES:
            raise ValueError("max_source must be 1..%d, got %r" % (ipdnet_step.MAX_SOURCES, max_source))
        self.arch = IPDnet() if arch is None else arch
        self.train_on_device = bool(train_on_device)
        self.tar_useVAD = tar_useVAD
        self.ch_mode = ch_mode
        self.nfft = nfft
        self.fre_max = fs / 2
        self.max_source = int(max_source)
        mic = _DEFAULT_MICS if mic_pos is None else mic_pos
        mic = mic.detach().cpu().numpy() if isinstance(mic, torch.Tensor) else np.asarray(mic)
        self.mic_pos = np.ascontiguousarray(mic, dtype=np.float32).reshape(-1, 3)
        if 2 * self.mic_pos.shape[0] != getattr(self.arch, "input_size", 2 * self.mic_pos.shape[0]):
            raise ValueError("mic_pos has %d microphones but the network takes %d channels (pass arch=IPDnet(2 * nmic, 256, "
                             "max_source, True))" % (self.mic_pos.shape[0], self.arch.input_size))
        self.is_linear_array, self.is_planar_array = is_linear_array, is_planar_array
        self.res_the, self.res_phi, self.exp_name = res_the, res_phi, exp_name
        self.speed = 340.0
        self.vad_th = 0.001                                          # runIPDnetOn.py:274
        self.fre_range_used = range(1, int(self.nfft / 2) + 1, 1)
        self.dev = device
        # mapping IPD to DOA and calculating the metrics (runIPDnetOn.py:127)
        self.get_metric = PredDOA(mic_location=self.mic_pos, is_linear_array=is_linear_array, is_planar_array=is_planar_array,
                                  max_track=self.max_source, dev=device)
        self.last_metrics = None

    def forward(self, x):
        if self.train_on_device and self.arch.training and torch.is_grad_enabled():
            return self.arch.forward_train(x)                        # opt-in: every trainable width (hidden 128 / 256)
        return self.arch(x)

    def _log(self, name, value, **kw):
        if hasattr(self, "log") and getattr(self, "_trainer", None) is not None:
            self.log(name, value, **kw)

    def _forward_loss(self, batch):
        """(loss, pred_batch, gt_batch) of one batch: data_preprocess, forward, cal_loss."""
        data_batch = self.data_preprocess(batch[0], batch[1])
        pred_batch = self(data_batch[0])
        gt_batch = data_batch[1:]
        return self.cal_loss(pred_batch=pred_batch, gt_batch=gt_batch), pred_batch, gt_batch

    def _step_loss(self, batch):
        return self._forward_loss(batch)[0]

    def _eval_step(self, batch, stage, idx):
        """:156-180 — the loss as ``_step_loss`` forms it, then the metrics of the same prediction under ``no_grad``; the
        dict of one-element device tensors stays on ``self.last_metrics`` and is logged when a trainer is attached."""
        loss, pred_batch, gt_batch = self._forward_loss(batch)
        self._log(stage + "/loss", loss, sync_dist=True)
        with torch.no_grad():
            metric = self.get_metric(pred_batch=pred_batch, gt_batch=gt_batch, idx=idx)
        self.last_metrics = metric
        for m in metric:
            self._log(stage + '/' + m, metric[m], sync_dist=True)
        return loss

    def training_step(self, batch, batch_idx: int = 0):
        loss = self._step_loss(batch)
        self._log("train/loss", loss, prog_bar=True)
        return {"loss": loss}

    def validation_step(self, batch, batch_idx: int = 0):
        """The loss and the DOA metrics of runIPDnetOn.py:156-167; returns the loss."""
        return self._eval_step(batch, "valid", None)

    def test_step(self, batch, batch_idx: int = 0):
        return self._eval_step(batch, "test", batch_idx)

    @torch.no_grad()
    def predict_step(self, batch, batch_idx: int = 0):
        """batch [nb, nch, ns] -> the first utterance's prediction [nt // 12, 512, nmic - 1, max_source] (:182-186)."""
        data_batch = self.data_preprocess(mic_sig_batch=batch.permute(0, 2, 1))
        return self.forward(data_batch[0])[0]

    @torch.no_grad()
    def predict_stream(self, chunk, state=None):
        """Online ``predict_step``: chunk [nb, nch, n] = the NEXT n samples (any n) -> (preds, state).  ``preds`` is what
        ``predict_step`` returns on the whole signal for the segments this chunk completes — the first utterance's
        [new segments, 512, nmic - 1, max_source] — or None when it completes none; ``state`` (None for the first chunk) is
        the ``fnssl.stream.OnlineLocalizer`` that carries the sample tail, the normalisation and the network state."""
        from fnssl import stream
        if state is None:
            state = stream.OnlineLocalizer(self.arch, stream.StreamFrontEnd("array", chunk.shape[1], sample_length=280, eps=1e-6))
        pred, _ = state.push(chunk.permute(0, 2, 1).to(self.dev))
        return (None if pred is None else pred[0]), state

    def open_stream_pool(self, nch: int, slots: int, localize: bool = False):
        """A ``fnssl.stream.LstmStreamPool`` on ``self.arch``: ``slots`` independent streams of ``nch`` microphones, each
        with its own start and chunk sizes, served by one front-end launch and one network call per push
        (``pool.open()``, ``pool.push({slot: chunk [n, nch]})``, ``pool.close(slot)``).  ``localize=True`` maps every
        prediction to ``get_metric._localize``'s (DOA, VAD), narrowed to the slot's row."""
        from fnssl import stream
        return stream.LstmStreamPool(self.arch, nch, slots, localize=self.get_metric._localize if localize else None,
                                     sample_length=280, eps=1e-6)

    def cal_loss(self, pred_batch=None, gt_batch=None, batch_idx=None):
        """Frame-level PIT-MSE (:196-206) — one HIP kernel that emits its own gradient; a scalar with a ``grad_fn``."""
        return ipdnet_step.PitMSE.apply(pred_batch, gt_batch[1])

    def data_preprocess(self, mic_sig_batch=None, acoustic_scene_batch=None, vad_batch=None, eps=1e-6):
        """:237-290 on device.  Returns [features [nb, 2 nch, 256, nt], doa, ipd.view(nb * nt2, 512, nmic - 1, nsrc),
        dp_vad (if ``tar_useVAD``)]; without ``acoustic_scene_batch`` just the features (``predict_step``)."""
        sig = mic_sig_batch.to(self.dev)
        spec, magsum = ops.stft(sig)                                                 # once, for the features and the VAD
        x, _ = ops.array_features(spec, magsum, eps, 280, 0)
        data = [x.permute(0, 3, 2, 1)]                                               # = ops.preprocess_array(sig)
        if acoustic_scene_batch is None:
            return data
        dp = acoustic_scene_batch['dp_signal'].to(self.dev)
        if dp.ndim != 4 or dp.shape[3] != self.max_source or tuple(dp.shape[:2]) != tuple(sig.shape[:2]):
            raise RuntimeError("data_preprocess: dp_signal must be [nb, ns, nch, %d] like the mixture %s, got %s"
                               % (self.max_source, tuple(sig.shape), tuple(dp.shape)))
        dp_spec, _ = ops.stft(dp[:, :, 0, :])                                        # channel 0 only (:230), read in place
        dp_vad = ipdnet_step.dp_vad(spec, dp_spec)
        doa = acoustic_scene_batch['doa'].to(self.dev)
        if tuple(doa.shape[:2]) != tuple(dp_vad.shape[:2]) or doa.shape[-1] != self.max_source:
            raise RuntimeError("data_preprocess: doa %s does not match the %d segments x %d sources of the signals"
                               % (tuple(doa.shape), dp_vad.shape[1], self.max_source))
        mic, non_source = ipdnet_step.non_source_device(self.mic_pos, doa.device)
        ipd = ipdnet_step.ipdnet_targets(doa.float(), dp_vad, mic, non_source, 1, int(self.nfft / 2), int(self.nfft / 2) + 1,
                                         self.fre_max, self.speed, self.vad_th)
        nb, nt2, nf2, nm1, nsrc = ipd.shape
        data += [doa, ipd.view(nb * nt2, nf2, nm1, nsrc)]
        if self.tar_useVAD:
            data += [dp_vad]
        return data

    def configure_optimizers(self):
        optimizer = torch.optim.Adam(self.arch.parameters(), lr=0.0005)
        lr_scheduler = torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma=0.975, last_epoch=-1)
        return {'optimizer': optimizer, 'lr_scheduler': {'scheduler': lr_scheduler, 'monitor': 'valid/loss'}}
