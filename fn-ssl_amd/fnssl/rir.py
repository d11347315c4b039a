"""Room simulation on the device under gpuRIR's names and argument order, as the reference's ``Dataset.py`` uses them:
``import fnssl.rir as gpuRIR`` makes ``AcousticScene.simulate()`` and ``getRandomScene()`` run unchanged.

The kernels are csrc/rir.hip (image-source part, diffuse tail, moving-source mixing); the model is DESIGN.md §17.  It is
written from the published algorithm (Allen & Berkley 1979; Diaz-Guerra, Miguel & Beltran 2021) and is not bit compatible
with gpuRIR; only the ``"omni"`` patterns are built.

numpy in gives numpy out (computed on ``cuda:0``, one copy each way); ROCm tensors in give tensors out on their device with no
host round trip; CPU tensors are rejected like everywhere else in this package.
"""
from __future__ import annotations

import inspect
import math

import numpy as np
import torch

from . import ops

__all__ = ["att2t_SabineEstimator", "t2n", "beta_SabineEstimation", "simulateRIR", "simulateRIRBatch", "simulateTrajectory",
           "simulateTrajectoryBatch", "sample_counts"]


def att2t_SabineEstimator(att_dB, T60):
    """Time (s) for the sound to decay by ``att_dB`` in a room of reverberation time ``T60`` (Sabine's exponential decay)."""
    return att_dB / 60.0 * T60


def t2n(T, rooms_sz, c=343.0):
    """Images per axis that cover ``T`` seconds: ceil(2 T c / rooms_sz), a list of ints."""
    return [int(v) for v in np.ceil(2.0 * T * c / np.asarray(rooms_sz, dtype=np.float64))]


def beta_SabineEstimation(room_sz, T60, abs_weights=[1.0] * 6):
    """Reflection coefficients of the six walls (x0, x1, y0, y1, z0, z1) that give ``T60`` by Sabine's formula, the walls'
    absorptions in the ratios ``abs_weights``: with w normalised by its maximum, x = 0.161 V / (T60 S_w) clamped to [0, 1]
    and beta = sqrt(1 - x w) — the closed form of the equation gpuRIR solves with a bounded 1-D minimiser."""
    room = np.asarray(room_sz, dtype=np.float64).reshape(-1)
    w = np.asarray(abs_weights, dtype=np.float64).reshape(-1)
    if room.shape != (3,) or w.shape != (6,):
        raise ValueError("beta_SabineEstimation: room_sz has 3 entries and abs_weights 6")
    if not (room > 0).all() or (w < 0).any() or w.max() <= 0 or T60 < 0:
        raise ValueError("beta_SabineEstimation: room_sz > 0, abs_weights >= 0 with a positive one, T60 >= 0")
    w = w / w.max()
    area = np.array([room[1] * room[2]] * 2 + [room[0] * room[2]] * 2 + [room[0] * room[1]] * 2)
    sw = float((area * w).sum())
    x = 1.0 if T60 == 0 else min(1.0, max(0.0, 0.161 * float(room.prod()) / (T60 * sw)))
    return np.sqrt(1.0 - x * w)


def sample_counts(Tdiff, Tmax, fs):
    """(nISM, nSamples): ceil(T fs) made even; ``Tdiff`` None or beyond ``Tmax`` means ``Tmax``."""
    if Tdiff is None or Tdiff > Tmax:
        Tdiff = Tmax
    nism = int(math.ceil(Tdiff * fs))
    ns = int(math.ceil(Tmax * fs))
    return nism + nism % 2, ns + ns % 2


def _reject_cpu_tensors(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and not x.is_cuda:
            raise RuntimeError("fnssl.rir: expected a ROCm device tensor or a numpy array (this path has no CPU implementation), "
                               "got a tensor on %s" % x.device)


def _positions_host(pos, room, what):
    """The positions on the host in float64 [M, 3], checked: at least one, finite, strictly inside the room."""
    if isinstance(pos, torch.Tensor):
        host = pos.detach().to(torch.float32).reshape(-1, 3).cpu().numpy().astype(np.float64)
    else:
        host = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    if host.shape[0] < 1:
        raise ValueError("simulateRIR: no %s position" % what)
    if not (np.isfinite(host).all() and (host > 0).all() and (host < room[None, :]).all()):
        raise ValueError("simulateRIR: every %s position must lie strictly inside the room %s" % (what, room.tolist()))
    return host


def _positions(pos, room, what):
    """Host check (positions are small): [M, 3], strictly inside the room.  Returns an uploader, so that every argument is
    checked before anything touches the device."""
    host = _positions_host(pos, room, what)
    if isinstance(pos, torch.Tensor):
        return lambda dev: pos.detach().to(torch.float32).reshape(-1, 3)
    return lambda dev: torch.from_numpy(host.astype(np.float32)).to(dev)


def simulateRIR(room_sz, beta, pos_src, pos_rcv, nb_img, Tmax, fs, Tdiff=None, spkr_pattern="omni", mic_pattern="omni",
                orV_src=None, orV_rcv=None, c=343.0, *, seed=0):
    """RIRs [M_src, M_rcv, nSamples] float32 between every source and receiver position: the image-source method up to
    ``Tdiff`` (``nb_img`` images per axis), this project's diffuse tail from there to ``Tmax``, its noise
    drawn from ``seed``.  Only the ``"omni"`` patterns exist; ``orV_*`` are accepted and ignored under them."""
    _check_patterns(spkr_pattern, mic_pattern, pos_src, pos_rcv)
    as_numpy = not (isinstance(pos_src, torch.Tensor) or isinstance(pos_rcv, torch.Tensor))
    dev = next((p.device for p in (pos_src, pos_rcv) if isinstance(p, torch.Tensor)), torch.device("cuda:0"))
    room, bet, nb, nism, ns = _check_room(room_sz, beta, nb_img, Tmax, fs, Tdiff, c)
    src = _positions(pos_src, room, "source")
    rcv = _positions(pos_rcv, room, "receiver")
    src, rcv = src(dev), rcv(dev)
    rir = ops.rir_ism(src, rcv, room, bet, nb, nism, ns, fs, c)
    if ns > nism:
        ops.rir_tail(rir, src, rcv, room, bet, nism, fs, c, seed)
    return rir.cpu().numpy() if as_numpy else rir


def _check_patterns(spkr_pattern, mic_pattern, pos_src, pos_rcv):
    for name, pat in (("spkr_pattern", spkr_pattern), ("mic_pattern", mic_pattern)):
        if pat != "omni":
            raise NotImplementedError("simulateRIR: %s %r is not built (only 'omni')" % (name, pat))
    _reject_cpu_tensors(pos_src, pos_rcv)


def _check_room(room_sz, beta, nb_img, Tmax, fs, Tdiff, c):
    """simulateRIR's host checks of everything but the positions -> (room, beta, nb_img, nISM, nSamples)."""
    room = np.asarray(room_sz, dtype=np.float64).reshape(-1)
    bet = np.asarray(beta, dtype=np.float64).reshape(-1)
    if room.shape != (3,) or bet.shape != (6,) or not (room > 0).all() or (bet < 0).any() or (bet > 1).any():
        raise ValueError("simulateRIR: room_sz is 3 positive lengths and beta 6 coefficients in [0, 1]")
    nb = [int(v) for v in np.asarray(nb_img).reshape(-1)]
    if len(nb) != 3 or min(nb) < 1:
        raise ValueError("simulateRIR: nb_img is 3 positive counts, got %s" % (nb,))
    if not (Tmax > 0 and fs > 0 and c > 0 and (Tdiff is None or Tdiff > 0)):
        raise ValueError("simulateRIR: Tmax, Tdiff, fs and c must be positive")
    nism, ns = sample_counts(Tdiff, Tmax, fs)
    return room, bet, nb, nism, ns


def _upload_packed(arrays, dtype, dev):
    """Several small host arrays in ONE pinned buffer and one asynchronous copy -> their device views, in order."""
    flat = [np.ascontiguousarray(a, dtype=dtype).reshape(-1) for a in arrays]
    host = torch.from_numpy(np.concatenate(flat) if flat else np.zeros(0, dtype=dtype))
    if dev.type == "cuda":
        host = host.pin_memory()
    whole = host.to(dev, non_blocking=True)
    views, off = [], 0
    for a, f in zip(arrays, flat):
        views.append(whole[off:off + f.size].view(np.shape(a)))
        off += f.size
    return views


_RIR_SIGNATURE = inspect.signature(simulateRIR)


def simulateRIRBatch(jobs, out=None, *, _device=None):
    """``simulateRIR`` for several independent jobs in one launch set (fnssl_rir_ism_batch, fnssl_rir_tail_batch): ``jobs`` is a
    list of dicts or tuples of ``simulateRIR``'s arguments -> list of RIRs [M_src, M_rcv, nSamples], each bit for bit what
    ``simulateRIR`` gives the job alone, whatever else is in the batch.  Every host check of every job comes first (a refused
    job is named by its index and nothing has touched the device); then every position of every job goes up in one pinned
    buffer and one copy.  numpy in every job gives numpy out.  ``out``: the device tensors to write, one per job.
    ``_device`` (fnssl.scene): compute there and return device tensors whatever the positions are."""
    jobs = list(jobs)
    if not jobs:
        raise ValueError("simulateRIRBatch: no job")
    if out is not None and len(out) != len(jobs):
        raise ValueError("simulateRIRBatch: %d outputs for %d jobs" % (len(out), len(jobs)))
    recs, hosts, any_tensor, dev = [], [], False, None
    for k, job in enumerate(jobs):
        try:
            a = (_RIR_SIGNATURE.bind(**job) if isinstance(job, dict) else _RIR_SIGNATURE.bind(*job))
            a.apply_defaults()
            a = a.arguments
            _check_patterns(a["spkr_pattern"], a["mic_pattern"], a["pos_src"], a["pos_rcv"])
            room, bet, nb, nism, ns = _check_room(a["room_sz"], a["beta"], a["nb_img"], a["Tmax"], a["fs"], a["Tdiff"], a["c"])
            if nism > ops._lib.RIR_MAX_ISM_SAMPLES:
                raise ValueError("simulateRIR: nISM = %d samples (at most %d: the image-source part of one RIR is one LDS tile; "
                                 "use a shorter Tdiff)" % (nism, ops._lib.RIR_MAX_ISM_SAMPLES))
            src = _positions_host(a["pos_src"], room, "source")
            rcv = _positions_host(a["pos_rcv"], room, "receiver")
        except (ValueError, NotImplementedError, RuntimeError, TypeError) as e:
            err = type(e)("simulateRIRBatch: job %d: %s" % (k, e))
            err.job = k
            raise err from None
        for p in (a["pos_src"], a["pos_rcv"]):
            if isinstance(p, torch.Tensor):
                any_tensor, dev = True, dev or p.device
        hosts += [src, rcv]
        recs.append(dict(room_sz=room, beta=bet, nb_img=nb, nism=nism, nsamples=ns, fs=a["fs"], c=a["c"], seed=a["seed"]))
    dev = _device or dev or torch.device("cuda:0")
    views = _upload_packed(hosts, np.float32, dev)
    for k, rec in enumerate(recs):
        rec["pos_src"], rec["pos_rcv"] = views[2 * k], views[2 * k + 1]
    if out is None:
        sizes = [r["pos_src"].shape[0] * r["pos_rcv"].shape[0] * r["nsamples"] for r in recs]
        flat = torch.empty((sum(sizes),), dtype=torch.float32, device=dev)      # every sample is written: ISM part, then tail
        out, off = [], 0
        for r, size in zip(recs, sizes):
            out.append(flat[off:off + size].view(r["pos_src"].shape[0], r["pos_rcv"].shape[0], r["nsamples"]))
            off += size
    rirs = ops.rir_ism_batch(recs, list(out))
    ops.rir_tail_batch(recs, rirs)
    return rirs if any_tensor or _device is not None else [r.cpu().numpy() for r in rirs]


def _w_ini(npts, nsamples, timestamps, fs):
    if timestamps is None:
        fs = nsamples / npts
        timestamps = np.arange(npts)
    elif fs is None:
        raise ValueError("simulateTrajectory: timestamps need fs")
    ts = np.asarray(timestamps.detach().cpu().numpy() if isinstance(timestamps, torch.Tensor) else timestamps, dtype=np.float64)
    if ts.shape != (npts,):
        raise ValueError("simulateTrajectory: %d timestamps for %d RIRs" % (ts.size, npts))
    w = np.append((ts * fs).astype(np.int64), nsamples)
    return np.clip(w, 0, nsamples).astype(np.int32)


def simulateTrajectoryBatch(source_signals, RIRs, timestamps=None, fs=None):
    """``simulateTrajectory`` for several independent (signal, RIR set) pairs, FNSSL_RIR_TRAJ_MAX_BATCH (16) per launch (a
    scene: 2 sources x {full, direct path, VAD}; a batch of scenes: as many groups of 16 as it takes, in order);
    ``timestamps`` is None, one array for all, or a list with one entry per pair."""
    n = len(source_signals)
    if n != len(RIRs) or n < 1:
        raise ValueError("simulateTrajectoryBatch: %d signals and %d RIR sets" % (n, len(RIRs)))
    _reject_cpu_tensors(*source_signals, *RIRs)
    per_item = isinstance(timestamps, (list, tuple)) and len(timestamps) == n and not np.isscalar(timestamps[0])
    as_numpy = not any(isinstance(a, torch.Tensor) for a in list(source_signals) + list(RIRs))
    dev = next((a.device for a in list(source_signals) + list(RIRs) if isinstance(a, torch.Tensor)), torch.device("cuda:0"))
    xs, rs, ws = [], [], []
    for k in range(n):
        x = source_signals[k] if isinstance(source_signals[k], torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(source_signals[k], dtype=np.float32)).to(dev)
        r = RIRs[k] if isinstance(RIRs[k], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(RIRs[k], dtype=np.float32)).to(dev)
        x = x.to(torch.float32).reshape(-1)
        if r.ndim != 3:
            raise ValueError("simulateTrajectory: RIRs are [nPts, M_rcv, lenRIR], got %s" % (tuple(r.shape),))
        w = _w_ini(r.shape[0], x.numel(), timestamps[k] if per_item else timestamps, fs)
        xs.append(x)
        rs.append(r.to(torch.float32))
        ws.append(w)
    ws = _upload_packed(ws, np.int32, dev)                                 # every w_ini in one copy
    ys = ops.rir_trajectory_batch(xs, rs, ws)                              # groups of FNSSL_RIR_TRAJ_MAX_BATCH, in order
    return [y.cpu().numpy() for y in ys] if as_numpy else ys


def simulateTrajectory(source_signal, RIRs, timestamps=None, fs=None):
    """Filter ``source_signal`` [nSamples] through the RIRs [nPts, M_rcv, lenRIR] of a moving source -> [nSamples + lenRIR - 1,
    M_rcv]: sample s is radiated from point p when w_ini[p] <= s < w_ini[p + 1], w_ini = append(int(timestamps fs), nSamples)
    (``timestamps=None``: the points share the signal equally).  gpuRIR's segment / convolve / overlap-add as one gather:
    y[t, m] = sum_k RIRs[p(t - k), m, k] x[t - k]."""
    return simulateTrajectoryBatch([source_signal], [RIRs], timestamps, fs)[0]
