"""The rest of the reference's data stage on the device, under the names and argument order of its ``Dataset.py``:
``acoustic_power``, ``NoiseDataset.gen_diffuse_noise`` / ``mix_signals`` (Habets' arbitrary noise field generator) and
``AcousticScene.simulate``.  The kernels are csrc/scene.hip (and csrc/rir.hip through fnssl/rir.py); the model is DESIGN.md
§18.  Drop-in::

    Dataset.AcousticScene.simulate = fnssl.scene.simulate
    Dataset.NoiseDataset.gen_diffuse_noise = staticmethod(fnssl.scene.gen_diffuse_noise)
    Dataset.NoiseDataset.mix_signals = staticmethod(fnssl.scene.mix_signals)

and for whole training batches in one launch set::

    Dataset.RandomTrajectoryDataset.get_batch = fnssl.scene.get_batch

numpy in gives numpy out, float32 (computed on ``cuda:0``, one host copy each way); ROCm tensors in give tensors out on their
device with no host round trip; CPU tensors are rejected like everywhere else in this package.  Built: the ``'spherical'``
field, the ``'cholesky'`` method, ``'omni'`` patterns, ``nfft = 256``, at most 16 microphones and 4 sources.

The labels of a training batch (csrc/labels.hip): ``trajectory_doa`` (the interpolation and
``cart2sph`` of ``getRandomScene``), ``Segmenting_SRPDNN`` (the reference's transform, usable in ``dataset.transforms``),
``segment_batch`` (the transform and the padded ``gts`` dict for a whole batch in one launch set) and ``training_batch``
(draw, simulate, segment -> ``(mic, gts)`` for ``training_step``).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops, rir
from .rir import _reject_cpu_tensors

__all__ = ["acoustic_power", "gen_diffuse_noise", "mix_signals", "simulate", "simulate_batch", "get_batch", "trajectory_doa",
           "Segmenting_SRPDNN", "segment_batch", "training_batch"]


def _is_t(a):
    return isinstance(a, torch.Tensor)


def _device(*xs):
    return next((a.device for a in xs if _is_t(a)), torch.device("cuda:0"))


def _up(a, dev, dtype=torch.float32):
    if _is_t(a):
        return a.detach().to(dtype)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32 if dtype == torch.float32 else np.float64)).to(dev)


def _check_field(nfft, m):
    if int(nfft) != _lib.ANF_NFFT:
        raise ValueError("fnssl.scene: nfft = %d (only %d is built)" % (int(nfft), _lib.ANF_NFFT))
    if not 1 <= m <= _lib.ANF_MAX_MICS:
        raise ValueError("fnssl.scene: %d microphones (1 .. %d)" % (m, _lib.ANF_MAX_MICS))


def acoustic_power(s):
    """Acoustic power of ``s`` [n] after removing the silences: the mean square of the windows of 512 every 256 that exceed
    0.01 x the largest.  A numpy array gives a float32 scalar, a ROCm tensor a 0-dim tensor.  ``n < 512`` (no window) is an
    error, as in the reference."""
    _reject_cpu_tensors(s)
    n = int(s.numel() if _is_t(s) else np.asarray(s).size)
    if n < 512:
        raise ValueError("acoustic_power: %d samples (at least one window of 512)" % n)
    p = ops.scene_power(_up(s, _device(s)).reshape(-1, 1))[0]
    return p if _is_t(s) else p.cpu().numpy()[()]


def _factor_of(dc):
    return ops.anf_factor(dc)[0]


def mix_signals(noise, DC, method="cholesky"):
    """noise [L, M] (or [B, L, M]) mutually independent signals, DC [M, M, 129] (or [B, M, M, 129]) the desired coherence per
    bin -> [L + ((-L) mod 64), M] signals with that coherence.  The reference's own output shape: the whole last hop is
    kept.  A bin whose matrix is not positive definite raises ``numpy.linalg.LinAlgError`` naming it."""
    if method != "cholesky":
        raise NotImplementedError("mix_signals: method %r is not built (only 'cholesky')" % (method,))
    _reject_cpu_tensors(noise, DC)
    as_numpy = not (_is_t(noise) or _is_t(DC))
    dshape = tuple(DC.shape)
    nshape = tuple(noise.shape)
    if len(nshape) not in (2, 3) or len(dshape) not in (3, len(nshape) + 1) or (len(dshape) == 4 and dshape[0] != nshape[0]):
        raise ValueError("mix_signals: noise is [L, M] or [B, L, M] and DC [M, M, bins] or [B, M, M, bins], got %s and %s" % (nshape, dshape))
    _check_field(2 * (dshape[-1] - 1), nshape[-1])
    if dshape[-2] != nshape[-1] or dshape[-3] != nshape[-1]:
        raise ValueError("mix_signals: DC %s for %d signals" % (dshape, nshape[-1]))
    dev = _device(noise, DC)
    x = _up(noise, dev)
    dc = _up(DC, dev, torch.float64)
    y = ops.anf_mix(x if x.ndim == 3 else x[None], _factor_of(dc if dc.ndim == 4 else dc[None]))
    y = y if len(nshape) == 3 else y[0]
    return y.cpu().numpy() if as_numpy else y


def gen_diffuse_noise(noise, T, fs, mic_pos, nfft=256, c=343.0, type_nf="spherical"):
    """Diffuse noise of a spherically isotropic field at the microphones ``mic_pos`` [M, 3] from the flat ``noise`` [>= M L], L =
    int(T fs): the vector's mean is removed, signal m is noise[m L : (m + 1) L], the coherence is sinc(w d / c) and the mixing
    ``mix_signals``.  A leading batch dimension on ``noise`` [B, .] and / or ``mic_pos`` [B, M, 3] is accepted.
    Returns [L + ((-L) mod 64), M] (the reference's shape; ``simulate`` slices it)."""
    if type_nf != "spherical":
        raise NotImplementedError("gen_diffuse_noise: noise field %r is not built (only 'spherical')" % (type_nf,))
    _reject_cpu_tensors(noise, mic_pos)
    as_numpy = not (_is_t(noise) or _is_t(mic_pos))
    m = int(mic_pos.shape[-2])
    _check_field(nfft, m)
    length = int(T * fs)
    nd = noise.ndim
    if nd not in (1, 2) or mic_pos.ndim not in (2, 3) or mic_pos.shape[-1] != 3 or noise.shape[-1] < m * length or length < 1:
        raise ValueError("gen_diffuse_noise: noise %s, mic_pos %s for %d signals of %d samples" % (tuple(noise.shape), tuple(mic_pos.shape), m, length))
    dev = _device(noise, mic_pos)
    v = _up(noise, dev)
    v = v if nd == 2 else v[None]
    if v.stride(1) != 1:
        v = v.contiguous()
    pos = _up(mic_pos, dev, torch.float64)
    pos = pos if pos.ndim == 3 else pos[None]
    if pos.shape[0] not in (1, v.shape[0]) and v.shape[0] != 1:
        raise ValueError("gen_diffuse_noise: %d noise vectors for %d microphone sets" % (v.shape[0], pos.shape[0]))
    if v.shape[0] == 1 and pos.shape[0] > 1:
        v = v.expand(pos.shape[0], -1)
    cfac = _factor_of(ops.anf_coherence(pos, fs, nfft, c))
    mean = ops.anf_mean(v)
    x = v[:, :m * length].unflatten(1, (m, length)).transpose(1, 2)          # [B, L, M] in place: signal m is a row of the vector
    y = ops.anf_mix(x, cfac, mean, nfft)
    y = y if (nd == 2 or mic_pos.ndim == 3) else y[0]
    return y.cpu().numpy() if as_numpy else y


def _rir_times(scene):
    """(Tdiff, Tmax, nb_img) of a scene's full RIRs, as the reference's simulate() chooses them."""
    if scene.T60 == 0:
        return 0.1, 0.1, [1, 1, 1]
    Tdiff = rir.att2t_SabineEstimator(12, scene.T60)                  # image sources until the RIRs have decayed 12 dB
    Tmax = rir.att2t_SabineEstimator(40, scene.T60)                   # the diffuse model until 40 dB
    if scene.T60 < 0.15:
        Tdiff = Tmax
    return Tdiff, Tmax, rir.t2n(Tdiff, scene.room_sz)


def simulate(scene, *, seed=None, keep=False):
    """``AcousticScene.simulate`` on any object with its attributes (room_sz, T60, beta, noise_signal, SNR, source_signal, fs,
    array_setup, mic_pos, timestamps, traj_pts, t and optionally source_vad): the microphone signals [len(t), M].  Sets
    ``dp_mic_signals_sources`` [n, M, S] and, with ``source_vad``, ``mic_vad_sources`` [n, S] and ``mic_vad`` [n] (bool), and
    fills ``noise_signal`` when it was None, as the reference does (both of its variants).

    Every source's RIRs run on the current stream, all 2 S (with VAD 3 S) trajectory mixings are ONE launch, then two power
    calls and one finish call; nothing is read back on the way.  ``seed``: source s draws its diffuse tail from ``seed + s``
    (the tail's key is (seed, point, receiver, t): equal seeds would give two sources the same tail noise).  ``seed=None``
    draws the base from ``np.random.randint`` — it consumes numpy's global stream once, before the noise is drawn.
    ``keep=True`` returns (mic_signals, parts): the per-source signals, the noise used, both power vectors, g and the VAD
    trajectories as the device stored them."""
    pattern = getattr(scene.array_setup, "mic_pattern", "omni")
    if pattern != "omni":
        raise NotImplementedError("simulate: mic_pattern %r is not built (only 'omni')" % (pattern,))
    has_vad = hasattr(scene, "source_vad")
    ins = [scene.source_signal, scene.traj_pts, scene.mic_pos, scene.noise_signal] + ([scene.source_vad] if has_vad else [])
    _reject_cpu_tensors(*ins)
    as_numpy = not any(_is_t(a) for a in ins)
    dev = _device(*ins)
    n = len(scene.t)
    nsrc = int(scene.traj_pts.shape[-1])
    m = int(scene.mic_pos.shape[0])
    if not 1 <= nsrc <= _lib.SCENE_MAX_SOURCES:
        raise ValueError("simulate: %d sources (1 .. %d)" % (nsrc, _lib.SCENE_MAX_SOURCES))
    if n < 512:
        raise ValueError("simulate: %d samples (acoustic_power needs one window of 512)" % n)
    Tdiff, Tmax, nb_img = _rir_times(scene)
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 31 - 1))
    src = _up(scene.source_signal, dev)
    pts = _up(scene.traj_pts, dev)
    mic_pos = _up(scene.mic_pos, dev)
    vad_in = _up(scene.source_vad, dev) if has_vad else None
    orv = scene.array_setup.mic_orV
    sigs, rirs = [], []
    dp_rirs = []
    for s in range(nsrc):
        p = pts[:, :, s]
        full = rir.simulateRIR(scene.room_sz, scene.beta, p, mic_pos, nb_img, Tmax, scene.fs, Tdiff=Tdiff, orV_rcv=orv,
                               mic_pattern=pattern, seed=seed + s)
        dp = rir.simulateRIR(scene.room_sz, scene.beta, p, mic_pos, [1, 1, 1], 0.1, scene.fs, orV_rcv=orv, mic_pattern=pattern)
        x = src[:, s].contiguous()
        sigs += [x, x]
        rirs += [full, dp]
        dp_rirs.append(dp)
    if has_vad:
        for s in range(nsrc):
            sigs.append(vad_in[:, s].contiguous())
            rirs.append(dp_rirs[s])
    ys = rir.simulateTrajectoryBatch(sigs, rirs, timestamps=scene.timestamps, fs=scene.fs)
    if min(y.shape[0] for y in ys) < n:
        raise ValueError("simulate: the source signals give %d samples, len(t) = %d" % (min(y.shape[0] for y in ys), n))
    full_sig, dp_sig = ys[0:2 * nsrc:2], ys[1:2 * nsrc:2]
    vads = ys[2 * nsrc:] if has_vad else None

    if scene.noise_signal is None:
        drawn = np.random.standard_normal((n, m))
        noise = _up(drawn, dev)
        scene.noise_signal = drawn if as_numpy else noise
    else:
        noise = _up(scene.noise_signal, dev)
    if noise.ndim != 2 or noise.shape[1] != m or noise.shape[0] < n:
        raise ValueError("simulate: noise_signal %s for [>= %d, %d]" % (tuple(noise.shape), n, m))
    power = ops.scene_power(dp_sig, n)
    power_noise = ops.scene_power([noise], noise.shape[0])            # over the WHOLE noise, as the reference does
    fin = ops.scene_finish(full_sig, noise, power, power_noise, float(scene.SNR), n, vads)

    host = (lambda a: a.cpu().numpy()) if as_numpy else (lambda a: a)
    scene.dp_mic_signals_sources = host(torch.stack([a[:n] for a in dp_sig], dim=2))
    if has_vad:
        scene.mic_vad_sources = host(fin["vad_sources"].bool())
        scene.mic_vad = host(fin["vad"].bool())
    mic = host(fin["mic"])
    if not keep:
        return mic
    parts = {"mic_signals_sources": full_sig, "dp_mic_signals_sources": dp_sig, "noise": noise, "power": power,
             "power_noise": power_noise, "g": fin["g"], "seed": seed, "rirs": rirs[0:2 * nsrc:2], "dp_rirs": dp_rirs}
    if has_vad:
        parts.update(vad_signals=vads, vad_max=fin["vmax"])
    return mic, parts


def _host_f32(a):
    """A small array (positions) on the host in float32, the values ``simulate`` uploads."""
    if _is_t(a):
        return a.detach().to(torch.float32).cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def _scene_shape(scene):
    """The host checks ``simulate`` makes on one scene before it touches the device -> its facts."""
    pattern = getattr(scene.array_setup, "mic_pattern", "omni")
    if pattern != "omni":
        raise NotImplementedError("mic_pattern %r is not built (only 'omni')" % (pattern,))
    has_vad = hasattr(scene, "source_vad")
    ins = [scene.source_signal, scene.traj_pts, scene.mic_pos, scene.noise_signal] + ([scene.source_vad] if has_vad else [])
    _reject_cpu_tensors(*ins)
    n, nsrc, m = len(scene.t), int(scene.traj_pts.shape[-1]), int(scene.mic_pos.shape[0])
    if not 1 <= nsrc <= _lib.SCENE_MAX_SOURCES:
        raise ValueError("%d sources (1 .. %d)" % (nsrc, _lib.SCENE_MAX_SOURCES))
    if n < 512:
        raise ValueError("%d samples (acoustic_power needs one window of 512)" % n)
    noise = scene.noise_signal
    if noise is not None and (noise.ndim != 2 or noise.shape[1] != m or noise.shape[0] < n):
        raise ValueError("noise_signal %s for [>= %d, %d]" % (tuple(noise.shape), n, m))
    return {"pattern": pattern, "has_vad": has_vad, "n": n, "nsrc": nsrc, "m": m, "fs": float(scene.fs),
            "tensors": any(_is_t(a) for a in ins), "device": next((a.device for a in ins if _is_t(a)), None)}


def simulate_batch(scenes, *, seeds=None, keep=False):
    """``simulate`` for a batch of independent scenes in ONE launch set whose size does not grow with the batch (until a
    descriptor block is full) -> the microphone signals [B, n, M], every scene bit for bit what
    ``simulate(scene, seed=seeds[b])`` gives it alone.  Sets ``dp_mic_signals_sources``, ``mic_vad_sources``, ``mic_vad`` and
    a drawn ``noise_signal`` on every scene as ``simulate`` does (``mic_vad`` and ``mic_vad_sources`` from the batch's VAD
    tensors, ``dp_mic_signals_sources`` stacked per scene from its direct-path signals, as ``simulate`` stacks them).

    Scenes may differ in room, beta, T60, SNR, source count, trajectory points, timestamps and noise length; they share fs,
    M, len(t) and the presence of ``source_vad`` (a mixed batch raises ``ValueError`` naming the first offending scene before
    anything touches the device).  ``seeds=None`` draws as B ``simulate`` calls in order would: per scene first the seed,
    then its noise if None.  numpy in every scene gives numpy out.  ``keep=True`` returns (mic, [parts of scene b])."""
    scenes = list(scenes)
    if not scenes:
        raise ValueError("simulate_batch: no scene")
    facts = []
    for b, sc in enumerate(scenes):
        try:
            facts.append(_scene_shape(sc))
        except (ValueError, NotImplementedError, RuntimeError) as e:
            raise type(e)("simulate_batch: scene %d: %s" % (b, e)) from None
        for key, what in (("m", "microphones"), ("fs", "Hz"), ("n", "samples (len(t))")):
            if facts[b][key] != facts[0][key]:
                raise ValueError("simulate_batch: scene %d: %g %s, scene 0 has %g (a batch shares M, fs and len(t))"
                                 % (b, facts[b][key], what, facts[0][key]))
        if facts[b]["has_vad"] != facts[0]["has_vad"]:
            raise ValueError("simulate_batch: scene %d: source_vad is %s, in scene 0 it is %s (a batch shares its presence)"
                             % (b, *("present" if f["has_vad"] else "absent" for f in (facts[b], facts[0]))))
    if seeds is not None and len(seeds) != len(scenes):
        raise ValueError("simulate_batch: %d seeds for %d scenes" % (len(seeds), len(scenes)))
    n, m, has_vad, fs = facts[0]["n"], facts[0]["m"], facts[0]["has_vad"], scenes[0].fs
    as_numpy = not any(f["tensors"] for f in facts)
    dev = next((f["device"] for f in facts if f["device"] is not None), torch.device("cuda:0"))

    # numpy's stream, as B simulate() calls in order consume it
    seed_of, drawn = [], []
    for b, sc in enumerate(scenes):
        seed_of.append(int(np.random.randint(0, 2 ** 31 - 1)) if seeds is None else int(seeds[b]))
        drawn.append(np.random.standard_normal((n, m)) if sc.noise_signal is None else None)

    # every RIR of the batch: per source the full RIRs and the direct-path RIRs
    jobs, scene_of_job = [], []
    for b, sc in enumerate(scenes):
        Tdiff, Tmax, nb_img = _rir_times(sc)
        scene_of_job += [b] * (2 * facts[b]["nsrc"])
        pts, mic_pos, orv = _host_f32(sc.traj_pts), _host_f32(sc.mic_pos), sc.array_setup.mic_orV
        for s in range(facts[b]["nsrc"]):
            common = dict(room_sz=sc.room_sz, beta=sc.beta, pos_src=pts[:, :, s], pos_rcv=mic_pos, fs=sc.fs, orV_rcv=orv,
                          mic_pattern=facts[b]["pattern"])
            jobs.append(dict(common, nb_img=nb_img, Tmax=Tmax, Tdiff=Tdiff, seed=seed_of[b] + s))
            jobs.append(dict(common, nb_img=[1, 1, 1], Tmax=0.1))
    try:
        all_rirs = rir.simulateRIRBatch(jobs, _device=dev)
    except (ValueError, NotImplementedError) as e:
        raise type(e)("simulate_batch: scene %d: %s" % (scene_of_job[e.job], e)) from None

    # every mixing of the batch: per scene 2 S (with VAD 3 S) pairs, in groups of 16
    sigs, rirs, stamps, first, k = [], [], [], [], 0
    for b, sc in enumerate(scenes):
        nsrc = facts[b]["nsrc"]
        src = _up(sc.source_signal, dev)
        first.append(len(sigs))
        for s in range(nsrc):
            x = src[:, s].contiguous()
            sigs += [x, x]
            rirs += [all_rirs[k + 2 * s], all_rirs[k + 2 * s + 1]]
        if has_vad:
            vad_in = _up(sc.source_vad, dev)
            for s in range(nsrc):
                sigs.append(vad_in[:, s].contiguous())
                rirs.append(all_rirs[k + 2 * s + 1])
        stamps += [sc.timestamps] * (len(sigs) - first[b])
        k += 2 * nsrc
    ys = rir.simulateTrajectoryBatch(sigs, rirs, timestamps=stamps, fs=fs)
    short = min(y.shape[0] for y in ys)
    if short < n:
        raise ValueError("simulate_batch: the source signals give %d samples, len(t) = %d" % (short, n))

    descs, noises = [], []
    for b, sc in enumerate(scenes):
        nsrc, y = facts[b]["nsrc"], ys[first[b]:]
        if drawn[b] is not None:
            noise = _up(drawn[b], dev)
            sc.noise_signal = drawn[b] if as_numpy else noise
        else:
            noise = _up(sc.noise_signal, dev)
        noises.append(noise)
        descs.append({"sig": y[0:2 * nsrc:2], "dp": y[1:2 * nsrc:2], "noise": noise, "snr_db": float(sc.SNR),
                      "vads": y[2 * nsrc:3 * nsrc] if has_vad else None})
    fin = ops.scene_mix_batch(descs, n)

    host = (lambda a: a.cpu().numpy()) if as_numpy else (lambda a: a)
    vad_all = host(fin["vad"].bool()) if has_vad else None
    parts, k = [], 0
    for b, sc in enumerate(scenes):
        nsrc, d = facts[b]["nsrc"], descs[b]
        sc.dp_mic_signals_sources = host(torch.stack([a[:n] for a in d["dp"]], dim=2))
        if has_vad:
            sc.mic_vad_sources = host(fin["vad_sources"][b].bool())
            sc.mic_vad = vad_all[b]
        part = {"mic_signals_sources": d["sig"], "dp_mic_signals_sources": d["dp"], "noise": noises[b], "power": fin["power"][b],
                "power_noise": fin["power_noise"][b], "g": fin["g"][b:b + 1], "seed": seed_of[b],
                "rirs": all_rirs[k:k + 2 * nsrc:2], "dp_rirs": all_rirs[k + 1:k + 2 * nsrc:2]}
        if has_vad:
            part.update(vad_signals=d["vads"], vad_max=fin["vmax"][b])
        parts.append(part)
        k += 2 * nsrc
    mic = host(fin["mic"])
    return (mic, parts) if keep else mic


def get_batch(dataset, idx1, idx2):
    """The reference's ``RandomTrajectoryDataset.get_batch`` with one ``simulate_batch`` call for the whole batch:
    ``dataset.getRandomScene(idx)`` for idx1 <= idx < idx2, the simulation, ``dataset.transforms`` per scene if any ->
    (the stacked signals, the list of scenes)."""
    scenes = [dataset.getRandomScene(idx) for idx in range(idx1, idx2)]
    mics = simulate_batch(scenes)
    sigs = []
    for b, mic in enumerate(mics):
        for t in getattr(dataset, "transforms", None) or ():
            mic, scenes[b] = t(mic, scenes[b])
        sigs.append(mic)
    return (torch.stack(sigs) if _is_t(sigs[0]) else np.stack(sigs)), scenes


# ------------------------------------------------------------------------------------------------------------------------
# labels: trajectory -> DOA, the Segmenting_SRPDNN transform, the padded gts dict
# ------------------------------------------------------------------------------------------------------------------------
def num_windows(L, K, step):
    """The reference's ``N_w = floor(L / step - K / step + 1)``, evaluated in float64 as it does (where ``step`` divides
    ``L - K`` the two rounded quotients may give one window fewer than ``(L - K) // step + 1``; never one more)."""
    return int(np.floor(L / step - K / step + 1))


def window_times(L, K, step, fs):
    """The reference's ``tw = arange(0, L - K, step) / fs``: ``N_w`` entries, ``N_w - 1`` where ``step`` divides ``L - K``."""
    return np.arange(0, (L - K), step) / fs


def _host_timestamps(ts, who):
    """The timestamps as given, checked on the host: [P], finite, increasing (a device tensor's P numbers are copied down for
    it: np.interp's bisection means nothing otherwise, and the kernel would give wrong labels silently)."""
    host = ts.detach().cpu().numpy() if _is_t(ts) else ts
    host = np.asarray(host, dtype=np.float64)
    if host.ndim != 1 or host.size < 1 or not np.all(np.isfinite(host)) or np.any(np.diff(host) <= 0):
        raise ValueError("%s: timestamps must be [P] finite and increasing" % who)
    return ts if _is_t(ts) else host


def trajectory_doa(traj_pts, timestamps, n, fs, array_pos):
    """What ``getRandomScene`` does after drawing its trajectory points: ``trajectory[:, i, s] = np.interp(arange(n) / fs,
    timestamps, traj_pts[:, i, s])`` and ``DOA[:, :, s] = cart2sph(trajectory[:, :, s] - array_pos)[:, 1:3]`` (elevation from
    the z axis, azimuth) -> (trajectory [n, 3, S], DOA [n, 2, S]), float64, computed on the device in double."""
    _reject_cpu_tensors(traj_pts, timestamps, array_pos)
    as_numpy = not (_is_t(traj_pts) or _is_t(timestamps))
    dev = _device(traj_pts, timestamps)
    pos = np.asarray(array_pos.detach().cpu().numpy() if _is_t(array_pos) else array_pos, dtype=np.float64).reshape(-1)
    if pos.shape != (3,) or tuple(traj_pts.shape[1:2]) != (3,) or len(traj_pts.shape) != 3:
        raise ValueError("trajectory_doa: traj_pts is [P, 3, S] and array_pos [3], got %s and %s" % (tuple(traj_pts.shape), pos.shape))
    if not 1 <= traj_pts.shape[2] <= _lib.SCENE_MAX_SOURCES:
        raise ValueError("trajectory_doa: %d sources (1 .. %d)" % (traj_pts.shape[2], _lib.SCENE_MAX_SOURCES))
    if int(n) < 1:
        raise ValueError("trajectory_doa: %d samples" % int(n))
    ts = _host_timestamps(timestamps, "trajectory_doa")
    item = {"traj_pts": _up(traj_pts, dev, torch.float64), "timestamps": _up(ts, dev, torch.float64), "n": int(n), "fs": float(fs),
            "array_pos": pos}
    traj, doa = ops.scene_doa_batch([item])[0]
    return (traj.cpu().numpy(), doa.cpu().numpy()) if as_numpy else (traj, doa)


def _vad_u8(v, dev):
    """A VAD (bool / 0-1 numbers) as a uint8 device tensor."""
    if _is_t(v):
        return v if v.dtype in (torch.uint8, torch.bool) else (v != 0)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v) != 0).view(np.uint8)).to(dev)


class Segmenting_SRPDNN(object):
    """The reference's segmenting transform (``Dataset.py``), on the device: ``__call__(x, acoustic_scene)`` cuts the scene's
    ``DOA`` [L, 2, S] into ``N_w = floor(L / step - K / step + 1)`` windows of ``K`` every ``step`` and sets ``DOAw`` [N_w, 2, S]
    (the window means, unwrapped where the azimuth jumps by more than pi inside a window and folded back into (-pi, pi]),
    ``mic_vad`` [N_w, K] and ``mic_vad_sources`` [N_w, K, S] (zero-extended to ``L``; only if the scene has them) and ``tw``
    (numpy, as the reference computes it).  A scene held in ROCm tensors keeps tensors (``DOAw`` float64, the VADs uint8); a
    scene held in numpy gets numpy float64, the reference's dtypes.  ``window`` is stored and, as in the reference, never
    applied."""

    BAD_WINDOW = 'window must be a NumPy window function or a Numpy vector with length K'      # the reference's message

    def __init__(self, K, step, window=None):
        self.K, self.step = K, step
        self.w = self._window(K, window)

    @classmethod
    def _window(cls, K, window):
        """None -> ones; a function of K -> its value; a vector of length K -> itself; anything else raises."""
        if window is None:
            return np.ones(K)
        try:
            w = window(K) if callable(window) else window if len(window) == K else None
        except Exception:
            w = None
        if w is None:
            raise Exception(cls.BAD_WINDOW)
        return w

    def __call__(self, x, acoustic_scene):
        sc = acoustic_scene
        L = int(x.shape[0])
        if self.K > L:
            raise Exception('The window size can not be larger than the signal length ({})'.format(L))
        elif self.step > L:
            raise Exception('The window step can not be larger than the signal length ({})'.format(L))
        vads = [getattr(sc, name) for name in ("mic_vad_sources", "mic_vad") if hasattr(sc, name)]
        _reject_cpu_tensors(x, sc.DOA, *vads)
        as_numpy = not any(_is_t(a) for a in [sc.DOA] + vads)
        dev = _device(sc.DOA, *vads, x)
        nsrc = int(sc.DOA.shape[2])
        nw = num_windows(L, self.K, self.step)
        if not 1 <= nsrc <= _lib.SCENE_MAX_SOURCES:
            raise ValueError("Segmenting_SRPDNN: %d sources (1 .. %d)" % (nsrc, _lib.SCENE_MAX_SOURCES))
        for name in ("mic_vad_sources", "mic_vad"):
            if hasattr(sc, name) and getattr(sc, name).shape[0] > L:
                raise ValueError("Segmenting_SRPDNN: %s has %d samples, the signal %d" % (name, getattr(sc, name).shape[0], L))
        if hasattr(sc, "mic_vad_sources") and tuple(sc.mic_vad_sources.shape[1:]) != (nsrc,):
            raise ValueError("Segmenting_SRPDNN: mic_vad_sources %s for %d sources" % (tuple(sc.mic_vad_sources.shape), nsrc))
        if len(vads) == 2 and vads[0].shape[0] != vads[1].shape[0]:
            raise ValueError("Segmenting_SRPDNN: mic_vad_sources has %d samples, mic_vad %d" % (vads[0].shape[0], vads[1].shape[0]))
        item = {"ns": nsrc, "doa": _up(sc.DOA, dev, torch.float64)}
        for name, key in (("mic_vad_sources", "vad_sources"), ("mic_vad", "vad")):
            if hasattr(sc, name):
                item[key] = _vad_u8(getattr(sc, name), dev)
        out = ops.scene_segment_batch([item], L, self.K, self.step, nw, nsrc, with_vad=len(vads) > 0)
        host = (lambda a: a.cpu().numpy().astype(np.float64)) if as_numpy else (lambda a: a)
        sc.DOAw = host(out["doa"][0])
        if hasattr(sc, "mic_vad"):
            sc.mic_vad = host(out["vad"][0])
        if hasattr(sc, "mic_vad_sources"):
            sc.mic_vad_sources = host(out["vad_sources"][0])
        sc.tw = window_times(L, self.K, self.step, sc.fs)
        return x, sc


def _label_facts(b, sc, mic, K, step, with_pos):
    """The host checks of one scene of ``segment_batch`` -> its facts; nothing touches the device."""
    dp, vs, v = sc.dp_mic_signals_sources, sc.mic_vad_sources, sc.mic_vad
    ins = [mic, dp, vs, v] + ([sc.traj_pts] if with_pos else [sc.DOA])
    try:
        _reject_cpu_tensors(*ins)
    except RuntimeError as e:
        raise RuntimeError("segment_batch: scene %d: %s" % (b, e)) from None
    if len(mic.shape) != 2 or len(dp.shape) != 3 or len(vs.shape) != 2 or len(v.shape) != 1:
        raise ValueError("segment_batch: scene %d: signals %s, dp_mic_signals_sources %s, mic_vad_sources %s, mic_vad %s for [L, M], "
                         "[L, M, S], [n, S], [n]" % (b, tuple(mic.shape), tuple(dp.shape), tuple(vs.shape), tuple(v.shape)))
    L, m, nsrc = int(mic.shape[0]), int(mic.shape[1]), int(vs.shape[1])
    if K > L:
        raise ValueError("segment_batch: scene %d: the window size %d is larger than the signal length %d" % (b, K, L))
    if step > L:
        raise ValueError("segment_batch: scene %d: the window step %d is larger than the signal length %d" % (b, step, L))
    if vs.shape[0] > L or v.shape[0] > L:
        raise ValueError("segment_batch: scene %d: a VAD of %d samples for a signal of %d" % (b, max(vs.shape[0], v.shape[0]), L))
    if v.shape[0] != vs.shape[0]:
        raise ValueError("segment_batch: scene %d: mic_vad_sources has %d samples, mic_vad %d" % (b, vs.shape[0], v.shape[0]))
    if tuple(dp.shape) != (L, m, nsrc):
        raise ValueError("segment_batch: scene %d: dp_mic_signals_sources %s for [%d, %d, %d]" % (b, tuple(dp.shape), L, m, nsrc))
    need = (num_windows(L, K, step) - 1) * step + K
    if with_pos:
        pts = sc.traj_pts
        if len(pts.shape) != 3 or pts.shape[1] != 3 or pts.shape[2] != nsrc or len(sc.t) < need:
            raise ValueError("segment_batch: scene %d: traj_pts %s, len(t) = %d for %d sources and %d samples"
                             % (b, tuple(pts.shape), len(sc.t), nsrc, need))
        _host_timestamps(sc.timestamps, "segment_batch: scene %d" % b)
    elif sc.DOA is None or len(sc.DOA.shape) != 3 or tuple(sc.DOA.shape[1:]) != (2, nsrc) or sc.DOA.shape[0] < need:
        raise ValueError("segment_batch: scene %d: DOA %s for [>= %d, 2, %d] (pass array_pos to compute it on the device)"
                         % (b, None if sc.DOA is None else tuple(sc.DOA.shape), need, nsrc))
    return {"L": L, "m": m, "nsrc": nsrc, "fs": float(sc.fs), "tensors": any(_is_t(a) for a in ins),
            "device": next((a.device for a in ins if _is_t(a)), None)}


def segment_batch(mics, scenes, K, step, max_source=None, array_pos=None):
    """``Segmenting_SRPDNN(K, step)`` on every scene and the ``gts`` dict of ``FixTrajectoryDataset.__getitem__``, zero-padded to
    ``max_source`` sources and stacked, for the whole batch in one launch set.  ``mics`` [B, L, M] (or B signals
    [L, M]); ``scenes``: objects with ``DOA`` [L, 2, S_b], ``mic_vad_sources`` [n, S_b], ``mic_vad`` [n], ``dp_mic_signals_sources``
    [L, M, S_b] and ``fs`` — what ``simulate_batch`` leaves behind; the scenes are not modified.  Returns ``gts``::

        doa [B, N_w, 2, Smax] float64      vad_sources [B, N_w, K, Smax] uint8      vad_count [B, N_w, Smax] int32 (ones per window)
        dp_signal [B, L, M, Smax] float32  mic_vad [B, N_w, K] uint8                num_source [B]
        array_setup [B, M, 3] (the scenes' ``array_setup.mic_pos``; None if a scene has none)

    With ``array_pos`` (one [3] per scene) the DOA is computed on the device from ``traj_pts`` / ``timestamps`` / ``len(t)`` as
    ``trajectory_doa`` does and ``scene.DOA`` is not read (it may be None).  ``max_source`` defaults to the batch's largest
    source count; a scene with more raises ``ValueError`` naming it, as do scenes that differ in L, M or fs, a VAD longer than
    L, ``K`` or ``step`` > L, and a CPU tensor (``RuntimeError``) — all before anything touches the device.  numpy in every
    scene gives numpy out."""
    scenes = list(scenes)
    if not scenes:
        raise ValueError("segment_batch: no scene")
    if len(mics) != len(scenes):
        raise ValueError("segment_batch: %d signals for %d scenes" % (len(mics), len(scenes)))
    if array_pos is not None and len(array_pos) != len(scenes):
        raise ValueError("segment_batch: %d array positions for %d scenes" % (len(array_pos), len(scenes)))
    K, step = int(K), int(step)
    if K < 1 or step < 1:
        raise ValueError("segment_batch: K = %d, step = %d" % (K, step))
    facts = []
    for b, sc in enumerate(scenes):
        facts.append(_label_facts(b, sc, mics[b], K, step, array_pos is not None))
        for key, what in (("L", "samples"), ("m", "microphones"), ("fs", "Hz")):
            if facts[b][key] != facts[0][key]:
                raise ValueError("segment_batch: scene %d: %g %s, scene 0 has %g (a batch shares L, M and fs)"
                                 % (b, facts[b][key], what, facts[0][key]))
    smax = max(f["nsrc"] for f in facts) if max_source is None else int(max_source)
    if not 1 <= smax <= _lib.SCENE_MAX_SOURCES:
        raise ValueError("segment_batch: max_source = %d (1 .. %d)" % (smax, _lib.SCENE_MAX_SOURCES))
    for b, f in enumerate(facts):
        if not 1 <= f["nsrc"] <= smax:
            raise ValueError("segment_batch: scene %d: %d sources (1 .. max_source = %d)" % (b, f["nsrc"], smax))
    poss = None
    if array_pos is not None:
        poss = [np.asarray(p.detach().cpu().numpy() if _is_t(p) else p, dtype=np.float64).reshape(-1) for p in array_pos]
        for b, p in enumerate(poss):
            if p.shape != (3,) or not np.all(np.isfinite(p)):
                raise ValueError("segment_batch: scene %d: array_pos must be three finite numbers" % b)
    L, m = facts[0]["L"], facts[0]["m"]
    nw = num_windows(L, K, step)
    as_numpy = not any(f["tensors"] for f in facts) and not _is_t(mics)
    dev = next((f["device"] for f in facts if f["device"] is not None), mics.device if _is_t(mics) else torch.device("cuda:0"))

    if poss is not None:
        doas = [d for _, d in ops.scene_doa_batch(
            [{"traj_pts": _up(sc.traj_pts, dev, torch.float64), "timestamps": _up(sc.timestamps, dev, torch.float64),
              "n": len(sc.t), "fs": sc.fs, "array_pos": poss[b]} for b, sc in enumerate(scenes)])]
    else:
        doas = [_up(sc.DOA, dev, torch.float64) for sc in scenes]
    items = [{"ns": facts[b]["nsrc"], "doa": doas[b], "vad_sources": _vad_u8(sc.mic_vad_sources, dev), "vad": _vad_u8(sc.mic_vad, dev)}
             for b, sc in enumerate(scenes)]
    out = ops.scene_segment_batch(items, L, K, step, nw, smax)
    dp = ops.scene_pack_batch([_up(sc.dp_mic_signals_sources, dev) for sc in scenes], L, m, smax)
    setups = [getattr(getattr(sc, "array_setup", None), "mic_pos", None) for sc in scenes]
    if any(a is None for a in setups):
        setup = None
    elif any(_is_t(a) for a in setups):
        setup = torch.stack([a if _is_t(a) else torch.from_numpy(np.asarray(a)).to(dev) for a in setups])
    else:
        setup = np.stack([np.asarray(a) for a in setups])
        setup = setup if as_numpy else torch.from_numpy(setup).to(dev)
    nums = np.array([f["nsrc"] for f in facts], dtype=np.int64)
    host = (lambda a: a.cpu().numpy()) if as_numpy else (lambda a: a)
    return {"doa": host(out["doa"]), "vad_sources": host(out["vad_sources"]), "vad_count": host(out["vad_count"]),
            "dp_signal": host(dp), "mic_vad": host(out["vad"]), "num_source": nums if as_numpy else torch.from_numpy(nums).to(dev),
            "array_setup": setup}


def training_batch(dataset, idx1, idx2, K=3328, step=3072, max_source=2):
    """One training batch without a host round trip of the signals: ``dataset.getRandomScene(idx)`` for idx1 <= idx < idx2,
    ``simulate_batch``, ``segment_batch`` -> (mic [B, n, M], gts), ready to be the ``batch`` of ``IPDnet.train_step.MyModel.
    training_step`` and of ``predict_step.MyModel.data_preprocess``.  ``K`` and ``step`` default to the reference's training
    setting (``seg_fra_ratio = 12`` frames of hop 256 with a 512 window).  Scenes that carry ``array_pos`` get their DOA
    computed on the device from the trajectory points; otherwise ``scene.DOA`` is used."""
    scenes = [dataset.getRandomScene(idx) for idx in range(idx1, idx2)]
    mic = simulate_batch(scenes)
    poss = [getattr(sc, "array_pos", None) for sc in scenes]
    return mic, segment_batch(mic, scenes, K, step, max_source, None if any(p is None for p in poss) else poss)
