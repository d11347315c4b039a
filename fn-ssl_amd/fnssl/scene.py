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
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops, rir
from .rir import _reject_cpu_tensors

__all__ = ["acoustic_power", "gen_diffuse_noise", "mix_signals", "simulate", "simulate_batch", "get_batch"]


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
