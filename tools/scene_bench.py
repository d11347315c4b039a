#!/usr/bin/env python3
"""What the scene finish costs for one training utterance at the reference's settings (Simu.py / Dataset.py): 4.79 s at
16 kHz, 2, 4 and 8 microphones (rings of radius 5 cm), two sources moving through 50 trajectory points in a room of 8 x 7 x
4 m at T60 = 0.8 s, diffuse noise, source VAD.

Per launch set of csrc/scene.hip the time between device events (medians over ``--reps`` calls after a warm-up) beside the
time its bytes would take at the measured HBM rate (6.29 TB/s) — a floor it cannot beat, not a target it was tuned to:

    factor        fnssl_anf_coherence + fnssl_anf_factor (the status word is not read)
    mean          fnssl_anf_mean over the M L noise vector
    mix           fnssl_anf_mix, [L, M] -> [L + pad, M] (also with 2 and 16 output hops per wave; the default sizes them)
    power         fnssl_scene_power on the two direct-path signals, and on the noise
    finish        fnssl_scene_finish, two sources with VAD

``gen_diffuse_noise`` as a whole (device tensors in and out, the status read included) stands beside the scipy call sequence
of the reference on this machine's CPU and a torch restatement on the device (torch.stft, torch.linalg.cholesky, einsum,
torch.istft).  A whole two-source ``simulate`` with VAD, noise generation included, stands beside the route this project had
before: fnssl.rir as gpuRIR with numpy arrays, tests/scene_ref.py's float64 finish on the host and the scipy noise.  Whole
routes are host clocks around work that ends in a device synchronise.  Nothing is asserted about the figures.  No CPU fallback.

    python tools/scene_bench.py [--reps 5] [--json profiles/r22/scene.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fn-ssl_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FS = 16000.0
T = 4.79
L = int(T * FS)
ROOM = [8.0, 7.0, 4.0]
NPTS = 50
T60 = 0.8
HBM_B_PER_S = 6.29e12


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "calls": reps}


def wall(fn, reps, warm=1, sync=True):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3), "calls": reps}


def floor(res, nbytes):
    res["bytes"] = int(nbytes)
    res["hbm_floor_ms"] = float("%.4g" % (nbytes / HBM_B_PER_S * 1e3))
    res["ratio_to_floor"] = float("%.4g" % (res["median_ms"] / res["hbm_floor_ms"]))
    return res


def scipy_gen_diffuse_noise(noise, mic_pos):
    """The reference's call sequence (gen_diffuse_noise -> mix_signals) on the CPU, float64."""
    import scipy.linalg
    import scipy.signal
    import scene_ref as R
    m = mic_pos.shape[0]
    noise = noise - np.mean(noise)
    cols = noise[:m * L].reshape(m, L).T
    dc = R.coherence(mic_pos, FS)
    k_ = 256
    x = np.vstack([np.zeros([k_ // 2, m]), cols, np.zeros([k_ // 2, m])]).transpose()
    _, _, n = scipy.signal.stft(x, window="hann", nperseg=k_, noverlap=0.75 * k_, nfft=k_)
    out = np.zeros(n.shape, dtype=complex)
    for k in range(1, k_ // 2 + 1):
        c = scipy.linalg.cholesky(dc[:, :, k])
        out[:, k, :] = np.dot(n[:, k, :].transpose(), np.conj(c)).transpose()
    _, y = scipy.signal.istft(out, window="hann", nperseg=k_, noverlap=0.75 * k_, nfft=k_)
    return y.transpose()[k_ // 2:-k_ // 2, :]


def torch_gen_diffuse_noise(noise, dc):
    """The same on the device with ATen: noise [M L] float32, dc [M, M, 129] float64."""
    m = dc.shape[0]
    x = (noise - noise.mean())[:m * L].reshape(m, L)
    x = torch.nn.functional.pad(x, (128, 128 + 64))                        # (a whole hop more: torch.stft drops a ragged end)
    win = torch.hann_window(256, periodic=True, device=x.device)
    n = torch.stft(x, 256, hop_length=64, window=win, center=True, pad_mode="constant", return_complex=True)   # [M, 129, T]
    c = torch.zeros_like(dc)
    c[:, :, 1:] = torch.linalg.cholesky(dc[:, :, 1:].permute(2, 0, 1), upper=True).permute(1, 2, 0)
    out = torch.einsum("qpk,qkt->pkt", c.to(torch.complex64), n)
    y = torch.istft(out, 256, hop_length=64, window=win, center=True)
    return y[:, 128:128 + L].t()


def geometry(m):
    centre = np.array([4.1, 3.4, 1.5])
    ang = np.arange(m) * 2 * np.pi / m
    mics = centre + 0.05 * np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1)
    a, b = np.array([1.2, 1.0, 1.4]), np.array([6.5, 5.8, 1.9])
    traj = np.linspace(a, b, NPTS) + 0.05 * np.sin(np.linspace(0, 6, NPTS))[:, None]
    return np.stack([traj, traj[::-1] + np.array([0.3, -0.2, 0.1])], axis=2), mics


def a_scene(m, conv, noise, rs):
    from fnssl import rir
    pts, mics = geometry(m)
    env = (np.sin(np.arange(L) / 3000.0) > -0.5).astype(np.float32)
    src = (rs.standard_normal((L, 2)) * 0.1).astype(np.float32) * env[:, None]
    sc = types.SimpleNamespace(room_sz=ROOM, T60=T60, beta=rir.beta_SabineEstimation(ROOM, T60), SNR=15.0, fs=FS,
                               noise_signal=noise, source_signal=conv(src), mic_pos=conv(mics.astype(np.float32)),
                               array_setup=types.SimpleNamespace(mic_orV=None, mic_pattern="omni"),
                               timestamps=np.arange(NPTS) * T / NPTS, traj_pts=conv(pts.astype(np.float32)), t=np.arange(L) / FS)
    sc.source_vad = conv(np.stack([env, env], axis=1))
    return sc


def parent_route(m, rs, noise_flat, mics):
    """fnssl.rir as gpuRIR (numpy in and out), the scipy noise and scene_ref's float64 finish on the host."""
    import fnssl.rir as gpuRIR
    import scene_ref as R
    sc = a_scene(m, lambda a: a, None, rs)
    noise = scipy_gen_diffuse_noise(noise_flat, mics)
    tdiff, tmax = gpuRIR.att2t_SabineEstimator(12, T60), gpuRIR.att2t_SabineEstimator(40, T60)
    nb = gpuRIR.t2n(tdiff, ROOM)
    full, dp, vads = [], [], []
    for s in range(2):
        h = gpuRIR.simulateRIR(ROOM, sc.beta, sc.traj_pts[:, :, s], sc.mic_pos, nb, tmax, FS, Tdiff=tdiff, seed=s)
        hd = gpuRIR.simulateRIR(ROOM, sc.beta, sc.traj_pts[:, :, s], sc.mic_pos, [1, 1, 1], 0.1, FS)
        full.append(gpuRIR.simulateTrajectory(sc.source_signal[:, s], h, timestamps=sc.timestamps, fs=FS))
        dp.append(gpuRIR.simulateTrajectory(sc.source_signal[:, s], hd, timestamps=sc.timestamps, fs=FS))
        vads.append(gpuRIR.simulateTrajectory(sc.source_vad[:, s], hd, timestamps=sc.timestamps, fs=FS))
    return R.finish(full, dp, noise, sc.SNR, L, vads)["mic"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--no-host", action="store_true", help="leave out the CPU routes (scipy noise, parent route)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_bench: needs a ROCm device (no CPU fallback)")
    from fnssl import ops, scene
    dev = torch.device("cuda:0")
    up = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "samples": L, "fs": FS, "T60": T60, "reps": args.reps, "cases": {}}
    for m in (2, 4, 8):
        rs = np.random.RandomState(2200 + m)
        pts, mics = geometry(m)
        noise_flat = rs.standard_normal(m * L).astype(np.float32)
        noise_dev, pos_dev = up(noise_flat), up(mics, np.float64)
        lout = L + (-L) % 64
        res = {}
        res["factor"] = floor(timed(lambda: ops.anf_factor(ops.anf_coherence(pos_dev[None], FS), sync=False), args.reps),
                              m * m * 129 * 8 * 2 + m * (m + 1) // 2 * 128 * 4)
        cfac, _ = ops.anf_factor(ops.anf_coherence(pos_dev[None], FS))
        res["mean"] = floor(timed(lambda: ops.anf_mean(noise_dev[None]), args.reps), m * L * 4)
        mean = ops.anf_mean(noise_dev[None])
        x = noise_dev[None].unflatten(1, (m, L)).transpose(1, 2)
        res["mix"] = floor(timed(lambda: ops.anf_mix(x, cfac, mean), args.reps), (L + lout) * m * 4 + m * (m + 1) // 2 * 128 * 4)
        for tile in (2, 16):
            res["mix_tile%d" % tile] = timed(lambda: ops.anf_mix(x, cfac, mean, _tile_hops=tile), args.reps)
        noise = ops.anf_mix(x, cfac, mean)[0]
        sigs = [up(rs.standard_normal((L + 2000, m)) * 0.1) for _ in range(4)]
        res["power_sources"] = floor(timed(lambda: ops.scene_power(sigs[:2], L), args.reps), 2 * L * m * 4)
        res["power_noise"] = floor(timed(lambda: ops.scene_power([noise]), args.reps), lout * m * 4)
        p, pn = ops.scene_power(sigs[:2], L), ops.scene_power([noise])
        res["finish"] = floor(timed(lambda: ops.scene_finish(sigs[:2], noise, p, pn, 15.0, L, sigs[2:]), args.reps),
                              (2 + 1 + 2 * 2 + 1) * L * m * 4 + 3 * L)
        res["gen_diffuse_noise"] = timed(lambda: scene.gen_diffuse_noise(noise_dev, T, FS, pos_dev), args.reps)
        dc = ops.anf_coherence(pos_dev[None], FS)[0]
        res["gen_diffuse_noise_torch"] = timed(lambda: torch_gen_diffuse_noise(noise_dev, dc), args.reps)
        a = scene.gen_diffuse_noise(noise_dev, T, FS, pos_dev)[:L].cpu().numpy().astype(np.float64)
        b = torch_gen_diffuse_noise(noise_dev, dc)[:L].cpu().numpy().astype(np.float64)
        res["gen_diffuse_noise_torch"]["max_abs_from_kernels"] = float(np.abs(a - b).max())

        def new_route():
            sc = a_scene(m, up, None, np.random.RandomState(1))
            sc.noise_signal = scene.gen_diffuse_noise(noise_dev, T, FS, pos_dev)
            return scene.simulate(sc, seed=0)
        res["simulate_with_noise"] = wall(new_route, args.reps)
        res["simulate_with_noise_device_events"] = timed(new_route, args.reps, warm=0)
        if not args.no_host:
            res["gen_diffuse_noise_scipy_cpu"] = wall(lambda: scipy_gen_diffuse_noise(noise_flat.astype(np.float64), mics), 3, sync=False)
            ref = scipy_gen_diffuse_noise(noise_flat.astype(np.float64), mics)[:L]
            res["gen_diffuse_noise"]["max_abs_from_scipy"] = float(np.abs(a - ref).max())
            res["parent_route_with_noise"] = wall(lambda: parent_route(m, np.random.RandomState(1), noise_flat.astype(np.float64), mics), 3)
            got = new_route().cpu().numpy().astype(np.float64)
            want = parent_route(m, np.random.RandomState(1), noise_flat.astype(np.float64), mics)
            res["simulate_with_noise"]["max_abs_from_parent_route"] = float(np.abs(got - want).max())
            res["simulate_with_noise"]["peak"] = float(np.abs(want).max())
        out["cases"]["M%d" % m] = res
        for k, v in res.items():
            print("M = %d %-34s %s" % (m, k, json.dumps(v)), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
