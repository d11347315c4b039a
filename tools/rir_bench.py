#!/usr/bin/env python3
"""What the room simulation costs for one training utterance at the reference's settings (Simu.py / Dataset.py): a source
moving through 50 trajectory points in a room of 8 x 7 x 4 m, 4.79 s at 16 kHz, Tdiff / Tmax = the 12 dB / 40 dB times of
the T60, nb_img = t2n(Tdiff) — for 2, 4 and 15 microphones and T60 of 0.3, 0.8 and 1.3 s.

Per kernel (csrc/rir.hip) the time between device events (medians over ``--reps`` calls after a warm-up) and its work:

    ism          fnssl_rir_ism on the 50 x M RIRs; work = window evaluations (taps of the images whose window meets [0, nISM))
    tail         fnssl_rir_tail; work = tail samples written
    trajectory   fnssl_rir_trajectory, one (signal, RIR set) pair; work = multiply-adds (ns x lenRIR x M, less the corners)
    scene_batch  fnssl_rir_trajectory on the six pairs of a scene in one launch: 2 sources x {full, direct path, VAD}

with work / time against the fp32 vector rate (157.3 TFLOP/s spec = 78.6 T multiply-adds/s) and the time the kernel's bytes
would take at the measured HBM rate (6.29 TB/s) — a floor it cannot beat, not a target it was tuned to.  Two restatements are
timed on the same scene: torch on the device (images x taps tensors scattered with index_add_, mixing by FFT per segment) and
the numpy float64 reference of tests/rir_ref.py (its image loop on ONE of the RIRs, scaled to the scene; its mixing loop on
the whole signal; ``--no-numpy`` leaves it out).  Nothing is asserted about the figures.  No CPU fallback.

    python tools/rir_bench.py [--reps 5] [--json profiles/r21/rir.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fn-ssl_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FS = 16000.0
ROOM = [8.0, 7.0, 4.0]
NPTS = 50
NS = int(4.79 * FS)
FMA_PER_S = 157.3e12 / 2
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


def with_work(res, work, unit, nbytes):
    res["work"] = int(work)
    res["work_unit"] = unit
    res["work_per_s"] = float("%.4g" % (work / (res["median_ms"] * 1e-3)))
    res["ratio_to_fp32_valu_fma_rate"] = float("%.4g" % (res["work_per_s"] / FMA_PER_S))
    res["bytes"] = int(nbytes)
    res["hbm_floor_ms"] = float("%.4g" % (nbytes / HBM_B_PER_S * 1e3))
    return res


def geometry(m):
    rs = np.random.RandomState(21)
    centre = np.array([4.1, 3.4, 1.5])
    ang = np.arange(m) * 2 * np.pi / m
    mics = centre + 0.05 * np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1)
    a, b = np.array([1.2, 1.0, 1.4]), np.array([6.5, 5.8, 1.9])
    traj = np.linspace(a, b, NPTS) + 0.05 * np.sin(np.linspace(0, 6, NPTS))[:, None]
    return traj, mics, rs


def ism_window_evals(traj, mics, beta, nb, nism, c=343.0):
    """Taps of every image whose window meets [0, nISM), from the float64 image positions."""
    import rir_ref as R
    tw = 8e-3 * FS
    n = 0
    for s in range(len(traj)):
        ax = [np.array(R.axis_images(nb[a], ROOM[a], traj[s][a], beta[2 * a], beta[2 * a + 1])[0]) for a in range(3)]
        for r in range(len(mics)):
            d2 = ((ax[0] - mics[r][0]) ** 2)[:, None, None] + ((ax[1] - mics[r][1]) ** 2)[None, :, None] + \
                 ((ax[2] - mics[r][2]) ** 2)[None, None, :]
            tau = np.sqrt(d2) * FS / c
            lo, hi = np.maximum(np.ceil(tau - tw / 2), 0), np.minimum(np.floor(tau + tw / 2), nism - 1)
            n += int(np.maximum(hi - lo + 1, 0).sum())
    return n


def torch_ism(src, rcv, room, beta, nb, nism, c=343.0):
    """The image-source part with torch ops on the device, one source position at a time (images x taps, index_add_)."""
    dev = src.device
    tw = 8e-3 * FS
    ntap = int(tw) + 1
    out = torch.zeros((src.shape[0], rcv.shape[0], nism), device=dev)
    k = torch.arange(ntap, device=dev, dtype=torch.float32)
    for s in range(src.shape[0]):
        pos, amp = [], []
        for a in range(3):
            n = torch.arange(nb[a], device=dev) - nb[a] // 2
            odd = (n % 2) == 1
            pos.append(torch.where(odd, (n + 1) * room[a] - src[s, a], n * room[a] + src[s, a]))
            more, less = (n.abs() + 1) // 2, n.abs() // 2
            c0, c1 = torch.where(n > 0, less, more), torch.where(n > 0, more, less)
            amp.append(beta[2 * a] ** c0 * beta[2 * a + 1] ** c1)
        am = (amp[0][:, None, None] * amp[1][None, :, None] * amp[2][None, None, :]).reshape(-1)
        for r in range(rcv.shape[0]):
            d = torch.sqrt(((pos[0] - rcv[r, 0]) ** 2)[:, None, None] + ((pos[1] - rcv[r, 1]) ** 2)[None, :, None]
                           + ((pos[2] - rcv[r, 2]) ** 2)[None, None, :]).reshape(-1)
            tau = d * (FS / c)
            keep = tau - tw / 2 < nism
            tau, a_ = tau[keep], (am / (4 * np.pi * d))[keep]
            t = torch.ceil(tau - tw / 2)[:, None] + k[None, :]
            x = t - tau[:, None]
            v = a_[:, None] * 0.5 * (1 + torch.cos(2 * np.pi * x / tw)) * torch.sinc(x)
            ok = (t >= 0) & (t < nism) & (x.abs() <= tw / 2)
            out[s, r].index_add_(0, t[ok].long(), v[ok])
    return out


def torch_trajectory(x, rirs, w):
    """Segment, FFT-convolve, overlap-add with torch ops on the device."""
    npts, m, length = rirs.shape
    y = torch.zeros((x.numel() + length - 1, m), device=x.device)
    for p in range(npts):
        seg = x[w[p]:w[p + 1]]
        if seg.numel() == 0:
            continue
        n = seg.numel() + length - 1
        nfft = 1 << (n - 1).bit_length()
        conv = torch.fft.irfft(torch.fft.rfft(seg, nfft)[None, :] * torch.fft.rfft(rirs[p], nfft), nfft)[:, :n]
        y[w[p]:w[p] + n] += conv.T
    return y


def traj_macs(ns, length, m):
    """Pairs (s, k) with 0 <= s < ns, 0 <= k < length: every source sample meets every tap once."""
    return ns * length * m


def case(m, t60, reps, numpy_too, dev):
    import fnssl.rir as gpuRIR
    import rir_ref as R
    from fnssl import ops
    traj, mics, rs = geometry(m)
    beta = gpuRIR.beta_SabineEstimation(ROOM, t60)
    tdiff, tmax = gpuRIR.att2t_SabineEstimator(12, t60), gpuRIR.att2t_SabineEstimator(40, t60)
    nb = gpuRIR.t2n(tdiff, ROOM)
    nism, nsam = gpuRIR.sample_counts(tdiff, tmax, FS)
    src = torch.from_numpy(traj.astype(np.float32)).to(dev)
    rcv = torch.from_numpy(mics.astype(np.float32)).to(dev)
    plan = ops.rir_plan(NPTS, m, nb, nism)
    res = {"T60": t60, "microphones": m, "nb_img": nb, "nISM": nism, "nSamples": nsam, "rirs": NPTS * m, "plan": plan}
    rir = torch.zeros((NPTS, m, nsam), device=dev)
    evals = ism_window_evals(traj, mics, beta, nb, nism)
    res["ism"] = with_work(timed(lambda: ops.rir_ism(src, rcv, ROOM, beta, nb, nism, nsam, FS, out=rir), reps), evals,
                           "window evaluations", 4 * NPTS * m * nism * (1 + (2 * plan["nchunks"] if plan["nchunks"] > 1 else 0)))
    res["tail"] = with_work(timed(lambda: ops.rir_tail(rir, src, rcv, ROOM, beta, nism, FS, seed=1), reps),
                            NPTS * m * (nsam - nism), "tail samples", 4 * NPTS * m * nsam)
    x = torch.from_numpy(rs.standard_normal(NS).astype(np.float32)).to(dev)
    w_host = gpuRIR._w_ini(NPTS, NS, np.arange(NPTS) * NS / FS / NPTS, FS)
    w = torch.from_numpy(w_host).to(dev)
    res["trajectory"] = with_work(timed(lambda: ops.rir_trajectory_batch([x], [rir], [w]), reps), traj_macs(NS, nsam, m),
                                  "multiply-adds", 4 * (NS + NPTS * m * nsam + (NS + nsam - 1) * m))
    dp = gpuRIR.simulateRIR(ROOM, beta, src, rcv, [1, 1, 1], 0.1, FS)
    sigs = [x, x, x.abs(), x.flip(0), x.flip(0), x.flip(0).abs()]
    sets = [rir, dp, dp, rir, dp, dp]
    macs = sum(traj_macs(NS, r_.shape[2], m) for r_ in sets)
    nbytes = sum(4 * (NS + r_.numel() + (NS + r_.shape[2] - 1) * m) for r_ in sets)
    res["scene_batch"] = with_work(timed(lambda: ops.rir_trajectory_batch(sigs, sets, [w] * 6), reps), macs, "multiply-adds", nbytes)
    # restatements
    few = max(2, reps // 2)
    res["torch_ism"] = timed(lambda: torch_ism(src, rcv, ROOM, [float(b) for b in beta], nb, nism), few, warm=1)
    res["torch_trajectory"] = timed(lambda: torch_trajectory(x, rir, w_host), few, warm=1)
    err = (torch_trajectory(x, rir, w_host) - ops.rir_trajectory_batch([x], [rir], [w])[0]).abs().max().item()
    res["torch_trajectory_max_abs_diff"] = float("%.3g" % err)
    err = (torch_ism(src[:1], rcv, ROOM, [float(b) for b in beta], nb, nism) - rir[:1, :, :nism]).abs().max().item()
    res["torch_ism_max_abs_diff"] = float("%.3g" % err)
    if numpy_too:
        t0 = time.perf_counter()
        R.ism(ROOM, beta, traj[:1], mics[:1], nb, nism, FS)
        one = time.perf_counter() - t0
        res["numpy_f64_ism"] = {"one_rir_ms": round(one * 1e3, 1), "scaled_to_scene_ms": round(one * 1e3 * NPTS * m, 0)}
        xh, rh = x.cpu().numpy(), rir.cpu().numpy()
        t0 = time.perf_counter()
        R.trajectory(xh, rh, np.arange(NPTS) * NS / FS / NPTS, FS)
        res["numpy_f64_trajectory"] = {"ms": round((time.perf_counter() - t0) * 1e3, 0)}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mics", type=int, nargs="*", default=[2, 4, 15])
    ap.add_argument("--t60", type=float, nargs="*", default=[0.3, 0.8, 1.3])
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "r21", "rir.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rir_bench needs a ROCm device (no CPU fallback)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "room": ROOM, "points": NPTS, "signal_samples": NS, "fs": FS,
           "unit": "milliseconds between device events around one call (median of --reps)",
           "fp32_valu_fma_per_s": FMA_PER_S, "hbm_bytes_per_s": HBM_B_PER_S, "cases": []}
    for t60 in args.t60:
        for m in args.mics:
            res = case(m, t60, args.reps, not args.no_numpy, dev)
            out["cases"].append(res)
            print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v) for k, v in res.items()
                              if k != "plan"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
