#!/usr/bin/env python3
"""What a batch of scenes costs in one launch set (fnssl.scene.simulate_batch) beside the same scenes through
B sequential ``simulate`` calls in the same run.

Settings are Simu.py's: two microphones 8 cm apart, two sources with VAD moving through 50 trajectory points, 4.5 s at
16 kHz; rooms from 6 x 6 x 2.5 to 10 x 8 x 6 m, T60 from 0.2 to 1.3 s, the array between 35 % and 65 % (height 30 % .. 50 %)
of the room and the SNR from -5 to 15 dB, all drawn from a fixed seed.  The signals and the noise are device tensors, the
positions and timestamps numpy arrays (what getRandomScene makes): nothing but the positions goes up in the timed region.

For B = 1, 4, 16, 32 (and B = 16 with four and eight microphones):
    batch        simulate_batch per batch and per scene: host clock around one synchronise, median of ``--reps``
    sequential   B simulate calls on the same scenes, then one synchronise, the same way
    launches     launch sets per kernel name and their summed device time in one untimed pass of each route
                 (ops.timing_enable / timing_collect; the bracketing events are why that pass is not the timed one)
    workspace    what the per-job chunk plan asks for (every job is planned to fill the device by itself)

Nothing is asserted about the figures.  No CPU fallback.

    python tools/scene_batch_bench.py [--reps 7] [--json profiles/r23/scene_batch.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fn-ssl_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FS = 16000.0
T = 4.5
L = int(T * FS)
NPTS = 50
NSRC = 2


def draw_scene(rs, m, dev):
    from fnssl import rir
    room = rs.uniform([6.0, 6.0, 2.5], [10.0, 8.0, 6.0])
    t60 = float(rs.uniform(0.2, 1.3))
    beta = rir.beta_SabineEstimation(room, t60, rs.uniform(0.5, 1.0, 6))
    centre = room * rs.uniform([0.35, 0.35, 0.3], [0.65, 0.65, 0.5])
    mics = centre + np.stack([[0.08 * (i - (m - 1) / 2), 0.0, 0.0] for i in range(m)])
    pts = np.zeros((NPTS, 3, NSRC))
    for s in range(NSRC):                                                   # a straight walk between two points in the room
        a, b = (room * rs.uniform(0.1, 0.9, 3) for _ in range(2))
        pts[:, :, s] = np.linspace(a, b, NPTS)
    env = (np.sin(np.arange(L) / rs.uniform(2000.0, 4000.0)) > -0.5).astype(np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    sc = types.SimpleNamespace(
        room_sz=room.tolist(), T60=t60, beta=beta, SNR=float(rs.uniform(-5.0, 15.0)), fs=FS, noise_signal=up(rs.standard_normal((L, m))),
        source_signal=up(rs.standard_normal((L, NSRC)) * 0.1 * env[:, None]), mic_pos=mics.astype(np.float32),
        array_setup=types.SimpleNamespace(mic_orV=None, mic_pattern="omni"), timestamps=np.arange(NPTS) * T / NPTS,
        traj_pts=pts.astype(np.float32), t=np.arange(L) / FS)
    sc.source_vad = up(np.stack([env] * NSRC, axis=1))
    return sc


def wall(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3), "calls": reps}


def launches(fn):
    from fnssl import ops
    ops.timing_enable(True)
    try:
        ops.timing_collect()
        fn()
        torch.cuda.synchronize()
        got = ops.timing_collect()
    finally:
        ops.timing_enable(False)
    return {name: {"count": int(v["count"]), "ms": round(v["ms"], 4)} for name, v in sorted(got.items())}


def workspace_of(scenes):
    """The chunk plans of the batch's full-RIR jobs on this device: workgroups, bytes."""
    from fnssl import ops, rir, scene
    jobs = []
    for sc in scenes:
        tdiff, tmax, nb = scene._rir_times(sc)
        nism, _ = rir.sample_counts(tdiff, tmax, FS)
        jobs += [dict(m_src=NPTS, m_rcv=int(sc.mic_pos.shape[0]), room_sz=sc.room_sz, nb_img=nb, nism=nism)] * NSRC
    plans, total = ops.rir_batch_plan(jobs)
    return {"jobs": len(jobs), "workspace_bytes": int(total), "ism_workgroups": int(sum(p["grid_x"] * p["grid_y"] for p in plans)),
            "images_per_rir": [int(p["images"]) for p in plans[::NSRC]], "chunks_per_rir": [int(p["nchunks"]) for p in plans[::NSRC]]}


def case(nb, m, reps, dev):
    from fnssl import scene
    rs = np.random.RandomState(2300 + m)                                    # the first scenes of a larger batch are the smaller one's
    scenes = [draw_scene(rs, m, dev) for _ in range(nb)]
    seeds = list(range(100, 100 + nb))

    def batch():
        return scene.simulate_batch(scenes, seeds=seeds)

    def sequential():
        return [scene.simulate(sc, seed=seeds[b]) for b, sc in enumerate(scenes)]

    same = all(torch.equal(a, b) for a, b in zip(batch(), sequential()))
    res = {"scenes": nb, "mics": m, "T60": [round(sc.T60, 3) for sc in scenes], "bit_identical": bool(same),
           "plan": workspace_of(scenes), "batch": wall(batch, reps), "sequential": wall(sequential, reps),
           "launches_batch": launches(batch), "launches_sequential": launches(sequential)}
    for route in ("batch", "sequential"):
        res[route]["per_scene_ms"] = round(res[route]["median_ms"] / nb, 3)
    res["sequential_over_batch"] = round(res["sequential"]["median_ms"] / res["batch"]["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_batch_bench: needs a ROCm device (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "samples": L, "fs": FS, "points": NPTS, "sources": NSRC, "reps": args.reps,
           "cases": {}}
    for nb, m in ((1, 2), (4, 2), (16, 2), (32, 2), (16, 4), (16, 8)):
        key = "B%d_M%d" % (nb, m)
        out["cases"][key] = r = case(nb, m, args.reps, dev)
        print("%-7s batch %8.3f ms (%7.3f / scene)   sequential %8.3f ms (%7.3f / scene)   x%.2f   bits %s" % (
            key, r["batch"]["median_ms"], r["batch"]["per_scene_ms"], r["sequential"]["median_ms"], r["sequential"]["per_scene_ms"],
            r["sequential_over_batch"], "same" if r["bit_identical"] else "DIFFER"), flush=True)
        print("        launches batch %s" % {k: v["count"] for k, v in r["launches_batch"].items()}, flush=True)
        print("        launches sequential %s" % {k: v["count"] for k, v in r["launches_sequential"].items()}, flush=True)
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
