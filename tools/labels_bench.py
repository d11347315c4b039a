#!/usr/bin/env python3
"""What the labels of a training batch cost on the device (fnssl.scene.segment_batch / training_batch) beside the
route the code before them forces, in the same run.

Settings are Simu.py's: two microphones 8 cm apart, two sources with VAD moving through 50 trajectory points, 72 000 samples
at 16 kHz, K = 3328, step = 3072 (23 windows); rooms, T60, array position and SNR drawn from a fixed seed as in
tools/scene_batch_bench.py.  The signals and the noise are device tensors, the positions, timestamps and DOA numpy arrays
(what getRandomScene makes).

For B = 1, 4, 16, 32:
    segment_pos     segment_batch(..., array_pos=...) on simulated scenes: DOA from the trajectory points on the device
    segment_doa     segment_batch on the same scenes with the float64 DOA [72 000, 2, 2] uploaded per scene
    training        simulate_batch + segment_batch(array_pos) — a whole training_batch without getRandomScene
    host_labels     the route without this stage, labels only: every scene's VAD and direct-path signals copied to the host,
                    tests/labels_ref.py's float64 transform per scene, stack / pad, upload
    host_training   simulate_batch + host_labels
    launches        launch sets per kernel name of segment_pos and segment_doa in one untimed pass (ops.timing_collect)
Each figure is the host clock around one synchronise, median of ``--reps``.  Nothing is asserted about the figures; the two
label routes are compared once (VADs and signals equal, angles within 1e-12).  No CPU fallback.

    python tools/labels_bench.py [--reps 7] [--json profiles/r24/labels.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fn-ssl_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import labels_ref as R  # noqa: E402
import scene_batch_bench as SB  # noqa: E402

K, STEP, SMAX = 3328, 3072, 2


def draw(nb, dev):
    rs = np.random.RandomState(2400)
    scenes, poss = [], []
    for _ in range(nb):
        sc = SB.draw_scene(rs, 2, dev)
        pos = np.asarray(sc.mic_pos, dtype=np.float64).mean(axis=0)          # the array's centre
        sc.array_setup.mic_pos = np.asarray(sc.mic_pos, dtype=np.float64) - pos
        _, sc.DOA = R.trajectory_doa(sc.traj_pts.astype(np.float64), sc.timestamps, SB.L, SB.FS, pos)
        scenes.append(sc)
        poss.append(pos)
    return scenes, poss


def host_labels(mic, scenes, dev):
    """The labels without the device stage: copy down, numpy, stack and pad, copy up."""
    seg = [R.transform(SB.L, {"DOA": sc.DOA, "mic_vad_sources": sc.mic_vad_sources.cpu().numpy(), "mic_vad": sc.mic_vad.cpu().numpy(),
                              "fs": sc.fs}, K, STEP) for sc in scenes]
    g = R.gts(seg, [sc.dp_mic_signals_sources.cpu().numpy() for sc in scenes], SMAX)
    return {"doa": torch.from_numpy(g["doa"]).to(dev), "vad_sources": torch.from_numpy(g["vad_sources"].astype(np.uint8)).to(dev),
            "dp_signal": torch.from_numpy(g["dp_signal"].astype(np.float32)).to(dev)}


def case(nb, reps, dev):
    from fnssl import scene
    scenes, poss = draw(nb, dev)
    seeds = list(range(100, 100 + nb))
    mic = scene.simulate_batch(scenes, seeds=seeds)

    def segment_pos():
        return scene.segment_batch(mic, scenes, K, STEP, SMAX, array_pos=poss)

    def segment_doa():
        return scene.segment_batch(mic, scenes, K, STEP, SMAX)

    def training():
        return scene.segment_batch(scene.simulate_batch(scenes, seeds=seeds), scenes, K, STEP, SMAX, array_pos=poss)

    def host():
        return host_labels(mic, scenes, dev)

    def host_training():
        return host_labels(scene.simulate_batch(scenes, seeds=seeds), scenes, dev)

    a, b, h = segment_pos(), segment_doa(), host()
    same = all(torch.equal(a[k], x[k]) for k in ("vad_sources", "dp_signal") for x in (b, h))
    res = {"scenes": nb, "windows": scene.num_windows(SB.L, K, STEP), "exact_parts_equal": bool(same),
           "doa_pos_vs_uploaded": float((a["doa"] - b["doa"]).abs().max()), "doa_device_vs_host": float((b["doa"] - h["doa"]).abs().max())}
    for name, fn in (("segment_pos", segment_pos), ("segment_doa", segment_doa), ("training", training), ("host_labels", host),
                     ("host_training", host_training)):
        res[name] = SB.wall(fn, reps)
        res[name]["per_scene_ms"] = round(res[name]["median_ms"] / nb, 3)
    res["launches_segment_pos"] = SB.launches(segment_pos)
    res["launches_segment_doa"] = SB.launches(segment_doa)
    res["host_over_device_labels"] = round(res["host_labels"]["median_ms"] / res["segment_pos"]["median_ms"], 2)
    res["host_over_device_training"] = round(res["host_training"]["median_ms"] / res["training"]["median_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default="")
    ap.add_argument("--batches", default="1,4,16,32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("labels_bench: needs a ROCm device (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "samples": SB.L, "fs": SB.FS, "K": K, "step": STEP, "max_source": SMAX,
           "reps": args.reps, "cases": {}}
    for nb in (int(v) for v in args.batches.split(",")):
        out["cases"]["B%d" % nb] = r = case(nb, args.reps, dev)
        print("B%-3d segment_pos %8.3f ms  segment_doa %8.3f ms  host_labels %9.3f ms (x%.1f)   training %8.3f ms  host_training %9.3f ms (x%.2f)"
              % (nb, r["segment_pos"]["median_ms"], r["segment_doa"]["median_ms"], r["host_labels"]["median_ms"], r["host_over_device_labels"],
                 r["training"]["median_ms"], r["host_training"]["median_ms"], r["host_over_device_training"]), flush=True)
        print("     launches segment_pos %s   segment_doa %s   parts equal %s, doa %.2e / %.2e" % (
            {k: v["count"] for k, v in r["launches_segment_pos"].items()}, {k: v["count"] for k, v in r["launches_segment_doa"].items()},
            r["exact_parts_equal"], r["doa_pos_vs_uploaded"], r["doa_device_vs_host"]), flush=True)
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
