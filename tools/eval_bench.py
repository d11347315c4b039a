#!/usr/bin/env python3
"""What an evaluation step's metrics cost: ``get_metric`` (template search + DOA metrics) on the device against the
float64 host restatement of the reference's loops (tests/doa_metric_ref.py), at the two real validation shapes:

    ipdnet_c3   IPDnet.Module.PredDOA, 64 utterances x 25 segments x 2 tracks, 8 microphones (7 pairs, 180 candidates)
    fnssl_c2    Module.PredDOA, 32 utterances x 25 segments, 4 microphones 'MM' (6 pairs, 37 candidates), one source

Device: 5 warm-up calls, then 20 calls between two HIP events, three windows; host: wall time of one evaluation of the
same inputs.  The kernels are latency-bound by design, so the device figure is mostly launch overhead.  No threshold is
attached.  Writes one JSON document (default profiles/r09/eval_bench.json) and fails without a GPU.

    python tools/eval_bench.py [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fn-ssl_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import doa_metric_ref as R  # noqa: E402
import frontend_doa_ref as F  # noqa: E402

MICS4 = np.array([[0.04, 0.0, 0.0], [0.0, 0.04, 0.0], [-0.04, 0.0, 0.0], [0.0, -0.04, 0.02]])
MICS8 = np.stack([0.05 * np.cos(np.arange(8) * np.pi / 4), 0.05 * np.sin(np.arange(8) * np.pi / 4),
                  0.01 * (np.arange(8) % 2)], axis=1)
WARMUP, CALLS, WINDOWS = 5, 20, 3


def device_ms(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / CALLS)
    return out


def ipdnet_c3(dev):
    from IPDnet import Module as ip_module
    pred, doa_gt, vad_gt = R.g20_pred(MICS8, 64, 25, 3301)
    pd = ip_module.PredDOA(mic_location=MICS8, dev=str(dev)).to(dev)
    p, gt = torch.from_numpy(pred).to(dev), [torch.from_numpy(doa_gt).to(dev), torch.from_numpy(vad_gt).to(dev)]
    ms = device_ms(lambda: pd(p, gt, None))
    metric = {k: float(v) for k, v in pd(p, gt, None).items()}
    t0 = time.perf_counter()
    _idx, doa, vad, _ = R.pred2doa(pred, MICS8)
    ref = R.get_metric(R.degrees(doa_gt), vad_gt, R.degrees(doa.astype(np.float32)), vad.astype(np.float32), "multiple", ("azi",), 10,
                       True, (0.001, 0.5))
    host_s = time.perf_counter() - t0
    return {"shape": "64 utterances x 25 segments x 2 tracks, 8 microphones", "device_ms_per_call": ms, "host_float64_s": host_s,
            "device_metrics": metric, "host_metrics": {k: float(ref[k]) for k in ("ACC", "MDR", "FAR")}}


def fnssl_c2(dev):
    import Module as fn_module
    pd = fn_module.PredDOA(device=str(dev), mic_location=MICS4).to(dev)
    bank = pd.bank.cpu().numpy()
    rs = np.random.RandomState(3302)
    nb, nt = 32, 25
    pick = rs.randint(0, 37, (nb, nt))
    pred = (0.6 * bank.reshape(37, 512, 6)[pick] + 0.3 * np.tanh(rs.standard_normal((nb, nt, 512, 6)))).astype(np.float32)
    net = np.ascontiguousarray(pred.transpose(0, 3, 1, 2).reshape(nb * 6, nt, 512))                  # the network's layout
    azi = np.linspace(0, np.pi, 37)[pick] + rs.uniform(-0.1, 0.1, (nb, nt))
    doa_gt = np.stack((np.full((nb, nt, 1), np.pi / 2), azi[..., None]), axis=2).astype(np.float32)
    vad_gt = (rs.rand(nb, nt, 1) < 0.8).astype(np.float32)
    p = torch.from_numpy(net).to(dev)
    gt = {"doa": torch.from_numpy(doa_gt).to(dev), "vad_sources": torch.from_numpy(vad_gt).to(dev)}
    ms = device_ms(lambda: pd(p, dict(gt)))
    metric = pd(p, dict(gt))
    t0 = time.perf_counter()
    idx, vad, _ss, _sc, _r = F.ipd2doa64(pred, bank, 1, False)
    doa = np.stack((np.full(idx.shape, np.pi / 2), np.linspace(0, np.pi, 37)[idx]), axis=2).astype(np.float32)
    ref = R.get_metric(R.degrees(doa_gt), vad_gt, R.degrees(doa), np.ones_like(vad_gt), "single", ("azi",), 5, True, (2 / 3, 2 / 3))
    host_s = time.perf_counter() - t0
    return {"shape": "32 utterances x 25 segments, 4 microphones 'MM', 1 source", "device_ms_per_call": ms, "host_float64_s": host_s,
            "device_metrics": {"ACC": float(metric["ACC"]), "MAE": float(metric["MAE"][0])},
            "host_metrics": {"ACC": float(ref["ACC"]), "MAE": float(ref["MAE"]["azi"])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "eval_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: no ROCm device (the evaluation path has no CPU implementation)")
    dev = torch.device("cuda:0")
    res = {"what": "get_metric (localisation + DOA metrics) per call: %d warm-up, %d calls between HIP events, %d windows; "
                   "host: one float64 numpy evaluation (tests/doa_metric_ref.py) of the same inputs" % (WARMUP, CALLS, WINDOWS),
           "device": torch.cuda.get_device_name(0), "ipdnet_c3": ipdnet_c3(dev), "fnssl_c2": fnssl_c2(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
