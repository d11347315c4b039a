#!/usr/bin/env python3
"""What IPDnet2's evaluation costs: the drop-in ``IPDnet2.Module.PredDOA.forward`` (MSE template search of both tracks +
DOA metrics) on the device beside a torch-CPU evaluation of the same batch, at a validation-like shape:

    ipdnet2_c5   16 utterances x 100 frames x 2 tracks, 5 microphones (4 pairs, 360 candidates x 2048 values)

Device: 5 warm-up calls, then 20 calls between two HIP events, three windows.  CPU: wall time of one evaluation with the
reference's arithmetic in torch on the host (the broadcast ``mean((pred - template) ** 2)``, one utterance at a time to
bound memory, ``argmin``) followed by the float64 restatement of its metrics (tests/ipdnet2_eval_ref.py).  No threshold is
attached: the figures are what this run measured.  Writes one JSON document (default profiles/r10/eval2_bench.json) and
fails without a GPU.

    python tools/eval2_bench.py [--out PATH]
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

import ipdnet2_eval_ref as R2  # noqa: E402

WARMUP, CALLS, WINDOWS = 5, 20, 3
MULTI = ("ACC", "MDR", "FAR", "MAE", "RMSE")


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


def batch(nb, nt, seed):
    """Noisy near-field DP-IPDs of two sources per frame with their labels, as tests/ipdnet2_eval_ref.g21_inputs draws them."""
    rng = np.random.RandomState(seed)
    mic = R2.G21_MICS["mic5"]
    azi_deg = rng.uniform(-170.0, 170.0, (nb, nt, 2)).astype(np.float32)
    doa = (np.stack((np.full_like(azi_deg, 90.0), azi_deg), axis=2) / np.float32(180) * np.float32(np.pi)).astype(np.float32)
    distance = rng.uniform(0.5, 3.0, (nb, nt, 2)).astype(np.float32)
    vad = (rng.rand(nb, nt, 2) < 0.75).astype(np.float32)
    clean = R2.nearfield_targets(doa, distance, mic)
    sigma = np.where(rng.rand(nb, nt, 1, 1, 2) < 0.65, 0.2, 0.5)
    pred = (clean + sigma * rng.standard_normal(clean.shape)).astype(np.float32)
    return mic, azi_deg, distance, vad, pred


def cpu_evaluation(pred, bank32, azi_grid, azi_deg, vad):
    """The reference's search in torch on the host, then its metrics in float64."""
    nb, nt, nf2, nm1, ntrack = pred.shape
    flat = torch.from_numpy(bank32).reshape(bank32.shape[1], -1)                       # [ncand, X]
    p = torch.from_numpy(pred)
    idx = torch.empty((ntrack, nb, nt), dtype=torch.long)
    act = torch.empty((ntrack, nb, nt))
    for r in range(ntrack):
        for b in range(nb):
            x = p[b, :, :, :, r].reshape(nt, 1, -1)
            mse = torch.mean((x - flat[None]) ** 2, dim=-1)                             # [nt, ncand]
            act[r, b], idx[r, b] = mse.min(dim=-1)
    doa_est = np.stack((np.full(idx.shape, np.pi / 2), azi_grid[idx.numpy()]), axis=0).astype(np.float32).transpose(2, 3, 0, 1)
    return R2.evaluate(doa_est, act.numpy().transpose(1, 2, 0), azi_deg, vad)


def ipdnet2_c5(dev):
    from IPDnet2 import Module as ip2_module
    nb, nt = 16, 100
    mic, azi_deg, distance, vad, pred = batch(nb, nt, 5101)
    pd = ip2_module.PredDOA(mic_location=mic, dev=str(dev))
    T = lambda a: torch.from_numpy(a).to(dev)                                          # noqa: E731
    p = T(pred)
    gt = [T(azi_deg), torch.empty(0, device=dev), mic, T(distance), T(vad)]
    ms = device_ms(lambda: pd(p, gt, None))
    metric = {k: float(v) for k, v in pd(p, gt, None).items()}
    geo = pd.gerdpipd.geometry(dev)
    bank32, grid = geo["bank"].cpu().numpy(), geo["azi"].cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    ref = cpu_evaluation(pred, bank32, grid, azi_deg, vad)
    host_s = time.perf_counter() - t0
    return {"shape": "%d utterances x %d frames x 2 tracks, 5 microphones, 360 candidates" % (nb, nt), "device_ms_per_call": ms,
            "cpu_torch_s": host_s, "cpu_threads": torch.get_num_threads(), "device_metrics": metric,
            "cpu_metrics": {k: float(ref[k]) for k in MULTI}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "eval2_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval2_bench: no ROCm device (the evaluation path has no CPU implementation)")
    dev = torch.device("cuda:0")
    res = {"what": "IPDnet2 PredDOA.forward (MSE search + DOA metrics) per call: %d warm-up, %d calls between HIP events, %d "
                   "windows; cpu: one torch evaluation of the same batch on the host, metrics by tests/ipdnet2_eval_ref.py"
                   % (WARMUP, CALLS, WINDOWS),
           "device": torch.cuda.get_device_name(0), "ipdnet2_c5": ipdnet2_c5(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
