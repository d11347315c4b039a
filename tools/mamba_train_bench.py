#!/usr/bin/env python3
"""Forward and backward of one IPDnet2 Mamba block at BASELINE config 5's block shape (64 utterances x 16 compressed bins
= 1 024 sequences x 250 frames, fp32), time pooling 1 and layer 0's pooling 5: fnssl_sn_mamba, fnssl_sn_mamba_backward and
each backward phase (fnssl_timing_collect), each next to the time its compulsory HBM traffic would take, and the same
block's backward through torch autograd of the recurrent restatement (tests/mamba_train_ref.py) on the same device — what a
user has without the kernels.  Medians of --runs runs after --warmup, device events on the compute stream.  Secondary
measurement: bench.py's headline stays the inference metric.

    python tools/mamba_train_bench.py [--utts 64] [--bins 16] [--frames 250] [--runs 10] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "fn-ssl_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mamba_train_ref as R  # noqa: E402
from IPDnet2.IPDnet2 import LayerNorm, Mamba  # noqa: E402
from fnssl import ops  # noqa: E402
from fnssl import spatialnet as sn  # noqa: E402
from fnssl import spatialnet_train as T  # noqa: E402
from fnssl import weights as W  # noqa: E402

HBM = 6.29e12            # measured copy rate of the MI355X (8.0 TB/s spec), bytes/s
H, E, XP, NST = 96, 192, 40, 16
PHASES = ("sn_mamba_bwd_out", "sn_mamba_bwd_scan", "sn_mamba_bwd_xproj", "sn_mamba_bwd_in", "sn_mamba_bwd_wgrad")


def floats_per_point(pool, tc):
    """Compulsory traffic per point, in floats: every tensor a phase must read or write, once."""
    ck = 2.0 * NST * E / tc                                  # checkpoints, written and read back
    return {
        "sn_mamba (forward)": (H + 2 * E) + (E + XP) + (2 * E + XP + E) + (E + H + H / pool),
        "sn_mamba_bwd_out": H / pool + H + E,
        "sn_mamba_bwd_scan": (E + XP) + (3 * E + XP) + ck + (2 * E + XP),     # pass 1; pass 2 reads; checkpoints; writes
        "sn_mamba_bwd_xproj": (XP + 2 * E) + 4 * E,          # du += ddbl W_x; conv backward (xi, du -> dxi, u)
        "sn_mamba_bwd_in": 2 * E + 4 * H,                    # [dxi | dz], x, dO -> dx, ln
        "sn_mamba_bwd_wgrad": 4 * E + 2 * H + XP,            # y, dO, u, ddbl, ln, [dxi | dz]
    }


def median_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--bins", type=int, default=16)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mamba_train_bench: needs a ROCm device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    nb, nf, nt = args.utts, args.bins, args.frames
    npts = nb * nf * nt
    p = R.block_params(W.make_ipdnet2_state(0, num_layers=1))
    norm, mamba = LayerNorm(seq_last=False, normalized_shape=H), Mamba(H, NST, 4)
    norm.load_state_dict({"weight": torch.from_numpy(p["norm.weight"]), "bias": torch.from_numpy(p["norm.bias"])})
    mamba.load_state_dict({k: torch.from_numpy(p[k]) for k in R.PARAMS})
    norm, mamba = norm.to(dev), mamba.to(dev)
    params = [norm.weight, norm.bias] + [dict(mamba.named_parameters())[k] for k in R.PARAMS]
    sd = {"n.weight": p["norm.weight"], "n.bias": p["norm.bias"]}
    sd.update({"m." + k: p[k] for k in R.PARAMS})
    w, keep = sn.pack_mamba(sd, "n", "m", dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    x = sn._new_bfth(nb, nf, nt, dev).normal_(generator=g).requires_grad_(True)
    tc = T.backward_chunk()
    result = {"metric": "IPDnet2 Mamba block, forward and backward", "unit": "ms", "dtype": "fp32", "data": "synthetic",
              "config": {"sequences": nb * nf, "frames": nt, "points": npts, "checkpoint_chunk": tc, "runs": args.runs,
                         "hbm_rate_for_floors_TBps": HBM / 1e12},
              "backward_workspace_gb": round(T._lib.load().fnssl_sn_mamba_backward_workspace_bytes(nb, nt, nf) / 2**30, 3),
              "checkpoint_gb": round(nb * nf * ((nt + tc - 1) // tc) * NST * E * 4 / 2**30, 3), "pool": {}}
    for pool in (1, 5):
        fl = floats_per_point(pool, tc)
        floor = {k: v * 4 * npts / HBM * 1e3 for k, v in fl.items()}
        dout = sn._new_bfth(nb, nf, nt // pool, dev).normal_(generator=g)
        with torch.no_grad():
            fwd_ms, _ = median_ms(lambda: sn.mamba(x.detach(), w, residual=True, time_pool=pool), args.runs, args.warmup)
        out = T.mamba_train(x, norm, mamba, residual=True, time_pool=pool)
        bwd = lambda: torch.autograd.grad(out, [x] + params, dout, retain_graph=True)   # noqa: E731
        bwd_ms, bwd_all = median_ms(bwd, args.runs, args.warmup)
        phases = {k: [] for k in PHASES}
        ops.timing_enable(True)
        for _ in range(args.runs):
            bwd()
            torch.cuda.synchronize()
            tm = ops.timing_collect()
            for k in PHASES:
                phases[k].append(tm[k]["ms"] / max(1, tm[k]["count"]))
        ops.timing_enable(False)
        del out
        # what a user has today: autograd through the restatement on the device
        pt = {k: v.detach().clone().requires_grad_(True) for k, v in zip(("norm.weight", "norm.bias") + R.PARAMS, params)}
        xt = x.detach().clone().requires_grad_(True)

        def torch_step():
            o = R.forward(pt, xt, True, pool)
            return torch.autograd.grad(o, [xt] + list(pt.values()), dout)

        base_ms, _ = median_ms(torch_step, args.baseline_runs, 1)
        result["pool"][str(pool)] = {
            "forward_ms": round(fwd_ms, 3), "forward_floor_ms": round(floor["sn_mamba (forward)"], 3),
            "backward_ms": round(bwd_ms, 3), "backward_ms_all": [round(t, 3) for t in bwd_all],
            "backward_floor_ms": round(sum(floor[k] for k in PHASES), 3),
            "backward_over_forward": round(bwd_ms / fwd_ms, 2),
            "phases": {k: {"ms": round(float(np.median(v)), 3), "floor_ms": round(floor[k], 3)} for k, v in phases.items()},
            "torch_autograd_forward_plus_backward_ms": round(base_ms, 1),
            "torch_autograd_over_kernels": round(base_ms / (fwd_ms + bwd_ms), 1),
        }
    result["peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 1)
    del keep
    line = json.dumps(result)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "r13", "mamba_train.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
