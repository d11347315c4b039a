#!/usr/bin/env python3
"""Forward and backward of the f-conv branch, the full-band branch and a whole SpatialNetLayer at BASELINE config 5's
shapes (64 utterances x 250 frames, fp32): layer 0's fconv1 (256 bins, pooled by 2), full (128 bins) and fconv2 (128 bins,
pooled by 8); layers 1-7's branches (16 bins, 64 x 50 frames); ``layer_train`` for layer 0 (time pooling 5) and for a
layer 1-7.  Each figure stands next to the time its compulsory HBM traffic would take and next to torch autograd of the
restatement (tests/layer_train_ref.py) on the same device — what a user has without the kernels.  Medians of --runs runs
after --warmup, device events on the compute stream.  Secondary measurement: bench.py's headline stays the inference metric.

Every case runs in a child process of its own under its own time limit (--limit seconds); this process never opens the
device, and stops at the first case that fails.

    python tools/layer_train_bench.py [--utts 64] [--frames 250] [--runs 10] [--warmup 2] [--limit 240] [--out FILE]
    python tools/layer_train_bench.py --case fconv1_l0      # one case, in this process: prints its JSON
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), ROOT, os.path.join(ROOT, "fn-ssl_amd")):
    sys.path.insert(0, p)

HBM = 6.29e12            # measured copy rate of the MI355X (8.0 TB/s spec), bytes/s
H = 96
# case: (kind, bins, frames divisor, pool / time_pool)
CASES = {
    "fconv1_l0": ("fconv", 256, 1, 2),
    "full_l0": ("full", 128, 1, 1),
    "fconv2_l0": ("fconv", 128, 1, 8),
    "fconv_l1": ("fconv", 16, 5, 1),
    "full_l1": ("full", 16, 5, 1),
    "layer_0": ("layer", 256, 1, 5),
    "layer_1": ("layer", 16, 5, 1),
}
PHASES = {"fconv": ("sn_fconv_bwd", "sn_fconv_bwd_reduce"), "full": ("sn_full_bwd", "sn_full_bwd_reduce")}


def branch_floor_ms(kind, npts, pool):
    """Compulsory traffic of a branch: forward reads x and writes out; backward reads x and dout and writes dx."""
    row = H * 4.0 * npts / HBM * 1e3
    return row * (1 + 1.0 / pool), row * (2 + 1.0 / pool)


def run_case(name, args):
    import numpy as np
    import torch

    import layer_train_ref as R
    import mamba_train_bench as MB
    from IPDnet2.IPDnet2 import SpatialNetLayer
    from fnssl import ops
    from fnssl import spatialnet as sn
    from fnssl import spatialnet_train as T
    from fnssl import weights as W

    kind, nf, tdiv, pool = CASES[name]
    nb, nt = args.utts, args.frames // tdiv
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    first = kind == "layer" and nf == 256
    nfull = nf // 2 if first else nf
    sd = W.make_ipdnet2_state(0, num_layers=2)
    p = R.leg_params("layer", ("", nb, nf, nt, first, 1, "frame", None), sd)
    layer = SpatialNetLayer(dim_hidden=96, dim_squeeze=8, num_freqs=nfull, dropout=(0, 0, 0), kernel_size=(5, 3),
                            conv_groups=(8, 8), norms=["LN"] * 6, attention="mamba(16,4)", is_first=first)
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    layer = layer.to(dev).train()
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    x = sn._new_bfth(nb, nf, nt, dev).normal_(generator=g).requires_grad_(True)
    npts = nb * nf * nt
    pt = {k: v.detach().clone().requires_grad_(True) for k, v in layer.named_parameters()}
    if kind == "fconv":
        params = list(layer.fconv1.parameters())
        fwd = lambda: T.fconv_train(x, layer.fconv1, True, pool)   # noqa: E731
        ref = lambda xt: R.fconv_forward(pt, xt, True, pool, pre="fconv1.")   # noqa: E731
        ref_params = [pt["fconv1." + k] for k in R.FCONV_PARAMS]
        floor_f, floor_b = branch_floor_ms(kind, npts, pool)
    elif kind == "full":
        params = [layer.get_parameter(k) for k in R.FULL_PARAMS]
        fwd = lambda: T.full_train(x, layer, True)   # noqa: E731
        ref = lambda xt: R.full_forward(pt, xt, True)   # noqa: E731
        ref_params = [pt[k] for k in R.FULL_PARAMS]
        floor_f, floor_b = branch_floor_ms(kind, npts, 1)
    else:
        params = list(layer.parameters())
        fwd = lambda: T.layer_train(layer, x, pool)   # noqa: E731
        ref = lambda xt: R.layer_forward(pt, xt, first, pool)   # noqa: E731
        ref_params = list(pt.values())
        n1 = npts // 2 if first else npts                    # points after fconv1, after fconv2
        n2 = n1 // 8 if first else n1
        f1 = branch_floor_ms("fconv", npts, 2 if first else 1)
        f2 = branch_floor_ms("full", n1, 1)
        f3 = branch_floor_ms("fconv", n1, 8 if first else 1)
        tc = T.backward_chunk()
        mf = [MB.floats_per_point(q, tc) for q in (1, pool)]
        m_f = sum(m["sn_mamba (forward)"] for m in mf) * 4.0 * n2 / HBM * 1e3
        m_b = sum(m[k] for m in mf for k in MB.PHASES) * 4.0 * n2 / HBM * 1e3
        floor_f, floor_b = f1[0] + f2[0] + f3[0] + m_f, f1[1] + f2[1] + f3[1] + m_b
    with torch.no_grad():
        fwd_ms, _ = MB.median_ms(fwd, args.runs, args.warmup)
    out = fwd()
    dout = torch.empty_like(out).normal_(generator=g)
    bwd = lambda: torch.autograd.grad(out, [x] + params, dout, retain_graph=True)   # noqa: E731
    bwd_ms, bwd_all = MB.median_ms(bwd, args.runs, args.warmup)
    res = {"shape": {"utterances": nb, "bins": nf, "frames": nt, "points": npts, "pool": pool},
           "forward_ms": round(fwd_ms, 3), "forward_floor_ms": round(floor_f, 3),
           "backward_ms": round(bwd_ms, 3), "backward_ms_all": [round(t, 3) for t in bwd_all],
           "backward_floor_ms": round(floor_b, 3), "backward_over_forward": round(bwd_ms / fwd_ms, 2),
           "backward_over_floor": round(bwd_ms / floor_b, 2)}
    if kind in PHASES:
        ph = {k: [] for k in PHASES[kind]}
        ops.timing_enable(True)
        for _ in range(args.runs):
            bwd()
            torch.cuda.synchronize()
            tm = ops.timing_collect()
            for k in ph:
                ph[k].append(tm[k]["ms"] / max(1, tm[k]["count"]))
        ops.timing_enable(False)
        res["phases"] = {k: round(float(np.median(v)), 3) for k, v in ph.items()}
        res["backward_workspace_mb"] = round(getattr(T._lib.load(), "fnssl_sn_%s_backward_workspace_bytes" % kind)(nb, nt, nf)
                                             / 2**20, 2)
    del out
    xt = x.detach().clone().requires_grad_(True)

    def torch_step():
        return torch.autograd.grad(ref(xt), [xt] + ref_params, dout)

    base_ms, _ = MB.median_ms(torch_step, args.baseline_runs, 1)
    res["torch_autograd_forward_plus_backward_ms"] = round(base_ms, 2)
    res["torch_autograd_over_kernels"] = round(base_ms / (fwd_ms + bwd_ms), 1)
    res["peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per case")
    ap.add_argument("--case", default=None, choices=sorted(CASES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.case:
        print(json.dumps(run_case(args.case, args)))
        return
    result = {"metric": "IPDnet2 f-conv, full-band branch and layer, forward and backward", "unit": "ms", "dtype": "fp32",
              "data": "synthetic", "config": {"utterances": args.utts, "frames": args.frames, "runs": args.runs,
                                              "hbm_rate_for_floors_TBps": HBM / 1e12}, "cases": {}}
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name] + [
            "--%s=%d" % (k, getattr(args, k.replace("-", "_"))) for k in ("utts", "frames", "runs", "warmup", "baseline-runs")]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("layer_train_bench: case %s ran past its %d s limit; stopping" % (name, args.limit))
        if r.returncode != 0:
            raise SystemExit("layer_train_bench: case %s failed with status %d; stopping" % (name, r.returncode))
        result["cases"][name] = json.loads(r.stdout.strip().splitlines()[-1])
        print(name, json.dumps(result["cases"][name]), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "r14", "layer_train.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
