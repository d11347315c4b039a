#!/usr/bin/env python3
"""Training of the whole IPDnet2 network at BASELINE config 5's shapes (64 utterances x 250 frames x 256 bins, the shipped
8-layer net, fp32): forward and backward of the encoder and of the head, a whole ``forward_train`` + ``backward``, and a
whole ``training_step`` + ``backward`` + AdamW step of ``run_step.MyModel(train_on_device=True)``, with the per-phase
``TimedLaunch`` times of one network backward.  Next to the times: the time each operator's compulsory HBM traffic would
take at the chip's measured copy rate, torch autograd of the restatement (tests/net_train_ref.py) on the same device —
the only route a user had — and ``torch.cuda.max_memory_allocated()``.  Medians of --runs runs after --warmup, device
events on the compute stream.  Secondary measurement: bench.py's headline stays the inference metric.

Every case runs in a child process of its own under its own time limit (--limit seconds); this process never opens the
device, and stops at the first case that fails.

    python tools/net_train_bench.py [--utts 64] [--frames 250] [--layers 8] [--runs 10] [--warmup 2] [--limit 400] [--out FILE]
    python tools/net_train_bench.py --case encoder      # one case, in this process: prints its JSON
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
H, CIN, NF, RATIO = 96, 10, 256, 5
CASES = ("encoder", "head", "net", "step", "net_torch")


def make_net(sd, layers, dev):
    import torch
    from IPDnet2.IPDnet2 import OnlineSpatialNet
    net = OnlineSpatialNet(dim_input=CIN, dim_output=16, num_layers=layers, dim_hidden=96, num_heads=4, kernel_size=(5, 3),
                           conv_groups=(8, 8), norms=["LN", "LN", "GN", "LN", "LN", "LN"], dim_squeeze=8, num_freqs=NF,
                           attention='mamba(16,4)', rope=False, time_compression_layer=0, fre_compression_ratio=16,
                           time_compression_ratio=RATIO)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    return net.to(dev).train()


def run_case(name, args):
    import numpy as np
    import torch

    import mamba_train_bench as MB
    import net_train_ref as R
    from fnssl import ops
    from fnssl import spatialnet as sn
    from fnssl import spatialnet_train as T
    from fnssl import weights as W

    nb, nt, nl = args.utts, args.frames, args.layers
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    sd = W.make_ipdnet2_state(0, num_layers=nl)
    net = make_net(sd, nl, dev)
    res = {}

    def phases(fn, prefix):
        ops.timing_enable(True)
        acc = {}
        for _ in range(args.runs):
            fn()
            torch.cuda.synchronize()
            for k, v in ops.timing_collect().items():
                if k.startswith(prefix) and v["count"]:
                    acc.setdefault(k, []).append(v["ms"])
        ops.timing_enable(False)
        return {k: round(float(np.median(v)), 3) for k, v in sorted(acc.items())}

    if name == "encoder":
        x = torch.empty((nb, CIN, NF, nt), device=dev).normal_(generator=g)
        npts = nb * NF * nt
        fwd = lambda: T.encoder_train(x, net.encoder)   # noqa: E731
        params = [net.encoder.weight, net.encoder.bias]
        floor_f = 4.0 * (x.numel() + npts * H) / HBM * 1e3
        floor_b = 4.0 * (npts * H + x.numel() + CIN * 5 * H + H) / HBM * 1e3          # dY + x in, dW | db out
        pt = {k: v.detach().clone().requires_grad_(True) for k, v in (("w", params[0]), ("b", params[1]))}
        ref = lambda: R.encoder_forward(pt["w"], pt["b"], x)   # noqa: E731
        ref_params = list(pt.values())
        prefix = "sn_encoder_bwd"
        res["backward_workspace_mb"] = round(T._lib.load().fnssl_sn_encoder_backward_workspace_bytes(nb, CIN, NF, nt) / 2**20, 2)
    elif name == "head":
        nfc, nt2 = NF // 16, nt // RATIO
        x = sn._new_bfth(nb, nfc, nt2, dev).normal_(generator=g).requires_grad_(True)
        npts = nb * nfc * nt2
        fwd = lambda: T.head_train(x, net.freq_inverse, net.decoder)   # noqa: E731
        params = [x, net.freq_inverse.trans2.weight, net.freq_inverse.trans2.bias, net.decoder.weight, net.decoder.bias]
        floor_f = 4.0 * npts * (H + 256) / HBM * 1e3
        floor_b = 4.0 * npts * (H + 256 + H) / HBM * 1e3                              # x + dout in, dx out
        pt = {k: net.get_parameter(k).detach().clone().requires_grad_(True) for k in R.HEAD_PARAMS}
        ref = lambda: R.head_forward(pt, x)   # noqa: E731
        ref_params = [x] + list(pt.values())
        prefix = "sn_head_bwd"
        res["backward_workspace_mb"] = round(T._lib.load().fnssl_sn_head_backward_workspace_bytes(nb, nt2, nfc) / 2**20, 2)
    if name in ("encoder", "head"):
        with torch.no_grad():
            fwd_ms, _ = MB.median_ms(fwd, args.runs, args.warmup)
        out = fwd()
        dout = torch.empty_like(out).normal_(generator=g)
        bwd = lambda: torch.autograd.grad(out, params, dout, retain_graph=True)   # noqa: E731
        bwd_ms, bwd_all = MB.median_ms(bwd, args.runs, args.warmup)
        res.update({"points": npts, "forward_ms": round(fwd_ms, 3), "forward_floor_ms": round(floor_f, 3),
                    "backward_ms": round(bwd_ms, 3), "backward_ms_all": [round(t, 3) for t in bwd_all],
                    "backward_floor_ms": round(floor_b, 3), "backward_over_floor": round(bwd_ms / floor_b, 2),
                    "phases": phases(bwd, prefix)})
        if name == "encoder":                                # dx is its own launch, asked for only when x requires a gradient
            xg = x.detach().requires_grad_(True)
            out_g = T.encoder_train(xg, net.encoder)
            with_dx = lambda: torch.autograd.grad(out_g, [xg] + params, dout, retain_graph=True)   # noqa: E731
            dx_ms, _ = MB.median_ms(with_dx, args.runs, args.warmup)
            res["backward_with_dx_ms"] = round(dx_ms, 3)
            res["phases_with_dx"] = phases(with_dx, prefix)
            del out_g, xg
        base_ms, _ = MB.median_ms(lambda: torch.autograd.grad(ref(), ref_params, dout), args.baseline_runs, 1)
        res["torch_autograd_forward_plus_backward_ms"] = round(base_ms, 2)
        res["torch_autograd_over_kernels"] = round(base_ms / (fwd_ms + bwd_ms), 1)
    elif name in ("net", "net_torch"):
        x = torch.empty((nb, CIN, NF, nt), device=dev).normal_(generator=g)
        params = list(net.parameters())
        dout = torch.empty((nb, nt // RATIO, 2 * NF, 4, 2), device=dev).normal_(generator=g)
        if name == "net":
            with torch.no_grad():
                fwd_ms, _ = MB.median_ms(lambda: net.forward_train(x), args.runs, args.warmup)
            both = lambda: torch.autograd.grad(net.forward_train(x), params, dout)   # noqa: E731
            both_ms, both_all = MB.median_ms(both, args.runs, args.warmup)
            res.update({"parameters": len(params), "forward_ms": round(fwd_ms, 3), "forward_plus_backward_ms": round(both_ms, 3),
                        "forward_plus_backward_ms_all": [round(t, 3) for t in both_all],
                        "backward_ms": round(both_ms - fwd_ms, 3), "phases": phases(both, "sn_")})
        else:
            pt = {k: v.detach().clone().requires_grad_(True) for k, v in net.named_parameters()}
            ref = lambda: torch.autograd.grad(R.net_forward(pt, x, nl), list(pt.values()), dout)   # noqa: E731
            base_ms, _ = MB.median_ms(ref, args.baseline_runs, 1)
            res["torch_autograd_forward_plus_backward_ms"] = round(base_ms, 2)
    elif name == "step":
        import importlib.util
        import ipdnet2_eval_ref as R2
        spec = importlib.util.spec_from_file_location("fnssl_ipdnet2_run_step_bench", os.path.join(ROOT, "fn-ssl_amd", "IPDnet2", "run_step.py"))
        RS = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(RS)
        model = RS.MyModel(device="cuda:0", arch=net, train_on_device=True).to(dev).train()
        rng = np.random.RandomState(4501)
        ntg = nt // RATIO
        mic = R2.G21_MICS["mic5"]
        batch = [torch.from_numpy(a).to(dev) for a in (
            (rng.standard_normal((nb, 320 * (nt - 1), 5)) * 0.05).astype(np.float32),
            rng.uniform(-170.0, 170.0, (nb, ntg, 2)).astype(np.float32), np.ones((nb, ntg, 2), np.float32),
            np.repeat(mic[None], nb, axis=0), rng.uniform(0.5, 3.0, (nb, ntg, 2)).astype(np.float32))]
        opt = model.configure_optimizers()["optimizer"]
        losses = []

        def step():
            opt.zero_grad(set_to_none=True)
            loss = model.training_step(batch, 0)["loss"]
            loss.backward()
            opt.step()
            losses.append(loss.detach())

        ms, ms_all = MB.median_ms(step, args.runs, args.warmup)
        res.update({"training_step_backward_adamw_ms": round(ms, 3), "ms_all": [round(t, 3) for t in ms_all],
                    "loss_first": float(losses[0]), "loss_last": float(losses[-1])})
    res["peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="seconds per case")
    ap.add_argument("--case", default=None, choices=CASES)
    ap.add_argument("--skip", default="", help="comma-separated cases to leave out (recorded as not measured)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.case:
        print(json.dumps(run_case(args.case, args)))
        return
    result = {"metric": "IPDnet2 network training: encoder, head, forward_train + backward, training step", "unit": "ms",
              "dtype": "fp32", "data": "synthetic",
              "config": {"utterances": args.utts, "frames": args.frames, "bins": NF, "layers": args.layers, "runs": args.runs,
                         "hbm_rate_for_floors_TBps": HBM / 1e12}, "cases": {}}
    out = args.out or os.path.join(ROOT, "profiles", "r15", "net_train.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    for name in CASES:
        if name in args.skip.split(","):
            result["cases"][name] = "not measured"
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name] + [
            "--%s=%d" % (k, getattr(args, k.replace("-", "_"))) for k in ("utts", "frames", "layers", "runs", "warmup", "baseline-runs")]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("net_train_bench: case %s ran past its %d s limit; stopping" % (name, args.limit))
        if r.returncode != 0:
            raise SystemExit("net_train_bench: case %s failed with status %d; stopping" % (name, r.returncode))
        result["cases"][name] = json.loads(r.stdout.strip().splitlines()[-1])
        print(name, json.dumps(result["cases"][name]), flush=True)
        with open(out, "w") as f:                            # after every case: what was measured is kept
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
