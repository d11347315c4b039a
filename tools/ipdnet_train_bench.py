#!/usr/bin/env python3
"""IPDnet training-step throughput at the BASELINE config-3 geometry (IPDnet(16, 256, 2, True): 8 microphones, 256 bins
x 300 frames, fp32, 64 utterances) with a per-kernel breakdown.  The step is the reference's loop through the drop-in
module: forward in train() mode, PIT-MSE loss (fnssl.ipdnet_step.PitMSE; its own time is reported as ``loss_ms``),
loss.backward(), torch.optim.Adam(lr=5e-4).  Secondary measurement —
bench.py's headline stays the inference metric.

    python tools/ipdnet_train_bench.py [--utts 64] [--frames 300] [--steps 3] [--warmup 1] [--offline]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fn-ssl_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from IPDnet.FixedAarryIPDnet import IPDnet  # noqa: E402
from fnssl import ops  # noqa: E402
from fnssl import weights as W  # noqa: E402
from fnssl.ipdnet_step import PitMSE  # noqa: E402

ROOF = 157.3e12          # fp32 MFMA peak of the MI355X (flop/s)


def step_flops(nc, online, nf, nt, nb):
    """Algorithmic flops of one step: LSTM forward, BPTT and weight gradients (the same matmul volume each), the conv
    head forward, its input gradient (into the 256 FN-block channels) and its weight gradient."""
    nh, nd = (256, 1) if online else (128, 2)
    lstm = (2 * 4 * 128 * (nc + 128) * 2 + 2 * 4 * nh * (256 + nc + nh) * nd + 2 * 4 * 128 * (256 + nc + 128) * 2
            + 2 * 4 * nh * (256 + nc + nh) * nd)
    cout = 2 * (nc // 2 - 1) * 2
    conv_f = 2 * 9 * ((256 + nc) * 128 + 128 * 128 / 3 + 128 * cout / 12)
    conv_d = 2 * 9 * (128 * 256 + 128 * 128 / 3 + cout * 128 / 12)
    pts = float(nb) * nf * nt
    return {"lstm_forward": lstm * pts, "lstm_backward": 2 * lstm * pts, "conv_forward": conv_f * pts,
            "conv_backward": (conv_d + conv_f) * pts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--mics", type=int, default=8)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--offline", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    nc, online = 2 * args.mics, not args.offline
    sd = W.make_ipdnet_state(3, nc, 256, 2, online)
    net = IPDnet(nc, 256, 2, online)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    net = net.to(dev).train()
    net.dropout_seed = 1
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    g = torch.Generator(device=dev)
    g.manual_seed(100)
    x = torch.randn((args.utts, nc, args.bins, args.frames), generator=g, device=dev) * 0.5
    gt = torch.tanh(torch.randn((args.utts, args.frames // 12, 2 * args.bins, nc // 2 - 1, 2), generator=g, device=dev))

    def step():
        opt.zero_grad(set_to_none=True)
        loss = PitMSE.apply(net(x), gt)
        loss.backward()
        opt.step()
        return loss

    losses = [float(step().item()) for _ in range(args.warmup)]
    ops.cluster_fallbacks(dev, reset=True)
    times = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = step()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
        losses.append(float(loss.item()))
    fallbacks = ops.cluster_fallbacks(dev)
    # the loss alone (fnssl_pit_mse_loss: error matrices, permutation, gradient, sum) on the network's strided output
    with torch.no_grad():
        pred = net(x)
    PitMSE.apply(pred, gt)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        PitMSE.apply(pred, gt)
    e1.record()
    torch.cuda.synchronize()
    loss_ms = e0.elapsed_time(e1) / 20
    del pred
    ops.timing_enable(True)
    step()
    torch.cuda.synchronize()
    tm = ops.timing_collect()
    ops.timing_enable(False)
    kern = {k: {"ms": round(v["ms"], 2), "count": v["count"],
                "frac_of_roof": round(v["flops"] / (v["ms"] * 1e-3) / ROOF, 3) if v["flops"] > 0 and v["ms"] > 0 else None}
            for k, v in sorted(tm.items(), key=lambda kv: -kv[1]["ms"])}
    fl = step_flops(nc, online, args.bins, args.frames, args.utts)
    total = sum(fl.values())
    ms = sorted(times)[len(times) // 2]
    print(json.dumps({
        "metric": "IPDnet training step (forward + PIT-MSE + backward + Adam)",
        "value": round(ms, 1), "unit": "ms/step", "n_gpus": 1, "dtype": "fp32", "data": "synthetic",
        "config": {"workload": "IPDnet(%d, 256, 2, %s) training step, %d utterances, %d bins x %d frames"
                   % (nc, online, args.utts, args.bins, args.frames)},
        "step_ms_all": [round(t, 1) for t in times], "loss_ms": round(loss_ms, 3),
        "tflop_per_step": {k: round(v / 1e12, 2) for k, v in fl.items()}, "tflop_per_step_total": round(total / 1e12, 2),
        "achieved_tflops": round(total / (ms * 1e-3) / 1e12, 1), "frac_of_fp32_mfma_roof": round(total / (ms * 1e-3) / ROOF, 3),
        "conv_backward_frac_of_roof": {k: kern[k]["frac_of_roof"] for k in ("conv3x3_dgrad", "conv3x3_wgrad") if k in kern},
        "cluster_fallbacks": fallbacks, "losses": [round(v, 6) for v in losses],
        "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2**30, 1), "kernels": kern}))


if __name__ == "__main__":
    main()
