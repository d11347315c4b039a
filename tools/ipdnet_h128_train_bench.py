#!/usr/bin/env python3
"""Training of the default IPDnet (``IPDnet()``: two microphones, hidden_size 128 — full-band BiLSTM H = 64, online
narrow-band LSTM H = 128) at the reference's training size, 16 utterances x 2 microphones x 256 bins x 280 frames, on one
device.  A record, not a gate: the capability is new, the numbers say where it stands.

    hip      the drop-in on the HIP path: ``forward_train``, ``loss.backward()`` and the whole
             ``MyModel(train_on_device=True).training_step`` + Adam(lr 5e-4) from the waveforms; the ``TimedLaunch``
             totals of one step per phase (the four LSTM forwards, the four BPTTs, the weight gradients, the conv head);
             peak memory
    layers   every LSTM of the train graph alone, operands in the graph's natural layouts: reserve-saving forward and
             BPTT against their fp32-MFMA time (flops / 157.3 Tflop/s) — how far the one-wave-per-group H = 64 BPTT sits
             from it
    torch    torch-ROCm autograd of the same network (tests/ipdnet_train_ref.RefIPDnet: nn.LSTM / nn.Conv2d, the same
             keep-scale dropout masks, ATen PIT-MSE, Adam) on the same device: the only route a user had

Medians of ``--runs`` runs after ``--warmup`` warm-up runs, device events, every case in a process of its own.

    python tools/ipdnet_h128_train_bench.py [--out profiles/r17/ipdnet_h128_train.json] [--runs 10] [--warmup 2]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "fn-ssl_amd")):
    sys.path.insert(0, p)

ROOF = 157.3e12          # fp32 MFMA peak of the MI355X (flop/s)
NB, NC, NF, NT, HIDDEN = 16, 4, 256, 280, 128
BASE = 77


def _median(v):
    return sorted(v)[len(v) // 2]


def _timed(fn, runs, warmup, before=None):
    """Median device time (ms) of ``fn`` over ``runs`` runs after ``warmup``; ``before`` runs untimed ahead of each."""
    import torch
    out = []
    for i in range(warmup + runs):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1))
    return round(_median(out), 3), [round(t, 3) for t in out]


def _state():
    import torch
    from fnssl import weights as W
    return {k: torch.from_numpy(v.copy()) for k, v in W.make_ipdnet_state(3, NC, HIDDEN, 2, True).items()}


def _features(dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(100)
    x = torch.randn((NB, NC, NF, NT), generator=g, device=dev) * 0.5
    gt = torch.tanh(torch.randn((NB, NT // 12, 2 * NF, NC // 2 - 1, 2), generator=g, device=dev))
    return x, gt


def case_hip(runs, warmup):
    import torch
    from IPDnet.train_step import MyModel
    from fnssl import ops
    from fnssl.ipdnet_step import PitMSE
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model = MyModel(arch=None, train_on_device=True, device="cuda:0")
    model.arch.load_state_dict(_state())
    model = model.to(dev).train()
    net = model.arch
    net.dropout_seed = 1
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    x, gt = _features(dev)
    ns = 512 + (NT - 1) * 256
    g = torch.Generator(device=dev).manual_seed(101)
    dp = torch.randn((NB, ns, NC // 2, 2), generator=g, device=dev) * 0.05
    sig = dp.sum(dim=3) + torch.randn((NB, ns, NC // 2), generator=g, device=dev) * 0.025
    doa = torch.stack((torch.rand((NB, NT // 12, 2), generator=g, device=dev) * 2.7 + 0.2,
                       torch.rand((NB, NT // 12, 2), generator=g, device=dev) * 6.28 - 3.14), dim=2)
    batch = (sig, {"doa": doa, "dp_signal": dp})
    res = {}
    ops.cluster_fallbacks(dev, reset=True)
    hold = {}

    def fwd():
        hold["loss"] = PitMSE.apply(net.forward_train(x), gt)

    res["forward_train_ms"], res["forward_train_ms_all"] = _timed(fwd, runs, warmup)
    res["backward_ms"], res["backward_ms_all"] = _timed(lambda: hold["loss"].backward(), runs, warmup,
                                                        before=lambda: (opt.zero_grad(set_to_none=True), fwd()))

    def step():
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(batch, 0)["loss"]
        loss.backward()
        opt.step()
        hold["step_loss"] = loss

    torch.cuda.reset_peak_memory_stats()
    res["training_step_adam_ms"], res["training_step_adam_ms_all"] = _timed(step, runs, warmup)
    res["peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
    res["last_loss"] = round(float(hold["step_loss"].item()), 6)
    res["cluster_fallbacks"] = ops.cluster_fallbacks(dev)
    ops.timing_enable(True)
    step()
    torch.cuda.synchronize()
    tm = ops.timing_collect()
    ops.timing_enable(False)
    res["kernels"] = {k: {"ms": round(v["ms"], 3), "count": v["count"],
                          "frac_of_roof": round(v["flops"] / (v["ms"] * 1e-3) / ROOF, 3)
                          if v["flops"] > 0 and v["ms"] > 0 else None}
                      for k, v in sorted(tm.items(), key=lambda kv: -kv[1]["ms"])}
    phase = {"lstm_forward (4 layers)": ("lstm_h64", "lstm_h128"), "lstm_bptt (4 layers)": ("lstm_bwd_h64", "lstm_bwd_h128")}
    res["phases_ms"] = {p: round(sum(tm[n]["ms"] for n in names if n in tm), 3) for p, names in phase.items()}
    res["phases_ms"]["lstm_weight_grads"] = round(sum(v["ms"] for k, v in tm.items() if "wgrad" in k and "conv" not in k), 3)
    res["phases_ms"]["conv_head (forward + backward)"] = round(sum(v["ms"] for k, v in tm.items()
                                                                   if "conv" in k or "pool" in k), 3)
    res["phases_ms"]["everything timed"] = round(sum(v["ms"] for v in tm.values()), 3)
    return res


def case_layers(runs, warmup):
    import torch
    from IPDnet.FixedAarryIPDnet import IPDnet
    from fnssl import ipdnet_train, ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    net = IPDnet()
    net.load_state_dict(_state())
    net = net.to(dev).train()
    g = ipdnet_train.IPDnetTrainGraph(net)
    fw, bw, _, _ = g.streams(dev)
    gen = torch.Generator(device=dev).manual_seed(102)
    res = {}
    for L in g.lstms:
        nseq, nsteps = (NB * NT, NF) if L.mode == "full" else (NB * NF, NT)
        x0 = L.natural(NB, NT, NF, L.c0, dev).normal_(0, 0.5, generator=gen)
        x2 = L.natural(NB, NT, NF, L.c2, dev).normal_(0, 0.5, generator=gen) if L.c2 else None
        rsv = torch.empty(ops.lstm_reserve_floats(nseq, L.hidden, L.ndir, nsteps), device=dev)
        out = L.natural(NB, NT, NF, L.ndir * L.hidden, dev)
        dh = L.natural(NB, NT, NF, L.ndir * L.hidden, dev).normal_(0, 1, generator=gen)
        da = L.natural(NB, NT, NF, L.ndir * 4 * L.hidden, dev)
        dx = L.natural(NB, NT, NF, L.ndir * L.c0g, dev) if L.c0g else None
        fams = (ops.lstm_plan(L.mode, x0, None, x2, fw[L.name], L.hidden, out, reserve=rsv)[0],
                ops.lstm_backward(L.mode, rsv, dh, da, dx, bw[L.name], L.hidden, L.c0g, plan_only=True))
        f_ms, _ = _timed(lambda: ops.lstm_layer(L.mode, x0, None, x2, fw[L.name], L.hidden, out, reserve=rsv), runs, warmup)
        b_ms, _ = _timed(lambda: ops.lstm_backward(L.mode, rsv, dh, da, dx, bw[L.name], L.hidden, L.c0g), runs, warmup)
        pts = float(nseq) * nsteps * L.ndir
        f_fl = 2.0 * 4 * L.hidden * (L.c0 + L.c2 + L.hidden) * pts
        b_fl = 2.0 * 4 * L.hidden * (L.c0g + L.hidden) * pts
        groups = (nseq + 15) // 16 * L.ndir
        res[L.name] = {"shape (mode, H, ndir, c0, c2, c0g)": [L.mode, L.hidden, L.ndir, L.c0, L.c2, L.c0g],
                       "families": list(fams), "groups_x_dirs": groups,
                       "forward_ms": f_ms, "forward_mfma_ms": round(f_fl / ROOF * 1e3, 3),
                       "forward_frac_of_roof": round(f_fl / (f_ms * 1e-3) / ROOF, 3),
                       "bptt_ms": b_ms, "bptt_mfma_ms": round(b_fl / ROOF * 1e3, 3),
                       "bptt_frac_of_roof": round(b_fl / (b_ms * 1e-3) / ROOF, 3)}
        del x0, x2, rsv, out, dh, da, dx
        ops.release_workspaces()
        torch.cuda.empty_cache()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    res["device"] = {"cus": cus, "simds": 4 * cus}
    res["cluster_fallbacks"] = ops.cluster_fallbacks(dev)
    return res


def case_torch(runs, warmup):
    import torch
    import ipdnet_train_ref as R
    from fnssl import ipdnet_train, train
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ref = R.RefIPDnet(NC, HIDDEN, 2, True)
    ref.load_state_dict(_state())
    ref = ref.to(dev).train()
    opt = torch.optim.Adam(ref.parameters(), lr=5e-4)
    x, gt = _features(dev)
    masks = [train.dropout_scale((NB, NT, NF, HIDDEN), s, dev) for s in ipdnet_train.site_seeds(BASE)]
    hold = {}

    def fwd():
        hold["loss"] = R.pit_mse(ref(x, masks), gt)

    res = {}
    res["forward_ms"], res["forward_ms_all"] = _timed(fwd, runs, warmup)
    res["backward_ms"], res["backward_ms_all"] = _timed(lambda: hold["loss"].backward(), runs, warmup,
                                                        before=lambda: (opt.zero_grad(set_to_none=True), fwd()))

    def step():
        opt.zero_grad(set_to_none=True)
        fwd()
        hold["loss"].backward()
        opt.step()

    torch.cuda.reset_peak_memory_stats()
    res["step_adam_ms"], res["step_adam_ms_all"] = _timed(step, runs, warmup)
    res["peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)
    res["last_loss"] = round(float(hold["loss"].item()), 6)
    res["note"] = "features and targets given (no front end, no target kernels): forward + ATen PIT-MSE + backward + Adam"
    return res


CASES = {"hip": case_hip, "layers": case_layers, "torch": case_torch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "ipdnet_h128_train.json"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", choices=sorted(CASES), help="(internal) run one case in this process, print its JSON")
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(CASES[args.case](args.runs, args.warmup)))
        return 0
    doc = {"metric": "IPDnet() training at the reference's size on one MI355X",
           "shape": {"utterances": NB, "microphones": NC // 2, "bins": NF, "frames": NT, "hidden_size": HIDDEN,
                     "online": True, "dtype": "fp32", "data": "synthetic"},
           "method": "median of %d runs after %d warm-up runs, device events, one process per case" % (args.runs, args.warmup)}
    for case in ("hip", "layers", "torch"):        # a fresh child each: the parent never opens the device
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--runs", str(args.runs),
                            "--warmup", str(args.warmup)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=420)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print("case %s failed (exit %d): nothing further is started" % (case, r.returncode))
            return 1
        doc[case] = json.loads(lines[-1][len("RESULT "):])
    h, t = doc["hip"], doc["torch"]
    doc["summary"] = {"hip forward_train + backward (ms)": round(h["forward_train_ms"] + h["backward_ms"], 3),
                      "torch forward + backward (ms)": round(t["forward_ms"] + t["backward_ms"], 3),
                      "hip training_step + Adam from waveforms (ms)": h["training_step_adam_ms"],
                      "torch step + Adam from features (ms)": t["step_adam_ms"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["summary"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
