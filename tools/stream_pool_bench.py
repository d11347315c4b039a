#!/usr/bin/env python3
"""What one push costs when S independent five-microphone IPDnet2 streams share a device: a ``StreamPool`` against S
dedicated ``OnlineLocalizer``s.

For S in {1, 8, 32, 64} and the shipped network (8 layers, deterministic weights) in fp32 and bf16, every stream is pushed
1 600 samples (100 ms: exactly one group of 5 frames), waveform to prediction.  The legs are timed with device events,
alternating in one process, in ``--rounds`` rounds of ``--per-round`` pushes after a warm-up; medians are reported:

    pool_full    StreamPool.push of all S slots in order: one front-end launch, the network in place (no gather, no scatter)
    pool_half    StreamPool.push of every second slot: one front-end launch, gather, the network on S / 2 rows, scatter
    sequential   the same S streams as S OnlineLocalizers (batch 1 each) pushed one after another: what the library offered
                 before the pool
    gather / scatter   fnssl_sn_state_rows alone on the S / 2 rows of pool_half, with the bytes it moves (each float is
                 read once and written once) and the bandwidth that gives

The expectation "the pool beats S sequential localizers from S = 8 on" is recorded beside the numbers as holding or failing;
nothing asserts it.  No CPU fallback: without a ROCm device this fails.

    python tools/stream_pool_bench.py [--rounds 5] [--per-round 40] [--json profiles/r19/stream_pool.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fn-ssl_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from stream_bench import alternate  # noqa: E402  (tools/stream_bench.py: the event timing and its statistics)

NCH = 5
PUSH = 1600            # 5 hops of 320
PUSH_MS = 100.0
PRIME = PUSH + 256     # frames 0..4 are complete, and every further push of 1600 samples completes exactly 5 more
SIZES = (1, 8, 32, 64)


def network(bf16, dev):
    from IPDnet2.IPDnet2 import OnlineSpatialNet
    from fnssl import weights as W
    net = OnlineSpatialNet(dim_input=2 * NCH, dim_output=16, num_layers=8, dim_hidden=96, num_heads=4, kernel_size=(5, 3),
                           conv_groups=(8, 8), norms=["LN", "LN", "GN", "LN", "LN", "LN"], dim_squeeze=8, num_freqs=256,
                           attention='mamba(16,4)', rope=False, time_compression_layer=0, fre_compression_ratio=16,
                           time_compression_ratio=5)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in W.make_ipdnet2_state(0).items()})
    return (net.bfloat16() if bf16 else net).to(dev).eval()


def case(net, S, rounds, per_round, dev):
    from fnssl import _lib, stream
    g = torch.Generator(device=dev)
    g.manual_seed(19)
    first = torch.randn((S, PRIME, NCH), generator=g, device=dev) * 0.05
    chunk = first[:, :PUSH]
    full, half = stream.StreamPool(net, NCH, S), stream.StreamPool(net, NCH, S)
    locs = [stream.OnlineLocalizer(net, stream.CentredStreamFrontEnd(NCH)) for _ in range(S)]
    every, second = list(range(S)), list(range(0, S, 2))
    with torch.no_grad():
        for pool in (full, half):
            assert [pool.open() for _ in range(S)] == every
            assert len(pool.push({s: first[s] for s in every})) == S
        for s, loc in enumerate(locs):
            assert loc.push(first[s:s + 1])[0] is not None

        def pool_full():
            assert len(full.push({s: chunk[s] for s in every})) == S

        def pool_half():
            assert len(half.push({s: chunk[s] for s in second})) == len(second)

        def sequential():
            for s, loc in enumerate(locs):
                assert loc.push(chunk[s:s + 1])[0] is not None

        legs = {"pool_full": pool_full, "sequential": sequential}
        if S > 1:
            pool_half()                                                   # allocates the compact state
            legs.update({"pool_half": pool_half,
                         "gather": lambda: half._rows(second, _lib.SN_ROWS_GATHER),
                         "scatter": lambda: half._rows(second, _lib.SN_ROWS_SCATTER)})   # (puts back what gather took)
        res = alternate(legs, rounds, per_round)
    assert (full.gathers, full.scatters) == (0, 0)
    slot_floats = _lib.load().fnssl_sn_state_floats(C.byref(full._dn.net), 1, 256)
    for name in ("gather", "scatter"):
        if name in res:
            moved = 2 * 4 * slot_floats * len(second)                     # every float read once and written once
            res[name]["rows"] = len(second)
            res[name]["bytes_moved"] = moved
            res[name]["gb_per_s"] = round(moved / (res[name]["median_us"] * 1e-6) / 1e9, 1)
    for name in ("pool_full", "pool_half", "sequential"):
        if name in res:
            streams = len(second) if name == "pool_half" else S
            res[name]["streams_pushed"] = streams
            res[name]["us_per_stream"] = round(res[name]["median_us"] / streams, 2)
            res[name]["real_time_factor"] = round(res[name]["median_us"] / (PUSH_MS * 1e3), 5)
    res["pool_full_over_sequential"] = round(res["pool_full"]["median_us"] / res["sequential"]["median_us"], 3)
    res["state_floats_per_slot"] = slot_floats
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=40)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "r19", "stream_pool.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("stream_pool_bench needs a ROCm device (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev), "microphones": NCH, "push_frames": 5, "push_samples": PUSH,
           "push_ms": PUSH_MS, "unit": "microseconds between device events around one push of all the leg's streams",
           "real_time_factor": "median time per push / 100 ms of signal",
           "expectation": "pool_full beats sequential from S = 8 on", "legs": {}}
    holds = True
    for name, bf16 in (("fp32", False), ("bf16", True)):
        net = network(bf16, dev)
        out["legs"][name] = {}
        for S in SIZES:
            res = case(net, S, args.rounds, args.per_round, dev)
            out["legs"][name]["S%d" % S] = res
            if S >= 8:
                holds = holds and res["pool_full_over_sequential"] < 1.0
            print(name, "S", S, json.dumps(res), flush=True)
    out["expectation_holds"] = holds
    print("expectation (pool_full beats sequential from S = 8 on):", "holds" if holds else "FAILS", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
