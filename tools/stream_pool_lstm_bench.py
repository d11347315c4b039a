#!/usr/bin/env python3
"""What one push costs when S independent four-microphone FN-SSL / IPDnet streams share a device: an ``LstmStreamPool``
against S dedicated ``OnlineLocalizer``s of the same build, in the same process.

For S in {1, 8, 32} and the two hop-256 models (FN-SSL 4-mic 'MM': 6 pairs per stream; IPDnet 4-mic, hidden 256; fp32,
deterministic weights) every stream is pushed 3 072 samples (192 ms: exactly one group of 12 frames), waveform to
prediction.  The legs are timed with device events, alternating, in ``--rounds`` rounds of ``--per-round`` pushes after a
warm-up; medians are reported:

    pool_full    LstmStreamPool.push of all S slots in order: one front-end launch, forward_stream in place on the pool's
                 state (no gather, no scatter)
    pool_half    LstmStreamPool.push of every second slot: one front-end launch, gather, forward_stream on S / 2 streams,
                 scatter
    sequential   the same S streams as S OnlineLocalizers (batch 1 each) pushed one after another: what the library offered
                 before the pool
    gather / scatter   fnssl_state_rows alone on the S / 2 rows of pool_half, with the bytes it moves (each float is read
                 once and written once) and the bandwidth that gives

Nothing is asserted about the figures.  No CPU fallback: without a ROCm device this fails.

    python tools/stream_pool_lstm_bench.py [--rounds 3] [--per-round 10] [--json profiles/r20/stream_pool_lstm.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fn-ssl_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from stream_bench import alternate  # noqa: E402  (tools/stream_bench.py: the event timing and its statistics)

NCH = 4
PUSH = 3072            # 12 hops of 256
PUSH_MS = 192.0
PRIME = PUSH + 256     # frames 0..11 are complete, and every further push of 3072 samples completes exactly 12 more
SIZES = (1, 8, 32)


def network(kind, dev):
    """-> (net, front-end mode) as tools/stream_bench.py builds them."""
    from fnssl import weights as W
    if kind == "fnssl_4mic_MM":
        import Model
        net = Model.FN_SSL()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_fnssl_state(0).items()})
        mode = "pair"
    else:
        from IPDnet.FixedAarryIPDnet import IPDnet
        net = IPDnet(2 * NCH, 256, 2, True)
        net.load_state_dict({k: torch.from_numpy(np.array(v, dtype=np.float32))
                             for k, v in W.make_ipdnet_state(0, 2 * NCH, 256, 2, True).items()})
        mode = "array"
    return net.to(dev).eval(), mode


def case(net, mode, S, rounds, per_round, dev):
    from fnssl import _lib, stream
    g = torch.Generator(device=dev)
    g.manual_seed(20)
    first = torch.randn((S, PRIME, NCH), generator=g, device=dev) * 0.05
    chunk = first[:, :PUSH]
    full, half = stream.LstmStreamPool(net, NCH, S, "MM"), stream.LstmStreamPool(net, NCH, S, "MM")
    locs = [stream.OnlineLocalizer(net, stream.StreamFrontEnd(mode, NCH, "MM")) for _ in range(S)]
    every, second = list(range(S)), list(range(0, S, 2))
    with torch.no_grad():
        for pool in (full, half):
            assert [pool.open() for _ in range(S)] == every
            assert len(pool.push({s: first[s] for s in every})) == S      # the fresh set: through gather and scatter, once
        for s, loc in enumerate(locs):
            assert loc.push(first[s:s + 1])[0] is not None
        primed = (full.gathers, full.scatters)

        def pool_full():
            assert len(full.push({s: chunk[s] for s in every})) == S

        def pool_half():
            assert len(half.push({s: chunk[s] for s in second})) == len(second)

        def sequential():
            for s, loc in enumerate(locs):
                assert loc.push(chunk[s:s + 1])[0] is not None

        legs = {"pool_full": pool_full, "sequential": sequential}
        if S > 1:
            legs.update({"pool_half": pool_half,
                         "gather": lambda: half._rows(half._pool, half._compact, second, _lib.SN_ROWS_GATHER),
                         "scatter": lambda: half._rows(half._pool, half._compact, second, _lib.SN_ROWS_SCATTER)})   # (puts back what gather took)
        res = alternate(legs, rounds, per_round, warm=5)
    assert (full.gathers, full.scatters) == primed                        # every timed push of the full set ran in place
    table = full._segments(full._pool, full._compact)
    slot_floats = sum(int(seg.row_floats) for seg in table)
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
    res["state_segments"] = len(table)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--per-round", type=int, default=10)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "r20", "stream_pool_lstm.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("stream_pool_lstm_bench needs a ROCm device (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev), "microphones": NCH, "push_frames": 12, "push_samples": PUSH,
           "push_ms": PUSH_MS, "rounds": args.rounds, "per_round": args.per_round,
           "unit": "microseconds between device events around one push of all the leg's streams",
           "real_time_factor": "median time per push / 192 ms of signal", "legs": {}}
    for kind in ("fnssl_4mic_MM", "ipdnet_4mic"):
        net, mode = network(kind, dev)
        out["legs"][kind] = {}
        for S in SIZES:
            res = case(net, mode, S, args.rounds, args.per_round, dev)
            out["legs"][kind]["S%d" % S] = res
            print(kind, "S", S, json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
