#!/usr/bin/env python3
"""What one 5-frame push (1 600 samples = 100 ms of signal) costs online with IPDnet2, microphone samples in.

One utterance, the shipped five-microphone network (8 layers, deterministic weights), fp32 and bf16.  Three legs are timed
with device events, alternating in one process, in ``--rounds`` rounds of ``--per-round`` pushes each, every push
completing exactly one group of 5 frames:

    frontend     CentredStreamFrontEnd.push                      (ONE launch of fnssl_stream_frontend_centred + the tail)
    prediction   OnlineLocalizer.push                            (+ OnlineSpatialNet.forward_stream with carried state)
    doa          OnlineLocalizer.push with localize = PredDOA._search on two tracks   (+ the MSE template search)

For every leg: the median over all pushes after warm-up, the lowest / highest per-round median, and the real-time factor
= median time per push / 100 ms.  The algorithmic latency is a property of the framing, not a measurement: a frame is
complete 256 samples = 16 ms after its centre, and the network consumes groups of 5 frames = 100 ms, so a sample waits
for at most 16 ms + 100 ms of further signal before the prediction that covers it can be computed.

No CPU fallback: without a ROCm device this fails.

    python tools/stream2_bench.py [--rounds 5] [--per-round 100] [--json profiles/r18/stream2.json]
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

NCH = 5
PUSH = 1600            # 5 hops of 320
PUSH_MS = 100.0
PRIME = PUSH + 256     # frames 0..4 are complete, and every further push of 1600 samples completes exactly 5 more
MICS5 = np.array(((0.0, 0.0, 0.0), (0.04, 0.0, 0.0), (0.0, 0.04, 0.0), (-0.04, 0.0, 0.0), (0.0, -0.04, 0.0)))


def case(bf16, rounds, per_round, dev):
    from IPDnet2.IPDnet2 import OnlineSpatialNet
    from IPDnet2.Module import PredDOA
    from fnssl import stream
    from fnssl import weights as W
    net = OnlineSpatialNet(dim_input=2 * NCH, dim_output=16, num_layers=8, dim_hidden=96, num_heads=4, kernel_size=(5, 3),
                           conv_groups=(8, 8), norms=["LN", "LN", "GN", "LN", "LN", "LN"], dim_squeeze=8, num_freqs=256,
                           attention='mamba(16,4)', rope=False, time_compression_layer=0, fre_compression_ratio=16,
                           time_compression_ratio=5)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in W.make_ipdnet2_state(0).items()})
    if bf16:
        net = net.bfloat16()
    net = net.to(dev).eval()
    pd = PredDOA(mic_location=MICS5, dev=str(dev))
    g = torch.Generator(device=dev)
    g.manual_seed(18)
    first = torch.randn((1, PRIME, NCH), generator=g, device=dev) * 0.05
    chunk = first[:, :PUSH]
    fe = stream.CentredStreamFrontEnd(NCH)
    loc = stream.OnlineLocalizer(net, stream.CentredStreamFrontEnd(NCH))
    loc_doa = stream.OnlineLocalizer(net, stream.CentredStreamFrontEnd(NCH), localize=lambda p: pd._search(p[..., :2], 1))
    with torch.no_grad():
        assert fe.push(first).shape[1] == 5
        pred, _ = loc.push(first)
        _, doa = loc_doa.push(first)

        def frontend():
            assert fe.push(chunk).shape[1] == 5

        def prediction():
            assert loc.push(chunk)[0] is not None

        def with_doa():
            assert loc_doa.push(chunk)[1] is not None

        res = alternate({"frontend": frontend, "prediction": prediction, "doa": with_doa}, rounds, per_round)
    for leg in res.values():
        leg["real_time_factor"] = round(leg["median_us"] / (PUSH_MS * 1e3), 5)
    res["prediction_shape"] = list(pred.shape)
    res["doa_shape"] = list(doa[0].shape)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=100)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "r18", "stream2.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("stream2_bench needs a ROCm device (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev), "nb": 1, "microphones": NCH, "push_frames": 5, "push_samples": PUSH,
           "push_ms": PUSH_MS, "unit": "microseconds between device events around one push",
           "real_time_factor": "median time per push / 100 ms of signal",
           "algorithmic_latency_ms": {"look_ahead": 16.0, "group": "up to 100", "worst_case": 116.0,
                                      "note": "from the framing (256 samples after a frame's centre; groups of 5 hops of "
                                              "320 at 16 kHz), not measured; the compute time per push adds to it"},
           "legs": {}}
    for name, bf16 in (("fp32", False), ("bf16", True)):
        out["legs"][name] = case(bf16, args.rounds, args.per_round, dev)
        print(name, json.dumps(out["legs"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
