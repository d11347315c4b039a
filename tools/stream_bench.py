#!/usr/bin/env python3
"""What one 12-frame chunk (192 ms of signal) costs online, microphone samples in.

Front-end leg, per chunk, nb = 1: the streamed front end (fnssl/stream.py, ONE launch of fnssl_stream_frontend) beside
the only thing the whole-signal entries offer for the same 12 frames — ``ops.preprocess`` / ``ops.preprocess_array`` on a
3328-sample signal, i.e. three launches (transform, recursion, pack).  Three legs are timed with device events, alternating
in one process, in ``--rounds`` rounds of ``--per-round`` chunks each:

    composed   ops.preprocess(...) / ops.preprocess_array(...) on the 3328-sample window
    launch     fnssl_stream_frontend on the same window (the fused launch alone, frame index advancing)
    push       StreamFrontEnd.push of the next 3072 samples (the launch plus appending to the sample tail)

For every leg: the median over all chunks and the lowest / highest per-round median (the spread).  ``verdict`` says where
the fused launch's median lies relative to the composed leg's spread.

End-to-end leg: waveform -> prediction per chunk (OnlineLocalizer.push) for FN-SSL 4-mic 'MM' and IPDnet 4-mic, beside
the network alone on ready-made features (forward_stream).

No CPU fallback: without a ROCm device this fails.

    python tools/stream_bench.py [--rounds 5] [--per-round 120] [--e2e-chunks 100] [--json profiles/r11/stream.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fn-ssl_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CHUNK = 3072           # 12 hops
WINDOW = 3328          # 12 frames: 11 * 256 + 512


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def alternate(legs, rounds, per_round, warm=20):
    """legs: name -> callable.  Returns name -> {median_us, round_median_us_min/max, p10_us, p90_us, chunks}."""
    for _ in range(warm):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    per = {n: [] for n in legs}
    for _ in range(rounds):
        ev = {n: [] for n in legs}
        for _ in range(per_round):
            for n, fn in legs.items():
                ev[n].append(event_ms(fn))
        torch.cuda.synchronize()
        for n in legs:
            per[n].append([a.elapsed_time(b) * 1e3 for a, b in ev[n]])
    out = {}
    for n, rs in per.items():
        flat = sorted(x for r in rs for x in r)
        meds = [statistics.median(r) for r in rs]
        out[n] = {"median_us": round(statistics.median(flat), 2), "round_median_us_min": round(min(meds), 2),
                  "round_median_us_max": round(max(meds), 2), "p10_us": round(flat[len(flat) // 10], 2),
                  "p90_us": round(flat[len(flat) * 9 // 10], 2), "chunks": len(flat)}
    return out


def frontend_case(mode, nch, ch_mode, rounds, per_round, dev):
    from fnssl import _lib, ops, stream
    lib = _lib.load()
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    win = torch.randn((1, WINDOW, nch), generator=g, device=dev) * 0.05
    chunk = win[:, :CHUNK]
    sl = stream.DEFAULT_SAMPLE_LENGTH[mode]
    if mode == "pair":
        composed = lambda: ops.preprocess(win, ch_mode, 1e-6, sl, 0)            # noqa: E731
    else:
        composed = lambda: ops.preprocess_array(win, 1e-6, sl, 0)               # noqa: E731
    # the fused launch alone, as StreamFrontEnd.push issues it
    m, cm = _lib.STREAM_MODE[mode], _lib.CH_MODE[ch_mode]
    rows = ops.num_pairs(nch, ch_mode) if mode == "pair" else 1
    width = 4 if mode == "pair" else 2 * nch
    state = torch.zeros(lib.fnssl_stream_frontend_state_bytes(1, nch, m, cm, 12), dtype=torch.uint8, device=dev)
    ca, cb = stream._stream_coefs(sl, True, dev)
    sb, sn, sc = win.stride()
    frame = [0]

    def launch():
        x = torch.empty((rows, 12, 256, width), dtype=torch.float32, device=dev)
        ops.check(lib.fnssl_stream_frontend(ops._ptr(win), 1, WINDOW, nch, sb, sn, sc, m, cm, frame[0], 12, ops._ptr(ca),
                                            ops._ptr(cb), sl, 1e-6, ops._ptr(state), state.numel(), ops._ptr(x),
                                            ops._stream()), "stream_frontend")
        frame[0] = (frame[0] + 12) % (1 << 20)
        return x

    fe = stream.StreamFrontEnd(mode, nch, ch_mode)
    assert fe.push(win).shape[1] == 12                                           # primed: every further chunk emits 12

    def push():
        x = fe.push(chunk)
        assert x.shape[1] == 12
        return x

    # the three legs give the same kind of tensor
    assert tuple(composed().shape) == tuple(launch().shape) == tuple(push().shape)
    res = alternate({"composed": composed, "launch": launch, "push": push}, rounds, per_round)
    lo, hi, fused = res["composed"]["round_median_us_min"], res["composed"]["round_median_us_max"], res["launch"]["median_us"]
    res["verdict"] = ("fused launch below the composed leg's spread" if fused < lo else
                      "fused launch above the composed leg's spread" if fused > hi else
                      "fused launch inside the composed leg's spread")
    return res


def e2e_case(kind, chunks, dev):
    from fnssl import stream
    from fnssl import weights as W
    g = torch.Generator(device=dev)
    g.manual_seed(12)
    nch = 4
    first = torch.randn((1, WINDOW, nch), generator=g, device=dev) * 0.05
    chunk = first[:, :CHUNK]
    if kind == "fnssl_4mic_MM":
        import Model
        net = Model.FN_SSL()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_fnssl_state(0).items()})
        fe = stream.StreamFrontEnd("pair", nch, "MM")
    else:
        from IPDnet.FixedAarryIPDnet import IPDnet
        net = IPDnet(2 * nch, 256, 2, True)
        net.load_state_dict({k: torch.from_numpy(np.array(v, dtype=np.float32))
                             for k, v in W.make_ipdnet_state(0, 2 * nch, 256, 2, True).items()})
        fe = stream.StreamFrontEnd("array", nch)
    net = net.to(dev).eval()
    loc = stream.OnlineLocalizer(net, fe)
    with torch.no_grad():
        pred, _ = loc.push(first)
        feats = stream.StreamFrontEnd(fe.mode, nch, fe.ch_mode).push(first).permute(0, 3, 2, 1)
        st = {"s": None}

        def network():
            _, st["s"] = net.forward_stream(feats, st["s"])

        def e2e():
            p, _ = loc.push(chunk)
            assert p is not None

        res = alternate({"waveform_to_prediction": e2e, "network_on_features": network}, 1, chunks, warm=5)
    res["prediction_shape"] = list(pred.shape)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=120)
    ap.add_argument("--e2e-chunks", type=int, default=100)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "r11", "stream.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("stream_bench needs a ROCm device (there is no CPU path to time)")
    if args.rounds * args.per_round < 500:
        raise SystemExit("at least 500 chunks per leg (rounds x per-round)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev), "chunk_frames": 12, "window_samples": WINDOW, "nb": 1,
           "unit": "microseconds between device events around one chunk", "frontend": {}, "end_to_end": {}}
    for name, mode, nch, ch_mode in (("fnssl_4mic_MM", "pair", 4, "MM"), ("fnssl_2mic", "pair", 2, "MM"),
                                     ("ipdnet_4mic", "array", 4, "M"), ("ipdnet_8mic", "array", 8, "M")):
        out["frontend"][name] = frontend_case(mode, nch, ch_mode, args.rounds, args.per_round, dev)
        print(name, json.dumps(out["frontend"][name]), flush=True)
    for name in ("fnssl_4mic_MM", "ipdnet_4mic"):
        out["end_to_end"][name] = e2e_case(name, args.e2e_chunks, dev)
        print("e2e", name, json.dumps(out["end_to_end"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
