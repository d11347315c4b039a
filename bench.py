#!/usr/bin/env python3
"""Driver benchmark.  Default = the headline: DP-IPD forward throughput on BASELINE config 2
(4 mics, 257 bins x 300 frames, 32 utterances = 192 mic pairs per GPU, fp32).

    python bench.py --gpus N --steps K --warmup W [--config 2|3|4|5] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run (no --full) is lean: set up, W warm-up steps, K timed steps, the outputs of the last timed step to DIR if
--dump-outputs is given, and the one JSON line with the contract keys (`metric`, `value`, `unit`, `higher_is_better`,
`dtype`, `ms_per_step` = wall time of the K timed steps / K, ...), `config` and `cluster_fallbacks`.  Everything else
described below — the instrumented per-kernel pass, roofline, fp32-MFMA calibration, A/B legs, CPU baseline + parity,
strong-scaling efficiency, the nested `other_configs`, the detail file — runs only with --full.

--dump-outputs DIR: after the timed steps, what the timed path returned in its LAST step, as DIR/<name>.npy in float32
(configs 2, 3, 5: `dp_ipd`, the network output; config 4: `loss` and `params`, the flat parameter vector after the
step), rank 0's, at most 64 MB in all (a larger output is cut to a fixed, seeded sample of its flat entries, `dump_outputs`).
Inputs and weights are seeded, so the same arguments give the same inputs in every run.

--config picks the BASELINE.json configuration (configs[1] = 2 is the metric the headline is quoted on; 1 is the
reference's own CPU case and only a parity test):
  2  FN-SSL 4-mic forward, batch 32, fp32                (waveforms -> STFT -> features -> 3 FN blocks -> DP-IPD)
  3  IPDnet fixed-array 8-mic forward, batch 64, bf16    (waveforms -> features -> 2 FN blocks -> causal conv head)
  4  FN-SSL training step, 32 two-mic utterances / GPU   (features -> forward -> MSE -> BPTT -> all-reduce -> Adam)
  5  IPDnet2 (OnlineSpatialNet) 15-mic online forward    (features [B, 30, 256, T] -> DP-IPD; parity unpinned: Mamba)

A "step" is one pass of the hot path over one synthetic batch already resident in HBM.  Every rank runs the same
per-GPU batch (weak scaling; utterances are independent: no data-path collective, config 4 has the one gradient
all-reduce) — or, with --scaling strong (config 2), an even share of the configuration's GLOBAL batch, and a --full
line then carries `strong_scaling.efficiency` against one rank running the whole batch in the same run.  K steps are timed
between barrier + synchronize, max over ranks; rank 0 prints ONE JSON line (compact: < 4 KB, `compact_line`) whose `value`
is utterance-frames per second over all ranks; with --full the FULL record goes to --detail (default: see --detail).
The --full run of the default shape also measures config 2's 'M' pairing and is_online=False variants ("2M", "2off"), the
reference's real predict shape — ONE 4-mic utterance, whole ("2b1") and streamed in 12-frame chunks ("2s") — and configs
3, 4, 5: the stdout line carries {value, ms_per_step, roofline_frac, cpu_baseline, parity_ok} of each under
`other_configs`, the detail file their full lines (own roofline / cpu_baseline / parity).  Every line carries
`cluster_fallbacks` (LSTM launches of the timed region whose cluster-resident kernel gave up and were recomputed by the
guarded fallback kernels: must be 0, else `value` is null); a --full line also `peak_mem_gb` (of that configuration alone).
stdout line of a --full run:
  roofline     : the dominant kernel against its roof {bound, kernel, achieved, peak, frac, traffic, launches, avg_ms,
                 flop_per_launch}, timed with HIP events on the launch stream inside the timed region — only that kernel
                 is bracketed there (fnssl_timing_select); peak_measured / peak_measured_sustained = this device's own
                 fp32-MFMA ceiling, a 35-ms burst and >= 2 s of back-to-back launches (fnssl_mfma_f32_peak), with the
                 slowest / fastest XCD clock of the sustained run — what makes a slow box attributable from the line;
  cpu_baseline : the CPU restatement of the reference (oracle/) timed on this host on a bounded sample
                 (N = 1, rank 0 only), and `parity`: the same sample through the HIP path vs that CPU output;
  ab_gain_pct  : per same-process A/B leg, what the shipped default gains over the knob that restores the old kernels.
detail file only: `kernels` and `frontend` tables (instrumented pass before the timed region), `ab` legs in full, the
prose fields (`traffic_source`, `how`, `sample` unclipped).
A failed parity check nulls `value` and exits 1.
"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "fn-ssl_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 / 32x32x2 dense fp32
PEAK_BF16_MFMA_TFLOPS = 2500.0    # dense bf16
PEAK_HBM_GBS = 8000.0
FLOP_PER_TF_POINT = {True: 4997120, False: 4210688}   # LSTM matmuls only, by is_online
TRAFFIC_JSON = os.path.join("profiles", "r06", "hbm_traffic.json")     # per roofline kernel: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes
TRAFFIC_JSON_R03 = os.path.join("profiles", "r03", "hbm_traffic_lstm_h256.json")
# same-process A/B legs of the --full run: (label, environment of the B leg).  A = the shipped default.
AB_KNOBS = [
    # round 6: four hidden slices per pass with an LDS-DMA weight ring (lstm_static4.h) against the two-slice operand-ring kernel
    ("four_slices_per_pass_vs_two", {"FNSSL_NO_STATIC4": "1"}),
    # round 4: operand-ring narrow-band kernel (lstm_static3.h) against the one-slice rounds it replaced (round 3's two-slice
    # kernel was removed in round 5); issue priorities by phase and leftover-group rotation in the cluster-resident full-band
    # kernel (lstm_f32c.h)
    ("round4_kernels_vs_one_slice_rounds", {"FNSSL_NO_STATIC3": "1", "FNSSL_F32C_PRIO": "9", "FNSSL_F32C_NO_ROTATE": "1"}),
    # round 3: cluster-resident full-band kernel (lstm_f32c.h) against the per-wave rounds
    ("f32_cluster_vs_rounds", {"FNSSL_NO_F32_CLUSTER": "1"}),
]


SQ_JSON = os.path.join("profiles", "r05", "pmc_sq_sn_mamba_scan.json")


def sq_counters_of(kernel):
    """SQ counters of one kernel from the committed rocprofv3 --pmc summary (tools/pmc_summary.py), or None."""
    for path in (SQ_JSON, os.path.join("profiles", "r04", "h_pmc_sq_sn_mamba_scan.json")):
        full = os.path.join(ROOT, path)
        if os.path.exists(full):
            try:
                with open(full) as f:
                    d = json.load(f)
            except ValueError:
                continue
            for k, v in d.items():
                if kernel in k:
                    return v
    return None


def traffic_of(key):
    """(bytes per launch, source) of a roofline kernel from the committed PMC summaries, or (None, None): counter
    passes cannot run inside the timed region (gpurun refuses --pmc next to traces, and they perturb the clock)."""
    for rel in (TRAFFIC_JSON, os.path.join("profiles", "r05", "hbm_traffic.json"), os.path.join("profiles", "r04", "hbm_traffic.json")):
        path = os.path.join(ROOT, rel)
        if os.path.exists(path):
            with open(path) as f:
                d = json.load(f).get(key)
            if d and d.get("bytes_per_launch"):
                return d["bytes_per_launch"], rel + "[%s] (%s; not this run)" % (key, d.get("how", "rocprofv3 --pmc"))
    if key == "c2_lstm_h256" and os.path.exists(os.path.join(ROOT, TRAFFIC_JSON_R03)):
        with open(os.path.join(ROOT, TRAFFIC_JSON_R03)) as f:
            return json.load(f).get("bytes_per_launch"), TRAFFIC_JSON_R03 + " (round-3 build; rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, not this run)"
    return None, None


def log(msg):
    sys.stderr.write("[bench] %s\n" % msg)
    sys.stderr.flush()


def usable_cores():
    """Threads the CPU baseline may use: affinity mask capped by the cgroup CPU quota (and by 64:
    oneDNN's LSTM does not scale past that on these shapes)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 64))


def load_module(name, *path):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def kernel_roof(kern, name, label, peak, unit_scale=1e12, traffic=None, traffic_source=None):
    k = kern.get(name)
    if not k or k["ms"] <= 0 or not k["flops"]:
        return None
    achieved = k["flops"] / (k["ms"] * 1e-3) / unit_scale
    return {"name": name, "bound": "mfma", "kernel": label, "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_source": traffic_source,
            "launches": k["count"], "avg_ms": round(k["ms"] / max(1, k["count"]), 3),
            "flop_per_launch": k["flops"] / max(1, k["count"])}


def parity_of(got, want, rtol, atol, what):
    err = (got - want).abs()
    p = {"max_abs_err": float(err.max()), "rtol": rtol, "atol": atol, "sample": what,
         "ok": bool((err <= atol + rtol * want.abs()).all())}
    log("parity vs CPU reference (%s): max abs err %.3g ok=%s" % (what, p["max_abs_err"], p["ok"]))
    return p


# ------------------------------------------------------------------------------------------------------------ #
# config 2: FN-SSL forward (the headline)
# ------------------------------------------------------------------------------------------------------------ #
class FnsslForward:
    def __init__(self, args, dev, rank, world):
        import predict_step as ps
        from fnssl import ops
        from fnssl import weights as W
        self.args, self.dev, self.ops, self.world = args, dev, ops, world
        self.online = not args.offline
        self.nb = args.nb or 32
        if args.scaling == "strong":                  # fixed global batch split over the ranks
            if self.nb % world:
                raise SystemExit("--scaling strong: the global batch of %d utterances does not split over %d ranks" % (self.nb, world))
            self.global_nb, self.nb = self.nb, self.nb // world
        self.sd = W.make_fnssl_state(0, is_online=self.online)
        model = ps.MyModel(ch_mode=args.ch_mode, device=str(dev))
        if not self.online:
            import Model as at_model
            model.arch = at_model.FN_SSL(is_online=False)
        model.arch.load_state_dict({k: torch.from_numpy(v) for k, v in self.sd.items()})
        model.arch.chunk_pairs = args.chunk_pairs
        self.model = model.to(dev).eval()
        if args.bf16:
            self.model.arch.bfloat16()          # optional fast mode, see --bf16
        ns = 512 + (args.frames - 1) * 256
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234 + rank)
        self.batch = torch.randn((self.nb, args.nch, ns), generator=gen, device=dev, dtype=torch.float32)
        self.n_pairs = ops.num_pairs(args.nch, args.ch_mode)
        self.nt = ops.num_frames(ns)
        self.frames_per_step = self.nb * self.nt
        self.flop_per_utt_frame = FLOP_PER_TF_POINT[self.online] * 256 * self.n_pairs
        self.dtype = "bf16" if args.bf16 else "f32"
        self.metric = "TF-frames/sec DP-IPD forward, 4-mic 257-bin x 300-frame" + \
            (" [optional bf16 fast mode: NOT the BASELINE fp32 metric]" if args.bf16 else "")
        log("rank %d/%d on %s: %d utt x %d mics x %d frames, %d pairs" % (rank, world, torch.cuda.get_device_name(dev),
                                                                        self.nb, args.nch, self.nt, self.nb * self.n_pairs))
        # --stream-chunk T ("2s"): the online model driven chunk by chunk (Model.FN_SSL.forward_stream: the state carry the
        # reference's causality permits): a step = the NEXT T frames of every utterance, from the feature tensor
        self.chunk = int(getattr(args, "stream_chunk", 0) or 0)
        if self.chunk:
            if not self.online or args.bf16 or self.chunk % 12:
                raise SystemExit("--stream-chunk: online fp32 model, a multiple of 12 frames")
            self.feat = ops.preprocess(self.batch.permute(0, 2, 1), args.ch_mode, 1e-6, layout=1)     # [nb*np, 4, 256, nt]
            self.state, self.pos = None, 0
            self.frames_per_step = self.nb * self.chunk
            self.metric = "TF-frames/sec DP-IPD forward, streaming in %d-frame chunks (4-mic 257-bin)" % self.chunk

    def step(self):
        if self.chunk:
            if self.pos + self.chunk > self.nt:                       # next utterance: fresh state
                self.state, self.pos = None, 0
            y, self.state = self.model.arch.forward_stream(self.feat[..., self.pos:self.pos + self.chunk], self.state)
            self.pos += self.chunk
            return y
        return self.model.predict_step(self.batch, 0)

    def check(self, out):
        nseg = (self.chunk or self.nt) // 12
        assert tuple(out.shape) == (self.nb * self.n_pairs, nseg, 512) and bool(torch.isfinite(out).all())

    def outputs(self, out):
        return {"dp_ipd": out}

    def config(self):
        a = self.args
        return {"workload": "BASELINE configs[1]: FN-SSL (%s) DP-IPD forward, waveform->STFT->features->"
                            "3x(full-band BiLSTM + narrow-band LSTM)->head; %d utterances/GPU x %d mics ('%s' = %d pairs) "
                            "x 257 bins x %d frames, fp32; frame = one STFT frame of one utterance%s"
                            % ("online" if self.online else "offline", self.nb, a.nch, a.ch_mode, self.n_pairs, self.nt,
                               ("; STREAMING: a step = the next %d frames from the feature tensor through FN_SSL.forward_stream "
                                "(carried LSTM state), %d steps per utterance" % (self.chunk, self.nt // self.chunk)) if self.chunk else ""),
                "stream_chunk_frames": self.chunk,
                "utterances_per_gpu": self.nb, "global_batch": self.nb * self.world, "mics": a.nch,
                "pairs_per_utterance": self.n_pairs, "frames": self.nt,
                "bins": 257, "parallelism": "dp%d (utterance shards, no collective)" % self.world,
                "chunk_pairs": a.chunk_pairs, "gflop_per_frame": round(self.flop_per_utt_frame / 1e9, 3)}

    def extra(self, value, kern, steps):
        ex = {"whole_path_tflops": round(value * self.flop_per_utt_frame / 1e12 / self.world, 2)}
        # front end against ITS roof (HBM): 4 KB read + 24 KB written per 4-mic 'MM' utterance-frame
        fe = [kern.get(k) for k in ("stft", "ema", "pack")]
        if all(fe):
            ms = sum(k["ms"] for k in fe) / steps
            by = self.frames_per_step * (self.args.nch * 256 * 4 + self.n_pairs * 4 * 256 * 4)
            gbs = by / (ms * 1e-3) / 1e9
            ex["frontend"] = {"bound": "hbm", "kernel": "stft + ema + pack (3 launches: launch-latency sized)",
                              "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                              "frac": round(gbs / PEAK_HBM_GBS, 4), "traffic": None, "ms_per_step": round(ms, 4),
                              "algorithmic_bytes_per_step": by}
        return ex

    def roofline(self, kern):
        if not self.online:
            return kernel_roof(kern, "lstm_h128", "H = 128 layers (offline: every layer; full-band on the cluster-resident lstm_f32c_kernel, "
                               "narrow-band on lstm_static_kernel rounds)", PEAK_FP32_MFMA_TFLOPS)
        if self.chunk:
            traffic, src = traffic_of("c2s_lstm_h128")
            return kernel_roof(kern, "lstm_h128", "lstm_f32c_kernel<H=128, gate split> (full-band BiLSTM: 256 serial steps per chunk, one "
                               "16-sequence group per cluster of 8 CUs — latency-bound by the per-step hand-off, not by the matrix pipe)",
                               PEAK_FP32_MFMA_TFLOPS, traffic=traffic, traffic_source=src)
        if self.nb * self.n_pairs * 256 // 16 < 12 * 256:      # below the full-chip launch the narrow-band layers run lstm_f32c_kernel<256>
            traffic, src = (traffic_of("c2b1_lstm_h256") if self.nb == 1 and self.n_pairs == 6 else
                            traffic_of("c2M_lstm_h256") if self.nb * self.n_pairs == 96 else (None, None))
            return kernel_roof(kern, "lstm_h256", "lstm_f32c_kernel<H=256> (narrow-band LSTM: hidden slices over clusters of 16 CUs, weight "
                               "slice resident in LDS, groups as work items)", PEAK_FP32_MFMA_TFLOPS, traffic=traffic, traffic_source=src)
        if self.args.bf16:
            return kernel_roof(kern, "lstm_h256", "lstm_bf16_kernel<H=256> (narrow-band LSTM, bf16 MFMA operands)",
                               PEAK_BF16_MFMA_TFLOPS)
        traffic, src = traffic_of("c2_lstm_h256")
        if os.environ.get("FNSSL_NO_STATIC4"):
            return kernel_roof(kern, "lstm_h256", "lstm_static3_kernel<H=256> (narrow-band LSTM, two hidden slices per pass, x_t and h_{t-1} streamed)",
                               PEAK_FP32_MFMA_TFLOPS, traffic=traffic, traffic_source=src)
        return kernel_roof(kern, "lstm_h256", "lstm_static4_kernel<H=256> (narrow-band LSTM, four hidden slices per pass, x_t and h_{t-1} "
                           "streamed, LDS-DMA weight ring)", PEAK_FP32_MFMA_TFLOPS, traffic=traffic, traffic_source=src)

    def ab_knobs(self):
        return AB_KNOBS if (self.online and not self.args.bf16) else []

    def cpu_baseline(self):
        from oracle import torch_ref as R
        a = self.args
        cores = usable_cores()
        torch.set_num_threads(cores)
        net = R.build(self.sd, self.online)
        sample = self.batch[:a.cpu_utts].cpu()
        R.predict_step(net, sample[:, :, :512 + 11 * 256], a.ch_mode)       # warm-up (12 frames)
        p0 = time.perf_counter()
        R.predict_step(net, sample[:, :, :512 + 23 * 256], a.ch_mode)
        per_frame = (time.perf_counter() - p0) / 24.0
        cpu_frames = int(min(self.nt, max(24, (a.cpu_seconds / max(per_frame, 1e-9)) // 12 * 12)))
        log("cpu baseline: %d threads, probe %.3f s/frame -> timing %d frames" % (cores, per_frame, cpu_frames))
        cns = 512 + (cpu_frames - 1) * 256
        c0 = time.perf_counter()
        ref_out = R.predict_step(net, sample[:, :, :cns], a.ch_mode)
        cdt = time.perf_counter() - c0
        cpu = {"value": round(a.cpu_utts * cpu_frames / cdt, 2), "unit": "frames/s", "cores": cores, "kind": "port",
               "sample": "%d utterance(s) x %d mics x %d frames ('%s', %d pairs), PyTorch CPU restatement of the "
                         "reference (torch.stft + oneDNN nn.LSTM), %d threads, %.1f s"
                         % (a.cpu_utts, a.nch, cpu_frames, a.ch_mode, a.cpu_utts * self.n_pairs, cores, cdt)}
        # same-run parity gate on the same waveforms: the narrow-band LSTM is causal, the forgetting-norm recursive
        # and the full-band BiLSTM runs along frequency only, so a frame prefix is an exact sub-problem
        if self.chunk:     # the same frames chunk by chunk: what the streaming steps of the timed region compute
            feat = self.ops.preprocess(self.batch[:a.cpu_utts, :, :cns].permute(0, 2, 1), a.ch_mode, 1e-6, layout=1)
            st, parts = None, []
            for t0 in range(0, cpu_frames - cpu_frames % self.chunk, self.chunk):
                y, st = self.model.arch.forward_stream(feat[..., t0:t0 + self.chunk], st)
                parts.append(y)
            got = torch.cat(parts, dim=1).cpu()
            ref_out = ref_out[:, :got.shape[1]]
        else:
            got = self.model.predict_step(self.batch[:a.cpu_utts, :, :cns], 0).cpu()
        rt, at = (2e-2, 4e-3) if a.bf16 else (1e-4, 1e-5)
        return cpu, parity_of(got, ref_out, rt, at, "%d frames" % cpu_frames)


# ------------------------------------------------------------------------------------------------------------ #
# config 3: IPDnet fixed-array 8-mic, batch 64, bf16
# ------------------------------------------------------------------------------------------------------------ #
class IpdnetForward:
    def __init__(self, args, dev, rank, world):
        from fnssl import ops
        from fnssl import weights as W
        M = load_module("fnssl_ipdnet_dropin", "fn-ssl_amd", "IPDnet", "FixedAarryIPDnet.py")
        self.args, self.dev, self.ops, self.world = args, dev, ops, world
        self.nb, self.mics, self.hidden = args.nb or 64, 8, 256
        self.fp32 = args.fp32
        isz = 2 * self.mics
        self.sd = W.make_ipdnet_state(7, isz, self.hidden, 2, True)
        net = M.IPDnet(input_size=isz, hidden_size=self.hidden, max_track=2, is_online=True).eval()
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in self.sd.items()})
        self.net = net.to(dev)
        if not self.fp32:
            self.net.bfloat16()
        g = torch.Generator(device=dev)
        g.manual_seed(2000 + rank)
        self.nt = args.frames
        self.sig = torch.randn((self.nb, 256 * (self.nt + 1), self.mics), generator=g, device=dev) * 0.1
        self.frames_per_step = self.nb * self.nt
        self.dtype = "f32" if self.fp32 else "bf16"
        self.metric = "TF-frames/sec IPDnet DP-IPD forward, 8-mic 257-bin x 300-frame"
        # one stream is the product path; with FNSSL_IPDNET_STREAMS >= 2 (opt-in) the timed region runs part-batches on
        # several streams, and the per-kernel breakdown / roofline.alone come from an instrumented pass on one stream
        self.multi_stream = (not self.fp32) and os.environ.get("FNSSL_IPDNET_STREAMS", "1") not in ("", "0", "1") \
            and not os.environ.get("FNSSL_IPDNET_ONE_STREAM")
        self.probe_env = {"FNSSL_IPDNET_ONE_STREAM": "1"} if self.multi_stream else {}
        log("rank %d/%d: IPDnet %d utt x %d mics x %d frames, %s" % (rank, world, self.nb, self.mics, self.nt, self.dtype))

    def step(self):
        return self.net(self.ops.preprocess_array(self.sig))

    def check(self, out):
        assert tuple(out.shape) == (self.nb, self.nt // 12, 512, self.mics - 1, 2) and bool(torch.isfinite(out.float()).all())

    def outputs(self, out):
        return {"dp_ipd": out}

    def config(self):
        return {"workload": "BASELINE configs[2]: IPDnet fixed-array %d-mic (input 16 ch, hidden 256, online, 2 tracks) "
                            "DP-IPD forward, waveform->STFT->array features->2x(full-band BiLSTM + narrow-band LSTM, "
                            "concat skips)->causal 3x3 conv head; %d utterances/GPU x 257 bins x %d frames; %s"
                            % (self.mics, self.nb, self.nt,
                               "fp32" if self.fp32 else "bf16 weights / MFMA operands, fp32 accumulate, fp32 tensors in HBM"),
                "utterances_per_gpu": self.nb, "mics": self.mics, "frames": self.nt, "bins": 257,
                "parallelism": "dp%d (utterance shards, no collective)" % self.world}

    def extra(self, value, kern, steps):
        fl = sum(v["flops"] for v in kern.values()) / steps
        return {"tflop_per_step": round(fl / 1e12, 2),
                "whole_path_tflops": round(value / self.frames_per_step / self.world * fl / 1e12, 2)}

    def roofline(self, kern):
        if self.fp32:
            return kernel_roof(kern, "lstm_h256", "narrow-band LSTM H=256 (fp32 MFMA)", PEAK_FP32_MFMA_TFLOPS)
        traffic, src = traffic_of("c3_lstm_h256")
        r = kernel_roof(kern, "lstm_h256", "lstm_bf16c_kernel<H=256> (narrow-band LSTM, bf16 MFMA operands, weights resident "
                        "in the LDS of an 8-CU cluster)", PEAK_BF16_MFMA_TFLOPS, traffic=traffic, traffic_source=src)
        if r is not None and self.multi_stream:
            r["note"] = ("part-batches run on several streams: in the timed region a launch shares the chip with the "
                         "other streams' kernels, so its duration there is not exclusive; `alone` = the same kernel in "
                         "the one-stream instrumented pass")
        return r

    def ab_knobs(self):
        # round 6: full-band layers as 60 clusters x 20 tiles (3 + 2 parts per SIMD) against the full clusters of 24 (3 + 3)
        return [] if self.fp32 else [("full_band_clusters_of_20_vs_24_tiles", {"FNSSL_CLUSTER_FULL_TILES": "1"})]

    def cpu_baseline(self):
        from oracle import torch_ref as R
        cores = usable_cores()
        torch.set_num_threads(cores)
        net = R.build_ipdnet(self.sd, 2 * self.mics, self.hidden, 2, True)
        frames = 120 if self.nt >= 120 else self.nt // 12 * 12
        sig = self.sig[:1, :256 * (frames + 1)].cpu()
        with torch.no_grad():
            net(R.array_preprocess(sig[:, :256 * 13]))                             # warm-up (12 frames)
            c0 = time.perf_counter()
            want = net(R.array_preprocess(sig)).contiguous()                         # fp32 PyTorch CPU forward
            cdt = time.perf_counter() - c0
        cpu = {"value": round(frames / cdt, 2), "unit": "frames/s", "cores": cores, "kind": "port",
               "sample": "1 utterance x 8 mics x %d frames from the waveform, PyTorch CPU restatement of the reference "
                         "(oracle/torch_ref.py: torch.stft + oneDNN nn.LSTM + Conv2d), fp32, %d threads, %.1f s"
                         % (frames, cores, cdt)}
        got = self.net(self.ops.preprocess_array(self.sig[:1, :256 * (frames + 1)])).float().cpu()
        rt, at = (1e-4, 2e-5) if self.fp32 else (2e-2, 4e-3)                      # SURVEY 8d config-3 tolerance
        return cpu, parity_of(got, want, rt, at, "%d frames vs the fp32 PyTorch CPU forward" % frames)


# ------------------------------------------------------------------------------------------------------------ #
# config 4: FN-SSL training step
# ------------------------------------------------------------------------------------------------------------ #
class FnsslTrain:
    def __init__(self, args, dev, rank, world):
        import Model
        from fnssl import ops, train
        from fnssl import weights as W
        self.args, self.dev, self.ops, self.world, self.rank = args, dev, ops, world, rank
        self.nb, self.mics, self.nt = args.nb or 32, 2, args.frames
        self.sd = W.make_fnssl_state(3, 4, 256, True)
        net = Model.FN_SSL(is_online=True)
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in self.sd.items()})
        self.net = net.to(dev)
        self.eng = train.TrainEngine(self.net, seed=1, chunk_pairs=args.chunk_pairs or None)
        # --autograd: the step the reference's way (main.py:149-157 under strategy="ddp"): train-mode forward with a grad_fn
        # (fnssl/autograd.py), differentiable MSE, loss.backward(), torch.optim.Adam; DistributedDataParallel does the
        # gradient all-reduce when there is more than one rank.  Default: the fused engine (same kernels).
        self.autograd = bool(getattr(args, "autograd", False))
        self.ag = self._autograd_setup(world) if self.autograd else None
        # --c-step: the whole step as ONE C call (fnssl_train_step); single process only (no all-reduce inside)
        self.cstep = train.CTrainStep(self.eng) if args.c_step else None
        if self.cstep is not None and world > 1:
            raise SystemExit("--c-step is the single-process entry point (fnssl_train_step has no collective)")
        g = torch.Generator(device=dev)
        g.manual_seed(100 + rank)
        self.npair = self.mics * (self.mics - 1) // 2
        self.sig = torch.randn((self.nb, 256 * (self.nt + 1), self.mics), generator=g, device=dev) * 0.1
        self.gt = torch.tanh(torch.randn((self.nb, self.nt // 12, 512, self.npair), generator=g, device=dev))
        self.frames_per_step = self.nb * self.nt
        self.dtype = "f32"
        self.metric = "utt-frames/sec FN-SSL training step (forward + MSE + BPTT + gradient all-reduce + Adam)"
        self.flops = 3.0 * FLOP_PER_TF_POINT[True] * self.nb * self.npair * 256.0 * self.nt   # fwd + BPTT + dW GEMMs
        log("rank %d/%d: training step, %d utt x %d mics x %d frames per GPU" % (rank, world, self.nb, self.mics, self.nt))

    def _autograd_setup(self, world):
        import Model
        import predict_step as ps
        net = Model.FN_SSL(is_online=True)
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in self.sd.items()})
        net = net.to(self.dev).train()
        net.dropout_seed = 1
        model = net
        if world > 1:
            from torch.nn.parallel import DistributedDataParallel as DDP
            model = DDP(net, device_ids=[self.dev.index])
        return {"net": net, "model": model, "opt": torch.optim.Adam(net.parameters(), lr=1e-3), "loss": ps._MSELoss}

    def _autograd_step(self, ag):
        x = self.ops.preprocess(self.sig, "MM", layout=1)
        ag["opt"].zero_grad(set_to_none=True)
        loss = ag["loss"].apply(ag["model"](x), self.gt)
        loss.backward()
        ag["opt"].step()
        return loss.detach()

    def step(self):
        if self.ag is not None:
            return self._autograd_step(self.ag)
        x = self.ops.preprocess(self.sig, "MM", layout=1)
        if self.cstep is not None:
            self.cstep.step_nosync(x, self.gt, 1000003 + 8191 * (self.eng.step_count + 1))
            return self.eng.loss_dev
        return self.eng.step(x, self.gt, sync_loss=False, pair_offset=self.rank * self.nb * self.npair)

    def check(self, out):
        assert bool(torch.isfinite(out).all())

    def outputs(self, out):
        """The step's loss and the parameters it left behind (the fused engine keeps them in one flat vector)."""
        if self.ag is not None:
            params = torch.cat([p.detach().reshape(-1) for p in self.ag["net"].parameters()])
        else:
            params = self.eng.theta
        return {"loss": out, "params": params}

    def config(self):
        return {"workload": "BASELINE configs[3]: FN-SSL (online) training step, global batch %d two-mic utterances = %d per "
                            "GPU x %d GPU(s), 257 bins x %d frames, fp32; waveforms->features->forward (dropout on)->MSE->"
                            "BPTT + weight gradients->RCCL sum all-reduce of the flat 10 MB gradient->Adam"
                            % (self.nb * self.world, self.nb, self.world, self.nt),
                "utterances_per_gpu": self.nb, "global_batch": self.nb * self.world, "mics": self.mics, "frames": self.nt,
                "parallelism": "dp%d (utterance shards; one gradient all-reduce per step)" % self.world,
                "chunk_pairs": self.args.chunk_pairs}

    def extra(self, value, kern, steps):
        ex = {"tflop_per_step_per_gpu": round(self.flops / 1e12, 2),
              "whole_path_tflops": round(value / self.frames_per_step / self.world * self.flops / 1e12, 2)}
        # the exchange step alone: the same flat gradient, timed outside the step (inside it overlaps the backward)
        if self.world > 1:
            import torch.distributed as dist
            buf = torch.zeros_like(self.eng.grad)
            dist.all_reduce(buf)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                dist.all_reduce(buf)
            torch.cuda.synchronize()
            ex["comm_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
        else:
            ex["comm_ms"] = 0.0
        ex["comm_bytes"] = int(self.eng.grad.numel() * 4)
        ex["comm_exposed_ms"] = round(getattr(self.eng, "last_comm_wait_ms", 0.0), 3)
        ex["route"] = "autograd (torch.autograd.Function over the C-ABI kernels + torch.optim.Adam%s)" % (
            " + DistributedDataParallel" if self.world > 1 else "") if self.autograd else "fused engine (fnssl.train.TrainEngine)"
        # the same step through the OTHER route, a few steps after the timed region: what the reference's own training loop
        # (forward with a grad_fn, loss.backward(), torch optimizer) costs over the fused engine on the same kernels
        if self.world == 1 and not self.autograd and self.cstep is None:
            try:
                self.eng._scratch.clear()                  # the engine's activation buffers: make room for autograd's
                torch.cuda.empty_cache()
                ag = self._autograd_setup(1)
                self._autograd_step(ag)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                n = 3
                e0.record()
                for _ in range(n):
                    self._autograd_step(ag)
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1) / n
                eng_ms = self.frames_per_step / value * 1e3
                ex["autograd_route"] = {"ms_per_step": round(ms, 3), "over_engine": round(ms / eng_ms, 4), "steps": n,
                                        "how": "net.train(); loss = MSE(net(x), gt); loss.backward(); torch.optim.Adam.step() "
                                               "(main.py:149-157) on the same shard, after the timed region"}
                del ag
            except Exception as e:                         # evidence leg only
                ex["autograd_route"] = {"error": repr(e)}
        return ex

    def roofline(self, kern):
        traffic, src = traffic_of("c4_lstm_bwd_h256")
        return kernel_roof(kern, "lstm_bwd_h256", "lstm_bwd2_kernel<H=256> (narrow-band BPTT, two groups per wave set)", PEAK_FP32_MFMA_TFLOPS,
                           traffic=traffic, traffic_source=src)

    def cpu_baseline(self):
        from oracle import train_ref as TR
        cores = usable_cores()
        torch.set_num_threads(cores)
        frames, utts = 24, 1
        x = self.ops.preprocess(self.sig[:utts, :256 * (frames + 1)], "MM", layout=1).cpu().numpy()
        gt = self.gt[:utts, :frames // 12].cpu().numpy()
        c0 = time.perf_counter()
        loss, grads, *_ = TR.train_step(self.sd, x, gt, seed=12345)
        cdt = time.perf_counter() - c0
        cpu = {"value": round(utts * frames / cdt, 2), "unit": "frames/s", "cores": cores, "kind": "port",
               "sample": "%d utterance x 2 mics x %d frames, PyTorch CPU autograd restatement of training_step "
                         "(oracle/train_ref.py: forward + backward + Adam), %d threads, %.1f s" % (utts, frames, cores, cdt)}
        # same-step parity on that sample: a fresh engine with the oracle's seed -> compare the loss
        import Model
        from fnssl import train
        net = Model.FN_SSL(is_online=True)
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in self.sd.items()})
        eng = train.TrainEngine(net.to(self.dev), seed=0, process_group=False)
        eng.force_seed = 12345
        got = eng.step(torch.from_numpy(x).to(self.dev), torch.from_numpy(gt).to(self.dev), sync_loss=True)
        par = parity_of(torch.tensor([got]), torch.tensor([loss]), 1e-4, 1e-6, "loss of one step, %d frames" % frames)
        # ... and every parameter gradient of that step against the oracle's autograd (relative to each tensor's largest
        # entry: sums over ~1e5 terms in a different order; tests/test_gpu_train.py holds the same 5e-4)
        worst, worst_name = 0.0, None
        have = eng.gradients()
        for k, g in grads.items():
            scale = float(np.abs(g).max()) + 1e-30
            err = float(np.abs(have[k].cpu().numpy() - g).max()) / scale
            if err > worst:
                worst, worst_name = err, k
        par["gradients"] = {"tensors": len(grads), "max_err_of_largest_entry": worst, "worst": worst_name, "tol": 5e-4,
                            "ok": bool(worst <= 5e-4)}
        par["ok"] = bool(par["ok"] and worst <= 5e-4)
        return cpu, par


# ------------------------------------------------------------------------------------------------------------ #
# config 5: IPDnet2 (OnlineSpatialNet), 15-mic input, online / causal
# ------------------------------------------------------------------------------------------------------------ #
def ipdnet2_flops_per_frame(dim_input=10, dim_output=16, num_layers=8, H=96, Hs=8, F=256, ke=5, kf=5, groups=8, N=16,
                            Kc=4, ratio_f=16, ratio_t=5):
    """Algorithmic flop (2 per MAC of every matmul / conv; norms, activations and the scan's element-wise part counted
    at face value) per INPUT frame of one utterance of OnlineSpatialNet (IPDnet2/IPDnet2.py:259-368) — a counter of the
    model's arithmetic, kept here so that nothing outside the cpu_baseline / parity legs imports oracle/."""
    E, R = 2 * H, -(-H // 16)
    fc = lambda f: f * 2 * H * (H // groups) * kf                                              # noqa: E731
    fl = lambda f: f * (2 * H * Hs * 2) + 2 * Hs * f * f                                         # noqa: E731
    mb = lambda f: f * (2 * H * 2 * E + 2 * E * Kc + 2 * E * (R + 2 * N) + 2 * R * E + 7 * E * N + 2 * E * H)   # noqa: E731
    total = F * 2 * dim_input * ke * H                       # encoder
    total += fc(F) + fl(F // 2) + fc(F // 2) + 2 * mb(F // ratio_f)     # layer 0
    per = fc(F // ratio_f) * 2 + fl(F // ratio_f) + 2 * mb(F // ratio_f)
    total += (num_layers - 1) * per / ratio_t
    total += (F // ratio_f) * 2 * H * ratio_f * dim_output / ratio_t + F * 2 * dim_output * dim_output / ratio_t
    return float(total)



class Ipdnet2Forward:
    def __init__(self, args, dev, rank, world):
        from fnssl import ops
        from fnssl import weights as W
        M = load_module("fnssl_ipdnet2_dropin", "fn-ssl_amd", "IPDnet2", "IPDnet2.py")
        self.args, self.dev, self.ops, self.world = args, dev, ops, world
        self.nb, self.mics, self.layers = args.nb or 64, 15, 8
        self.nt = args.frames if args.frames != 300 else 250            # 4 s at hop 320 (run_IPDnet2.py:93)
        self.sd = W.make_ipdnet2_state(7, dim_input=2 * self.mics, num_layers=self.layers)
        net = M.OnlineSpatialNet(dim_input=2 * self.mics, dim_output=16, num_layers=self.layers, dim_hidden=96, num_heads=4,
                                 kernel_size=(5, 3), conv_groups=(8, 8), norms=["LN", "LN", "GN", "LN", "LN", "LN"],
                                 dim_squeeze=8, num_freqs=256, attention="mamba(16,4)", rope=False,
                                 time_compression_layer=0, fre_compression_ratio=16, time_compression_ratio=5).eval()
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in self.sd.items()})
        self.fp32 = args.fp32
        import copy
        self.net32 = None if self.fp32 else copy.deepcopy(net).to(dev)    # the exact-fp32 kernels: the bf16 mode's yardstick
        self.net = net.to(dev) if self.fp32 else net.to(dev).bfloat16()   # bf16 parameters select FNSSL_PRECISION_BF16
        g = torch.Generator(device=dev)
        g.manual_seed(3000 + rank)
        # waveforms [B, ns, 15] with ns = 320 (nt - 1): nt = ns // 320 + 1 frames (IPDnet2/Module.py:55).  --features-in
        # starts from the feature tensor instead (the round-2 measurement)
        self.features_in = args.features_in
        self.sig = torch.randn((self.nb, 320 * (self.nt - 1), self.mics), generator=g, device=dev) * 0.1
        self.x = ops.preprocess_ipdnet2(self.sig)
        assert tuple(self.x.shape) == (self.nb, 2 * self.mics, 256, self.nt)
        self.frames_per_step = self.nb * self.nt
        self.dtype = "f32" if self.fp32 else "bf16"
        self.metric = "utt-frames/sec IPDnet2 (OnlineSpatialNet) DP-IPD forward, 15-mic input, 512 outputs per frame"
        self.flop_per_frame = ipdnet2_flops_per_frame(dim_input=2 * self.mics, num_layers=self.layers)
        log("rank %d/%d: IPDnet2 %d utt x %d input channels x 256 bins x %d frames, %s"
            % (rank, world, self.nb, 2 * self.mics, self.nt, self.dtype))

    def step(self):
        if self.features_in:
            return self.net(self.x)
        return self.net(self.ops.preprocess_ipdnet2(self.sig))

    def check(self, out):
        assert tuple(out.shape) == (self.nb, self.nt // 5, 512, 4, 2) and bool(torch.isfinite(out).all())

    def outputs(self, out):
        return {"dp_ipd": out}

    def config(self):
        return {"workload": "BASELINE configs[4]: IPDnet2 OnlineSpatialNet (8 layers, hidden 96, mamba(16,4)), 15-mic "
                            "mapping dim_input 30 (SURVEY 8d), 256 bins -> 2F = 512 outputs, online / causal path; %s "
                            "-> [B, T/5, 512, 4, 2]; %d utterances/GPU x %d frames; %s; "
                            "parity: front end and non-Mamba blocks pinned to the reference, Mamba unpinned"
                            % ("features [B, 30, 256, T] resident in HBM" if self.features_in else
                               "waveforms [B, ns, 15] resident in HBM -> centred hop-320 STFT -> all-channel "
                               "forgetting_norm(249) features [B, 30, 256, T] (run_IPDnet2.py:277-288)",
                               self.nb, self.nt,
                               "fp32" if self.fp32 else "bf16 parameters; bf16 MFMA operands in the encoder, the grouped "
                               "frequency conv and the Mamba in / x / out projections, fp32 accumulate, fp32 tensors in HBM; "
                               "LayerNorm, depthwise conv, dt_proj, scan, full-band branch and head fp32"),
                "utterances_per_gpu": self.nb, "mics": self.mics, "frames": self.nt, "bins": 256,
                "parallelism": "dp%d (utterance shards, no collective)" % self.world,
                "mflop_per_frame": round(self.flop_per_frame / 1e6, 2)}

    def extra(self, value, kern, steps):
        return {"whole_path_tflops": round(value * self.flop_per_frame / 1e12 / self.world, 2)}

    def roofline(self, kern):
        # every kernel of this network is a small dense contraction (fp32 MFMA for the projections / convs, packed fp32
        # FMA for the scan): the roof is the fp32 matrix peak, which is also the packed-FMA rate
        dom = max((k for k in kern if k.startswith("sn_")), key=lambda k: kern[k]["ms"], default=None)
        if dom is None:
            return None
        on_bf16 = not self.fp32 and (dom in ("sn_encoder", "sn_mamba_in", "sn_mamba_xproj", "sn_mamba_out") or
                                     dom.startswith("sn_fconv"))
        if dom == "sn_mamba_scan":
            # The selective scan has NO matrix product: its roof is VALU issue.  Per (sequence, channel, step): 16 decays
            # exp2(dt*A_n) + softplus + SiLU = 22 quarter-rate transcendentals (16 issue cycles each per wave) + ~60 packed /
            # scalar fp32 instructions (4 cycles each) ~ 592 issue cycles per wave-step; a launch of S sequences x T steps
            # has S*192/64 waves on 1024 SIMDs.  achieved / peak are reported in wave-steps per second (the unit says so).
            k = kern[dom]
            nb = self.nb
            wave_steps = 2 * (nb * 16 * 192 // 64) * self.nt + 2 * (self.layers - 1) * (nb * 16 * 192 // 64) * (self.nt // 5)
            clock = 2.4e9
            peak = 1024 * clock / 592.0                                    # wave-steps per second, all SIMDs issuing
            ach = wave_steps * (k["count"] / (2.0 * self.layers)) / (k["ms"] * 1e-3) if k["ms"] > 0 else 0.0
            traffic, src = traffic_of("c5_sn_mamba_scan")
            roof = {"name": dom, "bound": "valu", "kernel": "sn_mamba_scan (selective scan: no matrix product; roof = VALU / "
                    "transcendental issue)", "achieved": round(ach / 1e9, 3), "unit": "G wave-steps/s", "traffic": traffic,
                    "traffic_source": src, "launches": k["count"], "avg_ms": round(k["ms"] / max(1, k["count"]), 4)}
            # The roof from COUNTERS (committed rocprofv3 --pmc pass of this kernel, like `traffic`): the fraction of its cycles a
            # SIMD spends issuing vector-ALU instructions = (SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES, per wave) x the waves resident
            # per SIMD (S sequences x 3 waves on 1024 SIMDs) — recomputable from the JSON; `peak` = achieved / frac.  The
            # instruction-count model of rounds 3 - 4 (592 issue cycles per wave-step at an assumed 2.4 GHz) is kept as
            # `frac_model` for comparison only.
            sq = sq_counters_of("sn_mamba_scan_kernel")
            waves_per_simd = min(8.0, nb * 16 * 3 / 1024.0)
            if sq and sq.get("SQ_WAVE_CYCLES"):
                frac = min(1.0, sq["SQ_ACTIVE_INST_VALU"] / sq["SQ_WAVE_CYCLES"] * waves_per_simd)
                roof.update({"frac": round(frac, 4), "peak": round(ach / frac / 1e9, 3) if frac > 0 else None,
                             "frac_source": SQ_JSON + ": SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES = %.3f per wave x %.2f waves resident per SIMD "
                                            "(not this run)" % (sq["SQ_ACTIVE_INST_VALU"] / sq["SQ_WAVE_CYCLES"], waves_per_simd),
                             "frac_model": round(ach / peak, 4)})
            else:
                roof.update({"frac": round(ach / peak, 4), "peak": round(peak / 1e9, 3),
                             "frac_source": "instruction-count model: 592 issue cycles per wave-step at 2.4 GHz (no committed SQ counters found)"})
            return roof
        r = kernel_roof(kern, dom, "%s (dominant kernel of the step%s)" % (dom, ", bf16 MFMA operands" if on_bf16 else
                                                                           ", fp32 arithmetic"),
                        PEAK_BF16_MFMA_TFLOPS if on_bf16 else PEAK_FP32_MFMA_TFLOPS)
        return r

    def cpu_baseline(self):
        from oracle import torch_ref as R
        cores = usable_cores()
        torch.set_num_threads(cores)
        frames = 50 if self.nt >= 50 else self.nt // 5 * 5
        sig = self.sig[:1, :320 * (frames - 1)].contiguous()
        sigc = sig.cpu()
        R.ipdnet2_forward(self.sd, R.array_preprocess(sigc[:, :320 * 4], 249, 320, True))      # warm-up (5 frames)
        c0 = time.perf_counter()
        want = R.ipdnet2_forward(self.sd, R.array_preprocess(sigc, 249, 320, True))            # fp32 PyTorch CPU forward
        cdt = time.perf_counter() - c0
        cpu = {"value": round(frames / cdt, 2), "unit": "frames/s", "cores": cores, "kind": "port",
               "sample": "1 utterance x 15 mics x %d frames from the waveform, PyTorch CPU restatement (oracle/torch_ref.py::"
                         "ipdnet2_forward: torch.stft, conv1d, layer_norm, matmul; the Mamba block = the published "
                         "algorithm with a python scan over frames, parity unpinned), fp32, %d threads, %.1f s"
                         % (frames, cores, cdt)}
        feats = self.ops.preprocess_ipdnet2(sig)
        if self.fp32:
            return cpu, parity_of(self.net(feats).cpu(), want, 1e-4, 5e-5, "%d frames vs the fp32 PyTorch CPU forward" % frames)
        # bf16 (BASELINE config 5 as written; no reference of that precision exists).  Two statements on the sample:
        #  (1) the SAME network on the exact-fp32 kernels against the fp32 CPU forward at the fp32 tolerance — this is what
        #      holds the kernels' arithmetic to the restated reference;
        #  (2) the bf16 mode against those fp32 kernels within a bound stated BEFORE measuring: operands rounded to bf16 carry
        #      a relative error of at most u = 2^-9 each; through S = 4 products per layer x 8 layers of a residual network the
        #      errors add like a random walk, rms <= u sqrt(S) of the outputs' rms (1.1 %); the largest of the sample's ~4e4
        #      outputs lies within 6 sigma of that.  (Measured: rms 0.5 %, max 2.4 sigma.)
        got32 = self.net32(feats).cpu()
        par = parity_of(got32, want, 1e-4, 5e-5, "%d frames, fp32 kernels vs the fp32 PyTorch CPU forward" % frames)
        got = self.net(feats).cpu()
        u, stages = 2.0 ** -9, 4 * self.layers
        out_rms = float(got32.pow(2).mean().sqrt())
        rms_bound = u * stages ** 0.5 * out_rms
        dev_ = (got - got32).abs()
        rms, mx = float(dev_.pow(2).mean().sqrt()), float(dev_.max())
        par["bf16_vs_fp32_kernels"] = {"rms": rms, "max": mx, "output_rms": out_rms, "rms_bound": rms_bound, "max_bound": 6.0 * rms_bound,
                                       "bound": "u sqrt(S) x output rms, u = 2^-9 (bf16 operand rounding), S = 4 products x %d layers; "
                                                "max within 6 sigma" % self.layers,
                                       "ok": bool(rms <= rms_bound and mx <= 6.0 * rms_bound)}
        par["max_abs_err_bf16_vs_cpu"] = float((got - want).abs().max())
        par["ok"] = bool(par["ok"] and par["bf16_vs_fp32_kernels"]["ok"])
        log("parity bf16 vs fp32 kernels: rms %.3g (bound %.3g), max %.3g (bound %.3g) ok=%s"
            % (rms, rms_bound, mx, 6.0 * rms_bound, par["bf16_vs_fp32_kernels"]["ok"]))
        return cpu, par


WORKLOADS = {2: FnsslForward, 3: IpdnetForward, 4: FnsslTrain, 5: Ipdnet2Forward}


# ------------------------------------------------------------------------------------------------------------ #
# the ONE stdout line: compact (< 4 KB); everything else goes to the detail file
# ------------------------------------------------------------------------------------------------------------ #
LINE_LIMIT = 4096
_CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
             "vs_baseline", "dtype", "data")
_ROOF_KEYS = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "launches", "avg_ms", "flop_per_launch",
              "peak_measured", "frac_of_peak_measured", "peak_measured_sustained", "slowest_xcd_mhz", "fastest_xcd_mhz")
_CPU_KEYS = ("value", "unit", "cores", "kind", "sample")
_TOP_KEYS = ("cluster_fallbacks", "rccl_world_size", "backend", "peak_mem_gb", "whole_path_tflops",
             "ms_per_step_median_hip_events", "ms_per_step_per_rank")


def _clip(s, n):
    return s if not isinstance(s, str) or len(s) <= n else s[:n - 1] + "~"


def _pick(d, keys, clip=None):
    if not isinstance(d, dict):
        return d
    return {k: (_clip(d[k], clip[k]) if clip and k in clip else d[k]) for k in keys if k in d}


def compact_line(full, detail_path=None, limit=LINE_LIMIT):
    """The stdout line of a run: the contract keys of the headline, its roofline / cpu_baseline / parity in numbers, and
    `other_configs` reduced to five numbers per key.  Per-kernel tables, A/B legs and the prose (`*_source`, `how`) stay
    in the full record (`detail_path`).  Guaranteed `len(json.dumps(result)) < limit`: optional keys are dropped in a
    fixed order if a line would still be too long (the contract keys never are)."""
    line = {k: full.get(k) for k in _CONTRACT}
    cfg = dict(full.get("config") or {})
    cfg["workload"] = _clip(cfg.get("workload", ""), 260)
    for k in list(cfg):
        if k != "workload" and isinstance(cfg[k], str):
            cfg[k] = _clip(cfg[k], 60)
    line["config"] = cfg
    line["roofline"] = _pick(full.get("roofline"), _ROOF_KEYS, {"kernel": 100})
    line["cpu_baseline"] = _pick(full.get("cpu_baseline"), _CPU_KEYS, {"sample": 150})
    par = full.get("parity")
    line["parity"] = _pick(par, ("max_abs_err", "rtol", "atol", "ok"))
    for k in _TOP_KEYS:
        if k in full:
            line[k] = full[k]
    fe = full.get("frontend")
    if isinstance(fe, dict):
        line["frontend"] = _pick(fe, ("bound", "achieved", "peak", "unit", "frac", "ms_per_step"))
    if isinstance(full.get("strong_scaling"), dict):
        line["strong_scaling"] = _pick(full["strong_scaling"], ("global_batch", "utterances_per_rank",
                                                                "one_rank_same_run_ms_per_step", "efficiency"))
    if isinstance(full.get("ab"), dict):        # the A/B legs as one number each: what the shipped default gains over the knob
        line["ab_gain_pct"] = {_clip(k, 40): v.get("gain_of_default_pct") for k, v in full["ab"].items()}
    others = full.get("other_configs")
    if isinstance(others, dict):
        small = {}
        for key, o in others.items():
            if not isinstance(o, dict) or o.get("error"):
                small[key] = {"error": _clip(str((o or {}).get("error", "?")), 80)}
                continue
            r, c, p = o.get("roofline") or {}, o.get("cpu_baseline") or {}, o.get("parity") or {}
            small[key] = {"value": o.get("value"), "ms_per_step": o.get("ms_per_step"), "dtype": o.get("dtype"),
                          "roofline_frac": r.get("frac"), "cpu_baseline": c.get("value"), "parity_ok": p.get("ok"),
                          "cluster_fallbacks": o.get("cluster_fallbacks"), "peak_mem_gb": o.get("peak_mem_gb")}
            if isinstance(o.get("ab"), dict):
                small[key]["ab_gain_pct"] = [v.get("gain_of_default_pct") for v in o["ab"].values()]
        line["other_configs"] = small
    if detail_path:
        line["detail"] = detail_path
    # fit: drop optional keys, least important first
    for victim in ("ms_per_step_per_rank", "frontend", "ab_gain_pct", "detail", "ms_per_step_median_hip_events", "backend",
                   "peak_mem_gb", "whole_path_tflops"):
        if len(json.dumps(line)) < limit:
            break
        if victim == "ms_per_step_per_rank" and len(line.get(victim) or []) <= 8:
            continue
        line.pop(victim, None)
    if len(json.dumps(line)) >= limit and isinstance(line.get("other_configs"), dict):
        line["other_configs"] = {k: (v if "error" in v else {"value": v.get("value"), "ms_per_step": v.get("ms_per_step")})
                                 for k, v in line["other_configs"].items()}
    if len(json.dumps(line)) >= limit:
        line["config"] = {"workload": _clip(cfg["workload"], 120)}
        if isinstance(line.get("cpu_baseline"), dict):
            line["cpu_baseline"]["sample"] = _clip(line["cpu_baseline"].get("sample"), 60)
    assert len(json.dumps(line)) < limit, "compact line still %d bytes" % len(json.dumps(line))
    return line


def write_detail(full, path):
    """The full record of the run (what the stdout line used to carry) as indented JSON; returns the path or None."""
    try:
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(path, "w") as f:
            json.dump(full, f, indent=1, sort_keys=False)
            f.write("\n")
        return path
    except OSError as e:
        log("could not write %s: %r" % (path, e))
        return None


DUMP_LIMIT_BYTES = 64 * 10 ** 6      # --dump-outputs: all files together, .npy headers included
DUMP_SEED = 20240601


def dump_outputs(arrays, out_dir, limit=DUMP_LIMIT_BYTES):
    """Write ``{name: tensor or array}`` as ``out_dir/<name>.npy`` in float32 (float64 stays float64).  If the data
    would exceed ``limit`` bytes, every array is cut to the same fraction of its flat entries, chosen by a fixed seed
    (sorted indices), so two runs with the same shapes sample the same entries.  Returns {name: (shape, entries written)}."""
    host = {}
    for name, a in arrays.items():
        if torch.is_tensor(a):
            a = a.detach()
            a = (a if a.dtype == torch.float64 else a.float()).cpu().numpy()
        a = np.asarray(a)
        host[name] = np.ascontiguousarray(a if a.dtype == np.float64 else a.astype(np.float32, copy=False))
    budget = limit - 4096 * len(host)                                   # np.save headers are < 4 KB each
    total = sum(a.nbytes for a in host.values())
    frac = 1.0 if total <= budget else budget / float(total)
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for name, a in host.items():
        flat = a.reshape(-1)
        keep = flat.size if frac >= 1.0 else int(flat.size * frac)
        if keep < flat.size:
            idx = np.sort(np.random.RandomState(DUMP_SEED).choice(flat.size, keep, replace=False))
            flat = flat[idx]
            log("--dump-outputs: %s %s cut to a seeded sample of %d of its %d entries" % (name, a.shape, keep, a.size))
        out = a if keep == a.size else flat
        np.save(os.path.join(out_dir, name + ".npy"), out)
        written[name] = (tuple(a.shape), int(out.size))
    return written


def free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(args):
    """`python bench.py --gpus N` (N > 1) outside torch.distributed.run: start the N ranks ourselves — one process per
    GPU, RCCL — by re-executing this script through torch.distributed.run (the reference's equivalent: Lightning DDP
    spawning one process per device, FN-SSL/Lightning/main.py:286-288).  Never falls back to fewer ranks: with fewer
    than N visible devices it exits 2."""
    import subprocess
    ndev = torch.cuda.device_count() if torch.cuda.is_available() else 0
    shared = os.environ.get("FNSSL_BENCH_SHARED_GPU") == "1"      # test hook: N ranks on cuda:0 over gloo (see tests)
    if ndev < args.gpus and not (shared and ndev >= 1):
        log("--gpus %d but only %d ROCm device(s) visible: refusing to run with fewer ranks" % (args.gpus, ndev))
        sys.exit(2)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    log("launching %d ranks: %s" % (args.gpus, " ".join(cmd)))
    sys.stdout.flush()
    sys.exit(subprocess.call(cmd, env=env))


def run_workload(args, cfg, dev, rank, world, dist, backend, steps, warmup, dump_dir=None):
    """Warm up, timed region (barrier + synchronize on both sides, max over ranks), the last step's outputs to
    ``dump_dir`` (rank 0).  With ``args.full`` also: the instrumented pass before the timed region, the roofline kernel
    bracketed inside it, and the evidence legs after it (calibration, A/B, strong scaling, CPU baseline + parity).
    Returns (line dict on rank 0 / None elsewhere, failed)."""
    from fnssl import ops
    full = bool(getattr(args, "full", False))
    wl = WORKLOADS[cfg](args, dev, rank, world)

    def sync_all():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    if full:
        torch.cuda.reset_peak_memory_stats(dev)      # peak_mem_gb is THIS configuration's, not the process's
    out = None
    for _ in range(warmup):
        out = wl.step()
    sync_all()
    probe_steps, probe_env, kern_all, roof_probe, roof_name, ev = 0, {}, {}, None, None, []
    if full:
        # Per-kernel breakdown: an instrumented pass of its own (every launch bracketed by HIP events), outside the timed
        # region — two event records per launch cost a 106-launch step (IPDnet2) 10 % of its time.  The timed region
        # below brackets only the roofline kernel, which is what `roofline.achieved` is computed from.
        probe_steps = max(1, min(3, steps))
        probe_env = getattr(wl, "probe_env", {})      # e.g. config 3: the instrumented pass runs on ONE stream (kernels alone)
        saved_env = {k: os.environ.get(k) for k in probe_env}
        os.environ.update(probe_env)
        ops._lib.refresh_tuning()       # FNSSL_* knobs are parsed by fnssl/_lib.py, not by the library: re-read them
        ops.timing_select(None)
        ops.timing_enable(True)
        for _ in range(probe_steps):
            out = wl.step()
        sync_all()
        ops.timing_enable(False)
        for k, v in saved_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        ops._lib.refresh_tuning()
        kern_all = ops.timing_collect()
        roof_probe = wl.roofline(kern_all)
        roof_name = roof_probe.get("name") if roof_probe else None
        ops.timing_select(roof_name)
        ops.timing_enable(roof_name is not None)     # HIP events on the launch stream around the roofline kernel only
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    # cluster-resident kernels that give up on a hand-off are recomputed by guarded fallback kernels (correct, slow): the
    # device counter every LSTM call carries is zeroed here and read after the timed region — it must still be 0
    ops.cluster_fallbacks(dev, reset=True)
    sync_all()
    t0 = time.perf_counter()
    for i in range(steps):
        if ev:
            ev[i][0].record()
        out = wl.step()
        if ev:
            ev[i][1].record()
    sync_all()
    dt_local = time.perf_counter() - t0
    assert out is not None
    if full:
        ops.timing_enable(False)
        ops.timing_select(None)
    if dump_dir and rank == 0:           # before anything else runs a step: `out` may live in a reused buffer
        written = dump_outputs(wl.outputs(out), dump_dir)
        log("config %d: outputs of the last timed step -> %s %s" % (cfg, dump_dir, written))
    kern, step_ms = {}, []
    if full:
        kern = ops.timing_collect()
        step_ms = sorted(a.elapsed_time(b) for a, b in ev)
        log("config %d rank %d: timed %d steps in %.3f s (median step %.3f ms by HIP events)"
            % (cfg, rank, steps, dt_local, step_ms[len(step_ms) // 2]))
    else:
        log("config %d rank %d: timed %d steps in %.3f s" % (cfg, rank, steps, dt_local))
    dt, per_rank = dt_local, [round(dt_local / steps * 1e3, 3)]
    if dist is not None:
        cdev = dev if backend == "nccl" else torch.device("cpu")
        tmax = torch.tensor([dt_local], dtype=torch.float64, device=cdev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
        if full:
            allt = [torch.zeros(1, dtype=torch.float64, device=cdev) for _ in range(world)]
            dist.all_gather(allt, torch.tensor([dt_local], dtype=torch.float64, device=cdev))
            per_rank = [round(float(t.item()) / steps * 1e3, 3) for t in allt]
    wl.check(out)
    fallbacks = ops.cluster_fallbacks(dev)
    if dist is not None:
        cdev = dev if backend == "nccl" else torch.device("cpu")
        fb = torch.tensor([fallbacks], dtype=torch.int64, device=cdev)
        dist.all_reduce(fb, op=dist.ReduceOp.SUM)
        fallbacks = int(fb.item())
    peak_mem_gb = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 1) if full else None
    value = wl.frames_per_step * steps * world / dt
    roof = wl.roofline(kern) if roof_name else None      # from the events recorded inside the timed region
    if roof is not None:
        roof.pop("name", None)
        if probe_env and roof_probe is not None:          # the same kernel measured ALONE in the instrumented pass
            roof["alone"] = {"achieved": roof_probe.get("achieved"), "frac": roof_probe.get("frac"),
                             "avg_ms": roof_probe.get("avg_ms"),
                             "how": "instrumented pass with %s (not co-scheduled with another stream's kernels)"
                                    % ", ".join("%s=%s" % kv for kv in sorted(probe_env.items()))}
    breakdown = {k: {"ms_per_step": round(v["ms"] / probe_steps, 3), "launches_per_step": v["count"] / probe_steps,
                     "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2) if v["ms"] > 0 and v["flops"] else None}
                 for k, v in sorted(kern_all.items())}
    extra = wl.extra(value, kern_all, probe_steps) if full else {}

    # ---- evidence legs, after the timed region (never inside it) ---------------------------------------------
    # (a) the box's own fp32-MFMA ceiling: a 2 % difference between two boxes must not hide or fake a 2 % kernel gain
    if roof is not None and roof.get("unit") == "TFLOP/s" and roof.get("peak") == PEAK_FP32_MFMA_TFLOPS and rank == 0:
        try:
            pm = ops.mfma_f32_peak()
            roof["peak_measured"] = round(pm, 1)
            roof["frac_of_peak_measured"] = round(roof["achieved"] / pm, 4) if pm > 0 else None
            roof["peak_measured_how"] = ("fnssl_mfma_f32_peak on this device in this process: v_mfma_f32_16x16x4_f32 only, 2 waves "
                                         "per SIMD on every CU, HIP events, best of 3")
            # ... and held for >= 2 s (the regime a 10-s timed region runs in), with the XCD clocks of the last launch
            if getattr(args, "sustained_seconds", 0) > 0:
                sp = ops.mfma_f32_peak_sustained(seconds=args.sustained_seconds)
                roof["peak_measured_sustained"] = round(sp["tflops_last_quarter"], 1)
                roof["slowest_xcd_mhz"], roof["fastest_xcd_mhz"] = sp["slowest_xcd_mhz"], sp["fastest_xcd_mhz"]
                roof["peak_sustained_detail"] = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in sp.items()}
                log("fp32 MFMA ceiling: burst %.1f, sustained %.1f TFLOP/s over %.1f s (last quarter %.1f); XCD clocks %s MHz"
                    % (pm, sp["tflops"], sp["seconds"], sp["tflops_last_quarter"], sp["xcd_mhz"]))
        except Exception as e:            # calibration only
            log("mfma_f32_peak failed: %r" % (e,))
    # (b) same-process A/B of the kernels this and the previous round changed (A = the shipped default, B = the knob):
    # alternating legs of a few steps each, so that box-to-box differences cancel
    ab = None
    if full and args.ab_steps > 0 and hasattr(wl, "ab_knobs") and world == 1:
        ab = {}
        for label, env in wl.ab_knobs():
            legs = {"A": [], "B": []}
            for _ in range(2):
                for which in ("A", "B"):
                    saved = {k: os.environ.get(k) for k in env}
                    if which == "B":
                        os.environ.update(env)
                    ops._lib.refresh_tuning()
                    wl.step()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _i in range(args.ab_steps):
                        wl.step()
                    e1.record()
                    e1.synchronize()
                    legs[which].append(round(e0.elapsed_time(e1) / args.ab_steps, 3))
                    for k, v in saved.items():
                        if v is None:
                            os.environ.pop(k, None)
                        else:
                            os.environ[k] = v
                    ops._lib.refresh_tuning()
            a_ms, b_ms = min(legs["A"]), min(legs["B"])
            ab[label] = {"A_ms_per_step": legs["A"], "B_ms_per_step": legs["B"], "env_B": env, "steps_per_leg": args.ab_steps,
                         "order": "A B A B (one untimed step after every switch)", "B_over_A": round(b_ms / a_ms, 4),
                         "gain_of_default_pct": round((b_ms / a_ms - 1.0) * 100.0, 2)}
            log("A/B %s: A %s ms, B %s ms" % (label, legs["A"], legs["B"]))
    # (c) strong scaling: the same GLOBAL batch on one rank, same run, so that the line carries its own efficiency
    strong = None
    if full and args.scaling == "strong" and hasattr(wl, "global_nb"):
        t1 = None
        if world > 1:
            if rank == 0:
                one = argparse.Namespace(**vars(args))
                one.scaling, one.nb = "weak", wl.global_nb
                w1 = WORKLOADS[cfg](one, dev, 0, 1)
                w1.step()
                torch.cuda.synchronize()
                p0 = time.perf_counter()
                for _i in range(max(2, min(steps, 5))):
                    w1.step()
                torch.cuda.synchronize()
                t1 = (time.perf_counter() - p0) / max(2, min(steps, 5))
                del w1
            sync_all()
        else:
            t1 = dt / steps
        if rank == 0:
            rate1 = wl.global_nb * wl.nt / t1
            strong = {"global_batch": wl.global_nb, "utterances_per_rank": wl.nb, "one_rank_same_run_ms_per_step": round(t1 * 1e3, 3),
                      "efficiency": round(value / (world * rate1), 4),
                      "how": "value / (n_gpus x frames/s of ONE rank running the whole global batch in the same run)"}

    cpu = parity = None
    if full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu, parity = wl.cpu_baseline()
    failed = (parity is not None and not parity["ok"]) or fallbacks != 0
    if fallbacks:
        log("config %d: %d LSTM launch(es) of the timed region fell back from a cluster-resident kernel: the number is not the "
            "kernels' — value nulled" % (cfg, fallbacks))
    line = None
    if rank == 0:
        line = {
            "metric": wl.metric, "value": None if failed else round(value, 2), "unit": "frames/s", "n_gpus": world,
            "steps": steps, "warmup": warmup, "ms_per_step": round(dt / steps * 1e3, 3),
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": wl.dtype, "data": "synthetic",
            "config": wl.config(), "cluster_fallbacks": fallbacks,
        }
    if rank == 0 and full:
        line.update({
            "roofline": roof, "cpu_baseline": cpu, "parity": parity,
            "ms_per_step_median_hip_events": round(step_ms[len(step_ms) // 2], 3), "ms_per_step_per_rank": per_rank,
            "rccl_world_size": (dist.get_world_size() if backend == "nccl" else 0) if dist is not None else 1,
            "backend": backend if dist is not None else None,
            "peak_mem_gb": peak_mem_gb, "kernels": breakdown,
            "kernels_source": "separate instrumented pass of %d steps (every launch bracketed); the timed region brackets only the roofline kernel" % probe_steps,
        })
        line.update(extra)
        if ab:
            line["ab"] = ab
        if strong:
            line["strong_scaling"] = strong
    # give the memory back before the next configuration (config 2 plans 90 GB, config 4 132 GB) — including the library-side
    # workspaces the ops cache per stream (round 5's nested lines carried config 2's 84 GB plan in their `peak_mem_gb`:
    # config 4 read 214 GB where the step itself peaks at 130)
    del wl, out
    import gc
    gc.collect()
    ops.release_workspaces()
    torch.cuda.empty_cache()
    return line, failed


def main():
    # stdout carries the ONE JSON line and nothing else: libraries that write to file descriptor 1 (RCCL prints a
    # version banner at init) are pointed at stderr for the duration of the run
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", type=int, default=2, choices=sorted(WORKLOADS), help="BASELINE.json configuration")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline: instrumented per-kernel pass and roofline, fp32-MFMA "
                         "calibration, A/B legs, CPU baseline + parity, strong-scaling efficiency, nested other "
                         "configurations, the detail file (default: off, a lean timed run)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the outputs of the last timed step as DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--other-configs", default=None,
                    help="--full: comma-separated configurations measured AFTER the primary one and nested under "
                         "'other_configs' of the same JSON line (default: 2M,2off,2b1,2s,3,4,5 when the primary is the "
                         "default config-2 headline run; '' = none); each runs its own BASELINE batch for at most "
                         "--other-steps steps")
    ap.add_argument("--other-steps", type=int, default=8)
    ap.add_argument("--nb", type=int, default=0, help="utterances per GPU (default: the configuration's batch)")
    ap.add_argument("--nch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--ch-mode", default="MM")
    ap.add_argument("--chunk-pairs", type=int, default=0)
    ap.add_argument("--stream-chunk", type=int, default=0,
                    help="config 2: streaming inference, a step = the next N frames (multiple of 12) through FN_SSL.forward_stream")
    ap.add_argument("--offline", action="store_true", help="config 2: is_online=False (bidirectional narrow-band LSTM)")
    ap.add_argument("--bf16", action="store_true",
                    help="config 2, NOT the BASELINE metric: the optional fast mode (bf16 MFMA operands in the LSTMs, "
                         "fp32 accumulate/tensors); reported with dtype 'bf16' and its measured deviation")
    ap.add_argument("--fp32", action="store_true", help="configs 3 and 5 in fp32 instead of bf16")
    ap.add_argument("--c-step", action="store_true", help="config 4: the step as one C call (fnssl_train_step)")
    ap.add_argument("--autograd", action="store_true",
                    help="config 4: the step through torch.autograd.Function + torch.optim.Adam (+ DDP with N > 1): the reference's own loop")
    ap.add_argument("--features-in", action="store_true",
                    help="config 5: start from features [B, 30, 256, T] already in HBM (round-2 behaviour) instead of waveforms")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline + parity legs")
    ap.add_argument("--cpu-utts", type=int, default=1, help="utterances in the bounded CPU sample (config 2)")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="target CPU time of the bounded sample (config 2)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: every rank runs the configuration's batch (default); strong: the configuration's batch is the "
                         "GLOBAL batch, split evenly over the ranks (config 2; the line then carries strong_scaling.efficiency)")
    ap.add_argument("--ab-steps", type=int, default=-1,
                    help="--full: steps per leg of the same-process A/B legs run after the timed region (config 2; default 3 "
                         "in the --full run of the default shape, else 0)")
    ap.add_argument("--sustained-seconds", type=float, default=-1.0,
                    help="--full: length of the sustained fp32-MFMA calibration after the timed region (roofline.peak_measured_sustained; "
                         "default 2 s for the primary configuration of a one-rank run, 0 = off)")
    ap.add_argument("--detail", default=os.path.join("gpurun_out", "bench_detail.json"),
                    help="--full: where the FULL record of the run goes (per-kernel tables, A/B legs, nested configurations in full); "
                         "stdout carries the compact line (< 4 KB) only.  Relative paths are taken from the repo root")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    if not args.full:
        asked = [flag for flag, on in (("--other-configs", bool(args.other_configs)), ("--ab-steps", args.ab_steps > 0),
                                       ("--sustained-seconds", args.sustained_seconds > 0)) if on]
        if asked:
            raise SystemExit("%s: measured only with --full" % ", ".join(asked))

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)           # does not return

    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm device (the HIP path has no CPU fallback)")
    shared = os.environ.get("FNSSL_BENCH_SHARED_GPU") == "1"      # test hook: all ranks on cuda:0, gloo instead of RCCL
    if shared:
        local_rank = 0
    elif torch.cuda.device_count() < world:
        raise SystemExit("%d ranks but only %d ROCm device(s) visible (one process per GPU)"
                         % (world, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist, backend = None, None
    if world > 1 or "RANK" in os.environ:       # launched by torch.distributed.run (also with one rank)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = "gloo" if shared else "nccl"
        if backend == "nccl":
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        log("rank %d: %s process group up, world size %d" % (rank, "RCCL" if backend == "nccl" else backend,
                                                             dist.get_world_size()))

    others = args.other_configs
    headline_shape = not (args.nb or args.offline or args.bf16 or args.frames != 300 or args.nch != 4 or args.ch_mode != "MM"
                          or args.chunk_pairs or args.stream_chunk) and args.scaling == "weak" and args.config == 2
    if others is None:
        others = "2M,2off,2b1,2s,3,4,5" if (headline_shape and args.full) else ""
    if args.ab_steps < 0:
        args.ab_steps = 3 if (headline_shape and args.full) else 0
    if args.sustained_seconds < 0:
        args.sustained_seconds = 2.0
    if args.scaling == "strong" and args.config != 2:
        raise SystemExit("--scaling strong is defined for config 2 (the fixed global batch of the headline)")
    other_ids = [c.strip() for c in others.split(",") if c.strip()]

    line, failed = run_workload(args, args.config, dev, rank, world, dist, backend, args.steps, args.warmup,
                                dump_dir=args.dump_outputs)
    nested = {}
    for key in other_ids:
        # "2M" / "2off": SURVEY 8d's secondary reports of config 2 — 'M' pairing (np = 3) and is_online=False — as their
        # own nested lines (5 steps each, bounded CPU sample); "3" / "4" / "5": the other BASELINE configurations
        variant = key if key in ("2M", "2off", "2b1", "2s") else None
        c = 2 if variant else (int(key) if key.isdigit() else -1)
        if (c == args.config and not variant) or c not in WORKLOADS:
            continue
        sub = argparse.Namespace(**vars(args))
        sub.nb, sub.frames, sub.nch, sub.ch_mode, sub.chunk_pairs = 0, 300, 4, "MM", 0
        sub.offline = sub.bf16 = sub.c_step = False
        sub.ab_steps, sub.scaling, sub.stream_chunk, sub.sustained_seconds = (4 if key == "3" else 0), "weak", 0, 0.0
        nsteps = max(1, min(args.steps, args.other_steps))
        if variant:
            # "2b1" / "2s": the reference's real predict shape (Learner.py:219-272: ONE recording) — one 4-mic utterance as a
            # whole, and streamed in 12-frame chunks
            sub.ch_mode, sub.offline = {"2M": ("M", False), "2off": ("MM", True)}.get(variant, ("MM", False))
            sub.cpu_seconds = min(args.cpu_seconds, 6.0)
            nsteps = max(1, min(args.steps, 5))
            if variant in ("2b1", "2s"):
                sub.nb, nsteps = 1, 25
                sub.stream_chunk = 12 if variant == "2s" else 0
        try:
            l2, f2 = run_workload(sub, c, dev, rank, world, dist, backend, nsteps, max(1, min(args.warmup, 2)))
        except Exception as e:                                     # a secondary configuration must not lose the headline
            log("config %s failed: %r" % (key, e))
            l2, f2 = {"error": repr(e)}, False
            if dist is not None:
                raise
        if l2 is not None:
            nested[key] = l2
        if f2:
            log("PARITY FAILED in config %s (its value is withheld; the headline stands)" % key)

    if rank == 0:
        if nested:
            line["other_configs"] = nested
        # the full record (per-kernel tables, A/B legs, prose) goes to the detail file; stdout gets the compact line only:
        # the driver keeps ~10 KB of stdout, and a line it cannot parse is an unmeasured round
        detail = None
        if args.full:
            detail = write_detail(line, args.detail if os.path.isabs(args.detail) else os.path.join(ROOT, args.detail))
        small = compact_line(line, os.path.relpath(detail, ROOT) if detail else None)
        log("headline: %s frames/s, %.3f ms/step, roofline frac %s, cpu_baseline %s; detail -> %s"
            % (small["value"], small["ms_per_step"], (small.get("roofline") or {}).get("frac"),
               (small.get("cpu_baseline") or {}).get("value"), detail))
        os.write(json_fd, (json.dumps(small) + "\n").encode())
    if dist is not None:
        dist.destroy_process_group()
    if failed:
        log("PARITY FAILED: value withheld")
        sys.exit(1)


if __name__ == "__main__":
    main()
