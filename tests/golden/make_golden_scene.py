#!/usr/bin/env python3
"""G23: the scene finish from the REAL reference (build container only: needs /root/reference).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_scene.py

Imports the reference's own ``Dataset.py`` (both variants) with the absent packages stubbed and, as ``gpuRIR``, a small adapter
of THIS project's float64 tests/rir_ref.py (ism, tail, trajectory; gpuRIR itself cannot run here), and records
  (a) ``NoiseDataset.gen_diffuse_noise`` for 2 and 4 microphones at L = 1000 and 1087 (input mean 0.3);
  (b) ``AcousticScene.simulate()`` with a given noise_signal and source_vad, 2 sources, 3 trajectory points, 2 microphones,
      4096 samples, at T60 = 0 and T60 = 0.2.
The inputs are tests/scene_ref.py's cases (exact in float32).  Only data is written.
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import scene_ref as R  # noqa: E402

for name in ("soundfile", "pandas", "webrtcvad", "matplotlib", "matplotlib.pyplot", "matplotlib.animation"):
    try:
        __import__(name)
    except Exception:
        sys.modules[name] = types.ModuleType(name)
if not hasattr(sys.modules["matplotlib"], "pyplot"):
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["matplotlib"].animation = sys.modules["matplotlib.animation"]

# ---- gpuRIR: an adapter of tests/rir_ref.py (float64).  Source s of a scene makes calls 2 s (full) and 2 s + 1 (direct path);
# its tail is drawn from seed_base + s, as fnssl.scene.simulate does.
gpuRIR = types.ModuleType("gpuRIR")
gpuRIR.calls = 0
gpuRIR.seed_base = 0
gpuRIR.att2t_SabineEstimator = lambda att_db, t60: att_db / 60.0 * t60
gpuRIR.t2n = lambda t, room, c=343.0: [int(v) for v in np.ceil(2.0 * t * c / np.asarray(room, dtype=np.float64))]


def _simulate_rir(room_sz, beta, pos_src, pos_rcv, nb_img, Tmax, fs, Tdiff=None, spkr_pattern="omni", mic_pattern="omni",
                  orV_src=None, orV_rcv=None, c=343.0):
    assert spkr_pattern == "omni" and mic_pattern == "omni"
    seed = gpuRIR.seed_base + gpuRIR.calls // 2
    gpuRIR.calls += 1
    return R.simulate_rir(room_sz, beta, np.asarray(pos_src, dtype=np.float64), np.asarray(pos_rcv, dtype=np.float64), nb_img, Tmax,
                          fs, Tdiff, c, seed)


gpuRIR.simulateRIR = _simulate_rir
gpuRIR.simulateTrajectory = lambda x, rirs, timestamps=None, fs=None: R.rir_ref.trajectory(x, rirs, timestamps, fs)
sys.modules["gpuRIR"] = gpuRIR


def load_dataset(variant):
    d = os.path.join("/root/reference", variant)
    sys.path.insert(0, d)
    try:
        spec = importlib.util.spec_from_file_location("ref_dataset_" + variant.replace("-", "_").replace("/", "_"), os.path.join(d, "Dataset.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(d)
        sys.modules.pop("utils_", None)
    return mod


def main():
    mods = [load_dataset("IPDnet"), load_dataset("FN-SSL")]
    arrs = {}
    # (a)
    for m in (2, 4):
        for length in (1000, 1087):
            v, t = R.diffuse_case(m, length)
            v = v.astype(np.float32)
            nd = object.__new__(mods[0].NoiseDataset)       # IPDnet's: FN-SSL/Dataset.py uses math without importing it
            nd.fs = R.FS
            out = nd.gen_diffuse_noise(v.astype(np.float64), t, R.FS, R.MICS[m])
            key = "a_%d_%d" % (m, length)
            arrs[key + "_noise"], arrs[key + "_T"], arrs[key + "_mic_pos"], arrs[key + "_out"] = v, np.float64(t), R.MICS[m], out
    # (b)
    for t60 in (0, 0.2):
        k = R.scene_case(t60)
        got = []
        for D in mods:
            sc = D.AcousticScene(room_sz=k["room_sz"], T60=k["T60"], beta=k["beta"], noise_signal=k["noise_signal"].copy(), SNR=k["SNR"],
                                 source_signal=k["source_signal"], fs=k["fs"], array_setup=D.dualch_array_setup, mic_pos=k["mic_pos"],
                                 timestamps=k["timestamps"], traj_pts=k["traj_pts"], trajectory=None, t=k["t"], DOA=None)
            sc.source_vad = k["source_vad"]
            gpuRIR.calls, gpuRIR.seed_base = 0, k["seed"]
            mic = sc.simulate()
            got.append((mic, sc.mic_vad_sources, sc.mic_vad, sc))
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
        mic, vs, v, sc = got[0]
        key = "b_%g" % t60
        for name in ("beta", "source_signal", "traj_pts", "mic_pos", "noise_signal"):
            arrs[key + "_" + name] = np.asarray(k[name]).astype(np.float32)
        arrs[key + "_source_vad"] = k["source_vad"].astype(np.uint8)
        arrs[key + "_timestamps"] = k["timestamps"]
        arrs[key + "_room_sz"] = np.asarray(k["room_sz"])
        arrs[key + "_scalars"] = np.array([k["T60"], k["SNR"], k["fs"], k["seed"], len(k["t"])], dtype=np.float64)
        arrs[key + "_mic_signals"] = mic
        arrs[key + "_mic_vad_sources"] = np.asarray(vs).astype(np.uint8)
        arrs[key + "_mic_vad"] = np.asarray(v).astype(np.uint8)
        arrs[key + "_dp_mic_signals_sources"] = sc.dp_mic_signals_sources.astype(np.float32)
    path = os.path.join(HERE, "g23_scene.npz")
    np.savez_compressed(path, **arrs)
    print("wrote g23_scene.npz, %d bytes" % os.path.getsize(path), {k: v.shape for k, v in arrs.items() if k.startswith("b_0.2")})


if __name__ == "__main__":
    main()
