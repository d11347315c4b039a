#!/usr/bin/env python3
"""G24: the label stage from the REAL reference (build container only: needs /root/reference).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_labels.py

Imports the reference's own ``IPDnet/Dataset.py`` with the absent packages stubbed and records
  (a) ``cart2sph`` on the centred trajectories of tests/labels_ref.py's four trajectory cases (n = 1000; every 4th row is kept);
  (b) ``Segmenting_SRPDNN(K, step).__call__`` on labels_ref.GOLDEN_SEG (L <= 2000, two sources): DOAw, the VAD windows, tw;
The ``gts`` padding of ``FixTrajectoryDataset.__getitem__`` is NOT recorded: the reference hard-codes its training shapes there
and reads its scenes from files, so it cannot run on these cases; tests/labels_ref.py's ``gts`` is a restatement and is named so.
The inputs are labels_ref's cases; they are named by their sha256 instead of being stored.  Only data is written.
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import labels_ref as R  # noqa: E402

for name in ("soundfile", "pandas", "webrtcvad", "gpuRIR", "matplotlib", "matplotlib.pyplot", "matplotlib.animation"):
    try:
        __import__(name)
    except Exception:
        sys.modules[name] = types.ModuleType(name)
if not hasattr(sys.modules["matplotlib"], "pyplot"):
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["matplotlib"].animation = sys.modules["matplotlib.animation"]


def load_dataset(variant):
    d = os.path.join("/root/reference", variant)
    sys.path.insert(0, d)
    try:
        spec = importlib.util.spec_from_file_location("ref_dataset_" + variant.replace("-", "_"), os.path.join(d, "Dataset.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(d)
        sys.modules.pop("utils_", None)
    return mod


def ref_transform(D, case, L, K, step):
    sc = types.SimpleNamespace(DOA=case["DOA"].copy(), mic_vad_sources=case["mic_vad_sources"].copy(),
                               mic_vad=case["mic_vad"].copy(), fs=case["fs"])
    x = np.zeros((L, 2))
    _, sc = D.Segmenting_SRPDNN(K, step)(x, sc)
    return sc


def main():
    D = load_dataset("IPDnet")
    arrs = {}
    # (a)
    for name in R.TRAJ_CASES:
        pts, ts, n, fs, pos = R.traj_case(name)
        traj, _ = R.trajectory_doa(pts, ts, n, fs, pos)
        for s in range(pts.shape[2]):
            cart = traj[:, :, s] - pos
            arrs["a_%s_%d_in" % (name, s)] = R.digest(cart)
            arrs["a_%s_%d_sph" % (name, s)] = D.cart2sph(cart)[::4]          # every 4th sample keeps the file small
            # the interpolation is numpy's own call in the reference
            assert np.array_equal(traj[:, :, s], np.array([np.interp(np.arange(n) / fs, ts, pts[:, i, s]) for i in range(3)]).T)
    # (b)
    for k, (shape, sources) in enumerate(R.GOLDEN_SEG):
        case = R.sub_scene(R.seg_case(*shape), sources)
        sc = ref_transform(D, case, *shape)
        key = "b_%d" % k
        arrs[key + "_in"] = R.digest(case["DOA"], case["mic_vad_sources"], case["mic_vad"])
        arrs[key + "_DOAw"] = sc.DOAw
        assert sc.mic_vad.dtype == np.float64 and sc.mic_vad_sources.dtype == np.float64
        arrs[key + "_mic_vad"] = np.packbits(sc.mic_vad.astype(np.uint8))
        arrs[key + "_mic_vad_sources"] = np.packbits(sc.mic_vad_sources.astype(np.uint8))
        arrs[key + "_vad_shape"] = np.array(sc.mic_vad_sources.shape)
        arrs[key + "_tw"] = sc.tw
    path = os.path.join(HERE, "g24_labels.npz")
    np.savez_compressed(path, **arrs)
    print("wrote g24_labels.npz, %d bytes, %d arrays" % (os.path.getsize(path), len(arrs)))


if __name__ == "__main__":
    main()
