"""CPU tests of fnssl/scene.py and of the argument checks of csrc/scene.hip that come before any device work."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from fnssl import _lib, scene

MICS2 = np.array([[-0.04, 0.0, 0.0], [0.04, 0.0, 0.0]])


def a_scene(**over):
    setup = types.SimpleNamespace(mic_orV=None, mic_pattern=over.pop("mic_pattern", "omni"))
    base = dict(room_sz=[3.2, 4.1, 2.6], T60=0.0, beta=[0.0] * 6, noise_signal=np.zeros((1024, 2)), SNR=10.0,
                source_signal=np.zeros((1024, 1)), fs=16000.0, array_setup=setup, mic_pos=MICS2 + 1.5, timestamps=np.array([0.0]),
                traj_pts=np.full((1, 3, 1), 1.0), t=np.arange(1024) / 16000.0)
    base.update(over)
    return types.SimpleNamespace(**base)


def test_unbuilt_variants_are_named():
    with pytest.raises(NotImplementedError, match="cylindrical"):
        scene.gen_diffuse_noise(np.zeros(2000), 0.0625, 16000.0, MICS2, type_nf="cylindrical")
    with pytest.raises(NotImplementedError, match="eigen"):
        scene.mix_signals(np.zeros((1000, 2)), np.ones((2, 2, 129)), method="eigen")
    with pytest.raises(NotImplementedError, match="cardioid"):
        scene.simulate(a_scene(mic_pattern="cardioid"))


def test_cpu_tensors_are_rejected_with_the_rir_message():
    msg = "expected a ROCm device tensor or a numpy array"
    with pytest.raises(RuntimeError, match=msg):
        scene.acoustic_power(torch.zeros(1024))
    with pytest.raises(RuntimeError, match=msg):
        scene.gen_diffuse_noise(torch.zeros(2000), 0.0625, 16000.0, MICS2)
    with pytest.raises(RuntimeError, match=msg):
        scene.mix_signals(np.zeros((1000, 2)), torch.ones((2, 2, 129)))
    with pytest.raises(RuntimeError, match=msg):
        scene.simulate(a_scene(source_signal=torch.zeros((1024, 1))))


def test_limits_are_checked_before_any_device_work():
    with pytest.raises(ValueError, match="511 samples"):
        scene.acoustic_power(np.zeros(511))
    with pytest.raises(ValueError, match="nfft = 512"):
        scene.gen_diffuse_noise(np.zeros(2000), 0.0625, 16000.0, MICS2, nfft=512)
    with pytest.raises(ValueError, match=r"17 microphones \(1 .. 16\)"):
        scene.gen_diffuse_noise(np.zeros(17 * 1000), 0.0625, 16000.0, np.zeros((17, 3)))
    with pytest.raises(ValueError, match="nfft = 512"):
        scene.mix_signals(np.zeros((1000, 2)), np.ones((2, 2, 257)))
    with pytest.raises(ValueError, match="17 microphones"):
        scene.mix_signals(np.zeros((1000, 17)), np.ones((17, 17, 129)))
    with pytest.raises(ValueError, match="DC"):
        scene.mix_signals(np.zeros((1000, 2)), np.ones((3, 3, 129)))
    with pytest.raises(ValueError, match="500 samples"):
        scene.simulate(a_scene(t=np.arange(500) / 16000.0))
    with pytest.raises(ValueError, match="5 sources"):
        scene.simulate(a_scene(traj_pts=np.full((1, 3, 5), 1.0)))


def last_error():
    return _lib.load().fnssl_last_error().decode()


def test_library_refusals_name_the_limit():
    """FNSSL_E_INVALID (1) with the message, before the stream is touched: the pointers below are never dereferenced."""
    lib = _lib.load()
    p = C.c_void_p(64)
    assert lib.fnssl_anf_mix(p, 0, 2, 1, None, p, 1, 1, 1000, 2, 512, 0, p, None) != 0
    assert "nfft = 512 (only 256 is built)" in last_error()
    assert lib.fnssl_anf_mix(p, 0, 17, 1, None, p, 1, 1, 1000, 17, 256, 0, p, None) != 0
    assert "17 microphones (1 .. 16)" in last_error()
    assert lib.fnssl_anf_factor(p, 1, 17, 256, p, p, None) != 0 and "17 microphones" in last_error()
    assert lib.fnssl_anf_coherence(p, 1, 2, 16000.0, 128, 343.0, p, None) != 0 and "nfft = 128" in last_error()
    assert lib.fnssl_anf_mix(p, 0, 2, 1, None, p, 2, 3, 1000, 2, 256, 0, p, None) != 0 and "2 factors for 3 items" in last_error()
    arr = (C.c_void_p * 4)(64, 64, 64, 64)
    assert lib.fnssl_scene_power(arr, 1, 511, 2, p, 1 << 20, p, None) != 0
    assert "511 samples (acoustic_power needs one window of 512)" in last_error()
    assert lib.fnssl_scene_power(arr, 5, 1024, 2, p, 1 << 20, p, None) != 0 and "5 summands (1 .. 4)" in last_error()
    assert lib.fnssl_scene_power(arr, 1, 1024, 2, p, 7, p, None) != 0 and "floats of scratch" in last_error()
    assert lib.fnssl_scene_finish(arr, 5, p, None, 1024, 2, p, p, 10.0, p, p, None, None, None, None) != 0 and "5 sources" in last_error()
    assert lib.fnssl_scene_finish(arr, 2, p, arr, 1024, 2, p, p, 10.0, p, p, None, None, None, None) != 0
    assert "VAD inputs without VAD outputs" in last_error()
    assert lib.fnssl_anf_mean(p, 1, 100000, 0, p, 6, p, None) != 0 and "7 needed" in last_error()


def test_binding_constants_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fnssl.h")).read()
    for name, value in (("ANF_NFFT", _lib.ANF_NFFT), ("ANF_BINS", _lib.ANF_BINS), ("ANF_MAX_MICS", _lib.ANF_MAX_MICS),
                        ("ANF_MEAN_CHUNK", _lib.ANF_MEAN_CHUNK), ("SCENE_MAX_SOURCES", _lib.SCENE_MAX_SOURCES)):
        assert int(re.search(r"#define FNSSL_%s (\d+)" % name, hdr).group(1)) == value
