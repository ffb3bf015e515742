"""OLFX_KIND_SYNTH on the CPU: the host core's tables, field split, Polyvoice router and control
fan-out (tests/cpp/test_synth_host.cpp, linked with olfx_host.cpp, no GPU), and the kind through the
C ABI and its Python mirror."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ol_dsp_amd as ofx
from ol_dsp_amd import _lib, workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAS_GPU = os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK)


def test_synth_host_core(tmp_path):
    """Its own build line: the test and olfx_host.cpp, no library, no HIP header."""
    exe = str(tmp_path / "test_synth_host")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_synth_host.cpp"),
           os.path.join(ROOT, "ol_dsp_amd", "csrc", "olfx_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "8 tests, 0 failures" in r.stdout


def test_synth_kind_info_and_names():
    info = ofx.kind_info(ofx.KIND_SYNTH)
    assert info.kind == 11 and _lib.KIND_SYNTH == 11 and ofx.KIND_NAMES["synth"] == 11
    assert (info.n_params, info.in_channels, info.out_channels) == (28, 0, 2)
    rack, voice = ofx.kind_info(ofx.KIND_FXRACK), ofx.kind_info(ofx.KIND_VOICE_MOOG)
    # the 4-voice figure: the rack, one set of voice coefficients, four voices' state
    assert info.state_bytes_per_instance == rack.state_bytes_per_instance + 19 * 4 + 4 * (
        voice.state_bytes_per_instance - 19 * 4)
    names = ofx.PARAMS[ofx.KIND_SYNTH]
    assert len(names) == 28 and len(set(names)) == 28
    assert names[:16] == ofx.PARAMS[ofx.KIND_VOICE]
    assert names[16:] == ["rack_" + p for p in ofx.PARAMS[ofx.KIND_FXRACK]]
    assert ofx.load().olfx_abi_version() == 2
    r = workload.RANGES["synth"]
    assert len(r) == 28 and r[:16] == workload.RANGES["voice"] and r[16:27] == workload.RANGES["fxrack"][:11]
    assert r[27] == 1.0
    p = workload.instance_params("synth", 0, 9, 5)
    assert p.shape == (28, 9) and np.all(p[27] == 1.0)


def test_synth_control_map_binding():
    m = ofx.synth_control_map(41, 64)
    assert [f for f, _ in m] == ["filter_cutoff", "rack_filter_cutoff"]
    assert m[0][1] == ofx.control_map("voice_moog", 41, 64)[1]
    assert m[1][1] == ofx.control_map("fxrack", 45, 64)[1]
    assert m[0][1] != m[1][1]                                   # each handler's own scaling
    assert ofx.synth_control_map(35, 0.5, "hw") == [("rack_delay_time", 0.5)]
    assert ofx.synth_control_map(37, 0.5, "hw") == []          # DelayFx takes these in MIDI only
    assert ofx.synth_control_map(114, 100) == [("update_only", ofx.control_map("voice_moog", 114, 100)[1])]
    assert ofx.synth_control_map(3, 64) == [] and ofx.synth_control_map(45, 64) == []
    with pytest.raises(ofx.OlfxError):
        ofx.control_map("synth", 41, 64)                        # OLFX_E_KIND: two fields, see synth_control_map


def test_synth_create_reaches_the_device_probe():
    """Kind 11 is known: olfx_create and olfx_create_synth get as far as the device (OLFX_E_NODEVICE
    without one), never OLFX_E_KIND; 0 and 9 voices are refused before the probe."""
    lib = ofx.load()
    h = ctypes.c_void_p()
    for voices in (0, 9):
        assert lib.olfx_create_synth(0, 4, voices, 48000.0, 256, ctypes.byref(h)) == _lib.OLFX_E_ARG
        assert not h.value and b"voices" in lib.olfx_last_error(None)
    assert lib.olfx_create_synth(0, 0, 4, 48000.0, 256, ctypes.byref(h)) == _lib.OLFX_E_ARG
    assert lib.olfx_synth_voices(None) == 0
    for create in (lambda: lib.olfx_create(ofx.KIND_SYNTH, 0, 4, 48000.0, 256, ctypes.byref(h)),
                   lambda: lib.olfx_create_synth(0, 4, 8, 48000.0, 256, ctypes.byref(h))):
        rc = create()
        if rc == _lib.OLFX_OK:
            assert HAS_GPU and h.value
            assert lib.olfx_kernel_name(h) == b"synth_block_v1"
            assert lib.olfx_synth_voices(h) in (4, 8)
            # the calls this kind refuses, with the code each uses for a wrong kind
            off = (ctypes.c_uint32 * 2)(0, 1)
            order = (ctypes.c_uint32 * 1)(0)
            assert lib.olfx_mix_config(h, 1, off, order) == _lib.OLFX_E_STATE
            assert lib.olfx_mix(h, None, None, 4, 0, None) == _lib.OLFX_E_STATE
            assert lib.olfx_sample_bank(h, 0, None, None) == _lib.OLFX_E_STATE
            assert lib.olfx_sample_voices(h, None, 0) == _lib.OLFX_E_STATE
            assert lib.olfx_destroy(h) == _lib.OLFX_OK
        else:
            assert rc == _lib.OLFX_E_NODEVICE, (rc, lib.olfx_last_error(None))
            assert not h.value
            assert b"no HIP device" in lib.olfx_last_error(None)
    assert lib.olfx_create(9, 0, 4, 48000.0, 256, ctypes.byref(h)) == _lib.OLFX_E_KIND


def test_synth_bank_surface(tmp_path):
    """olfx::SynthBank (include/olfx_fx.hpp) builds against the plain C ABI with g++ alone; off-GPU
    construction throws OLFX_E_NODEVICE, on a GPU notes, Playing(), a control change and one block
    are checked (tests/cpp/test_synth_bank.cpp)."""
    exe = str(tmp_path / "test_synth_bank")
    lib_dir = os.path.join(ROOT, "ol_dsp_amd")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_synth_bank.cpp"), "-L" + lib_dir,
           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-lolfx"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    if HAS_GPU:
        assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr
    else:
        assert r.returncode == 2 and "no HIP device" in r.stdout and "(code -4)" in r.stdout, r.stdout + r.stderr
