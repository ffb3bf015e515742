"""OLFX_KIND_METER / OLFX_KIND_METER_MONO on the CPU: the host core's rows, window resolution, validation, packets
and reset (tests/cpp/test_meter_host.cpp, linked with olfx_host.cpp, no GPU), and the kinds through the C ABI and
its Python mirror."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ol_dsp_amd as ofx
from ol_dsp_amd import _lib, workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAS_GPU = os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK)


def test_meter_host_core(tmp_path):
    """Its own build line: the test and olfx_host.cpp, no library, no HIP header."""
    exe = str(tmp_path / "test_meter_host")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_meter_host.cpp"),
           os.path.join(ROOT, "ol_dsp_amd", "csrc", "olfx_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "6 tests, 0 failures" in r.stdout


def test_kind_info_names_and_ranges():
    assert (_lib.KIND_METER, _lib.KIND_METER_MONO) == (15, 16) == (ofx.KIND_METER, ofx.KIND_METER_MONO)
    assert ofx.KIND_NAMES["meter"] == 15 and ofx.KIND_NAMES["meter_mono"] == 16
    for kind, ch in ((15, 2), (16, 1)):
        info = ofx.kind_info(kind)
        assert (info.kind, info.n_params, info.in_channels, info.out_channels) == (kind, 2, ch, ch)
        assert info.state_bytes_per_instance == (5 * ch + 2) * 4
        assert ofx.PARAMS[kind] == ["window", "peak_hold"]
    for nobody in (0, 9, 13, 17):
        with pytest.raises(ofx.OlfxError) as err:
            ofx.kind_info(nobody)
        assert err.value.code == _lib.OLFX_E_KIND
    assert ofx.load().olfx_abi_version() == 2
    for name in ("meter", "meter_mono"):
        assert workload.RANGES[name] == [0.0, 96000.0]
        p = workload.instance_params(name, 3, 10)
        assert p.shape == (2, 10) and np.all(p[0] == 0) and np.all(p[1] == 96000)
        with pytest.raises(ofx.OlfxError) as err:
            ofx.control_map(name, 7, 64)                         # no control maps to a meter
        assert err.value.code == _lib.OLFX_E_KIND


def test_header_declares_the_new_symbols():
    src = open(os.path.join(ROOT, "include", "olfx.h")).read()
    assert re.search(r"\bint\s+olfx_meter_read\s*\(", src)
    assert "olfx_meter_read" in _lib.SIGNATURES and hasattr(ofx.load(), "olfx_meter_read")
    assert "OLFX_KIND_METER = 15" in src and "OLFX_KIND_METER_MONO = 16" in src and "13 stays unassigned" in src
    assert re.search(r"typedef struct olfx_meter_level \{ float rms, peak, sum, count, peak_count; \} olfx_meter_level;", src)
    assert "fabsf" in src                                        # the firmware's abs(...) is taken as fabsf, and says so
    assert ctypes.sizeof(_lib.MeterLevel) == 20 and [f for f, _ in _lib.MeterLevel._fields_] == ["rms", "peak", "sum", "count", "peak_count"]
    assert (_lib.MT_WINDOW, _lib.MT_PEAK_HOLD, _lib.MT_NPARAMS) == (0, 1, 2)
    assert re.search(r"enum \{ OLFX_MT_WINDOW = 0, OLFX_MT_PEAK_HOLD, OLFX_MT_NPARAMS \};", src)
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"meter_block_v1" in blob


def test_refusals_without_an_engine_and_create_reaches_the_device_probe():
    """olfx_meter_read refuses a null engine (and, on a GPU, another kind); kinds 15 and 16 are known: olfx_create gets
    as far as the device (OLFX_E_NODEVICE without one), never OLFX_E_KIND; the synth and kit creators refuse them."""
    lib = ofx.load()
    lv = (_lib.MeterLevel * 8)()                                # [4 instances][2 channels] at the most
    assert lib.olfx_meter_read(None, 0, 1, lv) == _lib.OLFX_E_ARG
    h = ctypes.c_void_p()
    for kind in (15, 16):
        assert lib.olfx_create(kind, 0, 0, 48000.0, 256, ctypes.byref(h)) == _lib.OLFX_E_ARG
        assert lib.olfx_create_synth_kind(kind, 0, 4, 4, 48000.0, 256, ctypes.byref(h)) == _lib.OLFX_E_KIND
        rc = lib.olfx_create(kind, 0, 4, 48000.0, 256, ctypes.byref(h))
        if rc == _lib.OLFX_OK:
            assert HAS_GPU and h.value
            assert lib.olfx_kernel_name(h) == b"meter_block_v1"
            assert lib.olfx_algorithmic_bytes_per_frame(h) == (16 if kind == 15 else 8)
            assert lib.olfx_algorithmic_read_bytes_per_frame(h) == (8 if kind == 15 else 4)
            assert lib.olfx_meter_read(h, 0, 4, lv) == _lib.OLFX_OK
            assert lib.olfx_meter_read(h, 3, 2, lv) == _lib.OLFX_E_ARG
            assert lib.olfx_meter_read(h, 0, 1, None) == _lib.OLFX_E_ARG
            assert lib.olfx_mix_config(h, 0, None, None) == _lib.OLFX_E_STATE
            assert lib.olfx_destroy(h) == _lib.OLFX_OK
        else:
            assert rc == _lib.OLFX_E_NODEVICE, (rc, lib.olfx_last_error(None))
            assert not h.value and b"no HIP device" in lib.olfx_last_error(None)
    if HAS_GPU:
        assert lib.olfx_create(ofx.KIND_FXRACK, 0, 4, 48000.0, 256, ctypes.byref(h)) == _lib.OLFX_OK
        assert lib.olfx_meter_read(h, 0, 1, lv) == _lib.OLFX_E_STATE
        assert lib.olfx_destroy(h) == _lib.OLFX_OK
