"""olfx_timed_instrument_params / olfx_timed_instrument_control on the CPU: the host core's raw pending list, controls
mapped at their frame, the launch's end at a boundary field, the union of times and the record cap, validation,
refusals and the packet's timed instrument section (tests/cpp/test_timed_instrument_params_host.cpp, linked with
olfx_host.cpp, no GPU), and the entry points through the C ABI."""
import ctypes
import os
import subprocess

import ol_dsp_amd as ofx
from ol_dsp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_timed_instrument_params_host_core(tmp_path):
    """Its own build line: the test and olfx_host.cpp, no library, no HIP header."""
    exe = str(tmp_path / "test_timed_instrument_params_host")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_timed_instrument_params_host.cpp"),
           os.path.join(ROOT, "ol_dsp_amd", "csrc", "olfx_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "11 tests, 0 failures" in r.stdout


def test_timed_instrument_params_abi():
    """The entry points exist, take the existing 16-byte records, refuse a null engine and leave the ABI version
    alone."""
    lib = ofx.load()
    assert ctypes.sizeof(_lib.TimedParam) == 16 and ctypes.sizeof(_lib.TimedControl) == 16
    assert lib.olfx_timed_instrument_params(None, None, 0) == _lib.OLFX_E_ARG
    assert lib.olfx_timed_instrument_control(None, None, 0) == _lib.OLFX_E_ARG
    assert lib.olfx_abi_version() == 2
    assert hasattr(ofx.Engine, "timed_instrument_params") and hasattr(ofx.Engine, "timed_instrument_control")


def test_header_compiles_as_c(tmp_path):
    """include/olfx.h is a C header: the new calls take the existing record types."""
    src = tmp_path / "abi.c"
    src.write_text('#include "olfx.h"\n'
                   "int f(olfx_engine *e) { struct olfx_timed_control c = {8, {0, 41, 0, OLFX_DK_CHANNEL_RACK, 64.0f}};\n"
                   "  olfx_timed_param p = {8, 0, OLFX_SY_RACK0 + OLFX_FR_FILTER_CUTOFF, 1.0f};\n"
                   "  return olfx_timed_instrument_control(e, &c, 1) + olfx_timed_instrument_params(e, &p, 1); }\n")
    r = subprocess.run([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        "-c", str(src), "-o", str(tmp_path / "abi.o")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
