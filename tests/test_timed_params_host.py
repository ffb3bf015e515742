"""olfx_timed_params / olfx_timed_control on the CPU: the host core's pending list, the union of event and
parameter times, the folds, the carry-over, validation, refusals, the span's two bounds and the packet's timed
coefficient section (tests/cpp/test_timed_params_host.cpp, linked with olfx_host.cpp, no GPU), and the entry
points through the C ABI and the Python binding."""
import ctypes
import os
import subprocess

import numpy as np

import ol_dsp_amd as ofx
from ol_dsp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_timed_params_host_core(tmp_path):
    """Its own build line: the test and olfx_host.cpp, no library, no HIP header."""
    exe = str(tmp_path / "test_timed_params_host")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_timed_params_host.cpp"),
           os.path.join(ROOT, "ol_dsp_amd", "csrc", "olfx_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "13 tests, 0 failures" in r.stdout


def test_timed_params_abi():
    """The records are 16 bytes each; the entry points exist, refuse a null engine and leave the ABI version
    alone."""
    lib = ofx.load()
    assert ctypes.sizeof(_lib.TimedParam) == 16 and _lib.TimedParam.value.offset == 12
    assert ctypes.sizeof(_lib.TimedControl) == 16 and _lib.TimedControl.ev.offset == 4
    assert lib.olfx_timed_params(None, None, 0) == _lib.OLFX_E_ARG
    assert lib.olfx_timed_control(None, None, 0) == _lib.OLFX_E_ARG
    assert lib.olfx_abi_version() == 2


def test_header_compiles_as_c(tmp_path):
    """include/olfx.h is a C header: the timed control record shares its name with the call, as a struct tag."""
    src = tmp_path / "abi.c"
    src.write_text('#include "olfx.h"\n'
                   "int f(olfx_engine *e) { struct olfx_timed_control c = {8, {0, 41, 0, 0, 64.0f}};\n"
                   "  olfx_timed_param p = {8, 0, 0, 1.0f}; return olfx_timed_control(e, &c, 1) + olfx_timed_params(e, &p, 1); }\n")
    r = subprocess.run([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        "-c", str(src), "-o", str(tmp_path / "abi.o")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_make_timed_records_layout():
    """The numpy records are the C structs, field for field."""
    rec = np.zeros(3, dtype=[("frame", "<u4"), ("inst", "<u4"), ("field", "<u4"), ("value", "<f4")])
    assert rec.dtype.itemsize == ctypes.sizeof(_lib.TimedParam)
    rec = ofx.Engine.make_timed_control([8, 12, 260], [1, 2, 3], 41, [10.0, 20.0, 30.0], source="hw")
    assert rec.dtype.itemsize == ctypes.sizeof(_lib.TimedControl) and len(rec) == 3
    c = ctypes.cast(rec.ctypes.data, ctypes.POINTER(_lib.TimedControl))
    assert [(c[k].frame, c[k].ev.inst, c[k].ev.control, c[k].ev.source, c[k].ev.value) for k in range(3)] == \
        [(8, 1, 41, 1, 10.0), (12, 2, 41, 1, 20.0), (260, 3, 41, 1, 30.0)]
