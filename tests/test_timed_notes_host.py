"""olfx_timed_notes on the CPU: the host core's routing over time, carry-over, validation, refusals and packet
bounds (tests/cpp/test_timed_notes_host.cpp, linked with olfx_host.cpp, no GPU), and the entry point through the C
ABI and the Python binding."""
import ctypes
import os
import subprocess

import ol_dsp_amd as ofx
from ol_dsp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_timed_notes_host_core(tmp_path):
    """Its own build line: the test and olfx_host.cpp, no library, no HIP header."""
    exe = str(tmp_path / "test_timed_notes_host")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_timed_notes_host.cpp"),
           os.path.join(ROOT, "ol_dsp_amd", "csrc", "olfx_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "9 tests, 0 failures" in r.stdout


def test_timed_notes_abi():
    """The record is the frame and a note event, 12 bytes; the entry point exists, refuses a null engine and leaves
    the ABI version alone."""
    lib = ofx.load()
    assert ctypes.sizeof(_lib.TimedNote) == 12 and _lib.TimedNote.ev.offset == 4
    assert lib.olfx_timed_notes(None, None, 0) == _lib.OLFX_E_ARG
    assert lib.olfx_abi_version() == 2


def test_make_timed_notes_layout():
    """The numpy records are the C struct, field for field."""
    rec = ofx.Engine.make_timed_notes([8, 12, 260], [1, 2, 3], _lib.EV_NOTE_ON, [60, 61, 62])
    assert rec.dtype.itemsize == ctypes.sizeof(_lib.TimedNote) and len(rec) == 3
    c = ctypes.cast(rec.ctypes.data, ctypes.POINTER(_lib.TimedNote))
    assert [(c[k].frame, c[k].ev.inst, c[k].ev.type, c[k].ev.note, c[k].ev.velocity) for k in range(3)] == \
        [(8, 1, 1, 60, 100), (12, 2, 1, 61, 100), (260, 3, 1, 62, 100)]
