"""The chorus kind's ring-free / ring kernel switch on the CPU: the host core's countdown, same-value
sets, sets before the first frame and reset (tests/cpp/test_ringfree_host.cpp, linked with
olfx_host.cpp, no GPU), and the accessor through the C ABI."""
import os
import subprocess

import ol_dsp_amd as ofx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ringfree_host_core(tmp_path):
    """Its own build line: the test and olfx_host.cpp, no library, no HIP header."""
    exe = str(tmp_path / "test_ringfree_host")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_ringfree_host.cpp"),
           os.path.join(ROOT, "ol_dsp_amd", "csrc", "olfx_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "7 tests, 0 failures" in r.stdout


def test_accessor_without_an_engine():
    assert ofx.load().olfx_chorus_ring_free(None) == -1
