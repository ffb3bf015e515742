"""OLFX_KIND_VOICE_SAMPLE on the CPU: the host core's tables, event folding with the seek bit, bank
and record validation (tests/cpp/test_sampler_host.cpp, linked with olfx_host.cpp, no GPU), the
kind through the C ABI and the Python binding, and olfx::SamplerBank's build against the C ABI."""
import ctypes
import os
import subprocess

import numpy as np

import ol_dsp_amd as ofx
from ol_dsp_amd import _lib, workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAS_GPU = os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK)


def test_sampler_host_core(tmp_path):
    """Its own build line: the test and olfx_host.cpp, no library, no HIP header."""
    exe = str(tmp_path / "test_sampler_host")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_sampler_host.cpp"),
           os.path.join(ROOT, "ol_dsp_amd", "csrc", "olfx_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "6 tests, 0 failures" in r.stdout


def test_sampler_kind_info():
    info = ofx.kind_info(ofx.KIND_VOICE_SAMPLE)
    assert info.kind == 10 and _lib.KIND_VOICE_SAMPLE == 10
    assert (info.n_params, info.in_channels, info.out_channels) == (16, 0, 1)
    voice = ofx.kind_info(ofx.KIND_VOICE)
    # the voice's words and the five Sample words; the bank is not state
    assert info.state_bytes_per_instance == voice.state_bytes_per_instance + 5 * 4
    assert ofx.PARAMS[ofx.KIND_VOICE_SAMPLE] == ofx.PARAMS[ofx.KIND_VOICE]
    assert ofx.KIND_NAMES["voice_sample"] == 10
    assert ofx.load().olfx_abi_version() == 2
    assert ctypes.sizeof(_lib.SampleVoice) == 32
    for cc in range(128):
        assert ofx.control_map("voice_sample", cc, 77) == ofx.control_map("voice", cc, 77)
        assert ofx.control_map("voice_sample", cc, 0.3, "hw") == ofx.control_map("voice", cc, 0.3, "hw")


def test_sampler_create_reaches_the_device_probe():
    """The kind is known: olfx_create gets as far as the device (OLFX_E_NODEVICE without one), never
    OLFX_E_KIND; the two new entry points refuse a null engine."""
    lib = ofx.load()
    h = ctypes.c_void_p()
    rc = lib.olfx_create(ofx.KIND_VOICE_SAMPLE, 0, 4, 48000.0, 256, ctypes.byref(h))
    if rc == _lib.OLFX_OK:
        assert HAS_GPU and h.value
        assert lib.olfx_kernel_name(h) == b"sampler_block_v1"
        assert lib.olfx_algorithmic_bytes_per_frame(h) == 8.0
        assert lib.olfx_algorithmic_read_bytes_per_frame(h) == 4.0
        assert lib.olfx_destroy(h) == _lib.OLFX_OK
    else:
        assert rc == _lib.OLFX_E_NODEVICE, (rc, lib.olfx_last_error(None))
        assert not h.value
    assert lib.olfx_sample_bank(None, 0, None, None) == _lib.OLFX_E_ARG
    assert lib.olfx_sample_voices(None, None, 0) == _lib.OLFX_E_ARG


def test_workload_bank_is_seeded():
    lens = [1, 3, 7, 1000]
    a, b = workload.sample_bank(lens, seed=3), workload.sample_bank(lens, seed=3)
    assert [len(x) for x in a] == lens and all(x.dtype == np.float32 for x in a)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[3], workload.sample_bank(lens, seed=4)[3])
    assert not np.array_equal(a[3][:7], a[2])
    big = np.concatenate(a)
    assert big.min() >= -0.5 and big.max() <= 0.5 and abs(float(a[3].mean())) < 0.05
    p = workload.instance_params("voice_sample", 0, 8)
    assert np.array_equal(p, workload.instance_params("voice", 0, 8))


def test_sampler_bank_surface(tmp_path):
    """olfx::SamplerBank (include/olfx_fx.hpp) builds against the plain C ABI with g++ alone; off-GPU
    construction throws OLFX_E_NODEVICE, on a GPU a kit is played and checked (tests/cpp/test_sampler_bank.cpp)."""
    exe = str(tmp_path / "test_sampler_bank")
    lib_dir = os.path.join(ROOT, "ol_dsp_amd")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_sampler_bank.cpp"), "-L" + lib_dir,
           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-lolfx"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    if HAS_GPU:
        assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr
    else:
        assert r.returncode == 2 and "no HIP device" in r.stdout and "(code -4)" in r.stdout, r.stdout + r.stderr
