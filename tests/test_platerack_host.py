"""OLFX_KIND_PLATERACK on the CPU: the host core's tables, defaults, coefficient record, control
table and validation (tests/cpp/test_platerack_host.cpp, linked with olfx_host.cpp, no GPU), and
the kind through the C ABI."""
import ctypes
import os
import subprocess

import ol_dsp_amd as ofx
from ol_dsp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_platerack_host_core(tmp_path):
    """Its own build line: the test and olfx_host.cpp, no library, no HIP header."""
    exe = str(tmp_path / "test_platerack_host")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_platerack_host.cpp"),
           os.path.join(ROOT, "ol_dsp_amd", "csrc", "olfx_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "5 tests, 0 failures" in r.stdout


def test_platerack_kind_info():
    info = ofx.kind_info(ofx.KIND_PLATERACK)
    assert info.kind == 8 and _lib.KIND_PLATERACK == 8
    assert (info.n_params, info.in_channels, info.out_channels) == (19, 2, 2)
    rack, plate = ofx.kind_info(ofx.KIND_FXRACK), ofx.kind_info(ofx.KIND_DATTORRO)
    # one instance: the rack's state and 64 (padded) plates
    assert info.state_bytes_per_instance == rack.state_bytes_per_instance + 64 * plate.state_bytes_per_instance
    names = ofx.PARAMS[ofx.KIND_PLATERACK]
    assert len(names) == 19 and names[:12] == ofx.PARAMS[ofx.KIND_FXRACK]
    assert names[12:] == ["verb_" + p for p in ofx.PARAMS[ofx.KIND_DATTORRO]]
    assert ofx.KIND_NAMES["platerack"] == 8
    assert ofx.load().olfx_abi_version() == 2


def test_platerack_control_map_binding():
    assert ofx.control_map("platerack", 55, 0.25, "hw") == ("verb_decay_diffusion", 0.25)
    assert ofx.control_map("platerack", 33, 0.5, "hw") == ("verb_damping", 0.5)
    assert ofx.control_map("platerack", 52, 64)[0] == "update_only"
    assert ofx.control_map("platerack", 35, 0.5, "hw") == ofx.control_map("fxrack", 35, 0.5, "hw")
    assert ofx.control_map("fxrack", 55, 0.25, "hw") is None


def test_platerack_create_reaches_the_device_probe():
    """The kind is known: olfx_create gets as far as the device (OLFX_E_NODEVICE without one), never
    OLFX_E_KIND."""
    lib = ofx.load()
    h = ctypes.c_void_p()
    rc = lib.olfx_create(ofx.KIND_PLATERACK, 0, 4, 48000.0, 256, ctypes.byref(h))
    has_gpu = os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK)
    if rc == _lib.OLFX_OK:
        assert has_gpu and h.value
        assert lib.olfx_kernel_name(h) == b"platerack_block_v1"
        assert lib.olfx_destroy(h) == _lib.OLFX_OK
    else:
        assert rc == _lib.OLFX_E_NODEVICE, (rc, lib.olfx_last_error(None))
        assert not h.value
        assert b"no HIP device" in lib.olfx_last_error(None)
    # a kind nobody has is still refused as a kind
    assert lib.olfx_create(9, 0, 4, 48000.0, 256, ctypes.byref(h)) == _lib.OLFX_E_KIND


def test_platerack_bank_surface(tmp_path):
    """olfx::PlateRackBank (include/olfx_fx.hpp) builds against the plain C ABI with g++ alone; off-GPU
    construction throws OLFX_E_NODEVICE, on a GPU the setters, a control change and both topologies
    are checked (tests/cpp/test_platerack_bank.cpp)."""
    exe = str(tmp_path / "test_platerack_bank")
    lib_dir = os.path.join(ROOT, "ol_dsp_amd")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_platerack_bank.cpp"), "-L" + lib_dir,
           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-lolfx"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    if os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK):
        assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr
    else:
        assert r.returncode == 2 and "no HIP device" in r.stdout and "(code -4)" in r.stdout, r.stdout + r.stderr
