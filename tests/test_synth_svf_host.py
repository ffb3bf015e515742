"""OLFX_KIND_SYNTH_SVF on the CPU: the host core's tables, topology validation, router and control
fan-out by topology (tests/cpp/test_synth_svf_host.cpp, linked with olfx_host.cpp, no GPU), and the kind
through the C ABI and its Python mirror."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ol_dsp_amd as ofx
from ol_dsp_amd import _lib, workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAS_GPU = os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK)


def test_synth_svf_host_core(tmp_path):
    """Its own build line: the test and olfx_host.cpp, no library, no HIP header."""
    exe = str(tmp_path / "test_synth_svf_host")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_synth_svf_host.cpp"),
           os.path.join(ROOT, "ol_dsp_amd", "csrc", "olfx_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "6 tests, 0 failures" in r.stdout


def test_kind_info_and_names():
    info = ofx.kind_info(ofx.KIND_SYNTH_SVF)
    assert info.kind == 12 and _lib.KIND_SYNTH_SVF == 12 and ofx.KIND_NAMES["synth_svf"] == 12
    assert (info.n_params, info.in_channels, info.out_channels) == (28, 0, 2)
    rack, voice = ofx.kind_info(ofx.KIND_FXRACK), ofx.kind_info(ofx.KIND_VOICE)
    # the synth's formula with OLFX_KIND_VOICE's per-voice figures: the rack, one set of voice
    # coefficients, four voices' state
    assert info.state_bytes_per_instance == rack.state_bytes_per_instance + 19 * 4 + 4 * (
        voice.state_bytes_per_instance - 19 * 4)
    assert info.state_bytes_per_instance < ofx.kind_info(ofx.KIND_SYNTH).state_bytes_per_instance
    assert ofx.PARAMS[ofx.KIND_SYNTH_SVF] == ofx.PARAMS[ofx.KIND_SYNTH] and len(ofx.PARAMS[12]) == 28
    assert ofx.load().olfx_abi_version() == 2
    r = workload.RANGES["synth_svf"]
    assert len(r) == 28 and r[:16] == workload.RANGES["voice"] and r[16:27] == workload.RANGES["fxrack"][:11]
    p, q = workload.instance_params("synth_svf", 0, 200, 5), workload.instance_params("synth", 0, 200, 5)
    assert p.shape == (28, 200) and set(np.unique(p[27])) == {0.0, 1.0}
    assert np.array_equal(p[:27], q[:27])                      # the synth's draw, field for field
    assert np.array_equal(workload.instance_params("synth_svf", 50, 20, 5), p[:, 50:70])


def test_control_map_binding():
    # kind 11 at topology 1 is synth_control_map as it was
    for cc, val, src in ((41, 64, "midi"), (35, 0.5, "hw"), (37, 0.5, "hw"), (114, 100, "midi"), (45, 64, "midi")):
        assert ofx.synth_control_map(cc, val, src, kind="synth", topology=1) == ofx.synth_control_map(cc, val, src)
    with pytest.raises(ofx.OlfxError):
        ofx.synth_control_map(41, 64, kind="synth", topology=0)
    with pytest.raises(ofx.OlfxError):
        ofx.synth_control_map(41, 64, kind="synth_svf", topology=2)
    with pytest.raises(ofx.OlfxError):
        ofx.synth_control_map(41, 64, kind="fxrack", topology=0)
    # kind 12: the voice's table, then the rack's at the topology
    m = ofx.synth_control_map(41, 64, kind="synth_svf", topology=1)
    assert [f for f, _ in m] == ["filter_cutoff", "rack_filter_cutoff"]
    assert m[0][1] == ofx.control_map("voice", 41, 64)[1] and m[1][1] == ofx.control_map("fxrack", 45, 64)[1]
    assert ofx.synth_control_map(41, 64, kind="synth_svf", topology=0) == [("filter_cutoff", m[0][1])]
    assert ofx.synth_control_map(45, 64, kind="synth_svf", topology=1) == []
    assert ofx.synth_control_map(45, 64, kind="synth_svf", topology=0) == [
        ("rack_filter_cutoff", ofx.control_map("fxrack", 45, 64)[1])]
    assert ofx.synth_control_map(7, 80, kind="synth_svf", topology=0) == [
        ("amp_env_amount", ofx.control_map("voice", 7, 80)[1]), ("rack_master_volume", ofx.control_map("fxrack", 7, 80)[1])]
    assert ofx.synth_control_map(7, 80, kind="synth_svf", topology=1) == [
        ("amp_env_amount", ofx.control_map("voice", 7, 80)[1])]
    for topology in (0, 1):
        for cc in range(128):
            for val, src in ((64, "midi"), (0.3, "hw")):
                want = []
                v = ofx.control_map("voice", cc, val, src)
                if v is not None:
                    want.append(v)
                as_cc, takes = cc, True
                if topology == 1:
                    takes = 41 <= cc <= 44 or 35 <= cc <= 39 or cc == 34
                    as_cc = cc + 4 if 41 <= cc <= 44 else cc
                r = ofx.control_map("fxrack", as_cc, val, src) if takes else None
                if r is not None:
                    want.append(("rack_" + r[0], r[1]))
                assert ofx.synth_control_map(cc, val, src, kind="synth_svf", topology=topology) == want, (topology, cc)
    with pytest.raises(ofx.OlfxError):
        ofx.control_map("synth_svf", 41, 64)                    # OLFX_E_KIND: two fields


def test_create_reaches_the_device_probe():
    """Kind 12 is known: olfx_create and olfx_create_synth_kind get as far as the device (OLFX_E_NODEVICE
    without one), never OLFX_E_KIND; 0 and 9 voices and kind 10 are refused before the probe."""
    lib = ofx.load()
    h = ctypes.c_void_p()
    for kind in (ofx.KIND_SYNTH, ofx.KIND_SYNTH_SVF):
        for voices in (0, 9):
            assert lib.olfx_create_synth_kind(kind, 0, 4, voices, 48000.0, 256, ctypes.byref(h)) == _lib.OLFX_E_ARG
            assert not h.value and b"voices" in lib.olfx_last_error(None)
    for kind in (ofx.KIND_VOICE_SAMPLE, ofx.KIND_VOICE, 9, 13):
        assert lib.olfx_create_synth_kind(kind, 0, 4, 4, 48000.0, 256, ctypes.byref(h)) == _lib.OLFX_E_KIND
        assert not h.value
    assert lib.olfx_create_synth_kind(ofx.KIND_SYNTH_SVF, 0, 0, 4, 48000.0, 256, ctypes.byref(h)) == _lib.OLFX_E_ARG
    assert lib.olfx_create_synth_kind(ofx.KIND_SYNTH_SVF, 0, 4, 4, 48000.0, 256, None) == _lib.OLFX_E_ARG
    creates = [(lambda: lib.olfx_create(ofx.KIND_SYNTH_SVF, 0, 4, 48000.0, 256, ctypes.byref(h)), b"synth_svf_block_v1", 4),
               (lambda: lib.olfx_create_synth_kind(ofx.KIND_SYNTH_SVF, 0, 4, 8, 48000.0, 256, ctypes.byref(h)),
                b"synth_svf_block_v1", 8),
               (lambda: lib.olfx_create_synth_kind(ofx.KIND_SYNTH, 0, 4, 3, 48000.0, 256, ctypes.byref(h)),
                b"synth_block_v1", 3)]
    for create, kernel, voices in creates:
        rc = create()
        if rc == _lib.OLFX_OK:
            assert HAS_GPU and h.value
            assert lib.olfx_kernel_name(h) == kernel and lib.olfx_synth_voices(h) == voices
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


def test_synth_bank_takes_the_kind(tmp_path):
    """olfx::SynthBank (include/olfx_fx.hpp) with kind = OLFX_KIND_SYNTH_SVF builds against the plain C ABI
    with g++ alone; off-GPU construction throws OLFX_E_NODEVICE, on a GPU one block at both topologies is
    checked (tests/cpp/test_synth_svf_bank.cpp)."""
    exe = str(tmp_path / "test_synth_svf_bank")
    lib_dir = os.path.join(ROOT, "ol_dsp_amd")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_synth_svf_bank.cpp"), "-L" + lib_dir,
           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-lolfx"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    if HAS_GPU:
        assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr
    else:
        assert r.returncode == 2 and "no HIP device" in r.stdout and "(code -4)" in r.stdout, r.stdout + r.stderr
