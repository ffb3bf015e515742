"""OLFX_KIND_DRUMKIT on the CPU: the host core's layout, per-slot bookkeeping, VoiceMap, routing and packet
(tests/cpp/test_drumkit_host.cpp, linked with olfx_host.cpp, no GPU), and the kind through the C ABI and its
Python mirror."""
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


def test_drumkit_host_core(tmp_path):
    """Its own build line: the test and olfx_host.cpp, no library, no HIP header."""
    exe = str(tmp_path / "test_drumkit_host")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_drumkit_host.cpp"),
           os.path.join(ROOT, "ol_dsp_amd", "csrc", "olfx_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "8 tests, 0 failures" in r.stdout


def test_kind_info_names_and_ranges():
    info = ofx.kind_info(ofx.KIND_DRUMKIT)
    assert info.kind == 14 and _lib.KIND_DRUMKIT == 14 and ofx.KIND_NAMES["drumkit"] == 14
    assert (info.n_params, info.in_channels, info.out_channels) == (140, 0, 2)
    rack, voice = ofx.kind_info(ofx.KIND_FXRACK), ofx.kind_info(ofx.KIND_VOICE_SAMPLE)
    # the 4-voice figure: the rack, and four voices' state, coefficients and Sample words
    assert voice.state_bytes_per_instance == (8 + 19 + 5) * 4
    assert info.state_bytes_per_instance == rack.state_bytes_per_instance + 4 * voice.state_bytes_per_instance
    with pytest.raises(ofx.OlfxError):
        ofx.kind_info(13)
    assert ofx.load().olfx_abi_version() == 2
    names = ofx.PARAMS[14]
    assert len(names) == 140 == _lib.DK_NPARAMS and len(set(names)) == 140
    assert names[0] == "v0_filter_cutoff" and names[16 * 7 + 15] == "v7_portamento"
    assert names[_lib.DK_RACK0:] == ["rack_" + f for f in ofx.PARAMS[ofx.KIND_FXRACK]]
    r = workload.RANGES["drumkit"]
    assert len(r) == 140 and all(r[16 * p:16 * p + 16] == workload.RANGES["voice"] for p in range(8))
    assert r[128:139] == workload.RANGES["fxrack"][:11] and r[139] == "int2"
    p = workload.instance_params("drumkit", 0, 200, 5)
    assert p.shape == (140, 200) and set(np.unique(p[139])) == {0.0, 1.0}
    assert not np.array_equal(p[0:16], p[16:32])                 # every pad has its own draw
    assert np.array_equal(workload.instance_params("drumkit", 50, 20, 5), p[:, 50:70])
    with pytest.raises(ofx.OlfxError):
        ofx.control_map("drumkit", 41, 64)                       # OLFX_E_KIND: the mapping needs a channel


def test_header_declares_the_new_symbols():
    src = open(os.path.join(ROOT, "include", "olfx.h")).read()
    for name in ("olfx_create_drumkit", "olfx_drumkit_map"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and hasattr(ofx.load(), name)
    assert "OLFX_KIND_DRUMKIT = 14" in src and "13 stays unassigned" in src
    assert ctypes.sizeof(_lib.DrumkitVoice) == 12
    for macro, value in (("OLFX_DK_NO_NOTE", "0xFFu"), ("OLFX_DK_NO_CHANNEL", "0xFFu"), ("OLFX_DK_CHANNEL_RACK", "16"),
                         ("OLFX_DK_NO_VOICE", "0xFFFFFFFFu")):
        assert re.search(r"#define\s+" + macro + r"\s+" + value, src), macro


def test_create_reaches_the_device_probe():
    """Kind 14 is known: olfx_create and olfx_create_drumkit get as far as the device (OLFX_E_NODEVICE without
    one), never OLFX_E_KIND; 0 and 9 voices are refused before the probe; olfx_create_synth_kind keeps refusing
    the kind."""
    lib = ofx.load()
    h = ctypes.c_void_p()
    for voices in (0, 9):
        assert lib.olfx_create_drumkit(0, 4, voices, 48000.0, 256, ctypes.byref(h)) == _lib.OLFX_E_ARG
        assert not h.value and b"voices" in lib.olfx_last_error(None)
    assert lib.olfx_create_drumkit(0, 0, 4, 48000.0, 256, ctypes.byref(h)) == _lib.OLFX_E_ARG
    assert lib.olfx_create_drumkit(0, 4, 4, 48000.0, 256, None) == _lib.OLFX_E_ARG
    assert lib.olfx_create_synth_kind(ofx.KIND_DRUMKIT, 0, 4, 4, 48000.0, 256, ctypes.byref(h)) == _lib.OLFX_E_KIND
    assert lib.olfx_drumkit_map(None, None, 0) == _lib.OLFX_E_ARG
    creates = [(lambda: lib.olfx_create(ofx.KIND_DRUMKIT, 0, 4, 48000.0, 256, ctypes.byref(h)), 4),
               (lambda: lib.olfx_create_drumkit(0, 4, 8, 48000.0, 256, ctypes.byref(h)), 8),
               (lambda: lib.olfx_create_drumkit(0, 4, 1, 48000.0, 256, ctypes.byref(h)), 1)]
    for create, voices in creates:
        rc = create()
        if rc == _lib.OLFX_OK:
            assert HAS_GPU and h.value
            assert lib.olfx_kernel_name(h) == b"drumkit_block_v1" and lib.olfx_synth_voices(h) == voices
            assert lib.olfx_algorithmic_bytes_per_frame(h) == 24 + 4 * voices
            assert lib.olfx_algorithmic_read_bytes_per_frame(h) == 8 + 4 * voices
            off = (ctypes.c_uint32 * 2)(0, 1)
            order = (ctypes.c_uint32 * 1)(0)
            assert lib.olfx_mix_config(h, 1, off, order) == _lib.OLFX_E_STATE
            assert lib.olfx_mix(h, None, None, 4, 0, None) == _lib.OLFX_E_STATE
            assert lib.olfx_sample_bank(h, 0, None, None) == _lib.OLFX_OK
            rec = (_lib.DrumkitVoice * 1)()
            rec[0].kit, rec[0].voice, rec[0].channel, rec[0].note = 0, voices, 0, 60
            assert lib.olfx_drumkit_map(h, rec, 1) == _lib.OLFX_E_ARG
            assert lib.olfx_destroy(h) == _lib.OLFX_OK
        else:
            assert rc == _lib.OLFX_E_NODEVICE, (rc, lib.olfx_last_error(None))
            assert not h.value
            assert b"no HIP device" in lib.olfx_last_error(None)
