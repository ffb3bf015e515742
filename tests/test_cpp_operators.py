"""The C++ operator surface (include/olfx_fx.hpp) driven from C++ as a reference caller would:
ReverbBank / ChorusBank / PitchShiftBank / VoiceBank against the CPU oracle
(tests/cpp/test_operators.cpp, gtest-style, in the manner of the reference's test/synth_test.cpp).
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
BIN = os.path.join(CPP, "test_operators")
ADAPTER_BIN = os.path.join(CPP, "test_adapter")


def _build():
    r = subprocess.run(["make", "-s", "-C", CPP], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return BIN


def test_cpp_operator_test_builds_and_fails_loudly_without_gpu():
    """Builds against the plain C ABI (g++ only, no HIP headers). Off-GPU every operator must
    throw OLFX_E_NODEVICE: there is no silent CPU path behind the surface."""
    _build()
    if os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK):
        pytest.skip("GPU visible: covered by the -m gpu run")
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert "no HIP device" in r.stdout and "(code -4)" in r.stdout


def test_cpp_block_adapter_host_logic():
    """include/olfx_adapter.hpp over CPU oracle banks: per-frame, ragged and
    interleaved callers get the bank's output delayed by exactly one block, bit for bit; queued
    CCs / notes land at the next block boundary in queue order; Queue() from a second thread."""
    _build()
    r = subprocess.run([ADAPTER_BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "4 tests, 0 failures" in r.stdout


def test_cpp_host_core():
    """The engine's HIP-free host core (ol_dsp_amd/csrc/olfx_host.cpp) linked into a stand-alone
    program: note-event folding, the event section's fixed slots and overflow list, packet
    layout, the setters' coefficient words, rejected calls and the rack's CC routing."""
    _build()
    r = subprocess.run([os.path.join(CPP, "test_host_core")], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "7 tests, 0 failures" in r.stdout


@pytest.mark.gpu
def test_cpp_operators_on_gpu():
    _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "17 tests, 0 failures" in r.stdout


ORACLE = os.path.join(os.path.dirname(HERE), "oracle")
REF_BIN = os.path.join(ORACLE, "_ref", "test_ref_surface")
REF_HDR = "/root/reference/modules/synthlib/Polyvoice.h"


def _build_ref():
    """oracle/Makefile `ref_surface`: include/olfx_ref.hpp under the reference's own, unmodified
    Polyvoice.h / VoiceMap.h / Voice.h / corelib, built into oracle/_ref where the reference is
    present; elsewhere the prebuilt binary is run."""
    if os.path.exists(REF_HDR):
        r = subprocess.run(["make", "-s", "-C", ORACLE, "ref_surface"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    if not os.path.exists(REF_BIN):
        pytest.skip("test_ref_surface not built (needs /root/reference at build time)")
    return REF_BIN


def test_ref_surface_compiles_against_reference_headers_and_fails_loudly_without_gpu():
    """The reference's Polyvoice / VoiceMap compile unmodified over ol::synth::SynthVoice and
    ol::fx::FxRack<2>; off-GPU the first Process throws OLFX_E_NODEVICE (no CPU path)."""
    _build_ref()
    if os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK):
        pytest.skip("GPU visible: covered by the -m gpu run")
    r = subprocess.run([REF_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert "no HIP device" in r.stdout and "(code -4)" in r.stdout


@pytest.mark.gpu
def test_ref_surface_on_gpu():
    """Reference-typed classes on the GPU: Polyvoice / VoiceMap sums, Voice gate / pitch calls,
    FxRack<2>(DelayFx&, ReverbFx&, FilterFx&) controls, ChorusFx<1|2>, vs the oracle one block late; the
    Daisy firmware's audio callback verbatim over standalone DelayFx<1> / ReverbFx<2> / FilterFx<2>."""
    _build_ref()
    r = subprocess.run([REF_BIN], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "6 tests, 0 failures" in r.stdout


def test_ref_header_standalone_without_gpu():
    """include/olfx_ref.hpp alone (its restated Voice / SoundSource): the reference's constructors
    compile, the filter component picks the kernel, a foreign SoundSource is refused with
    OLFX_E_KIND, and without a GPU the first Process throws OLFX_E_NODEVICE."""
    _build()
    if os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK):
        pytest.skip("GPU visible: the GPU suites cover the run path")
    r = subprocess.run([os.path.join(CPP, "test_ref_standalone")], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no HIP device" in r.stdout and "0 problems" in r.stdout
