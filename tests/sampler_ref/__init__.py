"""CPU reference for the sample-playback voice (OLFX_KIND_VOICE_SAMPLE): ctypes access to
tests/sampler_ref/sampler_ref.c, built on first use with the oracle's flags.  TEST INFRASTRUCTURE.

`SamplerVoices` mirrors the engine's surface (sample_bank, sample_voices, config, events, reset,
process) and exposes the bare Sample stream (`source`, `pause` / `play` / `seek`) for the pins of
tests/golden/sample_reference_runs.json.  The v_rcp_f32 model of its kernel arithmetic is
liboracle's oracle_rcp_model: whatever table oracle.set_rcp_table() installed (the `rcp_table`
fixture) is the one used here."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sampler_ref.c")
LIB = os.path.join(HERE, "libsampler_ref.so")
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-fPIC", "-Wall"]

_PF = ctypes.POINTER(ctypes.c_float)
_PU64 = ctypes.POINTER(ctypes.c_uint64)
_U64 = ctypes.c_uint64
_lib = None

NO_SAMPLE = None
ONESHOT, LOOP = 0, 1


def build() -> None:
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.run([os.environ.get("CC", "gcc"), *CFLAGS, "-shared", "-o", tmp, SRC, "-lm"], check=True)
    os.replace(tmp, LIB)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
            build()
        L = ctypes.CDLL(LIB)
        L.sref_create.restype = ctypes.c_void_p
        L.sref_create.argtypes = [ctypes.c_int, ctypes.c_float]
        L.sref_destroy.argtypes = [ctypes.c_void_p]
        L.sref_set_rcp.argtypes = [ctypes.c_void_p]
        L.sref_bank.argtypes = [ctypes.c_void_p, ctypes.c_int, _PU64, _PF]
        L.sref_assign.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _U64, _U64]
        L.sref_config.argtypes = [ctypes.c_void_p, ctypes.c_int, _PF]
        L.sref_event.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float]
        L.sref_sample_ctl.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _U64]
        L.sref_source.argtypes = [ctypes.c_void_p, ctypes.c_int, _PF, ctypes.c_int]
        L.sref_reset.argtypes = [ctypes.c_void_p]
        L.sref_process.argtypes = [ctypes.c_void_p, _PF, ctypes.c_int, ctypes.c_int]
        # v_rcp_f32: liboracle's model (the committed table once the rcp_table fixture installed it)
        L.sref_set_rcp(ctypes.cast(O.lib().oracle_rcp_model, ctypes.c_void_p))
        _lib = L
    return _lib


class SamplerVoices:
    """n SynthVoice(SampleSoundSource<1>, SvfFilter) over one bank.  kernel_arith: the kernels'
    arithmetic (oracle/voice_ref.c voice_tick_k) instead of the unfused restatement."""

    def __init__(self, n: int, sample_rate: float = 48000.0, kernel_arith: bool = False):
        self.n = n
        self.kernel = int(bool(kernel_arith))
        self.L = lib()
        self.h = self.L.sref_create(n, sample_rate)
        assert self.h

    def close(self):
        if getattr(self, "h", None):
            self.L.sref_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sample_bank(self, samples) -> None:
        arrs = [np.ascontiguousarray(np.asarray(a, dtype=np.float32).ravel()) for a in samples]
        off = np.zeros(len(arrs) + 1, np.uint64)
        if arrs:
            off[1:] = np.cumsum([len(a) for a in arrs])
        pcm = np.ascontiguousarray(np.concatenate(arrs) if arrs and off[-1] else np.zeros(1, np.float32))
        assert self.L.sref_bank(self.h, len(arrs), off.ctypes.data_as(_PU64), pcm.ctypes.data_as(_PF)) == 0

    def sample_voices(self, records) -> None:
        """(inst, sample or None[, play_mode[, loop_start[, loop_end]]]), as Engine.sample_voices."""
        for r in records:
            mode = r[2] if len(r) > 2 else 0
            assert self.L.sref_assign(self.h, int(r[0]), -1 if r[1] is None else int(r[1]), int(mode),
                                      int(r[3]) if len(r) > 3 else 0, int(r[4]) if len(r) > 4 else 0) == 0

    def config(self, inst: int, values) -> None:
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float32))
        assert v.shape == (16,)
        assert self.L.sref_config(self.h, inst, v.ctypes.data_as(_PF)) == 0

    def event(self, inst: int, type_: int, note: int = 0, value: float = 0.0) -> None:
        """OLFX_EV_*: 0 NoteOff, 1 NoteOn, 2 GateOn, 3 GateOff, 4 SetFrequency(value)."""
        assert self.L.sref_event(self.h, int(inst), int(type_), int(note), float(value)) == 0

    def events(self, evs) -> None:
        for e in evs:
            self.event(e[0], e[1], e[2] if len(e) > 2 else 0, e[3] if len(e) > 3 else 0.0)

    def reset(self) -> None:
        assert self.L.sref_reset(self.h) == 0

    def process(self, frames: int) -> np.ndarray:
        out = np.empty((1, frames, self.n), np.float32)
        assert self.L.sref_process(self.h, out.ctypes.data_as(_PF), frames, self.kernel) == 0
        return out

    # ---- the Sample alone ----
    def pause(self, inst: int) -> None:
        assert self.L.sref_sample_ctl(self.h, inst, 0, 0) == 0

    def play(self, inst: int) -> None:
        assert self.L.sref_sample_ctl(self.h, inst, 1, 0) == 0

    def seek(self, inst: int, frame: int) -> None:
        assert self.L.sref_sample_ctl(self.h, inst, 2, int(frame)) == 0

    def source(self, inst: int, frames: int) -> np.ndarray:
        out = np.empty(frames, np.float32)
        assert self.L.sref_source(self.h, inst, out.ctypes.data_as(_PF), frames) == 0
        return out
