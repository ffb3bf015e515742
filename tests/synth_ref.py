"""The reference for OLFX_KIND_SYNTH: a composition of the existing CPU oracles, no new arithmetic.

Per block, for n instruments of P voices ([2][frames][n] float32 out):
  1. v = O.Voice(P * n, moog=True, kernel_arith=True): voice p * n + i is voice p of instrument i
     (the voice kernels' arithmetic with the committed v_rcp_f32 model, oracle/voice_ref.c);
  2. mono = O.mix_ref(v, [[0 * n + i, 1 * n + i, ...]]): Polyvoice::Process, `*frame_out += sample`
     voice by voice from 0.0f (Polyvoice.h:28-33);
  3. out = O.FxRack(n) at topology 1 (the firmware callback, main.cpp:78-86) on (mono, 0).
The Polyvoice allocation rule (Polyvoice.h:35-77) is restated here to drive the oracle voices, as
tests/test_gpu_parity.py test_polyvoice_allocation_vs_oracle does: NoteOn goes to the first voice
with Playing() == 0, NoteOff to the first with Playing() == note, gates to every voice,
SetFrequency nowhere.

The v_rcp_f32 table: GPU tests take the `rcp_table` fixture (which installs it); CPU tests call
install_rcp() / remove_rcp() around their runs.

A test is a script, run here against the oracles (run_ref) and by tests/test_gpu_synth.py against
the engine; tests/test_synth_ref.py runs every GPU script's reference on the CPU and holds it to the
condition the GPU tests state (finite everywhere, both channels non-zero for every instrument).
"""
from __future__ import annotations

import numpy as np

import oracle as O
from ol_dsp_amd import workload

NV = len(O.VC_FIELDS)               # 16 voice fields, then the rack's 12
NR = len(O.FR_FIELDS)
FIELDS = list(O.VC_FIELDS) + ["rack_" + f for f in O.FR_FIELDS]
TOPOLOGY = NV + O.FR_FIELDS.index("topology")
EV_NOTE_OFF, EV_NOTE_ON, EV_GATE_ON, EV_GATE_OFF, EV_SET_FREQUENCY = 0, 1, 2, 3, 4


def install_rcp() -> None:
    import rcp_model
    O.set_rcp_table(rcp_model.load())


def remove_rcp() -> None:
    O.set_rcp_table(None)


def defaults() -> np.ndarray:
    """[28]: SynthVoice's member defaults, the rack's, topology 1."""
    d = np.concatenate([np.asarray(O.VOICE_DEFAULTS, np.float32), O.fxrack_defaults()])
    d[TOPOLOGY] = 1.0
    return d


class Synth:
    def __init__(self, n: int, voices: int = 4, sample_rate: float = 48000.0):
        self.n, self.P = n, voices
        self.voice = O.Voice(voices * n, sample_rate, moog=True, kernel_arith=True)
        self.rack = O.FxRack(n, sample_rate)
        self.p = np.tile(defaults()[:, None], (1, n)).astype(np.float32)
        for i in range(n):
            self.rack.set(i, "topology", 1.0)
        self.buses = [[p * n + i for p in range(voices)] for i in range(n)]
        self.playing = np.zeros((n, voices), np.int64)          # Playing() of voice p of instrument i

    # ---- parameters ----
    def set(self, inst: int, field, value: float) -> None:
        """One field; a voice field is UpdateConfig + Update of every voice of the instrument."""
        f = FIELDS.index(field) if isinstance(field, str) else int(field)
        self.p[f, inst] = np.float32(value)
        if f < NV:
            self.update(inst)
        else:
            assert f != TOPOLOGY or float(value) == 1.0
            self.rack.set(inst, f - NV, float(self.p[f, inst]))

    def update(self, inst: int) -> None:
        for p in range(self.P):
            self.voice.config(p * self.n + inst, self.p[:NV, inst])

    def set_params(self, p: np.ndarray) -> None:
        """p [28][n]."""
        assert p.shape == (NV + NR, self.n)
        self.p[:] = p
        for i in range(self.n):
            self.update(i)
            for f in range(NR):
                self.rack.set(i, f, float(p[NV + f, i]))

    def init_members(self, inst: int, values) -> None:
        """The voice members written before Init, no Update (the firmware's set-up order)."""
        self.p[:NV, inst] = np.asarray(values, np.float32)
        for p in range(self.P):
            self.voice.init_members(p * self.n + inst, self.p[:NV, inst])

    # ---- Polyvoice (Polyvoice.h:35-77) ----
    def event(self, inst: int, type_: int, note: int = 0) -> None:
        n, pl = self.n, self.playing[inst]
        if type_ == EV_NOTE_ON:
            for p in range(self.P):
                if not pl[p]:
                    self.voice.event(p * n + inst, EV_NOTE_ON, note)
                    pl[p] = note
                    return
        elif type_ == EV_NOTE_OFF:
            for p in range(self.P):
                if pl[p] == note:
                    self.voice.event(p * n + inst, EV_NOTE_OFF, note)
                    pl[p] = 0
                    return
        elif type_ in (EV_GATE_ON, EV_GATE_OFF):
            for p in range(self.P):
                self.voice.event(p * n + inst, type_, note)
        # SetFrequency: a nop

    def process(self, frames: int, threads: int = 4) -> np.ndarray:
        v = self.voice.process(frames, threads)
        x = np.zeros((2, frames, self.n), np.float32)
        x[0] = O.mix_ref(v, self.buses)
        return self.rack.process(x, threads)


# ---- scripts: what a test does, in order ----
# ("params", p[28][n]) | ("set", inst, field, value) | ("events", [(inst, type, note), ...]) |
# ("block", frames) | ("check_playing",)  (GPU side only: Engine.playing against the rule's table)
def run_ref(script, n: int, voices: int = 4, threads: int = 4, sample_rate: float = 48000.0):
    """The composed reference of a script: ([2][frames][n], the Synth)."""
    ref = Synth(n, voices, sample_rate)
    ref.trace = []
    out = []
    for step in script:
        if step[0] == "params":
            ref.set_params(step[1])
        elif step[0] == "set":
            ref.set(step[1], step[2], step[3])
        elif step[0] == "events":
            for inst, type_, note in step[1]:
                ref.event(inst, type_, note)
        elif step[0] == "block":
            out.append(ref.process(step[1], threads))
        elif step[0] == "check_playing":
            ref.trace.append(ref.playing.copy())         # [n][voices] at this point of the script
    return np.concatenate(out, 1), ref


def condition(yr: np.ndarray) -> None:
    """What every GPU test asserts of its reference: finite for every instrument, both channels
    non-zero for every instrument."""
    assert np.isfinite(yr).all(), np.argwhere(~np.isfinite(yr))[:4]
    for c in (0, 1):
        silent = np.flatnonzero(~np.any(yr[c] != 0, axis=0))
        assert silent.size == 0, (c, silent[:8])


def bits_equal(y: np.ndarray, yr: np.ndarray) -> bool:
    """tests/test_gpu_parity.py voice_bits_equal: bit-exact where the reference is finite, the same
    non-finite pattern elsewhere."""
    fin = np.isfinite(yr)
    if y.shape != yr.shape or not np.array_equal(fin, np.isfinite(y)):
        return False
    return np.array_equal(y[fin].view(np.uint32), yr[fin].view(np.uint32))


def notes_on(n: int, voices: int):
    """Every voice of every instrument gets a NoteOn: voice p of instrument i plays
    workload.voice_notes of (voices * i + p)."""
    notes = workload.voice_notes(0, n * voices)
    return [(i, EV_NOTE_ON, int(notes[voices * i + p])) for i in range(n) for p in range(voices)]


LINE_DELAYS = [0, 1, 15, 16, 17, 24000, 47999]        # tests/test_gpu_platerack.py
RACK_TIME = NV + O.FR_FIELDS.index("delay_time")


def delay_time(d: int) -> np.float32:
    t = np.float32((d + 0.5) / 48000.0)
    assert int(t * np.float32(48000.0)) == d
    return t


def params(n: int, seed: int) -> np.ndarray:
    return workload.instance_params("synth", 0, n, seed)


# ---- the GPU tests' scripts (tests/test_gpu_synth.py runs them on the engine) ----
def script_ragged_instances(n: int):
    return [("params", params(n, 5)), ("events", notes_on(n, 4))] + [("block", 256)] * 3


def script_voices(P: int, n: int = 65):
    return [("params", params(n, 6)), ("events", notes_on(n, P))] + [("block", 256)] * 3


def script_ragged_frames(n: int = 65):
    s = [("params", params(n, 5)), ("events", notes_on(n, 4))]
    for b, frames in enumerate([4, 20, 36, 256, 12]):
        if b == 2:
            s.append(("events", [(i, EV_NOTE_OFF, int(workload.voice_notes(0, n * 4)[4 * i + 1])) for i in range(0, n, 2)]))
        if b == 3:
            s.append(("events", [(i, EV_NOTE_ON, 40 + i % 50) for i in range(0, n, 3)]))
        if b == 4:
            s.append(("events", [(i, EV_GATE_OFF, 0) for i in range(1, n, 4)]))
        s.append(("block", frames))
    return s


def script_delay_lines(n: int = 65):
    p = params(n, 6)
    for k, d in enumerate(LINE_DELAYS):
        p[RACK_TIME, k % n] = delay_time(d)
        p[RACK_TIME, (n - 1 - k) % n] = delay_time(LINE_DELAYS[-1 - k])
    return [("params", p), ("events", notes_on(n, 4))] + [("block", 256)] * 3


def script_storm(n: int = 33, total: int = 6000, seed: int = 5):
    """Per block, random NOTE_ON / NOTE_OFF / GATE_* per instrument; block 1 sends a fifth note into
    full instruments, block 2 plays note 0 (NoteOn(0), then NoteOff(0))."""
    rng = np.random.default_rng(seed)
    s = [("params", params(n, seed)), ("events", notes_on(n, 4)), ("check_playing",)]
    done, b = 0, 0
    while done < total:
        evs = []
        if b == 1:
            evs += [(i, EV_NOTE_ON, 100) for i in range(n)]                # all four voices play: dropped
        elif b == 2:
            evs += [(i, EV_NOTE_OFF, int(workload.voice_notes(0, n * 4)[4 * i + 2])) for i in range(n)]
            evs += [(i, EV_NOTE_ON, 0) for i in range(0, n, 2)]            # gates voice 2, which stays free
            evs += [(i, EV_NOTE_OFF, 0) for i in range(0, n, 4)]           # hits the first free voice
        elif b > 2:
            for i in np.flatnonzero(rng.random(n) < 0.5):
                t = int(rng.choice([EV_NOTE_ON, EV_NOTE_ON, EV_NOTE_OFF, EV_GATE_ON, EV_GATE_OFF]))
                evs.append((int(i), t, int(rng.integers(36, 97))))
            for i in np.flatnonzero(rng.random(n) < 0.3):                   # a NoteOff that finds its note
                evs.append((int(i), -1, 0))
        s.append(("events", evs))
        s.append(("check_playing",))
        frames = int(rng.choice([256, 256, 256, 100, 20]))
        s.append(("block", frames))
        done += frames
        b += 1
    return s


def resolve_storm(script, n: int, voices: int = 4):
    """Replace the storm's (inst, -1, 0) placeholders by a NoteOff of a note the instrument plays
    (by the rule's own table), so that releases happen; returns the script with plain events."""
    pl = np.zeros((n, voices), np.int64)
    out = []
    for step in script:
        if step[0] != "events":
            out.append(step)
            continue
        evs = []
        for inst, t, note in step[1]:
            if t == -1:
                held = pl[inst][pl[inst] != 0]
                if held.size == 0:
                    continue
                t, note = EV_NOTE_OFF, int(held[-1])
            evs.append((inst, t, note))
            if t == EV_NOTE_ON:
                free = np.flatnonzero(pl[inst] == 0)
                if free.size:
                    pl[inst][free[0]] = note
            elif t == EV_NOTE_OFF:
                hit = np.flatnonzero(pl[inst] == note)
                if hit.size:
                    pl[inst][hit[0]] = 0
        out.append(("events", evs))
    return out


def script_param_change(n: int = 33):
    p, q = params(n, 5), params(n, 6)
    s = [("params", p), ("events", notes_on(n, 4)), ("block", 256)]
    s += [("set", i, f, float(q[f, i])) for i in range(0, n, 2) for f in (0, 1, 9, NV + 0, NV + 1, NV + 5, NV + 6)]
    s += [("block", 256), ("block", 256)]
    return s


GPU_SCRIPTS = {
    **{f"ragged_instances_{n}": (lambda n=n: (script_ragged_instances(n), n, 4)) for n in (1, 33, 65, 130)},
    **{f"voices_{P}": (lambda P=P: (script_voices(P), 65, P)) for P in (1, 2, 5, 8)},
    "ragged_frames": lambda: (script_ragged_frames(), 65, 4),
    "delay_lines": lambda: (script_delay_lines(), 65, 4),
    "storm": lambda: (resolve_storm(script_storm(), 33), 33, 4),
    "param_change": lambda: (script_param_change(), 33, 4),
}
