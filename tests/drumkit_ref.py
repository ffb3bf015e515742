"""The reference for OLFX_KIND_DRUMKIT: the existing CPU references composed, no new arithmetic.

Per block, for n kits of P voices ([2][frames][n] float32 out):
  1. v = sampler_ref.SamplerVoices(P * n, kernel_arith=True): voice p * n + i is voice slot p of kit i
     (sampler_block_v1's arithmetic with the committed v_rcp_f32 model), each with its own config and Sample;
  2. mono = O.mix_ref(v, [[voices of kit i that sit at a note, by ascending note]]): VoiceMap::Process
     (VoiceMap.h:64-73), `*frame_out += sample` voice by voice from 0.0f; unmapped voices still tick;
  3. out = O.FxRack(n) on (mono, 0) with instance i at kit i's topology (1 the firmware callback, 0
     FxRack<2>::Process with its master volume).
VoiceMap's tables and routing are restated here to drive the voices: SetVoice (note2voice[note] = voice;
channel2voice[channel] = voice), NoteOn / NoteOff to the voice at the note (none: ignored), a control on
channel c to the voice at channel2voice[c] through the voice kind's control map, on channel 16 to the rack
through the rack kind's map at the kit's topology.

A test is a script, run here (run_ref) and by tests/test_gpu_drumkit.py on the engine:
  ("params", p[140][n]) | ("set", kit, field, value) | ("bank", [arrays]) |
  ("samples", [(kit, slot, sample or None, mode, loop_start, loop_end), ...]) |
  ("map", [(kit, channel, note, voice or None), ...]) | ("events", [(kit, type, note), ...]) |
  ("control", [(kit, cc, value, source, channel), ...]) | ("block", frames) | ("check_playing",) | ("reset",)

condition() is what every script's reference must meet before anything is compared with it: finite
everywhere; channel 0 non-zero for every kit that has a mapped, assigned, triggered voice; channel 1 of those
kits non-zero over the frames at topology 1 and all +-0 (every kit) over the frames at topology 0; every kit
whose note order differs from its slot order has a frame where the note-order sum and the slot-order sum differ
in bits (else a kernel that summed in slot order would pass).
"""
from __future__ import annotations

import numpy as np

import oracle as O
import sampler_ref as SM
import synth_ref as SR
from ol_dsp_amd import _lib, workload
from ol_dsp_amd.engine import control_map

NV = len(O.VC_FIELDS)               # 16 fields per voice slot
SLOTS = 8
RACK0 = SLOTS * NV                  # 128
NR = len(O.FR_FIELDS)
NPARAMS = RACK0 + NR                # 140
TOPOLOGY = RACK0 + O.FR_FIELDS.index("topology")
MASTER = RACK0 + O.FR_FIELDS.index("master_volume")
RACK_TIME = RACK0 + O.FR_FIELDS.index("delay_time")
CH_RACK = 16
EV_NOTE_OFF, EV_NOTE_ON, EV_GATE_ON, EV_GATE_OFF, EV_SET_FREQUENCY = 0, 1, 2, 3, 4
install_rcp, remove_rcp, bits_equal = SR.install_rcp, SR.remove_rcp, SR.bits_equal


def defaults() -> np.ndarray:
    """[140]: SynthVoice's member defaults in every slot, the rack's, topology 1."""
    d = np.concatenate([np.tile(np.asarray(O.VOICE_DEFAULTS, np.float32), SLOTS), O.fxrack_defaults()])
    d[TOPOLOGY] = 1.0
    return d


class DrumKit:
    def __init__(self, n: int, voices: int = 4, sample_rate: float = 48000.0):
        self.n, self.P, self.sr = n, voices, sample_rate
        self.voice = SM.SamplerVoices(voices * n, sample_rate, kernel_arith=True)
        self.note2voice = -np.ones((n, 128), np.int64)
        self.chan2voice = -np.ones((n, 16), np.int64)
        self.sample = -np.ones((n, voices), np.int64)          # each voice's bank index, -1: unassigned
        self._fresh()

    def _fresh(self):
        n = self.n
        self.rack = O.FxRack(n, self.sr)
        self.p = np.tile(defaults()[:, None], (1, n)).astype(np.float32)
        for i in range(n):
            self.rack.set(i, "topology", 1.0)
        self.playing = np.zeros((n, self.P), np.int64)
        self.sounding = np.zeros(n, bool)             # a mapped, assigned voice got a NoteOn
        self.log = []                                 # per block: (frames, topology[n], orders, note sum, slot sum)
        self.trace = []

    def reset(self) -> None:
        """olfx_reset: state and parameters afresh; the map, the bank and the assignments stay."""
        self.voice.reset()
        log, trace = self.log, self.trace
        self._fresh()
        self.log, self.trace = log, trace

    # ---- parameters ----
    def set(self, kit: int, field: int, value: float) -> None:
        f = int(field)
        self.p[f, kit] = np.float32(value)
        if f < RACK0:
            slot = f // NV
            if slot < self.P:                         # Update() of that voice alone
                self.voice.config(slot * self.n + kit, self.p[slot * NV:(slot + 1) * NV, kit])
        else:
            assert f != TOPOLOGY or float(value) in (0.0, 1.0)
            self.rack.set(kit, f - RACK0, float(self.p[f, kit]))

    def set_params(self, p: np.ndarray) -> None:
        assert p.shape == (NPARAMS, self.n)
        self.p[:] = p
        for i in range(self.n):
            for slot in range(self.P):
                self.voice.config(slot * self.n + i, p[slot * NV:(slot + 1) * NV, i])
            for f in range(NR):
                self.rack.set(i, f, float(p[RACK0 + f, i]))

    # ---- samples ----
    def sample_bank(self, samples) -> None:
        self.voice.sample_bank(samples)
        self.sample[self.sample >= len(samples)] = -1        # an assignment the new bank lacks drops

    def sample_voices(self, recs) -> None:
        for kit, slot, sample, *rest in recs:
            self.voice.sample_voices([(slot * self.n + kit, sample, *rest)])
            self.sample[kit, slot] = -1 if sample is None else int(sample)

    # ---- VoiceMap (VoiceMap.h:27-82) ----
    def map(self, recs) -> None:
        n2v, c2v = self.note2voice.copy(), self.chan2voice.copy()
        for kit, channel, note, voice in recs:
            v = -1 if voice is None else int(voice)
            assert 0 <= kit < self.n and -1 <= v < self.P
            if note is not None:
                n2v[kit, note] = v
            if channel is not None:
                c2v[kit, channel] = v
        for kit in {r[0] for r in recs}:
            held = n2v[kit][n2v[kit] >= 0]
            if len(set(held.tolist())) != len(held):
                raise ValueError(f"a voice of kit {kit} would sit at two notes")
        self.note2voice, self.chan2voice = n2v, c2v

    def order(self, kit: int):
        return [int(v) for v in self.note2voice[kit] if v >= 0]

    def event(self, kit: int, type_: int, note: int) -> None:
        assert type_ in (EV_NOTE_ON, EV_NOTE_OFF)
        v = int(self.note2voice[kit, note])
        if v < 0:
            return
        self.voice.event(v * self.n + kit, type_, note)
        self.playing[kit, v] = note if type_ == EV_NOTE_ON else 0
        if type_ == EV_NOTE_ON and self.sample[kit, v] >= 0:
            self.sounding[kit] = True

    def control(self, kit: int, cc: int, value: float, source: str = "midi", channel: int = 0) -> None:
        if channel < 16:
            v = int(self.chan2voice[kit, channel])
            hit = control_map("voice_sample", cc, value, source) if v >= 0 else None
            if hit is None:
                return
            if hit[0] == "update_only":
                self.voice.config(v * self.n + kit, self.p[v * NV:(v + 1) * NV, kit])
            else:
                self.set(kit, v * NV + O.VC_FIELDS.index(hit[0]), hit[1])
        elif channel == CH_RACK:
            as_cc, takes = cc, True
            if self.p[TOPOLOGY, kit] == 1.0:          # the firmware's direct routing (olfx.h OLFX_FR_TOPOLOGY)
                takes = 41 <= cc <= 44 or 35 <= cc <= 39 or cc == 34
                as_cc = cc + 4 if 41 <= cc <= 44 else cc
            hit = control_map("fxrack", as_cc, value, source) if takes else None
            if hit is not None:
                self.set(kit, RACK0 + O.FR_FIELDS.index(hit[0]), hit[1])

    def process(self, frames: int, threads: int = 4) -> np.ndarray:
        n = self.n
        v = self.voice.process(frames)
        orders = [self.order(i) for i in range(n)]
        x = np.zeros((2, frames, n), np.float32)
        x[0] = O.mix_ref(v, [[p * n + i for p in o] for i, o in enumerate(orders)])
        by_slot = O.mix_ref(v, [[p * n + i for p in sorted(o)] for i, o in enumerate(orders)])
        self.log.append((frames, self.p[TOPOLOGY].copy(), orders, x[0].copy(), by_slot))
        self.last_voices = v
        return self.rack.process(x, threads)


def run_ref(script, n: int, voices: int = 4, threads: int = 4, sample_rate: float = 48000.0):
    """The composed reference of a script: ([2][frames][n], the DrumKit)."""
    ref = DrumKit(n, voices, sample_rate)
    out = []
    for step in script:
        op = step[0]
        if op == "params":
            ref.set_params(step[1])
        elif op == "set":
            ref.set(step[1], step[2], step[3])
        elif op == "bank":
            ref.sample_bank(step[1])
        elif op == "samples":
            ref.sample_voices(step[1])
        elif op == "map":
            ref.map(step[1])
        elif op == "events":
            for kit, type_, note in step[1]:
                ref.event(kit, type_, note)
        elif op == "control":
            for ev in step[1]:
                ref.control(*ev)
        elif op == "block":
            out.append(ref.process(step[1], threads))
        elif op == "check_playing":
            ref.trace.append(ref.playing.copy())
        elif op == "reset":
            ref.reset()
        else:
            raise ValueError(op)
    return np.concatenate(out, 1), ref


def condition(yr: np.ndarray, ref: DrumKit, sounding=None) -> None:
    """yr [2][frames][n] against the reference's own log (see the module docstring)."""
    topo = np.concatenate([np.tile(t[None, :], (f, 1)) for f, t, _, _, _ in ref.log], 0)
    assert topo.shape == yr.shape[1:]
    assert np.isfinite(yr).all(), np.argwhere(~np.isfinite(yr))[:4]
    sounding = ref.sounding if sounding is None else sounding
    silent = np.flatnonzero(sounding & ~np.any(yr[0] != 0, axis=0))
    assert silent.size == 0, ("channel 0 silent", silent[:8])
    at1, at0 = topo == 1.0, topo == 0.0
    assert np.all(at1 | at0)
    silent = np.flatnonzero(sounding & np.any(at1, axis=0) & ~np.any((yr[1] != 0) & at1, axis=0))
    assert silent.size == 0, ("channel 1 silent at topology 1", silent[:8])
    loud = np.argwhere((yr[1] != 0) & at0)
    assert loud.size == 0, ("channel 1 non-zero at topology 0", loud[:4])
    # the sum order is observable wherever it is not the slot order
    reordered = np.zeros(ref.n, bool)
    differs = np.zeros(ref.n, bool)
    for _, _, orders, by_note, by_slot in ref.log:
        for i, o in enumerate(orders):
            if o != sorted(o):
                reordered[i] = True
                differs[i] |= bool(np.any(by_note[:, i].view(np.uint32) != by_slot[:, i].view(np.uint32)))
    same = np.flatnonzero(reordered & ~differs)
    assert same.size == 0, ("note order indistinguishable from slot order", same[:8])


# ---------------------------------------------------------------------------------------------
# The GPU tests' scripts
# ---------------------------------------------------------------------------------------------
LENGTHS = [1, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1000]       # tests/test_gpu_sampler.py's bank


def loop_modes(L):
    """tests/test_gpu_sampler.py loop_modes: OneShot and the eight configurations of
    tests/golden/sample_reference_runs.json, scaled to an L-frame sample."""
    return [(0, 0, 0), (1, 0, 0), (1, 0, max(L - 1, 0)), (1, L // 5, 3 * L // 5), (1, 2 * L // 5, L + 2),
            (1, L + 4, 0), (1, 3 * L // 5, L // 5), (1, 2 * L // 5, 2 * L // 5), (0, 3, 2)]


def params(n: int, seed: int) -> np.ndarray:
    return workload.instance_params("drumkit", 0, n, seed)


def full_map(n: int, P: int):
    """Voice p of kit i at note 36 + (7 p + 3 i) % 29 (no two voices of a kit share a note: 7 p mod 29 is
    injective for p < 8) and on channel p: most kits' note order is not their slot order."""
    return [(i, p, 36 + (7 * p + 3 * i) % 29, p) for i in range(n) for p in range(P)]


def note_of(kit: int, p: int) -> int:
    return 36 + (7 * p + 3 * kit) % 29


def snote(kit: int, p: int) -> int:
    """The plain map's note of voice p: ascending with p, so a kit's note order is its slot order."""
    return 36 + 8 * p + kit % 8


def slot_map(n: int, P: int):
    """Voice p of kit i at snote(i, p) and on channel p.  The scripts that give some voices no sample or a
    one-frame sample use this map: sums with zeros in them do not tell one order from another, and condition()
    asks every reordered kit to show its order (script_sum_order and script_map_changes do that)."""
    return [(i, p, snote(i, p), p) for i in range(n) for p in range(P)]


def notes_on(n: int, P: int, slots=None, note=snote):
    return [(i, EV_NOTE_ON, note(i, p)) for i in range(n) for p in (range(P) if slots is None else slots)]


def assignments(n: int, P: int):
    """Round-robin over LENGTHS and "unassigned" with loop_modes cycling at another period, as
    tests/test_gpu_sampler.py assignments(); loops of 1, 2, 7, 8, 9, 15, 16 and 17 frames (around the 16-frame
    chunk) forced onto voices of the first and last kits, starting at odd cursors of the 1000-frame sample."""
    recs = []
    for i in range(n):
        for p in range(P):
            s = p * (n + 1) + i                       # (a kit's voices get different samples)
            k = s % (len(LENGTHS) + 1)
            if k == len(LENGTHS):
                recs.append((i, p, None, 0, 0, 0))
                continue
            mode, ls, le = loop_modes(LENGTHS[k])[(s // 2) % 9]
            recs.append((i, p, k, mode, ls, le))
    at = {(r[0], r[1]): j for j, r in enumerate(recs)}
    for j, (kit, p, m) in enumerate(forced_loops(n, P)):
        a = 101 + 62 * j                              # odd: no loop starts on a multiple of the fetch width
        recs[at[(kit, p)]] = (kit, p, 11, 1, a, a + m - 1)
    return recs


FORCED = [16, 1, 17, 15, 2, 7, 8, 9]      # loop lengths; the most telling first (an engine of few voices takes a prefix)


def forced_loops(n: int, P: int):
    """[(kit, slot, frames)]: each length of FORCED on a voice of its own, no voice twice.  The voices are taken
    from the edge kits inward, alternating between the two ends -- (0, 0), (n - 1, 0), (0, 1), (n - 1, 1), ...,
    then kits 1 and n - 2 -- so at P >= 4 the first and the last kit hold four lengths each, at P = 2 the first
    and last two kits two each, at P = 1 the first and last four kits one each; an engine of fewer than eight
    voices gets the first n P lengths."""
    voices = []
    for k in range((n + 1) // 2):
        for p in range(P):
            for kit in (k, n - 1 - k):
                if (kit, p) not in voices:
                    voices.append((kit, p))
    voices = voices[:len(FORCED)]
    out = [(kit, p, m) for (kit, p), m in zip(voices, FORCED)]
    assert len(out) == min(len(FORCED), n * P) and len({(k, p) for k, p, _ in out}) == len(out)
    # every length sits on one of the outermost kits that 8 voices need
    edge = -(-len(FORCED) // (2 * P))
    assert all(k < edge or k >= n - edge for k, _, _ in out)
    return out


def script_basic(n: int, P: int, blocks=(256, 256), seed: int = 5):
    bank = workload.sample_bank(LENGTHS, seed=11)
    return [("params", params(n, seed)), ("bank", bank), ("samples", assignments(n, P)), ("map", slot_map(n, P)),
            ("events", notes_on(n, P))] + [("block", b) for b in blocks]


def script_ragged_frames(n: int = 65, P: int = 4):
    """Blocks of 4, 20, 36, 256 and 12 frames: ends and loop turns inside a chunk, at a chunk edge and at a block
    edge; retriggers and releases between them."""
    s = script_basic(n, P, blocks=())
    for b, frames in enumerate([4, 20, 36, 256, 12]):
        if b == 2:
            s.append(("events", [(i, EV_NOTE_OFF, snote(i, 1 % P)) for i in range(0, n, 2)]))
        if b == 3:
            s.append(("events", notes_on(n, P, slots=[0]) + [(i, EV_NOTE_ON, 127) for i in range(n)]))   # 127: nobody
        if b == 4:
            s.append(("events", [(i, EV_NOTE_OFF, snote(i, 0)) for i in range(1, n, 4)]))
        s.append(("block", frames))
    return s


def script_sum_order(n: int = 70, P: int = 5):
    """The checked script: every voice sounds, 67 of the 70 kits sum in an order that is not their slot order."""
    bank = workload.sample_bank([1000, 300, 77, 5000], seed=11)
    p = params(n, 5)
    pv = workload.instance_params("voice_sample", 0, n * P, 3)
    for q in range(P):
        p[q * NV:(q + 1) * NV] = pv[:, q * n:(q + 1) * n]
    p[RACK0:] = workload.instance_params("synth_svf", 0, n, 5)[NV:]
    recs = [(i, q, (q * n + i) % 4, ((q * n + i) // 4) % 2, 10, 60) for i in range(n) for q in range(P)]
    return [("params", p), ("bank", bank), ("samples", recs), ("map", full_map(n, P)),
            ("events", notes_on(n, P, note=note_of)), ("block", 256), ("block", 100), ("block", 256), ("block", 256)]


def script_map_changes(n: int = 33, P: int = 4):
    """Over script_sum_order's set-up.  Between blocks: two voices swap their notes in one call, a voice is unmapped (it goes on ticking,
    unheard), a voice is displaced by another, a channel is repointed and a control follows it; kit 5 starts
    with an empty map and is mapped later; kit 6 stays empty."""
    s = script_sum_order(n, P)[:5]
    empty = [(i, None, note, None) for i in (5, 6) for note in range(128)] + [(i, c, None, None) for i in (5, 6) for c in range(16)]
    s.insert(4, ("map", empty))
    s += [("block", 256)]
    # (voices 0 and 2, not 0 and 1: float addition commutes, so [1, 0, 2, 3] sums to [0, 1, 2, 3]'s bits)
    swap = [(i, None, note_of(i, 0), 2) for i in range(0, n, 3) if i not in (5, 6)]
    swap += [(i, None, note_of(i, 2), 0) for i in range(0, n, 3) if i not in (5, 6)]
    s += [("map", swap), ("events", notes_on(n, P, slots=[0, 2], note=note_of)), ("block", 100)]
    s += [("map", [(i, None, note_of(i, 2 % P), None) for i in range(1, n, 3) if i not in (5, 6)]),
          ("events", notes_on(n, P, slots=[2 % P], note=note_of)), ("block", 256)]           # those NoteOns reach nobody now
    s += [("map", [(i, 3 % P, note_of(i, 3 % P), 0) for i in range(2, n, 3) if i not in (5, 6)] +
                  [(i, None, note_of(i, 0), None) for i in range(2, n, 3) if i not in (5, 6)] +
                  [(5, p, note_of(5, p), p) for p in range(P)]),
          ("events", notes_on(n, P, note=note_of)),
          ("control", [(i, 41, 90.0, "midi", 3 % P) for i in range(2, n, 3)]), ("block", 256)]
    return s


def script_topology_mix(n: int = 70, P: int = 4):
    """Even kits at topology 0, odd ones at 1 (both in every lane pair of D); masters none of them 1; switches
    between the blocks."""
    s = script_basic(n, P, blocks=())
    p = s[0][1]
    p[TOPOLOGY] = np.arange(n) % 2
    p[MASTER] = np.float32(0.25) + np.float32(1.35) * (np.arange(n) % 7).astype(np.float32) / np.float32(6)
    p[MASTER, p[MASTER] == 1.0] = 1.125
    s += [("block", 256)]
    s += [("set", i, TOPOLOGY, 1.0) for i in (0, 32, 64, 68)] + [("set", i, TOPOLOGY, 0.0) for i in (1, 33, 63, 69)]
    s += [("events", notes_on(n, P)), ("block", 100), ("set", 0, TOPOLOGY, 0.0), ("set", 69, TOPOLOGY, 1.0),
          ("events", notes_on(n, P)), ("block", 256)]
    return s


def script_params_and_controls(n: int = 33, P: int = 5):
    """Per-voice parameters: one field of one slot changes between blocks (that voice alone is Update()d);
    controls on a voice's channel (MIDI and hardware), on the rack channel, on an empty channel (9) and on an
    ignored one (40)."""
    q = params(n, 6)
    s = script_basic(n, P, blocks=(256,))
    s += [("set", i, slot * NV + f, float(q[slot * NV + f, i])) for i in range(0, n, 2) for slot in (0, P - 1) for f in (0, 1, 9)]
    s += [("set", i, RACK0 + f, float(q[RACK0 + f, i])) for i in range(1, n, 2) for f in (0, 1, 5, 6)]
    s += [("events", notes_on(n, P)), ("block", 256)]
    s += [("control", [(i, 41, 80.0, "midi", 1 % P) for i in range(n)] + [(i, 7, 0.6, "hw", 0) for i in range(0, n, 2)] +
           [(i, 41, 60.0, "midi", CH_RACK) for i in range(n)] + [(i, 45, 70.0, "midi", CH_RACK) for i in range(n)] +
           [(i, 41, 10.0, "midi", 9) for i in range(n)] + [(i, 41, 10.0, "midi", 40) for i in range(n)]),
          ("events", notes_on(n, P)), ("block", 256)]
    return s


def script_storm(n: int = 33, P: int = 4, total: int = 2000, seed: int = 5):
    """Per block, random NOTE_ON / NOTE_OFF per kit at mapped and unmapped notes; Engine.playing is checked
    after every block's events."""
    rng = np.random.default_rng(seed)
    s = script_basic(n, P, blocks=()) + [("check_playing",)]
    done = 0
    while done < total:
        evs = []
        for i in np.flatnonzero(rng.random(n) < 0.6):
            t = int(rng.choice([EV_NOTE_ON, EV_NOTE_ON, EV_NOTE_OFF]))
            note = note_of(int(i), int(rng.integers(0, P))) if rng.random() < 0.8 else int(rng.integers(0, 128))
            evs.append((int(i), t, note))
        frames = int(rng.choice([256, 256, 256, 100, 20]))
        s += [("events", evs), ("check_playing",), ("block", frames)]
        done += frames
    return s


def script_reset_and_bank(n: int = 33, P: int = 4):
    """A run, olfx_reset (map, bank and assignments stay; parameters and state do not), the same run again;
    then a smaller bank over it (assignments whose sample is gone drop, every Sample fresh) and a retrigger."""
    run = script_basic(n, P, blocks=(256, 100))
    small = workload.sample_bank(LENGTHS[:6], seed=13)
    again = [run[0], run[4]] + run[5:]
    return run + [("reset",)] + again + [("bank", small), ("block", 100), ("events", notes_on(n, P)), ("block", 256)]


def script_long_oneshot(n: int = 3, P: int = 2):
    """A 70,000-frame one-shot played through and past its end: the cursor crosses 65,536."""
    bank = workload.sample_bank([70000, 100, 50], seed=12)
    recs = [(0, 0, 0, 0, 0, 0), (0, 1, 2, 1, 5, 40), (1, 0, 1, 0, 0, 0), (1, 1, 0, 0, 0, 0), (2, 0, None, 0, 0, 0),
            (2, 1, 0, 1, 69990, 0)]
    return ([("params", params(n, 9)), ("bank", bank), ("samples", recs), ("map", slot_map(n, P)),
             ("events", notes_on(n, P))] + [("block", 2048)] * 34 + [("block", 632)])     # 70,264 frames


GPU_SCRIPTS = {
    **{f"ragged_instances_{n}": (lambda n=n: (script_basic(n, 4), n, 4)) for n in (1, 33, 65, 130)},
    **{f"voices_{P}": (lambda P=P: (script_basic(65, P, seed=6), 65, P)) for P in (1, 2, 5, 8)},
    "ragged_frames": lambda: (script_ragged_frames(), 65, 4),
    "sum_order": lambda: (script_sum_order(), 70, 5),
    "map_changes": lambda: (script_map_changes(), 33, 4),
    "topology_mix": lambda: (script_topology_mix(), 70, 4),
    "params_and_controls": lambda: (script_params_and_controls(), 33, 5),
    "storm": lambda: (script_storm(), 33, 4),
    "reset_and_bank": lambda: (script_reset_and_bank(), 33, 4),
    "long_oneshot": lambda: (script_long_oneshot(), 3, 2),
}
