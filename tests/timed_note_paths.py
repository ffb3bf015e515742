"""olfx_timed_notes beyond tests/timed_note_cases.py's 64-frame calls: the paths of the *_seg instrument kernels
and of the host around them that those cases never reach, as data.  No torch, no GPU.

  score()          a seeded score over calls of 64, 4, 12, 100, 300, 256, 20 and 8 frames: partial last chunks with
                   a segment start in them, launches that start off the 16-frame chunk grid, many pieces per V wave
                   in calls of more than four chunks, notes carried over one and two calls; score_facts() counts
                   what it is meant to contain, recut() queues the same absolute times up front for other calls
  case_capacity()  exactly kVevCap = 4 records in a voice-slot group (they fit the fixed slots), 5 (the first
                   overflow run), and both in the ragged last group
  case_kit_bank()  the kit's pads retriggered at 4, 8 and 12 frames into a chunk against the sampler suite's bank:
                   samples of 1 to 1000 frames, the nine loop modes, loops of 1 to 17 frames
  case_corners()   the three edge suites' corner parameters with their notes timed: envelopes restarted in mid-chunk
  case_ring()      272 event times in one call: 17 launches, one more than the engine has small packet slots
  case_coefs()     a set and a control between calls with notes pending: coefficient records and a multi-segment
                   event table in one packet
  case_scale()     a sparse, a dense and a sparse time at n = 8230 and 32838

The scripts are timed_note_cases' (resolve(), launches(), setup(), note_of(), notes_on()); one more step,
("control", [(inst, cc, value, source[, channel])]), is olfx_control: drumkit_ref takes it as it is, and
lower_controls() restates it for the synth references as the ("set", ...) steps the host's own fan-out table
names.  tests/test_timed_notes_ref.py holds every case's reference to its condition and facts on the CPU;
tests/test_gpu_timed_note_paths.py runs the cases on the engine."""
from __future__ import annotations

import numpy as np

import drumkit_edge_cases as DKE
import drumkit_ref as DK
import synth_ref as SR
import synth_svf_edge_cases as SVE
import synth_svf_ref as SV
import timed_note_cases as C
from edge_fused_cases import RAGGED_1024, synth_corner_condition, synth_corner_script
from ol_dsp_amd import workload
from ol_dsp_amd.engine import synth_control_map

KINDS = C.KINDS
NOTE_OFF, NOTE_ON, GATE_ON, GATE_OFF = C.NOTE_OFF, C.NOTE_ON, C.GATE_ON, C.GATE_OFF
CHUNK = 16                        # synth_pipeline.h kChunk: the frames a V wave publishes at a time
VEV_CAP = 4                       # olfx_layout.h kVevCap: a voice-slot group's fixed record slots per segment
KSLOTS = 16                       # olfx_engine::kSlots: the zero-copy packet slots
SCORE_FRAMES = [64, 4, 12, 100, 300, 256, 20, 8]
SCORE_TAIL = 64                   # one event-free call after them
SCORE_TOTAL = sum(SCORE_FRAMES) + SCORE_TAIL
SCORE_SHAPES = [(130, 4), (65, 5), (65, 8)]
SCORE_SEED = 5
RECUTS = [[SCORE_TOTAL], [36, 300, 492]]
P_TIME, P_DENSE, P_SPARSE, P_KNOWN = 0.3, 0.3, 0.04, 0.85
assert SCORE_TOTAL == 828 and all(sum(r) == SCORE_TOTAL for r in RECUTS)


# --------------------------------------------------------------------------------------------- references
def lower_controls(kind, script):
    """The script with every ("control", ...) step of a synth kind as the ("set", ...) steps of the host's fan-out
    (ol_dsp_amd.synth_control_map at the instrument's topology at that point of the script).  A kit's stay."""
    if kind == "drumkit":
        return list(script)
    topo, out = None, []
    for step in script:
        if step[0] == "params":
            topo = np.asarray(step[1][SR.TOPOLOGY]).copy()
        elif step[0] == "set" and step[2] == SR.TOPOLOGY:
            topo[step[1]] = step[3]
        if step[0] != "control":
            out.append(step)
            continue
        for inst, cc, value, source in step[1]:
            hits = synth_control_map(cc, value, source, kind=kind, topology=int(topo[inst]))
            assert hits and all(f != "update_only" for f, _ in hits)
            out += [("set", inst, SR.FIELDS.index(f), float(v)) for f, v in hits]
    return out


def run_reference(kind, script, n, voices, threads=4, sample_rate=48000.0):
    """timed_note_cases.run_reference with controls and at any sample rate."""
    mod = {"synth": SR, "synth_svf": SV, "drumkit": DK}[kind]
    return mod.run_ref(C.resolve(lower_controls(kind, script)), n, voices, threads=threads, sample_rate=sample_rate)


def bank_setup(n, voices, seed=5):
    """The kit against the sampler suite's bank: topologies 0 and 1 alternating, drumkit_ref's assignments (every
    sample length with the nine loop modes cycling, some voices with no sample, the FORCED loops on the edge
    kits) and the slot-order map."""
    p = DK.params(n, seed)
    p[DK.TOPOLOGY] = np.arange(n) % 2
    return [("params", p), ("bank", workload.sample_bank(DK.LENGTHS, seed=11)), ("samples", DK.assignments(n, voices)),
            ("map", DK.slot_map(n, voices))]


def steps_of(script, op):
    return [s for s in script if s[0] == op]


def schedule(script):
    """Per ("block", L) step of a timed script: (L, {frame: [(inst, type, note, calls carried)]}) of the notes that
    land inside it, frame 0's included (a note that landed as the previous call returned counts as frame 0 here:
    it is in that launch's first segment)."""
    pending, out = [], []
    for step in script:
        if step[0] == "timed":
            pending += [[ev[0], tuple(ev[1:]), 0] for ev in step[1]]
        elif step[0] == "block":
            L, at = step[1], {}
            for f, ev, carried in pending:
                if f < L:
                    at.setdefault(f, []).append(ev + (carried,))
            out.append((L, dict(sorted(at.items()))))
            pending = [[f - L, ev, carried + 1] for f, ev, carried in pending if f >= L]
    assert not pending
    return out


# ------------------------------------------------------------------------------------------------ the score
def score(kind, n, voices, seed=SCORE_SEED):
    """Calls of SCORE_FRAMES, then an event-free one.  Before each call but the 8-frame one, notes at a random set
    of quads from 0 to 12 frames past the call's end (what lies past it carries over), L - 4 always among them in
    a call of 16 frames or more; a time is dense (a note for every instrument) with probability 0.3, else sparse
    (about 4 % of them, one at least).  NoteOn and NoteOff, the synths' GateOn and GateOff too; most notes are
    note_of's, the others random: they reach nobody, or no free voice.  Fixed: every quad from 8 to 76 of the
    300-frame call and none before them, so its first launch ends ahead of frame 68; a note at frame 4 of the 12-frame
    call; one queued before the 4-frame call for frame 8 of the 100-frame call (two calls ahead); the 8-frame call
    queues nothing and takes frame 4's notes from the 20-frame call's queue.  Playing() follows every call."""
    rng = np.random.default_rng([seed, KINDS.index(kind), n, voices])
    note = C.note_of(kind, n, voices)
    types = [NOTE_ON, NOTE_ON, NOTE_OFF, NOTE_OFF] + ([] if kind == "drumkit" else [GATE_ON, GATE_OFF])

    def notes_at(frame, dense):
        who = range(n) if dense else (np.flatnonzero(rng.random(n) < P_SPARSE).tolist() or [int(rng.integers(0, n))])
        out = []
        for i in who:
            nt = note(int(i), int(rng.integers(0, voices))) if rng.random() < P_KNOWN else int(rng.integers(0, 128))
            out.append((frame, int(i), int(rng.choice(types)), nt))
        return out

    s = (bank_setup(n, voices) if kind == "drumkit" else C.setup(kind, n, voices)) + [("events", C.notes_on(kind, n, voices))]
    left = sum(SCORE_FRAMES)
    for L in SCORE_FRAMES:
        quads = {f for f in range(0, L + 16, 4) if rng.random() < P_TIME}
        if L >= 16:
            quads.add(L - 4)
        if L == 12:
            quads.add(4)
        if L == 4:
            quads.add(4 + 12 + 8)
        if L == 20:
            quads.add(20 + 4)
        if L == 8:
            quads = set()
        if L == 100:
            quads.discard(100 + 4)                              # (frame 4 of the 300-frame call)
        if L == 300:                                            # 0, 8, 12, ..., 76: the second launch starts at frame 68
            quads = (quads - set(range(0, 80, 4))) | set(range(8, 80, 4))
        timed = []
        for f in sorted(q for q in quads if q < left):          # nothing lands in the event-free call
            timed += notes_at(f, rng.random() < P_DENSE)
        s += [("timed", timed), ("block", L), ("check_playing",)]
        left -= L
    return s + [("block", SCORE_TAIL), ("check_playing",)]


def score_facts(script, n):
    """Counts of what a score is meant to contain (tests/test_timed_notes_ref.py asserts each is at least 1)."""
    facts = dict(unaligned_launch_after_a_full_one=0, start_in_a_partial_last_chunk=0, start_on_the_last_quad=0,
                 frame_4_of_the_8_frame_call=0, frame_4_of_the_12_frame_call=0, queued_two_calls_ahead=0,
                 calls_of_carried_notes_only=0, dense_past_chunk_4_of_256=0, sparse_past_chunk_4_of_256=0,
                 dense_past_chunk_4_of_300=0, sparse_past_chunk_4_of_300=0)
    for L, at in schedule(script):
        times = sorted({0} | set(at))
        for k in range(C.SEG_CAP, len(times), C.SEG_CAP):       # the launch before it had SEG_CAP segments
            facts["unaligned_launch_after_a_full_one"] += times[k] % CHUNK != 0
        past = [f for f in at if f > 0]
        facts["start_in_a_partial_last_chunk"] += sum(1 for f in past if L % CHUNK and f >= L - L % CHUNK)
        facts["start_on_the_last_quad"] += L - 4 in past
        if L in (8, 12):
            facts[f"frame_4_of_the_{L}_frame_call"] += 4 in at
        notes = [ev for evs in at.values() for ev in evs]
        facts["queued_two_calls_ahead"] += sum(1 for ev in notes if ev[3] >= 2)
        facts["calls_of_carried_notes_only"] += bool(notes) and all(ev[3] >= 1 for ev in notes)
        if L in (256, 300):
            for f, evs in at.items():
                if f >= 4 * CHUNK:
                    who = {ev[0] for ev in evs}
                    facts[f"dense_past_chunk_4_of_{L}"] += len(who) == n
                    facts[f"sparse_past_chunk_4_of_{L}"] += len(who) <= n // 8
    return {k: int(v) for k, v in facts.items()}


def recut(script, lengths):
    """The score's notes at their absolute times, queued up front in their order of arrival, and calls of other
    lengths: the same frames, Playing() read once at the end."""
    assert sum(lengths) == sum(s[1] for s in steps_of(script, "block"))
    head, timed, t0 = [], [], 0
    for step in script:
        if step[0] == "timed":
            timed += [(t0 + ev[0],) + tuple(ev[1:]) for ev in step[1]]
        elif step[0] == "block":
            t0 += step[1]
        elif step[0] != "check_playing":
            assert t0 == 0
            head.append(step)
    return head + [("timed", timed)] + [("block", m) for m in lengths] + [("check_playing",)]


# ------------------------------------------------------------------------------------- fixed-slot capacity
CAPACITY_N, CAPACITY_P = 70, 4
# frame: [(voice slot, the instruments whose note of that slot is released; it is retaken one quad later)]
CAPACITY_OFFS = {4: [(0, [0, 1, 31, 62])], 8: [(1, [2, 3, 32, 33, 61])], 12: [(0, [64, 65, 68, 69])],
                 20: [(0, [64, 66, 67, 68, 69])], 36: [(0, list(range(63)) + list(range(64, 70)))]}
# the records of voice-slot group (slot, instrument group) in the segment that starts at each frame
CAPACITY_COUNTS = {4: {(0, 0): 4}, 8: {(0, 0): 4, (1, 0): 5}, 12: {(1, 0): 5, (0, 1): 4}, 16: {(0, 1): 4},
                   20: {(0, 1): 5}, 24: {(0, 1): 5}, 36: {(0, 0): 63, (0, 1): 6}, 40: {(0, 0): 63, (0, 1): 6}}


def case_capacity(kind):
    """n = 70, P = 4: the last group holds 6 instruments.  After notes_on voice slot p of instrument i holds
    note(i, p), so its NoteOff -- and the NoteOn that retakes the note one quad later, which finds that voice free
    (a synth: the only free one; a kit: the one that sits at the note) -- is a record of group (p, i / 64).  Frame 4:
    4 records in group (0, 0), which fit the fixed slots.  Frame 8: 5 in group (1, 0), the first overflow run, beside
    the 4 that retake frame 4's notes in (0, 0).  Frames 12 and 16: 4 in the last group, instrument 69 among them.
    Frames 20 and 24: 5 there.  Frames 36 and 40: all 6 of the last group and 63 of group 0."""
    n, P = CAPACITY_N, CAPACITY_P
    note = C.note_of(kind, n, P)
    timed = []
    for f, groups in CAPACITY_OFFS.items():
        for p, who in groups:
            timed += [(f, i, NOTE_OFF, note(i, p)) for i in who] + [(f + 4, i, NOTE_ON, note(i, p)) for i in who]
    return C.setup(kind, n, P) + [("events", C.notes_on(kind, n, P)), ("check_playing",), ("timed", timed),
                                  ("block", C.NF), ("check_playing",), ("block", C.NF)]


def capacity_counts(kind, script):
    """{frame: {(voice slot, instrument group): records}} of the script, each note taken to the voice slot that
    notes_on gave it."""
    n, P = CAPACITY_N, CAPACITY_P
    note = C.note_of(kind, n, P)
    slot_of = {(i, note(i, p)): p for i in range(n) for p in range(P)}
    assert len(slot_of) == n * P
    out = {}
    for f, i, _, nt in steps_of(script, "timed")[0][1]:
        key = (slot_of[(i, nt)], i // 64)
        out.setdefault(f, {})
        out[f][key] = out[f].get(key, 0) + 1
    return out


# ------------------------------------------------------------------------- the kit against the sampler bank
KIT_BANK_SHAPES = [(65, 4), (33, 8)]
KIT_BANK_FIRST = 64
KIT_BANK_FRAMES = [4, 8, 12, 16 + 20, 16 + 40, 16 + 60]          # counted from the 16-frame call's first frame


def case_kit_bank(n, voices):
    """bank_setup(), every pad played; one 64-frame call later every pad is retriggered at frames 4, 8 and 12 of a
    16-frame call and at 20, 40 and 60 of the 64-frame call after it -- pieces of 4, 8 and 12 frames, in which the
    lanes whose sample ends or loops read one frame at a time beside lanes that read a plain run; then event-free
    calls of 20 and 256 frames."""
    timed = [(f, i, NOTE_ON, DK.snote(i, p)) for f in KIT_BANK_FRAMES for i in range(n) for p in range(voices)]
    return bank_setup(n, voices) + [("events", C.notes_on("drumkit", n, voices)), ("block", KIT_BANK_FIRST), ("timed", timed),
                                    ("block", 16), ("check_playing",), ("block", 64), ("check_playing",), ("block", 20),
                                    ("block", 256)]


def kit_bank_coverage(script, n, voices):
    """What the case is meant to contain, from its own steps: the (sample length, loop configuration) pairs and the
    FORCED loop lengths that get a timed NoteOn at a frame off the chunk grid, and those that assignments() makes;
    whether some one-shot has run out by its first retrigger and some voice is inside its loop by then."""
    recs = steps_of(script, "samples")[0][1]
    voice_at = {(kit, note): v for kit, _, note, v in steps_of(script, "map")[0][1]}
    t0, hit = 0, set()
    for step in script:
        if step[0] == "block":
            t0 += step[1]
        elif step[0] == "timed":
            first = min(ev[0] for ev in step[1]) + t0
            hit |= {(i, voice_at[(i, nt)]) for f, i, ty, nt in step[1] if ty == NOTE_ON and (t0 + f) % CHUNK}
    pair = lambda r: (DK.LENGTHS[r[2]], tuple(r[3:6]))
    made = {pair(r) for r in recs if r[2] is not None}
    got = {pair(r) for r in recs if r[2] is not None and (r[0], r[1]) in hit}
    by_voice = {(r[0], r[1]): r for r in recs}
    forced = {m for kit, p, m in DK.forced_loops(n, voices) if (kit, p) in hit
              and by_voice[(kit, p)][5] - by_voice[(kit, p)][4] + 1 == m}
    # a voice plays one frame per frame from its NoteOn at frame 0: its cursor at the first retrigger is `first`
    ended = any(r[2] is not None and r[3] == 0 and DK.LENGTHS[r[2]] <= first for r in recs)
    looping = any(r[2] is not None and r[3] == 1 and r[4] < r[5] < DK.LENGTHS[r[2]] and r[4] <= first for r in recs)
    return made, got, forced, ended, looping


# ------------------------------------------------------------------------------------------------- corners
CORNER_N, CORNER_P = 70, 8


def case_corners(kind):
    """The edge suites' corner scripts at (70, 8) with their two boundary event steps timed, over one pass of
    RAGGED_1024 = 256, 4, 100, 300, 364: each instrument's first P / 2 NoteOns at frame 4 and the others at frame 12
    of the first call; the NoteOffs queued before the 4-frame call, the even instruments' for frame 8 of its
    successor and the odd ones' for that call's last quad, 100 - 4."""
    n, P = CORNER_N, CORNER_P
    base = {"synth": synth_corner_script, "synth_svf": SVE.corner_script, "drumkit": DKE.corner_script}[kind](n, P)
    at = next(k for k, s in enumerate(base) if s[0] == "events")
    ons, offs = steps_of(base, "events")
    assert len(ons[1]) == n * P and len(offs[1]) == n and RAGGED_1024[:3] == [256, 4, 100]
    seen, on = {}, []
    for i, ty, nt in ons[1]:
        k = seen[i] = seen.get(i, -1) + 1
        on.append((4 if k < P // 2 else 12, i, ty, nt))
    off = [(4 + 8 if i % 2 == 0 else 4 + 100 - 4, i, ty, nt) for i, ty, nt in offs[1]]
    s = base[:at] + [("timed", on), ("block", 256), ("check_playing",), ("timed", off), ("block", 4), ("block", 100),
                     ("check_playing",), ("block", 300), ("block", 364)]
    assert [b[1] for b in steps_of(s, "block")] == RAGGED_1024
    return s


def corner_condition(kind, script, yr):
    n, P = CORNER_N, CORNER_P
    if kind == "synth":
        synth_corner_condition(n, P, yr)
    elif kind == "synth_svf":
        SVE.corner_condition(n, P, yr, script[0][1][SV.TOPOLOGY])
    else:
        DKE.corner_condition(n, P, yr, script[0][1][DK.TOPOLOGY])


# -------------------------------------------------------------------------------------------- engine paths
RING_FRAMES, RING_TIMES = 1088, 272


def case_ring(kind, n, voices):
    """272 event times in one call of 1088 frames -- every quad, frame 0 included -- which is 17 launches of 16
    segments, one more than the engine has small packet slots.  At 4 k the instruments of few(n) get voice 0's note,
    released for odd k and played for even k.  Then an event-free call."""
    note = C.note_of(kind, n, voices)
    timed = [(4 * k, i, NOTE_OFF if k % 2 else NOTE_ON, note(i, 0)) for k in range(RING_TIMES) for i in C.few(n)]
    s = C.setup(kind, n, voices) + [("events", C.notes_on(kind, n, voices)), ("timed", timed), ("block", RING_FRAMES),
                                    ("check_playing",), ("block", C.NF)]
    assert C.launches(s) == [[C.SEG_CAP] * (KSLOTS + 1), [1]]
    return s


def case_coefs(kind, n, voices):
    """Four calls of 64 frames, every note queued before the first: two times in each call, a note for every
    instrument at each.  Between calls 2 and 3, with the notes of calls 3 and 4 pending: a set of one voice field
    and one rack field on every other instrument, and a control on the others -- the synths' CC 41 (the voices'
    filter and, by the firmware's route, the rack's), the kit's CC 41 on pad 1's channel and on the rack's."""
    note, NF = C.note_of(kind, n, voices), C.NF
    timed = []
    for c in range(4):
        timed += [(c * NF + 12, i, NOTE_OFF, note(i, c % voices)) for i in range(n)]
        timed += [(c * NF + 40, i, NOTE_ON, note(i, c % voices)) for i in range(n)]
    if kind == "drumkit":
        q = DK.params(n, 6)
        sets = [("set", i, f, float(q[f, i])) for i in range(0, n, 2) for f in (0, DK.RACK0 + 5)]
        control = [(i, 41, 80.0, "midi", 1 % voices) for i in range(1, n, 2)] + [(i, 41, 60.0, "midi", DK.CH_RACK) for i in range(1, n, 2)]
    else:
        q = (SR if kind == "synth" else SV).params(n, 6)
        sets = [("set", i, f, float(q[f, i])) for i in range(0, n, 2) for f in (0, SR.NV + 5)]
        control = [(i, 41, 90.0, "midi") for i in range(1, n, 2)]
    s = C.setup(kind, n, voices) + [("events", C.notes_on(kind, n, voices)), ("timed", timed), ("block", NF), ("block", NF),
                                    ("check_playing",)] + sets + [("control", control), ("block", NF), ("check_playing",),
                                                                  ("block", NF), ("check_playing",), ("block", NF)]
    assert C.launches(s) == [[3]] * 4 + [[1]]
    return s


SCALE_SHAPES = [(8230, 8), (32838, 4)]


def case_scale(kind, n, voices):
    """One 64-frame call: a sparse time at 4 (every 25th instrument releases voice 0's note), a dense one at 12
    (every instrument releases its last voice's), a sparse one at 60 (every 25th retakes voice 0's note; the last
    instrument too).  A dense segment's records are past the 64 KiB from which a packet is copied."""
    note = C.note_of(kind, n, voices)
    some = sorted(set(range(0, n, 25)) | {n - 1})
    timed = [(4, i, NOTE_OFF, note(i, 0)) for i in some] + [(12, i, NOTE_OFF, note(i, voices - 1)) for i in range(n)]
    timed += [(60, i, NOTE_ON, note(i, 0)) for i in some]
    assert 8 * n >= 65536
    return C.setup(kind, n, voices) + [("events", C.notes_on(kind, n, voices)), ("timed", timed), ("block", C.NF), ("block", C.NF)]


def sampled(n, count=64):
    """About `count` instruments, the first and the last among them."""
    return sorted(set(range(0, n, max(1, n // (count - 1)))) | {n - 1})
