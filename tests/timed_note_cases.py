"""olfx_timed_notes (timed notes for OLFX_KIND_SYNTH, OLFX_KIND_SYNTH_SVF and OLFX_KIND_DRUMKIT): the cases as
data, and the driver that resolves a timed script into the plain scripts of the existing references
(tests/synth_ref.py, tests/synth_svf_ref.py, tests/drumkit_ref.py).  No torch, no GPU.

A timed script is a reference script (its steps as those modules define them) with one more step,
  ("timed", [(frame, inst, type, note), ...])        olfx_timed_notes
resolve() turns it into ("events", ...) / ("block", frames) steps, one block per distinct event frame -- the
split calls that include/olfx.h states as the contract.  It restates the routing rule without the engine's code:
a note is handed to the reference (whose Polyvoice / VoiceMap restatement routes it there and then) when the
frames reach it, in order of (frame, queueing order); a note at frame 0 at the call; a note at or past the call's
end stays pending with its frame reduced by the call's length, and one that lands on frame 0 is handed over as
the call returns, ahead of whatever the script queues next.

tests/test_timed_notes_ref.py holds every case's reference to the condition the GPU tests state (finite
everywhere; both channels non-zero for every instrument, channel 0 alone at topology 0; the expected Playing()
tables); tests/test_gpu_timed_notes.py runs the cases on the engine."""
from __future__ import annotations

import numpy as np

import drumkit_ref as DK
import synth_ref as SR
import synth_svf_ref as SV
from ol_dsp_amd import workload

KINDS = ["synth", "synth_svf", "drumkit"]
NOTE_OFF, NOTE_ON, GATE_ON, GATE_OFF = 0, 1, 2, 3
SEG_CAP = 16                      # olfx_layout.h kSegCap
NF = 64                           # a call, unless a case says otherwise
# mid-chunk, on the 16-frame chunk's edge, two in one chunk (16 and 20; 36 with the chunk's start at 32), the last quad
FRAMES = [4, 12, 16, 20, 36, 60]
KIT_LENGTHS = [20, 1000]          # a one-shot shorter than a call, and the sample the loops run in


# --------------------------------------------------------------------------------------------- the driver
def resolve(script):
    """The timed script as a plain reference script (see the module docstring)."""
    pending, arrival, out = [], 0, []

    def hand_over(notes):
        if notes:
            out.append(("events", [tuple(ev) for ev in notes]))

    for step in script:
        if step[0] == "timed":
            now = []
            for frame, inst, type_, note in step[1]:
                assert frame % 4 == 0 and 0 <= frame < 1 << 31
                if frame == 0:
                    now.append((inst, type_, note))
                else:
                    pending.append([frame, arrival, (inst, type_, note)])
                arrival += 1
            hand_over(now)
            pending.sort(key=lambda w: (w[0], w[1]))
        elif step[0] == "block":
            n_frames, at = step[1], 0
            while at < n_frames:
                hand_over([w[2] for w in pending if w[0] == at])
                pending = [w for w in pending if w[0] != at]
                until = min([w[0] for w in pending if w[0] < n_frames] + [n_frames])
                out.append(("block", until - at))
                at = until
            for w in pending:
                w[0] -= n_frames
            hand_over([w[2] for w in pending if w[0] == 0])      # as the call returns
            pending = [w for w in pending if w[0] != 0]
        else:
            out.append(step)
    return out


def launches(script):
    """Per ("block", ...) step of a timed script: the segments of each of its launches -- segment 0 starts at frame
    0, notes or none, and a launch ends ahead of the time that would be its segment SEG_CAP + 1."""
    pending, out = [], []
    for step in script:
        if step[0] == "timed":
            pending += [ev[0] for ev in step[1] if ev[0] > 0]
        elif step[0] == "block":
            times = sorted({0} | {f for f in pending if f < step[1]})
            out.append([len(times[k:k + SEG_CAP]) for k in range(0, len(times), SEG_CAP)])
            pending = [f - step[1] for f in pending if f >= step[1]]
            pending = [f for f in pending if f > 0]
    return out


def run_reference(kind, script, n, voices, threads=4):
    """([2][frames][n], the reference object) of a timed script."""
    mod = {"synth": SR, "synth_svf": SV, "drumkit": DK}[kind]
    return mod.run_ref(resolve(script), n, voices, threads=threads)


def condition(kind, yr, ref):
    """Finite everywhere; both channels non-zero for every instrument -- channel 0 alone over the frames an
    instrument spends at topology 0, where channel 1 is 0.0f x master."""
    if kind == "synth":
        SR.condition(yr)
    elif kind == "synth_svf":
        SV.condition(yr, ref.topology_of_frames())
    else:
        assert ref.sounding.all()
        DK.condition(yr, ref)


# ----------------------------------------------------------------------------------------------- set-ups
def setup(kind, n, voices, seed=5):
    """The steps ahead of the first note.  The Svf synth and the kit: topologies 0 and 1 alternate, so both sit
    in every lane pair of the delay waves.  The kit: every voice has a sample -- a 20-frame one-shot where
    kit + slot is even, else a 61-frame loop that first turns 64 .. 68 frames after a NoteOn -- and sits at
    drumkit_ref.snote(kit, slot), so a kit's note order is its slot order."""
    if kind == "synth":
        return [("params", SR.params(n, seed))]
    if kind == "synth_svf":
        p = SV.params(n, seed)
        p[SV.TOPOLOGY] = np.arange(n) % 2
        return [("params", p)]
    p = DK.params(n, seed)
    p[DK.TOPOLOGY] = np.arange(n) % 2
    recs = []
    for i in range(n):
        for q in range(voices):
            ls = 3 + i % 5
            recs.append((i, q, 0, 0, 0, 0) if (i + q) % 2 == 0 else (i, q, 1, 1, ls, ls + 60))
    return [("params", p), ("bank", workload.sample_bank(KIT_LENGTHS, seed=11)), ("samples", recs),
            ("map", DK.slot_map(n, voices))]


def note_of(kind, n, voices):
    """note(i, p): the note that notes_on() gives voice p of instrument i.  A synth's: 36 .. 67, no two voices of an
    instrument alike (a NoteOff finds the voice it is meant for) and none of them a note the cases play later."""
    if kind == "drumkit":
        return DK.snote
    return lambda i, p: 36 + 4 * p + i % 4


def notes_on(kind, n, voices):
    note = note_of(kind, n, voices)
    return [(i, NOTE_ON, note(i, p)) for i in range(n) for p in range(voices)]


def few(n):
    """At most three instruments of any 64-instrument group, its edges among them."""
    return sorted({0, 1, 63, 64, n - 1} & set(range(n)))


# ------------------------------------------------------------------------------------------------- cases
def case_sparse(kind, n, voices):
    """Every voice sounds from frame 0; then six event times with notes on few(n) only, so every voice-slot group's
    records fit its fixed slots.  A synth: voice 0 released at 4 and taken again at 12 (a NoteOn that finds the
    freed voice), every voice's gate closed at 16 and opened at 20, the new note released at 36, a NoteOn at 60.
    A kit: pad 0 released at 4 and retriggered at 12, pad 1 released at 16 and retriggered at 20, a note nobody sits
    at at 36 (an empty segment), pad 0 again at 60.  Then an event-free call."""
    note, w = note_of(kind, n, voices), few(n)
    if kind == "drumkit":
        q = 1 % voices
        per = [(4, NOTE_OFF, lambda i: note(i, 0)), (12, NOTE_ON, lambda i: note(i, 0)), (16, NOTE_OFF, lambda i: note(i, q)),
               (20, NOTE_ON, lambda i: note(i, q)), (36, NOTE_ON, lambda i: 127), (60, NOTE_ON, lambda i: note(i, 0))]
    else:
        per = [(4, NOTE_OFF, lambda i: note(i, 0)), (12, NOTE_ON, lambda i: 72), (16, GATE_OFF, lambda i: 0),
               (20, GATE_ON, lambda i: 0), (36, NOTE_OFF, lambda i: 72), (60, NOTE_ON, lambda i: 74)]
    assert [f for f, _, _ in per] == FRAMES
    timed = [(f, i, t, nt(i)) for f, t, nt in per for i in w]
    return setup(kind, n, voices) + [("events", notes_on(kind, n, voices)), ("timed", timed), ("block", NF),
                                     ("check_playing",), ("block", NF)]


def case_all_on(kind, n, voices):
    """Nothing at frame 0 (an empty segment 0).  At 12 every voice of every instrument gets its NoteOn, at 36 voice
    0's note is released everywhere, at 60 a NoteOn everywhere: every full voice-slot group is crowded (the overflow
    list) in three segments."""
    note = note_of(kind, n, voices)
    timed = [(12,) + ev for ev in notes_on(kind, n, voices)]
    timed += [(36, i, NOTE_OFF, note(i, 0)) for i in range(n)]
    timed += [(60, i, NOTE_ON, note(i, 0) if kind == "drumkit" else 72) for i in range(n)]
    return setup(kind, n, voices, seed=6) + [("timed", timed), ("block", NF), ("check_playing",), ("block", NF)]


ALLOCATION_PLAYING = [[72, 64], [72, 65]]          # Playing() of every instrument after calls 1 and 2


def case_allocation(kind, n):
    """Two voices.  Call 1: NoteOn 60 and 64 at frame 0, a third NoteOn at 4 (no free voice at its frame: dropped),
    NoteOff 60 at 8, NoteOn 72 at 12 (takes the voice freed at 8).  Call 2: NoteOff 64 and NoteOn 65 both at frame 4
    (the NoteOn finds the voice the NoteOff before it freed)."""
    assert kind != "drumkit"
    every = range(n)
    one = [(0, i, NOTE_ON, 60) for i in every] + [(0, i, NOTE_ON, 64) for i in every] + [(4, i, NOTE_ON, 67) for i in every]
    one += [(8, i, NOTE_OFF, 60) for i in every] + [(12, i, NOTE_ON, 72) for i in every]
    two = [(4, i, NOTE_OFF, 64) for i in every] + [(4, i, NOTE_ON, 65) for i in every]
    return setup(kind, n, 2) + [("timed", one), ("block", NF), ("check_playing",), ("timed", two), ("block", NF),
                                ("check_playing",), ("block", NF)]


def case_carry(kind, n, voices):
    """Three calls of 64 frames, everything queued before the first.  At frame 64 (frame 0 of call 2, routed as call
    1 returns): a synth's voice 0 is released, a kit's pad 0 retriggered.  Between calls 1 and 2 an untimed note:
    the synth's NoteOn 82 takes the voice that release freed; the kit's NoteOff of pad 0 lands behind the retrigger.
    At 2 x 64 + 4 the last voice is released and at 2 x 64 + 8 a NoteOn takes it (the kit: pad P - 1 off, then on)."""
    note, every, last = note_of(kind, n, voices), range(n), voices - 1
    if kind == "drumkit":
        timed = [(NF, i, NOTE_ON, note(i, 0)) for i in every]
        between = [(i, NOTE_OFF, note(i, 0)) for i in every]
        timed += [(2 * NF + 8, i, NOTE_ON, note(i, last)) for i in every]
    else:
        timed = [(NF, i, NOTE_OFF, note(i, 0)) for i in every]
        between = [(i, NOTE_ON, 82) for i in every]
        timed += [(2 * NF + 8, i, NOTE_ON, 81) for i in every]
    timed += [(2 * NF + 4, i, NOTE_OFF, note(i, last)) for i in every]
    return setup(kind, n, voices) + [("events", notes_on(kind, n, voices)), ("timed", timed), ("block", NF),
                                     ("check_playing",), ("events", between), ("check_playing",), ("block", NF),
                                     ("check_playing",), ("block", NF), ("check_playing",), ("block", NF)]


def case_seventeen(kind, n, voices):
    """One call of 128 frames with 17 distinct times -- frame 0 and every quad up to 64 -- which is two launches of
    64 frames; the second one's frames of channel 1 lie a whole call's plane from channel 0's.  At 4 k the
    instruments i = k (mod 5) get voice 0's note, released for odd k and played for even k."""
    note = note_of(kind, n, voices)
    timed = [(4 * k, i, NOTE_OFF if k % 2 else NOTE_ON, note(i, 0)) for k in range(1, 17) for i in range(k % 5, n, 5)]
    s = setup(kind, n, voices) + [("events", notes_on(kind, n, voices)), ("timed", timed), ("block", 2 * NF),
                                  ("check_playing",), ("block", NF)]
    assert launches(s) == [[16, 1], [1]]
    return s


def case_kit_map_change(n, voices=4):
    """Pad 0's note queued at frame 8 of calls 1 and 2; between the calls the even kits give that note to voice 1
    (whose own note goes, and voice 0 sits nowhere: the note order stays the slot order) and the odd kits take voice 0
    off it.  The note pending at the map change follows the new map: the even kits' reaches voice 1, the odd kits'
    nobody."""
    assert voices >= 2
    note = DK.snote
    timed = [(8, i, NOTE_ON, note(i, 0)) for i in range(n)] + [(NF + 8, i, NOTE_ON, note(i, 0)) for i in range(n)]
    swap = [r for i in range(0, n, 2) for r in ((i, None, note(i, 1), None), (i, None, note(i, 0), 1))]
    swap += [(i, None, note(i, 0), None) for i in range(1, n, 2)]
    return setup("drumkit", n, voices) + [("events", notes_on("drumkit", n, voices)), ("timed", timed), ("block", NF),
                                          ("map", swap), ("check_playing",), ("block", NF), ("check_playing",),
                                          ("block", NF)]


def case_kit_retrigger(n, voices=4):
    """Every pad played; one call later -- the 20-frame one-shots run out, the 61-frame loops turn 0 .. 4 frames into
    this call, some of them on the segment's first frame -- every pad is retriggered at frames 4 and 12, inside the
    first chunk.  The loops turn again at frame 12 + 64 .. 68, inside the event-free call that follows."""
    note = DK.snote
    timed = [(f, i, NOTE_ON, note(i, p)) for f in (4, 12) for i in range(n) for p in range(voices)]
    return setup("drumkit", n, voices) + [("events", notes_on("drumkit", n, voices)), ("block", NF), ("timed", timed),
                                          ("block", NF), ("check_playing",), ("block", NF)]


def cases(n=65):
    """Every case at its default shape: {name: (kind, script, n, voices)}."""
    out = {}
    for kind in KINDS:
        for voices in (1, 4, 5, 8):
            out[f"{kind}-sparse-P{voices}"] = (kind, case_sparse(kind, n, voices), n, voices)
            out[f"{kind}-all_on-P{voices}"] = (kind, case_all_on(kind, n, voices), n, voices)
        out[f"{kind}-carry"] = (kind, case_carry(kind, n, 4), n, 4)
        out[f"{kind}-seventeen"] = (kind, case_seventeen(kind, n, 4), n, 4)
        if kind != "drumkit":
            out[f"{kind}-allocation"] = (kind, case_allocation(kind, n), n, 2)
    out["drumkit-map_change"] = ("drumkit", case_kit_map_change(n), n, 4)
    out["drumkit-retrigger"] = ("drumkit", case_kit_retrigger(n), n, 4)
    return out
