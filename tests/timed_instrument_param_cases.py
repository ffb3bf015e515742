"""olfx_timed_instrument_params / olfx_timed_instrument_control (timed parameter and control changes for
OLFX_KIND_SYNTH, OLFX_KIND_SYNTH_SVF and OLFX_KIND_DRUMKIT): the cases as data, and the driver that resolves a timed
script into the plain scripts of the existing references.  No torch, no GPU.

A timed script is a tests/timed_note_cases.py script with two more steps,
  ("tparams",  [(frame, inst, field, value), ...])                      olfx_timed_instrument_params
  ("tcontrol", [(frame, inst, cc, value, source, channel), ...])        olfx_timed_instrument_control
(field: the kind's index; source "midi" / "hw"; channel: a kit's MIDI channel or 16 for its rack, else 0).
resolve() turns it into ("set", ...) / ("control", ...) / ("events", ...) / ("block", frames) steps, one block per
distinct time -- the split calls that include/olfx.h states as the contract: at a time, its records first, in queueing
order (both steps share one order), then its notes; a record or note at frame 0 at the call; one at or past the call's
end stays pending with its frame reduced by the call's length, and what lands on frame 0 is applied as the call
returns (records, then notes), ahead of whatever the script does next.  A script without the two steps resolves
through timed_note_cases.resolve itself, and tests/test_timed_instrument_params_ref.py holds this module's rule to
that one on the note-only cases.

for_reference() makes the resolved script one the references run: drumkit_ref takes ("control", ...) as it stands;
synth_ref and synth_svf_ref have no such step, so a synth's control becomes the ("set", ...) steps of its fan-out
under the instrument's topology at that point of the script (engine.synth_control_map; an update-only hit is a voice
field set to the value it has: UpdateConfig + Update() of the instrument's voices)."""
from __future__ import annotations

import numpy as np

import drumkit_ref as DK
import synth_ref as SR
import timed_note_cases as C
from ol_dsp_amd.engine import synth_control_map

KINDS, NF, FRAMES = C.KINDS, C.NF, C.FRAMES
NOTE_OFF, NOTE_ON = C.NOTE_OFF, C.NOTE_ON
CH_RACK = DK.CH_RACK
VC, FR = list(SR.O.VC_FIELDS), list(SR.O.FR_FIELDS)
# corelib/cc_map.h
CC_VOLUME, CC_PORTAMENTO, CC_REVERB_BALANCE, CC_DELAY_TIME = 7, 5, 34, 35
CC_CUTOFF, CC_RESONANCE, CC_DRIVE = 41, 42, 44
CC_FX_CUTOFF, CC_FX_RESONANCE, CC_FX_TYPE, CC_FX_DRIVE = 45, 46, 47, 48
CC_OSC_1_VOLUME = 114             # handled, sets no modelled field: Update() alone
CC_IGNORED = 3                    # no handler anywhere
RECORD_STEPS = ("tparams", "tcontrol")


def vf(kind, name, slot=0):
    """A voice field's index: the instrument's (a synth), voice slot `slot`'s (a kit)."""
    return (DK.NV * slot if kind == "drumkit" else 0) + VC.index(name)


def rf(kind, name):
    return (DK.RACK0 if kind == "drumkit" else SR.NV) + FR.index(name)


def ctl(frame, inst, cc, value, kind, channel=None, source="midi"):
    """A control record; a kit's goes to its rack unless a channel is given."""
    return (frame, inst, cc, value, source, (CH_RACK if channel is None else channel) if kind == "drumkit" else 0)


# --------------------------------------------------------------------------------------------- the driver
def resolve(script):
    """The timed script as split steps (see the module docstring)."""
    if not any(step[0] in RECORD_STEPS for step in script):
        return C.resolve(script)
    pending, arrival, out = [], 0, []          # [frame, arrival, step kind, payload]

    def apply(items):
        """Records in queueing order, then notes in queueing order."""
        for w in items:
            if w[2] == "tparams":
                out.append(("set",) + tuple(w[3]))
            elif w[2] == "tcontrol":
                out.append(("control", [tuple(w[3])]))
        notes = [tuple(w[3]) for w in items if w[2] == "timed"]
        if notes:
            out.append(("events", notes))

    for step in script:
        if step[0] in RECORD_STEPS + ("timed",):
            now = []
            for rec in step[1]:
                frame = rec[0]
                assert frame % 4 == 0 and 0 <= frame < 1 << 31
                (now if frame == 0 else pending).append([frame, arrival, step[0], tuple(rec[1:])])
                arrival += 1
            apply(now)
            pending.sort(key=lambda w: (w[0], w[1]))
        elif step[0] == "block":
            n_frames, at = step[1], 0
            while at < n_frames:
                apply([w for w in pending if w[0] == at])
                pending = [w for w in pending if w[0] != at]
                until = min([w[0] for w in pending if w[0] < n_frames] + [n_frames])
                out.append(("block", until - at))
                at = until
            for w in pending:
                w[0] -= n_frames
            apply([w for w in pending if w[0] == 0])             # as the call returns
            pending = [w for w in pending if w[0] != 0]
        else:
            out.append(step)
    return out


def for_reference(kind, resolved, n):
    """The resolved script as the kind's reference takes it."""
    if kind == "drumkit":
        return resolved
    p, out = np.tile(SR.defaults()[:, None], (1, n)).astype(np.float32), []
    for step in resolved:
        if step[0] == "params":
            p = np.array(step[1], np.float32)
        elif step[0] == "set":
            p[int(step[2]), step[1]] = np.float32(step[3])
        if step[0] != "control":
            out.append(step)
            continue
        for inst, cc, value, source, _ in step[1]:
            for name, v in synth_control_map(cc, value, source, kind, int(p[SR.TOPOLOGY, inst])):
                f = VC.index("amp_env_amount") if name == "update_only" else SR.FIELDS.index(name)
                v = float(p[f, inst]) if name == "update_only" else v
                p[f, inst] = np.float32(v)
                out.append(("set", inst, f, v))
    return out


def run_reference(kind, script, n, voices, threads=4):
    """([2][frames][n], the reference object) of a timed script."""
    mod = {"synth": SR, "synth_svf": C.SV, "drumkit": DK}[kind]
    return mod.run_ref(for_reference(kind, resolve(script), n), n, voices, threads=threads)


def launches(script, n, voices, kind):
    """Per ("block", ...) step: the frames of each of its launches -- a launch ends ahead of its 17th time, ahead of a
    boundary record (a delay field, the topology, CC 35-39 to a rack) and ahead of the time whose records would make
    more than the launch's cap (n; a kit: voices x n; a time's own count at most the cap)."""
    boundary_fields = {rf(kind, f) for f in FR if f.startswith("delay_") or f == "topology"}
    cap = n * voices if kind == "drumkit" else n
    pending, out = [], []                      # (frame, is record, is boundary)
    for step in script:
        if step[0] == "timed":
            pending += [(ev[0], False, False) for ev in step[1] if ev[0] > 0]
        elif step[0] == "tparams":
            pending += [(r[0], True, r[2] in boundary_fields) for r in step[1] if r[0] > 0]
        elif step[0] == "tcontrol":
            pending += [(r[0], True, CC_DELAY_TIME <= r[2] <= 39 and (kind != "drumkit" or r[5] == CH_RACK))
                        for r in step[1] if r[0] > 0]
        elif step[0] == "block":
            spans, start = [], 0
            while start < step[1]:
                segs, recs, end = 1, 0, step[1]
                for t in sorted({w[0] for w in pending if start < w[0] < step[1]}):
                    here = [w for w in pending if w[0] == t and w[1]]
                    if segs == C.SEG_CAP or any(w[2] for w in here) or recs + min(len(here), cap) > cap:
                        end = t
                        break
                    segs, recs = segs + 1, recs + min(len(here), cap)
                spans.append(end - start)
                start = end
            out.append(spans)
            pending = [(w[0] - step[1],) + w[1:] for w in pending if w[0] >= step[1]]
            pending = [w for w in pending if w[0] > 0]
    return out


def changes(script, kind, voices):
    """[(absolute frame, arrival numbers, instruments)] of the script's record times: what tests/
    test_timed_instrument_params_ref.py asks to be audible.  A control nothing takes -- CC_IGNORED, or a kit's channel
    nobody sits at (the set-ups map channel p to voice p) -- changes no instrument and is left out."""
    done, arrival, at = 0, 0, {}
    for step in script:
        if step[0] in RECORD_STEPS:
            for rec in step[1]:
                ignored = step[0] == "tcontrol" and (rec[2] == CC_IGNORED or (kind == "drumkit" and voices <= rec[5] < CH_RACK))
                if not ignored:
                    who = at.setdefault(done + rec[0], (set(), set()))
                    who[0].add(arrival)
                    who[1].add(rec[1])
                arrival += 1
        elif step[0] == "block":
            done += step[1]
    return [(t, at[t][0], sorted(at[t][1])) for t in sorted(at)]


def without(script, arrivals):
    """The script minus the records with these arrival numbers."""
    out, arrival = [], 0
    for step in script:
        if step[0] in RECORD_STEPS:
            keep = [rec for k, rec in enumerate(step[1]) if arrival + k not in arrivals]
            arrival += len(step[1])
            out.append((step[0], keep))
        else:
            out.append(step)
    return out


# ------------------------------------------------------------------------------------------------- cases
def sounding(kind, n, voices, seed=5):
    """The set-up and a NoteOn on every voice at frame 0.  A kit's changes go to slot loop_slot(i), whose 61-frame
    loop plays on; its one-shots have run out by frame 20."""
    return C.setup(kind, n, voices, seed) + [("events", C.notes_on(kind, n, voices))]


def loop_slot(i, voices):
    return (i + 1) % 2 if voices > 1 else 0


def slot_of(kind, i, voices):
    return loop_slot(i, voices) if kind == "drumkit" else 0


def retrigger(kind, n, voices, frame, who):
    """Notes that keep a one-voice kit's even kits sounding (their only sample is the 20-frame one-shot)."""
    note = C.note_of(kind, n, voices)
    return [(frame, i, NOTE_ON, note(i, 0)) for i in who if kind == "drumkit" and voices == 1 and i % 2 == 0]


def case_frames(kind, n, voices):
    """Records on few(n) at frames 4, 12, 16, 20, 36 and 60 of a 64-frame call -- mid-chunk, on a chunk's edge, two in
    one chunk, the last quad -- a voice field, a rack field and a control in turn; then an event-free call."""
    w = C.few(n)
    s = lambda i: slot_of(kind, i, voices)
    recs = [(4, i, vf(kind, "filter_cutoff", s(i)), 700.0 + i) for i in w]
    recs += [(12, i, rf(kind, "filter_cutoff"), 1500.0 + i) for i in w]
    recs += [(16, i, vf(kind, "filter_resonance", s(i)), 0.6) for i in w]
    recs += [(20, i, rf(kind, "reverb_balance"), 0.9) for i in w]
    recs += [(60, i, vf(kind, "filter_cutoff", s(i)), 2500.0 + i) for i in w]
    ctls = [ctl(36, i, CC_CUTOFF, 40.0 + i % 8, kind, channel=s(i)) for i in w]
    notes = [ev for f in (16, 36) for ev in retrigger(kind, n, voices, f, w)]
    return sounding(kind, n, voices) + [("tparams", recs), ("tcontrol", ctls), ("timed", notes), ("block", NF), ("block", NF)]


def case_voice_fields(kind, n, voices):
    """Voice fields alone, on every instrument: cutoff at 4, resonance at 12, the amp envelope's times at 16, portamento
    (heard by the synths' oscillators alone) and the Svf voice's drive at 20, the filter envelope's at 36."""
    every = range(n)
    s = lambda i: slot_of(kind, i, voices)
    recs = [(4, i, vf(kind, "filter_cutoff", s(i)), 500.0 + 3 * i) for i in every]
    recs += [(12, i, vf(kind, "filter_resonance", s(i)), 0.7) for i in every]
    recs += [(16, i, vf(kind, f, s(i)), v) for i in every for f, v in (("amp_attack", 0.02), ("amp_decay", 0.002), ("amp_sustain", 0.3))]
    if kind != "drumkit":
        recs += [(20, i, vf(kind, "portamento"), 0.05) for i in every]
    if kind != "synth":                       # (MoogFilter::SetDrive is a no-op)
        recs += [(20, i, vf(kind, "filter_drive", s(i)), 0.8) for i in every]
    recs += [(36, i, vf(kind, f, s(i)), v) for i in every for f, v in (("filter_env_amount", 0.9), ("filter_decay", 0.001), ("filter_sustain", 0.2))]
    # a NoteOn at 16 restarts the envelopes under the new times, and a synth's at 24 glides under the new portamento
    note = C.note_of(kind, n, voices)
    if kind == "drumkit":
        notes = [(16, i, NOTE_ON, note(i, s(i))) for i in every]
    else:
        notes = [(16, i, NOTE_OFF, note(i, 0)) for i in every] + [(16, i, NOTE_ON, 79) for i in every]
        notes += [(24, i, NOTE_OFF, 79) for i in every] + [(24, i, NOTE_ON, 55) for i in every]
    return sounding(kind, n, voices, 6) + [("timed", notes), ("tparams", recs), ("block", NF), ("block", NF)]


def case_rack_fields(kind, n, voices):
    """F-role fields alone, on every instrument: FILTER_TYPE through 1, 2, 3, 4 and back to 0, REVERB_BALANCE, and
    MASTER_VOLUME where the topology is 0 (the synth has none: its instruments sit at topology 1)."""
    every = range(n)
    recs = [(f, i, rf(kind, "filter_type"), float(t)) for f, t in ((4, 1), (12, 2), (16, 3), (20, 4), (60, 0)) for i in every]
    recs += [(36, i, rf(kind, "reverb_balance"), 0.8) for i in every]
    recs += [(36, i, rf(kind, "filter_cutoff"), 900.0 + i) for i in every]
    if kind != "synth":
        recs += [(44, i, rf(kind, "master_volume"), 0.3) for i in range(0, n, 2)]
    # (every instrument starts at type 0, whatever its draw, so each step changes the type)
    low = [("set", i, rf(kind, "filter_type"), 0.0) for i in every]
    return sounding(kind, n, voices) + low + [("tparams", recs), ("block", NF), ("block", NF)]


def case_controls(kind, n, voices):
    """CC 41-44 (a synth: the voice filter and, at topology 1, the rack's; a kit: channel q's voice alone, then the
    rack of the odd kits, which sit at topology 1 where it takes them), CC 45-48 and 7 (audible at topology 0, the even instruments of the Svf synth and the kit; the synth's CC 7
    is its voices' amp_env_amount), an update-only control on never-configured voices, an ignored control."""
    every = range(n)
    s = lambda i: slot_of(kind, i, voices)
    ctls = [ctl(4, i, CC_CUTOFF, 50.0, kind, channel=s(i)) for i in every]
    ctls += [ctl(12, i, CC_RESONANCE, 90.0, kind, channel=s(i)) for i in every]
    ctls += [ctl(12, i, CC_IGNORED, 64.0, kind, channel=s(i)) for i in every]
    ctls += [ctl(16, i, CC_DRIVE, 100.0, kind, channel=s(i)) for i in every if kind != "synth"]
    ctls += [ctl(20, i, cc, v, kind) for i in every for cc, v in ((CC_CUTOFF, 30.0), (CC_RESONANCE, 60.0)) if kind == "drumkit" and i % 2 == 1]
    ctls += [ctl(36, i, cc, v, kind) for i in every for cc, v in ((CC_FX_CUTOFF, 20.0), (CC_FX_RESONANCE, 80.0), (CC_FX_TYPE, 30.0),
                                                                   (CC_FX_DRIVE, 50.0)) if kind != "synth" and i % 2 == 0]
    ctls += [ctl(44, i, CC_VOLUME, 40.0, kind, source="hw" if i % 3 == 0 else "midi") for i in every if kind == "synth" or i % 2 == 0]
    ctls += [ctl(52, i, CC_REVERB_BALANCE, 100.0, kind) for i in every if kind == "synth" or i % 2 == 1]
    if kind == "drumkit":
        ctls += [ctl(56, i, CC_CUTOFF, 64.0, kind, channel=voices + 1) for i in every]          # nobody's channel
    return sounding(kind, n, voices) + [("tcontrol", ctls), ("block", NF), ("block", NF)]


def case_update_only(kind, n, voices):
    """No ("params", ...) step: the voices are as Init left them, never Update()d.  CC 114 at frame 12 is their first
    Update() (a kit: of channel 0's voice alone), with unchanged members."""
    s = [step for step in C.setup(kind, n, voices) if step[0] != "params"]
    ctls = [ctl(12, i, CC_OSC_1_VOLUME, 64.0, kind, channel=0) for i in range(n)]
    return s + [("events", C.notes_on(kind, n, voices)), ("tcontrol", ctls), ("block", NF), ("block", NF)]


def case_with_notes(kind, n, voices):
    """Records and notes at one frame on the same and on other instruments, a record at a frame with no note, and a
    NoteOn at 20 that retriggers envelopes whose times change at that very frame (the restart must take the
    segment's envelope words, not the stored ones)."""
    every, note = range(n), C.note_of(kind, n, voices)
    s = lambda i: slot_of(kind, i, voices)
    recs = [(8, i, vf(kind, "filter_cutoff", s(i)), 600.0 + i) for i in range(0, n, 2)]
    recs += [(12, i, rf(kind, "filter_cutoff"), 2000.0) for i in every]
    recs += [(20, i, vf(kind, f, s(i)), v) for i in every for f, v in (("amp_attack", 0.03), ("filter_attack", 0.004), ("amp_sustain", 0.5))]
    if kind == "drumkit":
        notes = [(8, i, NOTE_ON, note(i, s(i))) for i in range(1, n, 2)] + [(20, i, NOTE_ON, note(i, s(i))) for i in every]
    else:
        notes = [(8, i, NOTE_OFF, note(i, 0)) for i in range(1, n, 2)] + [(8, i, NOTE_OFF, note(i, 0)) for i in range(0, n, 4)]
        notes += [(20, i, NOTE_ON, 76) for i in every]
    return sounding(kind, n, voices) + [("timed", notes), ("tparams", recs), ("block", NF), ("block", NF)]


def case_boundary(kind, n, voices):
    """DELAY_TIME at frame 20 -- to a small delay that reaches the delay stage's patch window, on every third
    instrument a large one -- and to 0 at 36; the topology flipped at 12 on every other instrument (the synth accepts
    none but 1: it gets DELAY_FEEDBACK there); voice records and notes at those frames and at others in the launches
    between them."""
    every, note = range(n), C.note_of(kind, n, voices)
    s = lambda i: slot_of(kind, i, voices)
    small, large = float(SR.delay_time(3)), float(SR.delay_time(24000))
    recs = [(20, i, rf(kind, "delay_time"), large if i % 3 == 0 else small) for i in every]
    recs += [(36, i, rf(kind, "delay_time"), 0.0) for i in every]
    if kind == "synth":
        recs += [(12, i, rf(kind, "delay_feedback"), 0.8) for i in range(0, n, 2)]
    else:
        recs += [(12, i, rf(kind, "topology"), float(1 - i % 2)) for i in range(0, n, 2)]
    recs += [(f, i, vf(kind, "filter_cutoff", s(i)), 400.0 + 10 * f + i) for f in (8, 12, 20, 28, 36, 48) for i in every]
    if kind == "drumkit":
        notes = [(f, i, NOTE_ON, note(i, s(i))) for f in (12, 28, 36) for i in every]
    else:
        notes = [(12, i, NOTE_OFF, note(i, 0)) for i in every] + [(28, i, NOTE_ON, 70) for i in every]
        notes += [(36, i, NOTE_OFF, 70) for i in every] + [(48, i, NOTE_ON, 66) for i in every]
    sc = sounding(kind, n, voices) + [("timed", notes), ("tparams", recs), ("block", NF), ("block", NF)]
    assert launches(sc, n, voices, kind)[0] == [12, 8, 16, 28]
    return sc


def case_sizes(kind, n, voices):
    """Calls of 4, 12, 100 and 300 frames, everything queued up front: starts on a call's last quad, in a partial last
    chunk (frame 96 of 100), and records carried from call to call."""
    every = range(n)
    s = lambda i: slot_of(kind, i, voices)
    at = [0, 8, 12, 16 + 96, 16 + 100 + 4, 16 + 100 + 296]
    recs = [(f, i, vf(kind, "filter_cutoff", s(i)), 450.0 + f + i) for f in at[1:] for i in every]
    recs += [(f + 4, i, rf(kind, "filter_resonance"), 0.1 + 0.1 * k) for k, f in enumerate(at) for i in range(0, n, 3)]
    note = C.note_of(kind, n, voices)
    notes = [(f, i, NOTE_ON, note(i, s(i))) for f in (16 + 96, 16 + 100 + 200) for i in every if kind == "drumkit"]
    return sounding(kind, n, voices) + [("tparams", recs), ("timed", notes)] + [("block", b) for b in (4, 12, 100, 300, NF)]


def case_seventeen(kind, n, voices):
    """One call of 128 frames with 17 distinct times -- frame 0, eight note times and eight record times up to 64 --
    which is two launches of 64 frames."""
    note = C.note_of(kind, n, voices)
    s = lambda i: slot_of(kind, i, voices)
    notes = [(8 * k, i, NOTE_OFF if k % 2 else NOTE_ON, note(i, s(i) if kind == "drumkit" else 0)) for k in range(1, 9) for i in range(k % 5, n, 5)]
    recs = [(8 * k - 4, i, vf(kind, "filter_cutoff", s(i)), 300.0 + 50 * k) for k in range(1, 9) for i in C.few(n)]       # (under the record cap)
    sc = sounding(kind, n, voices) + [("timed", notes), ("tparams", recs), ("block", 2 * NF), ("check_playing",), ("block", NF)]
    assert launches(sc, n, voices, kind) == [[64, 64], [64]]
    return sc


def case_record_cap(kind, n, voices):
    """More records in one call than a launch takes: every instrument's voice field at frames 8 and 24 and its rack
    field at 8, 24 and 40 (a kit: every voice slot's field at those frames).  The launch ends where the count would pass
    the cap."""
    every = range(n)
    slots = range(voices) if kind == "drumkit" else (0,)
    recs = [(f, i, vf(kind, "filter_cutoff", q), 350.0 + f + q) for f in (8, 24, 40) for i in every for q in slots]
    recs += [(f, i, rf(kind, "filter_cutoff"), 1200.0 + f) for f in (8, 24) for i in every]
    sc = sounding(kind, n, voices) + [("tparams", recs), ("block", NF), ("block", NF)]
    assert len(launches(sc, n, voices, kind)[0]) >= 2
    return sc


def case_carry(kind, n, voices):
    """Three calls of 64 frames, everything queued before the first: a voice record at frame 64 (applied as call 1
    returns), an untimed set_param and a control between the calls (they land behind it, ahead of the pending ones), a
    control at 64 + 36, records at 2 x 64 + 4 and + 60."""
    every = range(n)
    s = lambda i: slot_of(kind, i, voices)
    recs = [(NF, i, vf(kind, "filter_cutoff", s(i)), 800.0 + i) for i in every]
    recs += [(2 * NF + 4, i, rf(kind, "filter_cutoff"), 1000.0 + i) for i in every]
    recs += [(2 * NF + 60, i, vf(kind, "filter_resonance", s(i)), 0.65) for i in every]
    ctls = [ctl(NF + 36, i, CC_RESONANCE, 100.0, kind, channel=s(i)) for i in every]
    between = [("set", i, vf(kind, "filter_env_amount", s(i)), 0.7) for i in range(0, n, 2)]
    between.append(("control", [ctl(0, i, CC_REVERB_BALANCE, 90.0, kind)[1:] for i in range(1, n, 2)]))
    return sounding(kind, n, voices) + [("tparams", recs), ("tcontrol", ctls), ("block", NF)] + between + [("block", NF)] * 3


def cases(n=65):
    """Every case at its default shape: {name: (kind, script, n, voices)}."""
    out = {}
    for kind in KINDS:
        for voices in (1, 4, 5, 8):
            out[f"{kind}-frames-P{voices}"] = (kind, case_frames(kind, n, voices), n, voices)
        for name, build in (("voice_fields", case_voice_fields), ("rack_fields", case_rack_fields), ("controls", case_controls),
                            ("update_only", case_update_only), ("with_notes", case_with_notes), ("boundary", case_boundary),
                            ("sizes", case_sizes), ("seventeen", case_seventeen), ("record_cap", case_record_cap),
                            ("carry", case_carry)):
            out[f"{kind}-{name}"] = (kind, build(kind, n, 4), n, 4)
    return out
