"""The reference for OLFX_KIND_PLATERACK: a composition of the existing CPU oracles, nothing else.

Per block, for n instances ([2][frames][n] float32 in and out):
  1. a = O.FxRack, topology 2 (DelayFx<2> alone, Fx.h:193-206); in the rack's topology 1 (DelayFx<1>,
     then stereo[0] = stereo[1]) channel 1 becomes a copy of channel 0;
  2. v = O.Dattorro on the mono sum (a0 + a1) / 2 formed in numpy float32 (ReverbFx.cpp:13-19): the
     reference's own verb.cpp build (ref=True) where oracle/_ref exists, else its restatement, which
     tests/test_oracle.py holds to that build bit for bit;
  3. b = v * bal + a * (float32(1) - bal) in float32, one rounding per operation (Fx.h:298);
  4. c = O.FxRack, topology 4 (FilterFx<2> alone: the Svf on channel 0, channel 1 in place);
  5. topology 0: out = (c0 * master, float32(0) * master) -- FxRack's buf_c[1] is never written;
     topology 1: out = (c0, b1), no master volume.

Parameters are the engine's fields (ol_dsp_amd.PARAMS[KIND_PLATERACK]): the rack's twelve, then the
plate's seven.  A change applies from the next process() call on, as the engine applies it at the
next block boundary.
"""
from __future__ import annotations

import numpy as np

import oracle as O

N_RACK = len(O.FR_FIELDS)          # 12, topology last
N_FIELDS = N_RACK + len(O.DT_FIELDS)
FIELDS = O.FR_FIELDS + ["verb_" + f for f in O.DT_FIELDS]
TOPOLOGY = O.FR_FIELDS.index("topology")
BALANCE = O.FR_FIELDS.index("reverb_balance")
MASTER = O.FR_FIELDS.index("master_volume")


def defaults() -> np.ndarray:
    """[19]: the rack's defaults, then the plate as ReverbFx::Init -> Update() would set it through
    the glue of ReverbFx.cpp:29-37 (0.5 for the five forwarded members that lie in their setter's
    domain), damping and pre-delay at DattorroVerb_create's own (verb.cpp:215-221)."""
    plate = {"pre_delay": 0.1, "pre_filter": 0.5, "input_diffusion1": 0.5, "input_diffusion2": 0.5,
             "decay_diffusion": 0.5, "decay": 0.5, "damping": 0.95}
    return np.concatenate([O.fxrack_defaults(), np.array([plate[f] for f in O.DT_FIELDS], np.float32)])


class PlateRack:
    def __init__(self, n: int, sample_rate: float = 48000.0):
        self.n = n
        self.delay = O.FxRack(n, sample_rate)
        self.filt = O.FxRack(n, sample_rate)
        self.verb = O.Dattorro(n, ref=O.ref_available())
        self.p = np.tile(defaults()[:, None], (1, n)).astype(np.float32)
        for i in range(n):
            self.delay.set(i, TOPOLOGY, 2.0)
            self.filt.set(i, TOPOLOGY, 4.0)
            for f in range(N_RACK, N_FIELDS):
                self.verb.set(i, f - N_RACK, float(self.p[f, i]))

    def set(self, inst: int, field, value: float) -> None:
        f = FIELDS.index(field) if isinstance(field, str) else int(field)
        v = np.float32(value)
        self.p[f, inst] = v
        if f == TOPOLOGY:
            assert v in (0.0, 1.0)
        elif f < N_RACK:
            self.delay.set(inst, f, float(v))
            self.filt.set(inst, f, float(v))
        else:
            self.verb.set(inst, f - N_RACK, float(v))

    def set_params(self, p: np.ndarray) -> None:
        """p [19][n] (or fewer leading fields)."""
        for f in range(p.shape[0]):
            for i in range(self.n):
                self.set(i, f, float(p[f, i]))

    def process(self, x: np.ndarray, threads: int = 1) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        f32 = np.float32
        fw = self.p[TOPOLOGY] == 1.0
        a = self.delay.process(x, threads)
        a[1][:, fw] = a[0][:, fw]
        mono = ((a[0] + a[1]) / f32(2)).astype(np.float32)
        v = self.verb.process(mono[None], threads)
        bal = self.p[BALANCE][None, None, :]
        b = (v * bal + a * (f32(1) - bal)).astype(np.float32)
        c = self.filt.process(b, threads)
        master = self.p[MASTER][None, :]
        out = np.empty_like(c)
        out[0] = np.where(fw[None, :], c[0], c[0] * master)
        out[1] = np.where(fw[None, :], c[1], f32(0) * master)
        return out
