"""tests/platerack_ref.py anchored to the oracle it extends: with REVERB_BALANCE = 0 the plate's
output is multiplied by 0 and the helper's delay -> mix -> filter -> master composition must equal
O.FxRack's own rack (whose ReverbSc stub drops out the same way), in topology 0 and topology 1."""
import numpy as np
import pytest

import oracle as O
import platerack_ref as PR
from helpers import fast_noise, fxrack_params


@pytest.mark.parametrize("topology", [0, 1])
def test_helper_equals_fxrack_at_zero_balance(topology):
    n, frames = 3, 1000
    rng = np.random.default_rng(21 + topology)
    p = fxrack_params(rng, n)
    p[PR.BALANCE] = 0.0
    x = fast_noise(n, frames, seed=7 + topology)
    rack, helper = O.FxRack(n), PR.PlateRack(n)
    for i in range(n):
        for f in range(11):
            rack.set(i, f, float(p[f, i]))
            helper.set(i, f, float(p[f, i]))
        rack.set(i, "topology", float(topology))
        helper.set(i, "topology", float(topology))
        helper.set(i, "verb_decay", float(rng.uniform(0.2, 0.9)))       # the plate runs; x 0 hides it
    want = np.concatenate([rack.process(x[:, :256]), rack.process(x[:, 256:])], 1)
    got = np.concatenate([helper.process(x[:, :256]), helper.process(x[:, 256:])], 1)
    assert np.isfinite(got).all() and np.abs(got[0]).max() > 0
    if topology == 1:
        assert np.abs(got[1]).max() > 0
    # +-0 may differ in sign (v * 0 + a against (0.8 a) * 0 + a): array_equal, not a bit compare
    assert np.array_equal(got, want)


def test_helper_defaults_and_fields():
    d = PR.defaults()
    assert len(d) == PR.N_FIELDS == 19 and len(PR.FIELDS) == 19
    assert np.array_equal(d[:12], O.fxrack_defaults())
    assert [float(v) for v in d[12:]] == [float(np.float32(v)) for v in (0.1, 0.5, 0.5, 0.5, 0.5, 0.5, 0.95)]


def test_helper_plate_is_audible():
    """Balance 1 in topology 1: channel 1 is the plate's right output alone, so the helper differs from
    the stub rack and equals O.Dattorro on the delay stage's mono output."""
    n, frames = 2, 2400
    x = fast_noise(n, frames, seed=3)
    helper, delay, verb = PR.PlateRack(n), O.FxRack(n), O.Dattorro(n, ref=O.ref_available())
    for i in range(n):
        helper.set(i, "reverb_balance", 1.0)
        helper.set(i, "topology", 1.0)
        delay.set(i, "topology", 2.0)
        for f, v in zip(O.DT_FIELDS, PR.defaults()[12:]):
            verb.set(i, f, float(v))
    a0 = delay.process(x)[0]
    v = verb.process(((a0 + a0) / np.float32(2))[None])
    got = helper.process(x)
    assert np.array_equal(got[1], v[1] * np.float32(1) + a0 * np.float32(0))
    assert np.abs(got[1]).max() > 0
