"""Records tests/golden/rms_reference_runs.json from the reference's own ol::core::Rms
(modules/corelib/ol_corelib.h:61-85) through rms_recorder.cpp, built into a temporary directory against the
reference tree's header.  tests/test_meter_ref.py imports the run list and the recording from here, so the
fixture and a fresh recording are made the same way.

    python tests/golden/gen_rms_golden.py [<reference root>]

The signals are workload.noise_np streams (xorshift32: pure integer arithmetic, the same on every machine)
scaled by a power of two; nothing but the runs' settings and the recorded bits goes into the file.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ol_dsp_amd.workload import noise_np  # noqa: E402

import meter_ref  # noqa: E402

FIXTURE = os.path.join(HERE, "rms_reference_runs.json")
REFERENCE = os.environ.get("OLFX_REFERENCE", "/root/reference")
HEADER = os.path.join("modules", "corelib", "ol_corelib.h")

W44 = float(np.float32(44100) / np.float32(375))      # 117.6 in fp32: never equals a count

# name, sample rate, Init's window, a second Init (frame, rate, window) or None, stream, scale, NaN frame or None
RUNS = [
    ("default_48k", 48000.0, 0.0, None, 1, 1.0, None),
    ("default_44k1", 44100.0, 0.0, None, 2, 1.0, None),
    ("default_96k", 96000.0, 0.0, None, 3, 1.0, None),
    ("window_1", 48000.0, 1.0, None, 4, 1.0, None),
    ("window_3", 48000.0, 3.0, None, 5, 1.0, None),
    ("window_117.6", 48000.0, W44, None, 6, 1.0, None),
    ("init_mid_run_larger", 48000.0, 16.0, (200, 48000.0, 128.0), 7, 1.0, None),
    ("init_mid_run_below_count", 48000.0, 300.0, (250, 48000.0, 100.0), 8, 1.0, None),
    ("scale_2^-70", 48000.0, 0.0, None, 9, 2.0 ** -70, None),
    ("one_nan", 48000.0, 0.0, None, 10, 1.0, 300),
]
FRAMES = 600
LONG_FRAMES = 70000
LONG_RATES = (48000.0, 44100.0, 96000.0)


def signal(stream: int, frames: int, scale: float = 1.0, nan_at=None) -> np.ndarray:
    x = noise_np(stream, 1, frames, ch=1)[0, :, 0] * np.float32(scale)
    if nan_at is not None:
        x[nan_at] = np.nan
    return np.ascontiguousarray(x, np.float32)


def have_reference(root: str = REFERENCE) -> bool:
    return os.path.exists(os.path.join(root, HEADER))


def build_recorder(tmpdir: str, root: str = REFERENCE, opt: str = "-O2") -> str:
    exe = os.path.join(tmpdir, "rms_recorder")
    cmd = [os.environ.get("CXX", "g++"), opt, "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(root, "modules"),
           "-o", exe, os.path.join(HERE, "rms_recorder.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return exe


def record(exe: str, x: np.ndarray, sr: float, window: float, again=None) -> np.ndarray:
    args = [exe, repr(float(sr)), repr(float(window))]
    if again is not None:
        args += [str(int(again[0])), repr(float(again[1])), repr(float(again[2]))]
    out = subprocess.run(args, input=x.tobytes(), capture_output=True, check=True, timeout=120).stdout
    y = np.frombuffer(out, np.float32)
    assert y.shape == x.shape
    return y


def restate(x: np.ndarray, sr: float, window: float, again=None) -> np.ndarray:
    """The same run through tests/meter_ref.py: one mono signal; a second Init is a window set between calls."""
    ref = meter_ref.MeterRef(1, 1, sr)
    ref.set("window", window)
    x3 = x[None, :, None]
    if again is None:
        return ref.process(x3)[0, :, 0]
    k, sr2, w2 = again
    head = ref.process(x3[:, :k])
    # Init(sr2, w2): the window alone (a 0 resolves against the new rate)
    ref.sample_rate = float(sr2)
    ref.set("window", w2)
    return np.concatenate([head, ref.process(x3[:, k:])], 1)[0, :, 0]


def record_all(exe: str) -> dict:
    runs = []
    for name, sr, window, again, stream, scale, nan_at in RUNS:
        y = record(exe, signal(stream, FRAMES, scale, nan_at), sr, window, again)
        runs.append({"name": name, "sample_rate": sr, "window": window, "init_again": again, "stream": stream,
                     "scale": scale, "nan_at": nan_at, "frames": FRAMES,
                     "rms_bits": "".join(f"{b:08x}" for b in y.view(np.uint32).tolist())})
    long_runs = []
    for k, sr in enumerate(LONG_RATES):
        y = record(exe, signal(20 + k, LONG_FRAMES), sr, 0.0)
        long_runs.append({"sample_rate": sr, "stream": 20 + k, "frames": LONG_FRAMES,
                          "fnv1a64": f"{meter_ref.fnv1a64(y):016x}", "last_bits": f"{int(y.view(np.uint32)[-1]):08x}"})
    return {"source": "ol::core::Rms, modules/corelib/ol_corelib.h:61-85, g++ -O2 -ffp-contract=off",
            "runs": runs, "long_runs": long_runs}


def main() -> None:
    root = sys.argv[1] if len(sys.argv) > 1 else REFERENCE
    with tempfile.TemporaryDirectory() as tmp:
        data = record_all(build_recorder(tmp, root))
    with open(FIXTURE, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes, {len(data['runs'])} runs, {len(data['long_runs'])} long runs")


if __name__ == "__main__":
    main()
