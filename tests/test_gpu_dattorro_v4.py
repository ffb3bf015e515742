"""dattorro_block_v4 -- the network of the 65,536-reverb workload and of every uniform-pre-delay
engine of 2 x 64 x CUs instances and more -- at the small, ragged shapes where kernels go wrong.

The engine would run dattorro_block_v5 at these sizes.  OLFX_DT_V4=1 forces v4 for uniform
pre-delays; the library reads it once per process, so tests/dattorro_v4_cases.py runs every case in
one child process started with the variable set, and writes a report; each test here asserts one
case's entry.  The child runs once per session (a module fixture), started fresh (no exec).

The child's wall time measured on an MI355X: 4.07 s alone and 4.25 s as this module's fixture (2.1 s
in the 59 cases, the rest imports and start-up): CHILD_SECONDS below.  Its time limit is three times
that, so that a hang is caught and a loaded machine does not trip it.
"""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RUNNER = os.path.join(HERE, "dattorro_v4_cases.py")
CHILD_SECONDS = 4.3           # measured: see the module docstring
CASES = [
    "ref_impulse", "ref_noise_10s", "ref_sweep_0", "ref_sweep_1", "ref_sweep_2", "ref_sweep_3",
    "ref_uniform_pd_0", "ref_uniform_pd_1", "ref_uniform_pd_3", "ref_uniform_pd_4", "ref_uniform_pd_5",
    "ref_uniform_pd_8", "ref_uniform_pd_9", "ref_uniform_pd_257", "ref_uniform_pd_4800", "ref_uniform_long",
    "ragged_n1", "ragged_n63", "ragged_n70", "ragged_n72", "ragged_n300",
    "long_run_n70_pd37", "long_run_n70_pd8191", "long_run_n72_pd37", "long_run_n72_pd8191",
    "predelay_sweep", "layout_switches_n70", "layout_switches_n96", "layout_switches_n300",
    "edge_subnormal_n70", "edge_burst_n70", "edge_loud100_n70", "edge_negzero_n70", "edge_ones_n70",
    "edge_alternating_n70", "edge_loud127_n70", "poisoned_n70",
    "edge_subnormal_n72", "edge_burst_n72", "edge_loud100_n72", "edge_negzero_n72", "edge_ones_n72",
    "edge_alternating_n72", "edge_loud127_n72", "poisoned_n72",
    "corners_pd0", "corners_pd4800",
    "contained_device_n1", "contained_host_n1", "contained_device_n63", "contained_host_n63",
    "contained_device_n70", "contained_host_n70", "contained_device_n72", "contained_host_n72",
    "host_io_equals_device_io", "tiny_blocks_n1", "tiny_blocks_n70", "param_change",
]


def test_case_list_equals_the_runner_s():
    """The runner's --list is the list parametrized here: no case drops out of either unnoticed."""
    out = subprocess.run([sys.executable, RUNNER, "--list"], capture_output=True, text=True, check=True).stdout
    assert out.split() == CASES and CASES


@pytest.fixture(scope="module")
def v4_report(cuda, tmp_path_factory):
    """(report, the child's last output): the runner, once, in a fresh child with OLFX_DT_V4=1."""
    path = str(tmp_path_factory.mktemp("dattorro_v4") / "report.json")
    try:
        r = subprocess.run([sys.executable, RUNNER, "--report", path], env={**os.environ, "OLFX_DT_V4": "1"},
                           capture_output=True, text=True, timeout=3 * CHILD_SECONDS)
        tail = f"exit status {r.returncode}\n" + (r.stdout + r.stderr)[-3000:]
    except subprocess.TimeoutExpired as err:
        out = err.stdout.decode(errors="replace") if isinstance(err.stdout, bytes) else (err.stdout or "")
        tail = f"no exit within {3 * CHILD_SECONDS} s\n" + out[-3000:]
    report = {}
    if os.path.exists(path):
        with open(path) as f:
            report = json.load(f)
    return report, tail


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_dattorro_v4_case(v4_report, name):
    report, tail = v4_report
    assert name in report, f"{name} is missing from the child's report; its last output:\n{tail}"
    entry = report[name]
    print(f"\n{name}: kernels {entry['kernels']}")
    assert entry["ok"], entry["detail"]
    assert "dattorro_block_v4" in entry["kernels"]
