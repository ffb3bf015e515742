"""The host core's control packets around the timed calls, pinned: tests/cpp/dump_packets.cpp (linked with
olfx_host.cpp alone, no GPU) drives a Shadow as olfx_process does through small scenarios of every timed call on
the voice kinds, the synths, the drum kit and the chorus, and prints per launch the span, the packet plan, the
segments, the dirty lists' sizes and a hash of the packet's words.  The output equals
tests/golden/host_packets.txt (below its first line, which says where the file comes from) byte for byte.  The
golden file was written by the host core that kept three parallel timed-record paths; it is not regenerated."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_packets_match_the_golden_dump(tmp_path):
    exe = str(tmp_path / "dump_packets")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function",
           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "dump_packets.cpp"),
           os.path.join(ROOT, "ol_dsp_amd", "csrc", "olfx_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()
    r = subprocess.run([exe], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    with open(os.path.join(ROOT, "tests", "golden", "host_packets.txt"), "rb") as f:
        header, want = f.read().split(b"\n", 1)
    assert header.startswith(b"# ")
    if r.stdout != want:
        got_lines, want_lines = r.stdout.decode().splitlines(), want.decode().splitlines()
        first = next((k for k, (a, b) in enumerate(zip(got_lines, want_lines)) if a != b), min(len(got_lines), len(want_lines)))
        raise AssertionError("line %d differs (got %d lines, want %d)\n got: %s\nwant: %s" % (
            first + 1, len(got_lines), len(want_lines), "\n".join(got_lines[first:first + 3]), "\n".join(want_lines[first:first + 3])))
