"""The records job's control-block layout (csrc/sets_ctrl.h), on the CPU.

graph_sets.hip's SetsJob and step.hip's kernels share one block of flags,
counters, per-bucket counts, their scan, overflow bytes, split counts,
partition-block item counts and look-back words.  sets_ctrl_test.cpp checks
every offset of CtrlLayout against the literal arithmetic the job used before
(B around the overflow bytes' word boundary, config 3's 196 buckets, with and
without split bounds), that no two regions overlap, and the enumerators'
values."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "karma_amd", "csrc")


def test_ctrl_layout_offsets():
    subprocess.run(["make", "-C", CSRC, "sets_ctrl_test"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "build", "sets_ctrl_test")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("ok (24 cases")


def test_ctrl_layout_header_is_host_only():
    hdr = open(os.path.join(CSRC, "sets_ctrl.h")).read()
    assert "#include <hip" not in hdr and "karma_internal.h\"" not in hdr
