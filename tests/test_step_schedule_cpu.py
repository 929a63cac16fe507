"""The deferred step's stream assignment (csrc/step_schedule.h), on the CPU.

run_deferred in csrc/step.hip places a step's records job, its plan and
profile, and its tail on the step's four streams by one pure function of
(world, xstream, one_comm, streams, A, sequential, flg, seq).
step_schedule_test.cpp checks hand-written rows of it (one process with small
and large batches, sequential, two processes with and without the exchange
stream and the side communicator, KARMA_STEP_STREAMS) and its invariants over
all 384 combinations of the inputs."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "karma_amd", "csrc")


def test_deferred_schedule_rows_and_invariants():
    subprocess.run(["make", "-C", CSRC, "step_schedule_test"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "build", "step_schedule_test")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("ok (384 cases")


def test_step_takes_its_streams_from_the_schedule():
    # the header stays host-only, and step.hip derives no stream choice of its own
    hdr = open(os.path.join(CSRC, "step_schedule.h")).read()
    assert "#include <hip" not in hdr and "karma_internal.h\"" not in hdr
    src = open(os.path.join(CSRC, "step.hip")).read()
    assert src.count("deferred_schedule(") == 1
    assert "kAltMaxRecords" not in src and "seq & 1" not in src
