"""The code-partition path's arithmetic (csrc/code_part.h), on the CPU.

graph_sets.hip's partition_kernel<CodeStream>, code_append_kernel and
code_reduce_kernel take their constants, a block's output need, the run split
and the append kernel's per-flush bookkeeping from one host header.
code_part_test.cpp drives one block's bookkeeping flush by flush (adversarial
and seeded histograms at 129, 293, 294, 391 and 512 code buckets) and checks
every staging, vector-table and slice index against the sizes the kernel
declares from the same header: the bound staged_bound(cap, nb) is reached and
never exceeded, and the size the staging array had before (cap + 8 NB) is
overrun from 294 buckets on, the 8-rank weak configuration's 391 included."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "karma_amd", "csrc")


def test_code_partition_bookkeeping_under_sanitizers():
    subprocess.run(["make", "-C", CSRC, "code_part_test"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "build", "code_part_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1].startswith("ok (")
    rows = {}
    for ln in lines[:-1]:
        m = re.match(r"nb (\d+): worst staged (\d+), bound (\d+), declared (\d+), earlier size (\d+)( \(overrun\))?$", ln)
        assert m, ln
        rows[int(m.group(1))] = tuple(int(x) for x in m.groups()[1:5]) + (m.group(6) is not None,)
    assert sorted(rows) == [129, 293, 294, 391, 512]
    # the worst region sums by hand: 16 nb + 8 floor((12288 - 2 nb) / 8)
    assert rows[391][:2] == (17760, 17760) and rows[512][:2] == (19456, 19456) and rows[294][:2] == (16400, 16400)
    for nb, (worst, bound, declared, earlier, overrun) in rows.items():
        assert worst <= bound <= declared == 19456 and earlier == 16384
        assert overrun == (worst > earlier) == (nb >= 294)


def test_code_partition_header_is_host_only():
    hdr = open(os.path.join(CSRC, "code_part.h")).read()
    assert "#include <hip" not in hdr and "karma_internal.h\"" not in hdr and "__device__" not in hdr
    # graph_sets.hip keeps no copy of the header's constants
    src = open(os.path.join(CSRC, "graph_sets.hip")).read()
    assert '#include "code_part.h"' in src
    for name in ("kPT", "kMaxListsPerBlock", "kCodeFill", "kAppendCap", "kNarrowBc", "kMaxBc", "kAppendMinBc",
                 "kCrPieces", "kCrSmax", "kCgShift", "kWin"):
        assert re.search(r"constexpr\s+int\s+%s\b" % name, hdr), name
        assert not re.search(r"constexpr\s+int\s+(\w+\s*=[^;,]*,\s*)*%s\s*=" % name, src), name
