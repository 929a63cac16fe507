#!/usr/bin/env python3
"""More eq-class hand cases, captured by running the REFERENCE
(ReadGraph.from_equivalence_classes, read_graph.py:61-148) like make_golden.py's
`eq_hand` and in its format.  They live in a file of their own,
tests/golden/eq_hand_boundary.json (one case per line), because golden.json is
already as large as a committed file may be.  tests/test_eq_reference_cpu.py
checks the oracle against them, tests/test_gpu_eq_graph.py the drop-in.

Usage:  python tests/golden/make_golden_eq_hand.py  (where make_golden.py runs)
"""
import json
import os

from make_golden import HERE, eq_case, import_reference


def cases():
    eqh = {}
    # a class past the per-thread size of the device's pair kernel, one member listed twice
    big = [str(i) for i in range(33)] + ["5"]
    eqh["class_of_34_one_duplicate"] = ("40\n2\n" + "".join(f"k{i}\n" for i in range(40)) + "34\t" + "\t".join(big)
                                        + "\t3\n2\t38\t5\t4\n", [f">k{i}" for i in range(40)])
    # a-b goes to 0 and a later class revives it: its place among a's edges is its first emission
    eqh["zero_sum_pair_revived"] = ("4\n6\na\nb\nc\nd\n2\t0\t2\t3\n2\t1\t0\t4\n2\t0\t3\t5\n2\t0\t1\t-4\n2\t1\t2\t2\n"
                                    "2\t0\t1\t6\n", [">a", ">b", ">c", ">d"])
    # a-c ends at 0 between the kept a-b and a-d
    eqh["zero_sum_pair_between_kept"] = ("4\n5\na\nb\nc\nd\n2\t0\t1\t5\n2\t0\t2\t7\n2\t0\t3\t2\n2\t2\t0\t-7\n2\t2\t3\t1\n",
                                         [">a", ">b", ">c", ">d"])
    eqh["size_token_1_three_members"] = ("3\n2\na\nb\nc\n1\t0\t1\t2\t9\n3\t2\t0\t1\t4\n", [">a", ">b", ">c"])
    return eqh


def main():
    _, RG, _, scratch = import_reference()
    out = {k: {"text": t, "fasta": f, "out": eq_case(RG, t, f, scratch, k)} for k, (t, f) in cases().items()}
    path = os.path.join(HERE, "eq_hand_boundary.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in out.items())
                + "\n}\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
