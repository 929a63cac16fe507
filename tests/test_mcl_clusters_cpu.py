"""karma_mcl_clusters without a device: the library's host tail of MCL
(csrc/mcl_clusters.cpp) against the model's interpret (tests/mcl_reference.py)
on final matrices of the model and on hand-made ones for every rule; the same
cases through the stand-alone program under AddressSanitizer + UBSan; and the
text handling of karma_amd.mcl (parsing, the stdout text) as far as it needs no
device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mcl_reference as ref
from karma_amd import _lib, engine
from karma_amd import mcl as kmcl

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "karma_amd", "csrc")


def _model_matrix(edges, n, rng=None, **kw):
    off, nbr, w = ref.csr_from_edges(n, edges, rng)
    return ref.mcl(off, nbr, w, **kw)[:3]


def _cases():
    """name -> (colptr, rows, vals)."""
    rng = np.random.default_rng(17)
    cases = {}
    edges, truth = ref.cliques([1, 2, 3, 4, 5, 6, 9, 12, 20], rng)
    cases["cliques"] = _model_matrix(edges, len(truth))
    cases["cliques_r32_i14"] = _model_matrix(edges, len(truth), resource=32, inflation=1.4)
    edges, truth = ref.cliques([1, 2, 3, 4, 5, 6, 9, 12, 20])
    cases["uniform_cliques"] = _model_matrix(edges, len(truth), resource=32)  # a clique: a system of all its members
    cases["uniform_cliques_r4"] = _model_matrix(edges, len(truth))  # ... of its 4 smallest members
    edges, _ = ref.planted(300, rng)
    cases["planted"] = _model_matrix(edges, 300, rng)
    for it in (1, 2, 3):  # stopped early: wide columns, systems of several attractors
        cases[f"planted_stop_{it}"] = _model_matrix(edges, 300, rng, max_iter=it)
        cases[f"star_stop_{it}"] = _model_matrix(ref.star_chain(60), 60, max_iter=it)
    cases["star"] = _model_matrix(ref.star_chain(60), 60)
    cases["n_1"] = ref.to_csc([[(0, 1.0)]])
    cases["system_of_two"] = ref.to_csc([[(0, 0.5), (1, 0.5)], [(0, 0.5), (1, 0.5)], [(1, 1.0)]])
    cases["one_way_system"] = ref.to_csc([[(0, 1.0)], [(0, 0.25), (1, 0.75)]])
    cases["equal_mass_tie"] = ref.to_csc([[(0, 0.5), (1, 0.5)], [(0, 0.5), (1, 0.5)], [(2, 1.0)],
                                          [(1, 0.5), (2, 0.5)]])
    cases["mass_is_summed"] = ref.to_csc([[(0, 0.5), (1, 0.5)], [(0, 0.5), (1, 0.5)], [(2, 1.0)],
                                          [(0, 0.25), (1, 0.25), (2, 0.5)]])
    # the in-order sum decides: 0.1 + 0.2 is above 0.3 in f64
    cases["mass_in_order"] = ref.to_csc([[(0, 0.5), (1, 0.5)], [(0, 0.5), (1, 0.5)], [(2, 1.0)],
                                         [(0, 0.1), (1, 0.2), (2, 0.3)]])
    cases["no_attractor_entry"] = ref.to_csc([[(0, 1.0)], [(2, 1.0)], [(1, 1.0)], [(0, 0.1), (1, 0.9)]])
    cases["label_order"] = ref.to_csc([[(0, 1.0)], [(1, 1.0)], [(1, 1.0)], [(4, 1.0)], [(4, 1.0)], [(4, 1.0)]])
    return cases


CASES = _cases()


def _library(colptr, rows, vals):
    n = len(colptr) - 1
    labels, count = np.full(n, -7, np.int32), ctypes.c_int32(-7)
    rc = _lib.load().karma_mcl_clusters(n, _lib.ptr(colptr), _lib.ptr(rows), _lib.ptr(vals), _lib.ptr(labels),
                                        ctypes.byref(count))
    return rc, labels, count.value


@pytest.mark.parametrize("name", sorted(CASES))
def test_library_equals_the_model(name):
    colptr, rows, vals = CASES[name]
    want, want_count = ref.interpret(colptr, rows, vals)
    rc, labels, count = _library(colptr, rows, vals)
    assert rc == _lib.KARMA_OK
    assert count == want_count and np.array_equal(labels, want)
    got, got_count = engine.mcl_clusters(colptr, rows, vals)
    assert got_count == want_count and np.array_equal(got, want)


def test_the_cases_cover_the_rules():
    """The inputs show what they are there for (judged by the model)."""
    def systems(name):
        cols = ref.from_csc(*CASES[name])
        att = [j for j, c in enumerate(cols) if any(i == j for i, _ in c)]
        return cols, att

    labels, count = ref.interpret(*CASES["uniform_cliques"])
    cols, att = systems("uniform_cliques")
    assert len(att) == len(cols) and count == 9  # all members attractors, one system per clique
    assert list(ref.interpret(*CASES["equal_mass_tie"])[0]) == [0, 0, 1, 0]
    assert list(ref.interpret(*CASES["mass_is_summed"])[0]) == [0, 0, 1, 0]
    assert 0.1 + 0.2 > 0.3 and list(ref.interpret(*CASES["mass_in_order"])[0]) == [0, 0, 1, 0]
    assert list(ref.interpret(*CASES["no_attractor_entry"])[0]) == [0, 1, 2, 0]
    assert list(ref.interpret(*CASES["label_order"])[0]) == [2, 1, 1, 0, 0, 0]
    assert ref.interpret(*CASES["n_1"])[1] == 1
    cols, att = systems("no_attractor_entry")
    assert any(not any(i in att for i, _ in c) for c in cols)  # a node with no attractor entry
    cols, att = systems("planted_stop_2")
    assert 0 < len(att) < len(cols)  # stopped early: followers and attractors both


def test_argument_errors():
    colptr, rows, vals = CASES["system_of_two"]
    for bad in ((np.array([1, 2, 3, 3], np.int64), rows, vals), (np.array([0, 2, 2, 5], np.int64), rows, vals),
                (colptr, np.array([0, 1, 0, 3, 1], np.uint32), vals), (colptr, np.array([1, 0, 0, 1, 1], np.uint32), vals)):
        rc, labels, count = _library(*bad)
        assert rc == _lib.KARMA_ERR_ARG and (labels == -7).all() and count == -7
        with pytest.raises(_lib.KarmaError) as e:
            engine.mcl_clusters(*bad)
        assert e.value.code == _lib.KARMA_ERR_ARG and "karma_mcl" in str(e.value)
    assert _lib.load().karma_mcl_clusters(3, None, _lib.ptr(rows), _lib.ptr(vals), None, None) == _lib.KARMA_ERR_ARG


def test_clusters_under_sanitizers(tmp_path):
    subprocess.run(["make", "-C", CSRC, "mcl_clusters_test"], check=True, capture_output=True)
    path = tmp_path / "cases.txt"
    with open(path, "w") as fh:
        for name in sorted(CASES):
            colptr, rows, vals = CASES[name]
            labels, count = ref.interpret(colptr, rows, vals)
            fh.write(f"{len(colptr) - 1} {len(rows)} {count}\n")
            fh.write(" ".join(str(int(v)) for v in colptr) + "\n")
            fh.write(" ".join(str(int(v)) for v in rows) + "\n")
            fh.write(" ".join(f"{int(v):x}" for v in vals.view(np.uint64)) + "\n")
            fh.write(" ".join(str(int(v)) for v in labels) + "\n")
    r = subprocess.run([os.path.join(CSRC, "build", "mcl_clusters_test"), str(path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(CASES)} cases from the file" in r.stdout and r.stdout.strip().splitlines()[-1].startswith("ok (")


def test_clusters_source_is_host_only():
    text = open(os.path.join(CSRC, "mcl_clusters.cpp")).read()
    assert "#include <hip" not in text and "karma_internal.h\"" not in text


# ---- the text side of karma_amd.mcl (no device) -------------------------------------------

def test_parse_abc():
    names, off, nbr, w = kmcl.parse_abc("b a 0.5\nc c 2.0\na d 0.25\n\nd b 1e-3\n")
    assert names == ["b", "a", "c", "d"]  # numbered by first appearance; the self-loop line only makes c present
    assert list(off) == [0, 2, 4, 4, 6]
    assert [sorted(nbr[off[j]:off[j + 1]].tolist()) for j in range(4)] == [[1, 3], [0, 3], [], [0, 1]]
    weights = {(j, int(i)): float(x) for j in range(4) for i, x in zip(nbr[off[j]:off[j + 1]], w[off[j]:off[j + 1]])}
    assert weights == {(0, 1): 0.5, (1, 0): 0.5, (1, 3): 0.25, (3, 1): 0.25, (3, 0): 1e-3, (0, 3): 1e-3}
    assert nbr.dtype == np.uint32 and off.dtype == np.int64 and w.dtype == np.float64
    # bytes as edge_list() gives them; no trailing newline
    assert kmcl.parse_abc(b"x y 0.1")[0] == ["x", "y"]
    assert kmcl.parse_abc("")[0] == []
    # repr(float) round-trips
    x = 0.1 + 0.2
    assert kmcl.parse_abc(f"p q {x!r}")[3][0] == x


def test_parse_abc_errors():
    for text in ("a b 1.0\nb a 2.0\n", "a b 1.0\na b 1.0\n"):
        with pytest.raises(ValueError, match="twice"):
            kmcl.parse_abc(text)
    with pytest.raises(ValueError):
        kmcl.parse_abc("a b\n")
    with pytest.raises(ValueError):
        kmcl.parse_abc("a b c d\n")
    with pytest.raises(ValueError):
        kmcl.parse_abc("a b heavy\n")
    assert kmcl.parse_abc("a a 1.0\na a 2.0\n")[0] == ["a"]  # a loop line twice: still only present


def test_cluster_text_and_its_consumer():
    names = ["k1", "k2", "k3", "k4", "k5"]
    text = kmcl.cluster_text(np.array([1, 0, 0, 1, 2], np.int32), 3, names)
    assert text == "k2\tk3\nk1\tk4\nk5\n"
    from karma_amd.read_graph import ReadGraph

    g = ReadGraph()
    g.add_nodes_from(names)
    leftovers = g.get_contigs_not_in_mcl_cluster_stdout(text, original_contigs=["k1", "k5"])
    assert sorted(leftovers) == ["k2", "k3"]
    assert sorted(sorted(c) for c in g.mcl_cluster) == [["k1", "k4"], ["k5"]]
    assert kmcl.cluster_text(np.zeros(0, np.int32), 0, []) == ""


def test_mcl_class_keeps_the_reference_names():
    m = kmcl.Mcl(threads=8, inflation="2.0")
    assert m.threads == 8 and m.inflation == 2.0 and kmcl.RESOURCE == 4
    assert callable(m.run_pipe) and callable(m.run)
    assert m.run_pipe("") == ""  # nothing to cluster: no device is reached
    source = open(os.path.join(REPO, "karma_amd", "mcl.py")).read()
    assert "subprocess" not in source and "Cmd(" not in source
