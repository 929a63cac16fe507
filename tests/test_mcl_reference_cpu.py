"""The MCL model itself (tests/mcl_reference.py): it must be a usable MCL before
it judges the device -- planted groups come back, a uniform clique converges
in one iteration, a hub's first iteration is as wide as the contract says."""

import numpy as np
import pytest

import mcl_reference as ref

SIZES = [1, 2, 3, 4, 5, 6, 9, 12, 20]


@pytest.mark.parametrize("resource", [2, 4, 8, 32])
@pytest.mark.parametrize("inflation", [1.4, 2.0, 6.0])
def test_cliques_recovered(resource, inflation):
    edges, truth = ref.cliques(SIZES, np.random.default_rng(11))
    off, nbr, w = ref.csr_from_edges(len(truth), edges)
    colptr, rows, vals, it, chaos = ref.mcl(off, nbr, w, inflation=inflation, resource=resource)
    assert chaos < 1e-3 and it < 100
    labels, count = ref.interpret(colptr, rows, vals)
    assert count == len(SIZES)
    assert ref.pair_agreement(labels, truth) == 1.0
    # label order: size descending
    assert [int(np.sum(labels == c)) for c in range(count)] == sorted(SIZES, reverse=True)


def test_uniform_cliques_one_iteration():
    edges, truth = ref.cliques(SIZES)
    off, nbr, w = ref.csr_from_edges(len(truth), edges)
    for resource in (4, 32):
        colptr, rows, vals, it, chaos = ref.mcl(off, nbr, w, resource=resource)
        assert it == 1 and chaos <= 2.0 ** -55
        labels, count = ref.interpret(colptr, rows, vals)
        assert count == len(SIZES) and ref.pair_agreement(labels, truth) == 1.0


@pytest.mark.parametrize("n", [300, 2000])
def test_planted_groups(n):
    edges, truth = ref.planted(n, np.random.default_rng(5))
    off, nbr, w = ref.csr_from_edges(n, edges, np.random.default_rng(6))
    colptr, rows, vals, it, chaos = ref.mcl(off, nbr, w)
    assert chaos < 1e-3
    labels, _ = ref.interpret(colptr, rows, vals)
    share = ref.pair_agreement(labels, truth)
    print(f"n = {n}: {it} iterations, pair agreement {share:.6f}")
    assert share >= 0.99


def test_star_first_iteration_is_wide():
    n = 400
    off, nbr, w = ref.csr_from_edges(n, ref.star_chain(n))
    *_, counts = ref.mcl(off, nbr, w, max_iter=2, with_counts=True)
    assert counts[0] > 100 * int(off[-1])
    assert counts[1] <= 16 * n  # from then on at most R * R per column


def test_interpret_rules():
    # two attractors in one system, a node split evenly between two systems, a node with no attractor entry
    cols = [[(0, 0.5), (1, 0.5)], [(0, 0.5), (1, 0.5)], [(2, 1.0)], [(1, 0.5), (2, 0.5)], [(3, 1.0)], [(6, 1.0)],
            [(5, 1.0)]]
    labels, count = ref.interpret(*ref.to_csc(cols))
    # systems {0, 1} and {2}; nodes 4, 5 and 6 name no attractor: each a cluster of its own
    assert labels[0] == labels[1] == labels[3]  # the tie goes to the system with the smallest attractor
    assert labels[2] != labels[0]
    assert len({labels[4], labels[5], labels[6], labels[0], labels[2]}) == 5
    assert count == 5
    assert list(labels[:4]) == [0, 0, 1, 0]
