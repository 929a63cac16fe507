"""Drop-in for karma/mcl.py: Markov clustering without the `mcl` binary.

The reference pipes ReadGraph.edge_list() into `mcl - -I <inflation> --abc -o -
-te <threads> -resource 4 -V all` (mcl.py:48-51) and reads the clusters from its
stdout.  Here the abc text is parsed on the host, the process runs on the
device (engine.mcl, resource 4) and the clusters are written back as the text
the binary's stdout would carry: one line per cluster, members tab-separated,
each line ending with a newline.  No `which mcl`, no child process.

The clusters are those of this library's own, bit-defined process
(include/karma.h); they are not claimed to equal the binary's (its pruning is
richer and has a tie order of its own).  ReadGraph.mcl is the route without
text.
"""

from __future__ import annotations

import os

import numpy as np

from .logs import logger

RESOURCE = 4  # mcl.py:30, :49: -resource 4


def parse_abc(text):
    """abc text ("A B w" per line, one undirected edge each) -> (names, off,
    nbr, w): names numbered by first appearance, the graph as symmetric CSR
    (karma_adj_get's layout).  An "A A w" line only makes A present; a repeated
    pair raises ValueError."""
    if isinstance(text, (bytes, bytearray)):
        text = bytes(text).decode("utf-8")
    number, names, seen = {}, [], set()
    ea, eb, ew = [], [], []
    for lineno, line in enumerate(text.split("\n"), 1):
        tok = line.split()
        if not tok:
            continue
        if len(tok) != 3:
            raise ValueError(f"line {lineno}: expected 'A B weight', not {line!r}")
        a, b = (number.setdefault(t, len(number)) for t in tok[:2])
        for t in tok[:2]:
            if number[t] == len(names):
                names.append(t)
        weight = float(tok[2])
        if a == b:
            continue
        pair = (min(a, b), max(a, b))
        if pair in seen:
            raise ValueError(f"line {lineno}: the pair {tok[0]} {tok[1]} is given twice")
        seen.add(pair)
        ea.append(a)
        eb.append(b)
        ew.append(weight)
    n = len(names)
    a, b, wt = np.array(ea, np.int64), np.array(eb, np.int64), np.array(ew, np.float64)
    src, dst, ww = np.r_[a, b], np.r_[b, a], np.r_[wt, wt]
    order = np.argsort(src, kind="stable")
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=off[1:])
    return names, off, dst[order].astype(np.uint32), ww[order]


def cluster_text(labels, n_clusters, names):
    """The binary's stdout for these clusters: a line per cluster in label
    order, members tab-separated in the order of their numbers."""
    members = [[] for _ in range(n_clusters)]
    for j, lab in enumerate(np.asarray(labels).tolist()):
        members[lab].append(str(names[j]))
    return "".join("\t".join(m) + "\n" for m in members)


class Mcl:
    """Run MCL clustering on a given graph (karma/mcl.py's names and arguments)."""

    def __init__(self, threads, inflation):
        self.threads = threads  # the device needs no thread count; kept for the callers' sake
        self.inflation = float(inflation)

    def run_pipe(self, graph_file):
        """graph_file: the abc text itself (ReadGraph.edge_list()), as the
        reference passes it to the binary's stdin.  Returns the stdout text."""
        from . import engine

        logger.debug("MCL clustering...")
        names, off, nbr, w = parse_abc(graph_file)
        if not names:
            return ""
        colptr, rows, vals, _, _ = engine.mcl(off, nbr, w, inflation=self.inflation, resource=RESOURCE)
        labels, count = engine.mcl_clusters(colptr, rows, vals)
        return cluster_text(labels, count, names)

    def run(self, graph_file, output_file):
        """graph_file: the path of an abc file; the clusters go to output_file."""
        logger.debug("MCL clustering...")
        if os.path.exists(output_file):
            os.remove(output_file)
        with open(graph_file, "r", encoding="utf-8") as fh:
            text = self.run_pipe(fh.read())
        with open(output_file, "w", encoding="utf-8") as fh:
            fh.write(text)
