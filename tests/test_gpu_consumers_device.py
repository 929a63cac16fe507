"""The device adjacency layer (karma_amd/csrc/consumers.hip, repr.h, and
sort.hip under them) tested directly through consumers.DeviceAdj and
consumers.NameTable, against the networkx model of tests/adj_reference.py
(pinned to networkx on the CPU by tests/test_adj_reference_cpu.py).

  a. repr(float) on both device paths (repr_f64 in the edge-list kernels,
     parts / parts_write in the one-launch view summary) over the f64 range;
  b. the view summary's four budgets (1,024 nodes, 4,096 entries, 16,384 name
     bytes, 24,576 text bytes), each exactly at the limit and one past it;
  c. from_edges / view / keep at the scan and radix tile edges and past the
     scan's 64-tile look-back window;
  d. cross_sums with keys over the whole int32 range and order-sensitive sums;
  e. karma_adj_edge_list's length-query / copy protocol.
Every comparison is exact: bytes, uint64 views of f64, integer arrays.
"""
import ctypes

import numpy as np
import pytest

import adj_reference as R
from karma_amd import _lib
from karma_amd._lib import KarmaError, call, ptr
from karma_amd.consumers import DeviceAdj, NameTable

pytestmark = pytest.mark.gpu

MAX_NODES, MAX_ENTRIES, MAX_NAME_BYTES, MAX_TEXT_BYTES = 1024, 4096, 16384, 24576


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def assert_layout(got, want, what=""):
    for name, g, w in zip(("ids", "off", "nbr"), got, want):
        assert np.array_equal(g, w), f"{what}: {name} differ"
    assert np.array_equal(bits(got[3]), bits(want[3])), f"{what}: weights differ"


def assert_stats(got, want, what=""):
    assert np.array_equal(got[0], want[0]), f"{what}: degrees differ"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{what}: node weights differ"


def device(layout):
    ids, off, nbr, w = layout
    return DeviceAdj.from_lists(off, nbr, w, ids=ids)


def simple_edges(rng, n, E, loops=0, hub=None):
    """E distinct unordered pairs on n nodes in random order and orientation,
    `loops` of them self-loops; hub = (node, degree): that many of them at one node."""
    a = np.zeros(0, np.int64)
    b = np.zeros(0, np.int64)
    if hub is not None:
        others = rng.permutation(n - 1)[:hub[1]]
        others = others + (others >= hub[0])
        a, b = np.full(hub[1], hub[0], np.int64), others.astype(np.int64)
    la = rng.choice(n, loops, replace=False) if loops else np.zeros(0, np.int64)
    seen = set(((np.minimum(a, b) << 32) | np.maximum(a, b)).tolist())
    need = E - loops - len(a)
    xs, ys = [], []
    while need > 0:
        x = rng.integers(0, n, 2 * need + 16)
        y = rng.integers(0, n, 2 * need + 16)
        for p, q in zip(x.tolist(), y.tolist()):
            key = (min(p, q) << 32) | max(p, q)
            if p == q or key in seen:
                continue
            seen.add(key)
            xs.append(p), ys.append(q)
            need -= 1
            if need == 0:
                break
    a = np.concatenate([a, la, np.array(xs, np.int64)])
    b = np.concatenate([b, la, np.array(ys, np.int64)])
    flip = rng.random(len(a)) < 0.5
    a, b = np.where(flip, b, a), np.where(flip, a, b)
    o = rng.permutation(len(a))
    assert len(a) == E
    return a[o], b[o]


def ascii_names(rng, n, lo=2, hi=6):
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789_", np.uint8)
    return [bytes(letters[rng.integers(0, len(letters), int(rng.integers(lo, hi + 1)))]).decode() for _ in range(n)]


# ---- a. repr(float) on both device paths -------------------------------------------
SPECIALS = [0.0, -0.0, 1.0, -1.0, 0.5, 0.1, 0.2, 0.3, 2.0 / 3, 1e16, 1e15, 9999999999999998.0, 1e-4, 9.999e-5,
            1e-5, 0.0001234, 5e-324, 2.2250738585072014e-308, 2.225073858507201e-308, 1.7976931348623157e308,
            float("inf"), -float("inf"), float("nan"), 9007199254740993.0, 123456789012345678.0, 1e22, 1e23,
            1e100, 1e-100, 1e-7, 1234.5, 0.1 + 0.2]  # test_repr_cpu.py::test_special_values_and_layout_boundaries
DECPT = [9.999999999999999e-05, 0.0001, 9999999999999998.0, 1e16, 1.2345678901234567e+16]
N_RANDOM, N_RANDOM_SUMMARY = 20_000, 2_000


@pytest.fixture(scope="module")
def repr_corpus():
    """(values, layout, names, table, adjacency, how many leading values go
    through the summary path): x_i is the weight of edge (2i, 2i + 1)."""
    pow2 = 2.0 ** np.arange(-1074, 1024, dtype=np.float64)
    pow10 = np.array([float(f"1e{e}") for e in range(-323, 309)])
    near = np.concatenate([np.nextafter(pow2, -np.inf), np.nextafter(pow2, np.inf)])
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000000], np.uint64).view(np.float64)
    rnd = np.random.default_rng(71).integers(0, 2**64, N_RANDOM, dtype=np.uint64).view(np.float64)
    head = np.concatenate([SPECIALS, DECPT, [np.inf, -np.inf], nans, pow2, pow10, near, -pow2[::7], -pow10[::5]])
    x = np.concatenate([head, rnd])
    assert (np.signbit(rnd).sum() > N_RANDOM // 3) and (~np.signbit(rnd)).sum() > N_RANDOM // 3
    n = 2 * len(x)
    off = np.arange(n + 1, dtype=np.int64)
    nbr = np.arange(n, dtype=np.uint32) ^ np.uint32(1)
    layout = (np.arange(n, dtype=np.uint32), off, nbr, np.repeat(x, 2))
    names = ascii_names(np.random.default_rng(72), n)
    return x, layout, names, NameTable(names), device(layout), len(head) + N_RANDOM_SUMMARY


def test_repr_general_path_whole_f64_range(repr_corpus):
    x, layout, names, table, adj, _ = repr_corpus
    want = R.edge_lines(layout, names)
    got = adj.edge_list(table).split(b"\n")
    assert len(want) == len(x) == len(got)
    bad = [(float(v).hex(), w, g) for v, w, g in zip(x.tolist(), want, got) if w != g]
    print(f"repr general path (repr_f64): {len(x)} values, {len(bad)} differ")
    assert not bad, bad[:5]
    assert_stats(adj.node_stats(), R.node_stats(layout), "matching")


def test_repr_summary_path_whole_f64_range(repr_corpus):
    x, layout, names, table, adj, n_sum = repr_corpus
    lines = R.edge_lines(layout, names)
    cost = [len(s) + 1 for s in lines]
    chunks, cur, used = [], [], 0
    for i in range(n_sum):  # greedy, from the model's own byte counts
        if used + cost[i] > MAX_TEXT_BYTES or 2 * (len(cur) + 1) > MAX_NODES:
            chunks.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += cost[i]
    chunks.append(cur)
    rng = np.random.default_rng(73)
    for c, chunk in enumerate(chunks):
        e = np.array(chunk, np.int64)
        if c % 2:
            e = rng.permutation(e)
        order = np.stack([2 * e, 2 * e + 1], 1)
        if c % 3 == 1:
            order = order[:, ::-1]  # the odd end first: the line is written from it
        order = order.ravel()
        v = R.view(layout, order)
        assert R.text_bytes(v, names) <= MAX_TEXT_BYTES and len(order) <= MAX_NODES
        r = adj.view_summary(order, table, True)
        assert r is not None, f"chunk {c} ({len(order)} nodes) was not served by the summary"
        want = R.edge_lines(v, names)
        got = r[2].split(b"\n")
        bad = [(w, g) for w, g in zip(want, got) if w != g]
        assert len(want) == len(got) and not bad, (c, bad[:5])
        assert_stats(r[:2], R.node_stats(v), f"chunk {c}")
    print(f"repr summary path (parts / parts_write): {n_sum} values in {len(chunks)} launches")
    assert sum(len(c) for c in chunks) == n_sum


# ---- b. the summary's budgets -------------------------------------------------------
def check_view(layout, adj, order, names, table, with_text, served, what):
    """General path == model; summary == general path when served, None when over.
    Returns the model's view layout."""
    v = R.view(layout, order)
    g = adj.view(order)
    assert_layout(g.layout(), v, what)
    stats = g.node_stats()
    assert_stats(stats, R.node_stats(v), what)
    text = g.edge_list(table)
    assert text == R.edge_list(v, names), f"{what}: edge list differs from the model"
    r = adj.view_summary(order, table, with_text)
    if not served:
        assert r is None, f"{what}: over the limit but served by the summary"
        return v
    assert r is not None, f"{what}: at the limit but not served by the summary"
    assert_stats(r[:2], stats, f"{what} (summary)")
    assert r[2] == (text if with_text else None), f"{what}: summary text differs from the general path"
    return v


def measures(v, names):
    return len(v[0]), len(v[2]), R.name_bytes(v, names), R.text_bytes(v, names)


@pytest.fixture(scope="module")
def path_graph():
    """1,300 nodes in a path, scattered over the positions: no budget but the node count binds."""
    rng = np.random.default_rng(81)
    n = 1300
    walk = rng.permutation(n)
    layout = R.from_edges(n, walk[:-1], walk[1:], rng.integers(1, 64, n - 1) / 64.0, ids=rng.permutation(n))
    names = ascii_names(rng, n, 1, 4)
    return layout, device(layout), names, NameTable(names), walk


@pytest.mark.parametrize("k,served", [(1024, True), (1025, False), (1, True)])
def test_summary_node_budget(path_graph, k, served):
    layout, adj, names, table, walk = path_graph
    for how in ("walk", "reversed", "shuffled"):
        order = walk[100:100 + k]
        order = {"walk": order, "reversed": order[::-1], "shuffled": np.random.default_rng(k).permutation(order)}[how]
        v = check_view(layout, adj, order, names, table, True, served, f"{k} nodes {how}")
        nodes, entries, nb, tb = measures(v, names)
        assert nodes == k and entries == 2 * (k - 1)
        assert nb <= MAX_NAME_BYTES and tb <= MAX_TEXT_BYTES  # nothing else binds
        check_view(layout, adj, order, names, table, False, served, f"{k} nodes {how}, no text")


def test_summary_view_without_edges(path_graph):
    layout, adj, names, table, walk = path_graph
    order = walk[0:2 * MAX_NODES:2][:MAX_NODES]  # every other node of the path
    order = np.concatenate([order[:600], order[600:650][::-1]])
    v = check_view(layout, adj, order, names, table, True, True, "edgeless view")
    assert measures(v, names)[1] == 0
    r = adj.view_summary(order, table, True)
    assert r[2] == b"" and not r[0].any() and not bits(r[1]).any()
    r = adj.view_summary(np.zeros(0, np.int64), table, True)
    assert r is not None and len(r[0]) == 0 and len(r[1]) == 0 and r[2] == b""


def ring(n, steps):
    u = np.arange(n)
    return np.concatenate([u] * len(steps)), np.concatenate([(u + s) % n for s in steps])


@pytest.mark.parametrize("extra,entries,served", [(None, 4096, True), ("loop", 4097, False), ("chord", 4098, False)])
def test_summary_entry_budget_without_text(extra, entries, served):
    rng = np.random.default_rng(82)
    n = MAX_NODES
    a, b = ring(n, (1, 2))
    if extra == "loop":
        a, b = np.r_[a, 500], np.r_[b, 500]
    if extra == "chord":
        a, b = np.r_[a, 10], np.r_[b, 700]
    o = rng.permutation(len(a))
    layout = R.from_edges(n, a[o], b[o], rng.standard_normal(len(a)), ids=rng.permutation(n))
    adj = device(layout)
    names = ascii_names(rng, n, 1, 3)
    table = NameTable(names)
    for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n)):
        v = check_view(layout, adj, order, names, table, False, served, f"{entries} entries")
        assert measures(v, names)[:2] == (n, entries)


@pytest.mark.parametrize("extra,entries,served", [(None, 4096, True), ("loop", 4097, False), ("edge", 4098, False)])
def test_summary_entry_budget_with_text(extra, entries, served):
    """A 64-clique with one-byte names and 32 pendant edges: 4,032 + 64 entries,
    and 2,048 short lines, far under the text budget."""
    rng = np.random.default_rng(83)
    iu, ju = np.triu_indices(64, 1)
    a, b = np.r_[iu, np.arange(32)], np.r_[ju, 64 + np.arange(32)]
    if extra == "loop":
        a, b = np.r_[a, 70], np.r_[b, 70]
    if extra == "edge":
        a, b = np.r_[a, 70], np.r_[b, 71]
    n = 110  # 14 nodes outside the view
    place = rng.permutation(n)  # where each of them sits in the source graph
    o = rng.permutation(len(a))
    layout = R.from_edges(n, place[a[o]], place[b[o]], rng.integers(1, 32, len(a)) / 32.0)
    adj = device(layout)
    one = [chr(c) for c in range(0x21, 0x7F)]
    names = [None] * n
    for i in range(n):
        names[place[i]] = one[i % len(one)] if i < 64 else one[i % len(one)] + "é"
    table = NameTable(names)
    for order in (place[:96], place[:96][::-1], rng.permutation(place[:96])):
        v = check_view(layout, adj, order, names, table, True, served, f"{entries} entries with text")
        nodes, ent, nb, tb = measures(v, names)
        assert (nodes, ent) == (96, entries) and nb <= MAX_NAME_BYTES and tb < MAX_TEXT_BYTES


@pytest.mark.parametrize("total,served", [(16384, True), (16385, False)])
def test_summary_name_byte_budget(total, served):
    rng = np.random.default_rng(84)
    n, k = 1100, MAX_NODES
    names = ["αβγδ" + s for s in ascii_names(rng, n, 8, 8)]  # 16 bytes, 12 characters
    place = rng.permutation(n)
    view_nodes = place[:k]
    names[view_nodes[0]] = "é" * 150          # 300 bytes
    for u in view_nodes[1:12].tolist() + view_nodes[13:38].tolist():
        names[u] = "x"                        # 1 byte
    names[view_nodes[12]] = "日本語" + "q" * 248  # 257 bytes
    fixed = sum(len(names[u].encode()) for u in view_nodes[:-1])
    names[view_nodes[-1]] = "z" * (total - fixed)
    assert 1 <= total - fixed <= 64
    # a few edges, the long and the one-byte names among their ends, some leaving the view
    a = np.r_[view_nodes[0], view_nodes[1], view_nodes[12], view_nodes[-1], rng.choice(place, 40, replace=False)]
    b = np.r_[view_nodes[1], view_nodes[2], view_nodes[-1], view_nodes[-1], rng.choice(place, 40, replace=False)]
    keep = np.r_[np.ones(4, bool), a[4:] != b[4:]]
    layout = R.from_edges(n, a[keep], b[keep], rng.random(int(keep.sum())))
    adj = device(layout)
    table = NameTable(names)
    for order in (view_nodes, view_nodes[::-1], rng.permutation(view_nodes)):
        v = check_view(layout, adj, order, names, table, True, served, f"{total} name bytes")
        nodes, ent, nb, tb = measures(v, names)
        assert nb == total and nodes == k and ent <= MAX_ENTRIES and tb <= MAX_TEXT_BYTES
        assert sum(len(names[u]) for u in order) < nb  # characters and bytes differ
    # the name budget belongs to the text: without it the same view is served
    assert adj.view_summary(view_nodes, table, False) is not None


def text_budget_view(total):
    """A view whose text is exactly `total` bytes: a ring with +-1, +-2 of
    400 nodes with 17-digit weights, edges dropped until the text is just
    under, and a pendant node whose name length supplies the last bytes."""
    rng = np.random.default_rng(85)
    n = 401
    a, b = ring(400, (1, 2))
    o = rng.permutation(len(a))
    a, b = np.r_[a[o], 400], np.r_[b[o], 7]  # the pendant edge last: never dropped
    w = rng.random(len(a)) * 10.0 ** rng.integers(-8, 3, len(a))
    names = ascii_names(rng, n, 4, 6)
    names[400] = "p"
    E = len(a)
    while True:
        layout = R.from_edges(n, a[-E:], b[-E:], w[-E:])
        t0 = R.text_bytes(layout, names)
        if t0 <= total:
            break
        E -= max(1, (t0 - total) // 40)
    assert 0 <= total - t0 < 64
    names[400] = "p" * (1 + total - t0)  # in one line only: one byte of name, one byte of text
    return layout, names


@pytest.mark.parametrize("total,served", [(24576, True), (24577, False)])
def test_summary_text_byte_budget(total, served):
    layout, names = text_budget_view(total)
    adj, table = device(layout), NameTable(names)
    rng = np.random.default_rng(86)
    for order in (np.arange(401), np.arange(401)[::-1], rng.permutation(401)):
        v = check_view(layout, adj, order, names, table, True, served, f"{total} text bytes")
        nodes, ent, nb, tb = measures(v, names)
        assert tb == total and nodes <= MAX_NODES and ent <= MAX_ENTRIES and nb <= MAX_NAME_BYTES
    assert adj.view_summary(np.arange(401), table, False) is not None


def summary_abi(adj, order, table, text_cap, fill=0xA5):
    """karma_adj_view_summary with the caller's own text buffer and text_cap."""
    order = np.ascontiguousarray(order, np.int64)
    k = len(order)
    deg, w = np.full(k, -7, np.int64), np.full(k, -7.0)
    text = np.full(max(1, text_cap) + 64, fill, np.uint8)
    done, tl = ctypes.c_int(-1), _lib._i64(-1)
    dn, do = table.device()
    call("karma_adj_view_summary", adj.h, ptr(order), k, dn, do, 1, ptr(deg), ptr(w), ptr(text), text_cap,
         ctypes.byref(tl), ctypes.byref(done))
    return done.value, tl.value, text, deg, w


def test_summary_text_cap_reports_over_and_never_truncates(path_graph):
    layout, adj, names, table, walk = path_graph
    order = walk[200:260]
    v = R.view(layout, order)
    want = R.edge_list(v, names)
    assert 0 < len(want) < 2000
    for cap in (len(want) - 1, len(want) // 2, 1, 0):
        done, tl, text, deg, w = summary_abi(adj, order, table, cap)
        assert done == 0, f"text_cap {cap} < {len(want)} text bytes, but the summary was served"
        assert (text == 0xA5).all() and (deg == -7).all(), "an over-limit summary wrote results"
    done, tl, text, deg, w = summary_abi(adj, order, table, len(want) + 1)
    assert done == 1 and tl == len(want) and text[:tl].tobytes() == want
    assert (text[len(want) + 1:] == 0xA5).all(), "text written past text_cap"
    assert_stats((deg, w), R.node_stats(v), "text_cap")


def test_summary_hub_of_view_degree_1000_and_self_loops():
    rng = np.random.default_rng(87)
    n, hub = 1200, 333
    a, b = simple_edges(rng, n, 1400, loops=0, hub=(hub, 1100))
    order = np.r_[a[(a != hub) & (b == hub)], b[(a == hub) & (b != hub)]]
    order = rng.permutation(order)[:1000]
    order = np.r_[order[:480], hub, order[480:]]  # neighbours on both sides of the hub
    first, mid, last = order[0], order[700], order[-1]
    a, b = np.r_[a, first, mid, last, hub], np.r_[b, first, mid, last, hub]
    o = rng.permutation(len(a))
    layout = R.from_edges(n, a[o], b[o], rng.integers(-32, 32, len(a)) / 64.0, ids=rng.permutation(n))
    adj = device(layout)
    names = ascii_names(rng, n, 1, 3)
    table = NameTable(names)
    for order_ in (order, order[::-1], rng.permutation(order)):
        v = check_view(layout, adj, order_, names, table, True, True, "hub view")
        deg = np.diff(v[1])
        assert measures(v, names)[1] <= MAX_ENTRIES and measures(v, names)[3] <= MAX_TEXT_BYTES
        assert deg.max() == 1001 and len(order_) == 1001  # 1,000 neighbours and its own loop
        assert int((v[2] == np.repeat(np.arange(len(deg)), deg)).sum()) == 4  # the four self-loops
        check_view(layout, adj, order_, names, table, False, True, "hub view, no text")


def test_summary_bad_order_raises_and_context_stays_usable(path_graph):
    layout, adj, names, table, walk = path_graph
    good = walk[300:340].copy()
    want = R.view(layout, good)
    for bad in (np.r_[good, good[5]], np.r_[good[:7], -1, good[7:]], np.r_[good, len(walk)], np.r_[good, 2**40]):
        with pytest.raises(KarmaError):
            adj.view_summary(bad, table, True)
        with pytest.raises(KarmaError):
            adj.view_summary(bad, table, False)
        r = adj.view_summary(good, table, True)
        assert r is not None and r[2] == R.edge_list(want, names)
        assert_stats(r[:2], R.node_stats(want), "after a bad order")
        assert_layout(adj.view(good).layout(), want, "after a bad order")


# ---- c. layout kernels at the scan and sort tile edges ------------------------------
@pytest.mark.parametrize("loops", [0, 1, 3])
@pytest.mark.parametrize("E", [2047, 2048, 2049, 4095, 4096, 4097])
def test_from_edges_at_tile_edges(E, loops):
    """2 E - loops entries around one 4,096-key radix tile (E near 2,048) and
    E + 1 = n + 1 scanned items around one 4,096-item scan tile (E near 4,096)."""
    rng = np.random.default_rng(E * 10 + loops)
    n = E
    a, b = simple_edges(rng, n, E, loops=loops)
    w = rng.standard_normal(E)
    ids = rng.permutation(n)
    want = R.from_edges(n, a, b, w, ids)
    g = DeviceAdj.from_edges(n, a, b, w, ids=ids)
    assert g.m == 2 * E - loops == len(want[2])
    assert_layout(g.layout(), want, f"from_edges E={E}")
    assert_stats(g.node_stats(), R.node_stats(want), f"from_edges E={E}")
    mask = rng.random(n) < 0.7
    assert_layout(g.keep(mask).layout(), R.keep(want, mask), f"keep E={E}")
    order = rng.permutation(n)[:n - 1]
    assert_layout(g.view(order).layout(), R.view(want, order), f"view E={E}")


def test_layouts_past_the_scan_look_back_window():
    """n + 1 = 270,001 scanned items: 66 tiles of 4,096, past the 64-tile window."""
    rng = np.random.default_rng(91)
    n, E, hub = 270_000, 140_000, 123_456
    assert -(-(n + 1) // 4096) == 66
    a, b = simple_edges(rng, n, E, loops=50, hub=(hub, 5000))
    w = rng.random(E)
    want = R.from_edges(n, a, b, w)
    g = DeviceAdj.from_edges(n, a, b, w)
    assert_layout(g.layout(), want, "from_edges")
    assert np.diff(want[1])[hub] >= 5000
    mask = rng.random(n) < 0.8
    mask[hub] = True
    kept = R.keep(want, mask)
    gk = g.keep(mask)
    assert_layout(gk.layout(), kept, "keep")
    assert_stats(gk.node_stats(), R.node_stats(kept), "keep")
    # a shuffled view of 100,000 nodes with the hub and all its neighbours
    around = np.unique(np.r_[hub, want[2][want[1][hub]:want[1][hub + 1]]])
    rest = np.setdiff1d(np.arange(n), around)
    order = rng.permutation(np.r_[around, rng.permutation(rest)[:100_000 - len(around)]])
    v = R.view(want, order)
    assert len(order) == 100_000 and np.diff(v[1]).max() >= 5000
    assert_layout(g.view(order).layout(), v, "view")


def test_view_of_keep_of_view():
    rng = np.random.default_rng(92)
    n = 3000
    a, b = simple_edges(rng, n, 9000, loops=40)
    w = rng.standard_normal(len(a))
    names = ascii_names(rng, n)
    table = NameTable(names)
    lay = R.from_edges(n, a, b, w, ids=rng.permutation(n))
    g = DeviceAdj.from_edges(n, a, b, w, ids=lay[0])
    o1 = rng.permutation(n)[:2200]
    lay, g = R.view(lay, o1), g.view(o1)
    mask = rng.random(2200) < 0.75
    lay, g = R.keep(lay, mask), g.keep(mask)
    o2 = rng.permutation(len(lay[0]))[:1500]
    lay, g = R.view(lay, o2), g.view(o2)
    deg = np.diff(lay[1])
    assert (lay[2] == np.repeat(np.arange(len(deg)), deg)).sum() >= 5  # self-loops survived
    assert_layout(g.layout(), lay, "three levels")
    assert_stats(g.node_stats(), R.node_stats(lay), "three levels")
    assert np.array_equal(g.degrees(), deg) and np.array_equal(bits(g.node_weights()), bits(R.node_stats(lay)[1]))
    assert g.edge_list(table) == R.edge_list(lay, names)


def through_every_accessor(g, lay, names, table):
    assert g.n == len(lay[0]) and g.m == len(lay[2])
    assert_layout(g.layout(), lay)
    want = R.node_stats(lay)
    assert_stats(g.node_stats(), want)
    assert np.array_equal(g.degrees(), want[0]) and np.array_equal(bits(g.node_weights()), bits(want[1]))
    assert g.edge_list(table) == R.edge_list(lay, names)
    sub = np.arange(g.n, dtype=np.int32) % 3
    got = g.cross_sums(sub, np.arange(g.n, dtype=np.int32), 0.0)
    for x, y in zip(got, R.cross_sums(lay, sub, np.arange(g.n), 0.0)):
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                              y.view(np.uint64) if y.dtype == np.float64 else y)


def test_keep_masks_and_empty_layouts():
    rng = np.random.default_rng(93)
    n = 500
    a, b = simple_edges(rng, 300, 700, loops=5)  # nodes 300.. are isolated
    w = rng.random(len(a))
    names = ascii_names(rng, n)
    table = NameTable(names)
    lay = R.from_edges(n, a, b, w)
    g = DeviceAdj.from_edges(n, a, b, w)
    deg = np.diff(lay[1])
    assert (deg == 0).sum() >= 200
    for mask in (np.ones(n, np.uint8), np.zeros(n, np.uint8), (deg > 0).astype(np.uint8)):
        through_every_accessor(g.keep(mask), R.keep(lay, mask), names, table)
    none = np.zeros(0, np.int64)
    through_every_accessor(g.view(none), R.view(lay, none), names, table)  # k = 0
    e32, ef = np.zeros(0, np.uint32), np.zeros(0, np.float64)
    empty = R.from_edges(0, none, none, ef)
    for g0 in (DeviceAdj.from_edges(0, e32, e32, ef), DeviceAdj.from_lists(np.zeros(1, np.int64), e32, ef)):  # n = 0
        through_every_accessor(g0, empty, names, table)
        through_every_accessor(g0.view(none), empty, names, table)
        through_every_accessor(g0.keep(np.zeros(0, np.uint8)), empty, names, table)
        r = g0.view_summary(none, table, True)
        assert r is not None and r[2] == b"" and len(r[0]) == 0
    r = g.view_summary(none, table, False)
    assert r is not None and r[2] is None and len(r[0]) == 0 and len(r[1]) == 0


# ---- d. cross_sums ------------------------------------------------------------------
WIDE = [0, 1, 255, 256, 65535, 65536, 2**24 - 1, 2**24, 2**24 + 257, 2**31 - 1, 2**31 - 2, 0x7F00FF01, 0x01020304,
        0x00FF00FF]


def assert_cross(got, want, what=""):
    for name, g, w in zip(("A", "B", "sum", "n_edges", "n_over"), got, want):
        if name == "sum":
            g, w = bits(g), bits(w)
        assert np.array_equal(g, w), f"{what}: {name} differ"


@pytest.fixture(scope="module")
def cross_graph():
    """400 nodes, 9,000 edges, 14 subclusters whose indices and ranks spread
    over the whole non-negative int32 range (every radix digit varies), some
    nodes in none; more cross entries than one 4,096-key sort tile."""
    rng = np.random.default_rng(95)
    n = 400
    a, b = simple_edges(rng, n, 9000, loops=10)
    which = rng.integers(-1, len(WIDE), n)
    sub = np.where(which < 0, -1, np.array(WIDE)[which]).astype(np.int64)
    rank = np.zeros(n, np.int64)
    for s in WIDE:
        members = np.flatnonzero(sub == s)
        pool = np.unique(np.r_[WIDE, rng.integers(0, 2**31, 64)])  # distinct inside a subcluster
        rank[members] = rng.permutation(pool)[:len(members)]
    rank[sub < 0] = rng.integers(0, 2**31, int((sub < 0).sum()))
    return n, a, b, sub, rank


def test_cross_sums_order_sensitive_over_the_int32_range(cross_graph):
    n, a, b, sub, rank = cross_graph
    rng = np.random.default_rng(96)
    w = rng.choice([-1.0, 1.0], len(a)) * (1 + rng.random(len(a))) * 2.0 ** rng.integers(-40, 41, len(a))
    lay = R.from_edges(n, a, b, w)
    g = DeviceAdj.from_edges(n, a, b, w)
    want = R.cross_sums(lay, sub, rank, 0.0)
    assert want[3].sum() > 4096 and len(want[0]) == len(WIDE) * (len(WIDE) - 1) // 2
    # the fixture is order sensitive: the same weights summed in another order give other bits
    u = np.repeat(np.arange(n), np.diff(lay[1]))
    sel = np.flatnonzero((sub[u] == 0) & (sub[lay[2]] == 1))  # pair (0, 1), in adjacency order
    other = 0.0
    for x in lay[3][sel].tolist():
        other += x
    assert len(sel) == want[3][0] >= 3 and other != want[2][0]
    for cutoff in (0.0, -1e6, 1e-3, 2.0 ** 30, float("inf"), -float("inf")):
        assert_cross(g.cross_sums(sub, rank, cutoff), R.cross_sums(lay, sub, rank, cutoff), f"cutoff {cutoff}")
    assert not R.cross_sums(lay, sub, rank, float("inf"))[4].any()
    assert np.array_equal(R.cross_sums(lay, sub, rank, -float("inf"))[4], want[3])
    # through a shuffled view: the same pairs from another adjacency order
    order = rng.permutation(n)
    assert_cross(g.view(order).cross_sums(sub[order], rank[order], 0.5),
                 R.cross_sums(R.view(lay, order), sub[order], rank[order], 0.5), "view")


def test_cross_sums_strict_cutoff_on_exact_running_sums(cross_graph):
    n, a, b, sub, rank = cross_graph
    rng = np.random.default_rng(97)
    w = rng.integers(-2048, 4096, len(a)) / 1024.0  # dyadic: every running sum is exact
    lay = R.from_edges(n, a, b, w)
    g = DeviceAdj.from_edges(n, a, b, w)
    # the running sums of the largest pair, in the model's order
    A, B, S, N, _ = R.cross_sums(lay, sub, rank, 0.0)
    p = int(np.argmax(N))
    u = np.repeat(np.arange(n), np.diff(lay[1]))
    sel = np.flatnonzero((sub[u] == A[p]) & (sub[lay[2]] == B[p]))
    sel = sel[np.lexsort((rank[lay[2][sel]], rank[u[sel]]))]
    run = np.cumsum(lay[3][sel])
    assert run[-1] == S[p] and len(run) == N[p] >= 20
    for cutoff in (float(run[len(run) // 2]), float(run[3]), float(run.max()), float(run.min())):
        want = R.cross_sums(lay, sub, rank, cutoff)
        assert (run == cutoff).any() and want[4][p] == int((run > cutoff).sum()) < (run >= cutoff).sum()
        assert_cross(g.cross_sums(sub, rank, cutoff), want, f"cutoff {cutoff}")


def test_cross_sums_without_cross_edges(cross_graph):
    n, a, b, sub, rank = cross_graph
    g = DeviceAdj.from_edges(n, a, b, np.ones(len(a)))
    for s in (np.full(n, -1), np.full(n, 2**31 - 1), np.zeros(n, np.int64)):
        got = g.cross_sums(s, rank, 0.0)
        assert all(len(x) == 0 for x in got)
    # two components, one subcluster each side of no edge
    iso = DeviceAdj.from_edges(4, [0, 2], [1, 3], [1.0, 2.0])
    assert all(len(x) == 0 for x in iso.cross_sums([5, 5, 9, 9], [0, 1, 0, 1], 0.0))
    assert iso.cross_sums([5, 9, 9, 5], [0, 1, 0, 1], 0.0)[3].tolist() == [2]


# ---- e. karma_adj_edge_list's two calls ---------------------------------------------
def edge_list_abi(adj, table, out=None, cap=0):
    dn, do = table.device()
    n = _lib._i64(-1)
    call("karma_adj_edge_list", adj.h, dn, do, table.n, 1, ptr(out), cap, ctypes.byref(n))
    return n.value


def test_edge_list_length_query_then_copy():
    rng = np.random.default_rng(98)
    n = 700
    a, b = simple_edges(rng, n, 2000, loops=6)
    w = rng.random(len(a))
    lay = R.from_edges(n, a, b, w)
    g = DeviceAdj.from_edges(n, a, b, w)
    names1 = ascii_names(rng, n)
    names2 = [x[::-1] + "é" for x in names1]
    t1, t2 = NameTable(names1), NameTable(names2)
    want1, want2 = R.edge_list(lay, names1), R.edge_list(lay, names2)
    assert want1 != want2 and len(want1) != len(want2)
    L = len(want1)
    assert edge_list_abi(g, t1) == L
    assert edge_list_abi(g, t1) == L  # the length query twice in a row
    buf = np.full(L + 8, 0xA5, np.uint8)
    with pytest.raises(KarmaError):
        edge_list_abi(g, t1, buf, L - 1)  # one byte short
    assert (buf == 0xA5).all()
    assert edge_list_abi(g, t1, buf, L) == L  # and the next correct call
    assert buf[:L].tobytes() == want1 and (buf[L:] == 0xA5).all()
    assert g.edge_list(t1) == want1
    # a second table on the same adjacency, with the first one's length query still pending
    assert edge_list_abi(g, t1) == L
    assert edge_list_abi(g, t2) == len(want2)
    assert g.edge_list(t2) == want2
    assert g.edge_list(t1) == want1
