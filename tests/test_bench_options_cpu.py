"""bench.py's --full and --dump-outputs (CPU): a plain run switches every
measurement beside the headline off, --full leaves the choice to the older
options, and dump_outputs writes a fixed, seeded sample of a step's outputs as
float64 .npy files within its size budget."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_plain_run_measures_the_headline_only():
    a = load_bench().parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 2, False, None)
    assert a.no_timing and a.no_e2e and a.no_parity and a.no_other_format and a.no_weak_leg
    assert a.cpu_baseline == "off"


def test_full_run_keeps_the_older_options():
    b = load_bench()
    a = b.parse(["--full"])
    assert a.full and a.cpu_baseline == "full"
    assert not (a.no_timing or a.no_e2e or a.no_parity or a.no_other_format or a.no_weak_leg)
    a = b.parse(["--full", "--no-parity", "--cpu-baseline", "off", "--dump-outputs", "out"])
    assert a.no_parity and a.cpu_baseline == "off" and not a.no_timing and a.dump_outputs == "out"


class HostBuf:
    """The part of _lib.DevBuf that dump_outputs uses, over a host array."""

    def __init__(self, arr):
        self.arr, self.shape = arr, arr.shape

    def view(self, start, n):
        return HostBuf(self.arr.reshape(-1)[start:start + n])

    def numpy(self):
        return self.arr.copy()


def fake_step(rows, M, E, n_glob):
    rng = np.random.default_rng(5)
    prof = rng.random((rows, M))
    edges = SimpleNamespace(a=np.arange(E, dtype=np.uint32), b=np.arange(E, dtype=np.uint32) + 1,
                            shared=rng.integers(1, 1 << 40, E), weight=rng.random(E),
                            totals=rng.integers(0, 1 << 40, n_glob))
    leg = SimpleNamespace(build=SimpleNamespace(native=None), rank=0, world=1)
    return leg, {"profile": HostBuf(prof), "edges": edges}, prof, edges


def load_dir(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_small_outputs_are_written_whole(tmp_path):
    b = load_bench()
    leg, res, prof, e = fake_step(300, 64, 1000, 300)
    b.dump_outputs(leg, res, str(tmp_path / "d"))
    d = load_dir(tmp_path / "d")
    assert sorted(d) == ["edges_a", "edges_b", "edges_index", "edges_shared", "edges_weight", "profile",
                         "profile_rows", "shape", "totals", "totals_index"]
    assert all(v.dtype == np.float64 for v in d.values())
    assert np.array_equal(d["profile"], prof) and np.array_equal(d["profile_rows"], np.arange(300))
    assert np.array_equal(d["edges_a"], e.a) and np.array_equal(d["edges_b"], e.b)
    assert np.array_equal(d["edges_shared"], e.shared) and np.array_equal(d["edges_weight"], e.weight)
    assert np.array_equal(d["totals"], e.totals) and np.array_equal(d["totals_index"], np.arange(300))
    assert d["shape"].tolist() == [300, 64, 1000, 300]


def test_dump_outputs_large_outputs_are_a_fixed_sample_within_64_mb(tmp_path, monkeypatch):
    b = load_bench()
    assert b.DUMP_BUDGET + (1 << 20) <= 64 * 10 ** 6  # the array data and room for the .npy headers
    # the same split of a 64 times smaller budget, so the test's arrays stay small
    monkeypatch.setattr(b, "DUMP_BUDGET", b.DUMP_BUDGET // 64)
    leg, res, prof, e = fake_step(3000, 128, 40_000, 90_000)
    for name in ("d1", "d2"):
        b.dump_outputs(leg, res, str(tmp_path / name))
    d1, d2 = load_dir(tmp_path / "d1"), load_dir(tmp_path / "d2")
    assert all(np.array_equal(d1[k], d2[k]) for k in d1), "two dumps of the same outputs differ"
    size = sum(os.path.getsize(tmp_path / "d1" / f) for f in os.listdir(tmp_path / "d1"))
    assert size <= b.DUMP_BUDGET + 10 * 128
    rows = d1["profile_rows"].astype(np.int64)
    assert 0 < len(rows) < 3000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(d1["profile"], prof[rows])
    ei, ti = d1["edges_index"].astype(np.int64), d1["totals_index"].astype(np.int64)
    assert 0 < len(ei) < 40_000 and 0 < len(ti) < 90_000
    assert np.array_equal(d1["edges_a"], e.a[ei]) and np.array_equal(d1["edges_weight"], e.weight[ei])
    assert np.array_equal(d1["edges_shared"], e.shared[ei]) and np.array_equal(d1["totals"], e.totals[ti])
    assert d1["shape"].tolist() == [3000, 128, 40_000, 90_000]
