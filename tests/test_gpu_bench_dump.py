"""GPU: `bench.py --dump-outputs DIR` on a plain run writes the outputs of the
step it timed.  The tiny config (5,000 contigs, 500k paired fragments, 5p6) is
run once as a plain benchmark; the files are compared, bit for bit, with the
same workload built in this process by a kept synchronous step
(ShardedBuild.run(keep=True), the path tests/test_gpu_configs.py holds to the
oracle's digests).  The tiny profile (5,000 x 1,088 f64 = 43.5 MB) exceeds its
share of the 64 MB, so the sampled path is the one exercised."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import digests as D
from karma_amd import _lib, engine
from karma_amd.comm import SoloComm
from karma_amd.distributed import ShardedBuild

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dump"))
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "tiny", "--dump-outputs", out], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    files = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    size = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
    return json.loads(lines[0]), files, size


@pytest.fixture(scope="module")
def kept():
    inp = D.bench_inputs("tiny", config="tiny")
    ctx = _lib.Context(0)
    build = ShardedBuild(ctx, SoloComm(), engine.kmode_of(inp["kmer"]), inp["n_glob"], inp["c_lo"], inp["n_loc"])
    store = engine.ContigStore(ctx, inp["blob"], inp["offs"], inp["key_len"])
    rec_dev = _lib.DevBuf.from_numpy(ctx, inp["rec"].view(np.int64).reshape(-1))
    try:
        res = build.run(store, rec_dev.ptr, len(inp["rec"]), keep=True)
        return {"profile": res["profile"].numpy(), "edges": res["edges"]}
    finally:
        build.close()
        store.close()
        rec_dev.close()
        ctx.close()


def test_plain_line_is_the_headline_only(dumped):
    line, _, _ = dumped
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    # value = (contigs + fragments) per second of the timed steps; ms_per_step is rounded to 1 us
    assert abs((5_000 + 500_000) / line["value"] * 1e3 - line["ms_per_step"]) <= 1e-3
    assert line["step_driver"]["deferred_steps"] >= 3  # the timed steps ran, as deferred ones
    for key in ("parity", "single_batch", "roofline", "profile_write_ceiling", "cpu_baseline"):
        assert line[key] is None, key
    assert line["kernels_ms_per_step"] == {}
    assert not {"records_other", "end_to_end", "eq_path", "dropin", "reference_measured", "weak"} & set(line)


def test_dump_is_float64_within_64_mb(dumped):
    _, files, size = dumped
    assert sorted(files) == ["edges_a", "edges_b", "edges_index", "edges_shared", "edges_weight", "profile",
                             "profile_rows", "shape", "totals", "totals_index"]
    assert all(v.dtype == np.float64 for v in files.values())
    assert size <= 64 * 10 ** 6


def test_dumped_outputs_equal_a_kept_step(dumped, kept):
    line, f, _ = dumped
    prof, e = kept["profile"], kept["edges"]
    assert f["shape"].tolist() == [prof.shape[0], prof.shape[1], len(e.a), len(e.totals)]
    assert line["config"]["columns_M"] == prof.shape[1] and line["config"]["edges"] == len(e.a)
    rows = f["profile_rows"].astype(np.int64)
    assert 0 < len(rows) < prof.shape[0] and np.all(np.diff(rows) > 0)  # sampled: 43.5 MB of profile
    assert np.array_equal(f["profile"].view(np.uint64), prof[rows].view(np.uint64))
    ei, ti = f["edges_index"].astype(np.int64), f["totals_index"].astype(np.int64)
    assert np.array_equal(ei, np.arange(len(e.a))) and np.array_equal(ti, np.arange(len(e.totals)))
    assert np.array_equal(f["edges_a"], e.a) and np.array_equal(f["edges_b"], e.b)
    assert np.array_equal(f["edges_shared"], e.shared)
    assert np.array_equal(f["edges_weight"].view(np.uint64), np.asarray(e.weight).view(np.uint64))
    assert np.array_equal(f["totals"], e.totals)
