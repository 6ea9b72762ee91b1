"""CPU rehearsal of how the driver starts the multi-GPU bench: `python bench.py --gpus N` as a plain process.
bench.py must start its own `torch.distributed.run` child (never touching the GPU in the parent), the ranks must
meet, and the shard layout must be BASELINE.json configs[3]'s: ONE SF10 lineitem table cut by chunk into 8 canonical
octants, rank r owning octants [r·8/N, (r+1)·8/N) (strong scaling); `--scaling weak` gives each rank an SF10 shard."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _dry_run(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run-layout", *extra], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout  # rank 0 alone prints, one JSON line
    return json.loads(lines[0])


@pytest.mark.parametrize("world", [2, 4])
def test_plain_start_spawns_the_ranks_and_shards_one_sf10_table(world):
    doc = _dry_run("--gpus", str(world))
    assert doc["n_gpus"] == world and doc["scaling"] == "strong" and doc["workload"] == "q1_sf10"
    assert doc["total_rows"] == 59986052 and doc["n_chunks"] == 458 and doc["rows_covered"] == doc["total_rows"]
    ranks = sorted(doc["ranks"], key=lambda r: r["rank"])
    assert [r["rank"] for r in ranks] == list(range(world))
    nxt_chunk, nxt_row = 0, 0
    for r in ranks:  # contiguous chunk ranges in rank order, octants [r·8/N, (r+1)·8/N)
        assert r["first_chunk"] == nxt_chunk and r["first_row"] == nxt_row
        assert r["octants"] == list(range(r["rank"] * 8 // world, (r["rank"] + 1) * 8 // world))
        assert r["first_chunk"] == doc["octant_chunk_begin"][r["octants"][0]]
        nxt_chunk += r["n_chunks"]
        nxt_row += r["local_rows"]
    assert nxt_chunk == 458


def test_weak_scaling_gives_every_rank_an_sf10_shard():
    doc = _dry_run("--gpus", "2", "--scaling", "weak")
    assert doc["scaling"] == "weak" and doc["total_rows"] == 2 * 59986052
    assert [r["local_rows"] for r in sorted(doc["ranks"], key=lambda r: r["rank"])] == [59986052, 59986052]


def test_one_rank_needs_no_launcher():
    doc = _dry_run()
    assert doc["n_gpus"] == 1 and doc["ranks"][0]["local_rows"] == 59986052 and doc["ranks"][0]["octants"] == list(range(8))


def test_a_rank_without_the_communicator_ends_every_rank_with_a_nonzero_code():
    """No fallback transport in a measurement: if ncclCommInitRank fails on ANY rank, all ranks agree (an all-reduce of the
    outcome) and leave with exit code 3 — rehearsed over gloo with rank 1 pretending; nothing is printed as a result."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run-layout", "--gpus", "2", "--dry-run-comm-failure", "1"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode != 0
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert "rank 0: the library's RCCL communicator could not be created on another rank" in p.stderr
    assert "rank 1: the library's RCCL communicator could not be created (rehearsed failure)" in p.stderr


def test_dump_outputs_writes_the_result_rows_as_float_arrays(tmp_path):
    """`--dump-outputs DIR`: the finalized rows of the last timed step as float64 .npy files (keys, aggregates, a NULL mask);
    beyond the size cap a seeded sample of the groups, the same one every time."""
    import importlib
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    abi = importlib.import_module("rust-llkv_amd.abi")
    V = abi.Value

    class Row:
        def __init__(self, keys, values):
            self.keys, self.values = keys, values

    rows = [Row([V(abi.DT_UTF8, False, "A"), V(abi.DT_INT64, False, 3)],
                [V(abi.DT_FLOAT64, False, 1.5), V(abi.DT_INT64, False, 7), V(abi.DT_DECIMAL128, False, 12345, 15, 2), V(abi.DT_FLOAT64, True, None)]),
            Row([V(abi.DT_UTF8, False, "NO"), V(abi.DT_INT64, True, None)],
                [V(abi.DT_FLOAT64, False, -2.5), V(abi.DT_INT64, False, 8), V(abi.DT_DECIMAL128, False, -5, 15, 2), V(abi.DT_FLOAT64, False, 3.0)])]
    out = tmp_path / "all"
    bench.dump_outputs(abi, str(out), rows)
    assert sorted(os.listdir(out)) == ["agg0.npy", "agg1.npy", "agg2.npy", "agg3.npy", "key0.npy", "key1.npy", "nulls.npy"]
    load = lambda name: np.load(out / name)
    assert all(load(n).dtype == np.float64 for n in os.listdir(out))
    assert load("key0.npy").tolist() == [[65.0, -1.0], [78.0, 79.0]]
    assert load("key1.npy")[0] == 3.0 and np.isnan(load("key1.npy")[1])
    assert load("agg0.npy").tolist() == [1.5, -2.5] and load("agg1.npy").tolist() == [7.0, 8.0]
    assert load("agg2.npy").tolist() == [123.45, -0.05]
    assert np.isnan(load("agg3.npy")[0]) and load("agg3.npy")[1] == 3.0
    assert load("nulls.npy").tolist() == [[0, 0, 0, 0, 0, 1], [0, 1, 0, 0, 0, 0]]

    many = [rows[i % 2] for i in range(1000)]
    limit, bench.DUMP_LIMIT_BYTES = bench.DUMP_LIMIT_BYTES, 10_000
    try:
        a, b = tmp_path / "a", tmp_path / "b"
        bench.dump_outputs(abi, str(a), many)
        bench.dump_outputs(abi, str(b), many)
    finally:
        bench.DUMP_LIMIT_BYTES = limit
    assert sum(os.path.getsize(a / n) for n in os.listdir(a)) < 10_000 + 128 * len(os.listdir(a))  # + the .npy headers
    kept = np.load(a / "sample.npy")
    assert 0 < len(kept) < 1000 and kept.tolist() == np.load(b / "sample.npy").tolist()
    assert np.load(a / "agg0.npy").tolist() == [many[int(i)].values[0].value for i in kept]
