"""bench.py's plain line and --dump-outputs: a plain run times exactly --steps steps and leaves the --full fields null; the
dumped arrays are float32 / float64, within the size cap, and identical inputs give the same outputs run to run."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

FULL_ONLY = ("roofline", "cpu_baseline", "eval", "dropin", "olp", "configs")
TABLES = ("entity_embeddings", "entity_adagrad_sum", "relation_embeddings", "relation_adagrad_sum")


def _bench(args, out_dir, env=None, launcher=()):
    cmd = [sys.executable, *launcher, os.path.join(ROOT, "bench.py"), *args, "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=420)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _load(out_dir):
    return {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_dump_rows_sample_is_fixed_and_within_budget():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.dump_rows(14543, 200, 14543 + 239) is None                    # S-FB: every row fits
    n_ent, n_rel, d = 2_500_000, 100_000, 256                                   # S-OLP: a sample
    ent, rel = bench.dump_rows(n_ent, d, n_ent + n_rel), bench.dump_rows(n_rel, d, n_ent + n_rel)
    assert (ent.size + rel.size) * (8 * d + 8) <= bench.DUMP_BYTES - 4096
    assert ent.size > 0.9 * n_ent * (bench.DUMP_BYTES - 4096) / ((8 * d + 8) * (n_ent + n_rel))
    assert np.all(np.diff(ent) > 0) and ent[-1] < n_ent and np.all(np.diff(rel) > 0) and rel[-1] < n_rel
    np.testing.assert_array_equal(ent, bench.dump_rows(n_ent, d, n_ent + n_rel))


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(okge_lib, tmp_path):
    args = ["--gpus", "1", "--steps", "3", "--warmup", "2"]
    d = _bench(args, tmp_path / "a")
    assert d["steps"] == 3 and d["warmup"] == 2 and d["timed_windows"] == 1 and d["ms_per_step"] > 0
    assert d["value"] > 0 and d["unit"] == "triples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert all(d[k] is None for k in FULL_ONLY), {k: d[k] for k in FULL_ONLY}
    a = _load(tmp_path / "a")
    assert set(a) == {"loss_sum", *TABLES}
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert a["loss_sum"].dtype == np.float64 and a["loss_sum"].shape == (1,)
    assert a["loss_sum"][0] == d["last_loss_sum"]
    assert a["entity_embeddings"].shape == a["entity_adagrad_sum"].shape == (14543, 200)
    assert a["relation_embeddings"].shape == a["relation_adagrad_sum"].shape == (239, 200)
    for k in TABLES:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all()
    assert (a["entity_adagrad_sum"] > 0).any() and (a["relation_adagrad_sum"] > 0).any()     # the steps trained
    _bench(args, tmp_path / "b")                                   # same arguments: same inputs, so the same outputs ...
    b = _load(tmp_path / "b")
    # ... up to the order of the prefix rows' float-atomic gradients, which Adagrad amplifies on a few tiny gradients
    # (the criterion of test_hip_parity.py::test_graphed_step_equals_plain_step)
    assert abs(b["loss_sum"][0] - a["loss_sum"][0]) <= 1e-6 * abs(a["loss_sum"][0])
    for k in TABLES:
        assert np.isclose(b[k], a[k], rtol=1e-4, atol=1e-5).mean() > 0.9999 and np.abs(b[k] - a[k]).max() < 1e-3, k


@pytest.mark.gpu
def test_dumped_outputs_two_ranks_one_gpu_rehearsal(okge_lib, tmp_path):
    """the sharded step's entity table comes back whole on rank 0 (gloo ranks on one GPU, as test_bench_multirank.py)"""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    launcher = ("-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", str(port))
    d = _bench(["--gpus", "2", "--steps", "2", "--warmup", "1"], tmp_path, env=dict(os.environ, OKGE_BENCH_ONE_GPU="1"),
               launcher=launcher)
    assert d["n_gpus"] == 2 and d["timed_windows"] == 1 and d["olp"] is None and d["roofline"] is None
    a = _load(tmp_path)
    assert a["loss_sum"][0] == d["last_loss_sum"]
    assert a["entity_embeddings"].shape == a["entity_adagrad_sum"].shape == (14543, 200)
    touched = (a["entity_adagrad_sum"] > 0).any(axis=1)
    assert touched[:7272].any() and touched[7272:].any()          # rows of both shards arrived (shard_range: 7272 / 7271)
    for k in TABLES:
        assert np.isfinite(a[k]).all()
