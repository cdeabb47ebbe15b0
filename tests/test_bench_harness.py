"""bench.py's launcher contract: `--gpus N` without a launcher spawns N ranks itself (one process per GPU, as the
reference does with mp.spawn, cat/shared/coreutils.py:493-504); a node with fewer GPUs gets a "not measured" line, never
an extrapolation; under torch.distributed.run the rank initialises RCCL ("nccl"), checks world size and device
distinctness, and with --full the DDP stand-in leg runs (1-rank NCCL on the single GPU of the test box)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_not_measured_when_gpus_missing():
    have = torch.cuda.device_count()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(have + 2), "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, r.stderr[-500:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["value"] is None and "not_measured" in d and d["n_gpus"] == have + 2


def test_full_legs_are_opt_in(monkeypatch):
    """A plain run times its steps and nothing else; the legs beside the headline run only with --full, and --ddp-head, which asks
    for one of them, is refused without it instead of being ignored."""
    bench = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--ddp-head"])
    a = bench.parse()
    assert a.full and a.ddp_head
    monkeypatch.setattr(sys, "argv", ["bench.py", "--ddp-head"])
    with pytest.raises(SystemExit):
        bench.parse()


@pytest.mark.gpu
def test_one_rank_nccl_with_ddp_stand_in():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--B", "8", "--T", "200", "--histories", "256", "--fanout", "8", "--full", "--no-cpu-baseline", "--ddp-head", "--ddp-layers", "1",
           "--ddp-steps", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-1500:]
    d = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 1 and d["config"]["world_size"] == 1 and len(d["config"]["devices"]) == 1
    assert d["value"] > 0 and d["roofline"]["frac"] > 0 and d["event_blocks"]["median_ms_per_step"] > 0
    assert d["ddp_head"]["value"] > 0 and d["ddp_head"]["gradient_bytes_per_step"] == 4 * d["ddp_head"]["parameters"]
    assert "DDP" in d["ddp_head"]["model"]


def test_committed_pmc_traffic_belongs_to_the_default_bench_line():
    """profiles/pmc_traffic.json (tools/pmc_summary.py) is what bench.py quotes as `roofline.traffic`: it must be keyed by the
    DEFAULT bench workload and by the kernel instantiation the timed (staged) schedule runs -- a file captured on another
    workload or on the serial schedule's instantiation would make every default bench line print `traffic: null` -- and the
    dominant kernel's bytes must be its algorithmic bytes, not some other kernel's."""
    d = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    assert d["workload"] == "B64_T1500_V72_S4097_A103791_full"
    assert d["den_kernel"].startswith("crf_fac_pair_kernel<true,1024,")
    alg = 2 * (64 * 1500 * (4 * 72 + 4 * 4097) + 12 * 103791 + 12 * 4097)
    assert 0.95 * alg <= d["kernels"]["crf_fac_pair_kernel"] <= 1.25 * alg
    assert 1.0 < d["whole_path"]["ratio"] < 3.0
    src = d["source"].split(":")[0]
    assert os.path.exists(os.path.join(ROOT, src)), src


def test_dump_outputs_stays_within_its_limit(tmp_path):
    """bench.py --dump-outputs: arrays that fit are written whole; past the limit a fixed, seeded sample of the flattened entries
    (values + float64 flat indices) fills what is left, the same sample on every run; everything is float32 / float64."""
    bench = _bench_module()
    grad = np.random.default_rng(1).normal(size=(4, 50, 72)).astype(np.float32)
    loss = np.array([1.5], dtype=np.float32)
    w = bench.dump_outputs(str(tmp_path / "whole"), {"loss": loss, "grad": grad})
    assert w == {"loss.npy": [1], "grad.npy": [4, 50, 72]}
    assert np.array_equal(np.load(tmp_path / "whole" / "grad.npy"), grad)
    limit = 20000
    for d in ("a", "b"):
        w = bench.dump_outputs(str(tmp_path / d), {"loss": loss, "grad": grad}, limit_bytes=limit)
        assert sorted(w) == ["grad_sample.npy", "grad_sample_index.npy", "loss.npy"]
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= limit
        val, idx = np.load(tmp_path / d / "grad_sample.npy"), np.load(tmp_path / d / "grad_sample_index.npy")
        assert val.dtype == np.float32 and idx.dtype == np.float64 and len(val) == len(idx) > 1000
        assert np.all(np.diff(idx) > 0) and np.array_equal(val, grad.reshape(-1)[idx.astype(np.int64)])
        assert np.array_equal(np.load(tmp_path / d / "loss.npy"), loss)
    assert all(np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)) for f in w)


@pytest.mark.gpu
def test_dump_outputs_of_the_last_timed_step(tmp_path):
    """Two runs with the same arguments: the same seeded inputs, so the dumped loss and gradient agree; the loss is the one the
    result line reports (a step on the same batch), the gradient has the caller's shape and is finite."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    B, T, V = 8, 200, 72
    runs = []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--B", str(B), "--T", str(T),
               "--histories", "256", "--fanout", "8", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-1500:]
        line = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        assert sorted(os.listdir(tmp_path / d)) == ["grad.npy", "loss.npy"]
        loss, grad = np.load(tmp_path / d / "loss.npy"), np.load(tmp_path / d / "grad.npy")
        assert loss.dtype == np.float32 and loss.shape == (1,) and grad.dtype == np.float32 and grad.shape == (B, T, V)
        assert np.isfinite(grad).all() and np.abs(grad).max() > 0
        assert abs(float(loss[0]) - line["loss"]) <= 1e-5 * abs(line["loss"])
        runs.append((loss, grad))
    assert abs(float(runs[0][0][0] - runs[1][0][0])) <= 1e-6 * abs(float(runs[1][0][0]))
    assert rel_err(runs[0][1], runs[1][1]) <= 1e-6
    print("two runs bit-identical:", bool(np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][0], runs[1][0])))
