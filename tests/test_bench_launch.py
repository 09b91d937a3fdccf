"""bench.py's N-rank launcher (VERDICT r2 "missing" #1), on CPU.

`python bench.py --gpus N` without WORLD_SIZE must start N ranks itself (as a
child torch.distributed.run tree, never by re-exec) and print exactly one JSON
line from rank 0 with n_gpus = N and parallelism dpN.  `--backend gloo
--dry-run` runs that path without any GPU work.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=240):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.pop("LOCAL_RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    return r, lines


@pytest.mark.parametrize("n", [2, 3])
def test_bench_launches_n_ranks(n):
    r, lines = _run(["--gpus", str(n), "--backend", "gloo", "--dry-run", "--steps", "3", "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == n
    assert d["config"]["parallelism"] == f"dp{n}"
    assert d["config"]["global_batch"] == n * 256
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["value"] > 0 and d["scaling"] == "weak" and d["higher_is_better"] is True


def test_bench_single_rank_dry_run():
    r, lines = _run(["--dry-run", "--steps", "2"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["config"]["parallelism"] == "dp1"


def test_bench_kernel_report_needs_full():
    # the kernel report comes from the --full passes: a plain run must refuse it, not drop it
    r, lines = _run(["--dry-run", "--kernel-report", os.devnull])
    assert r.returncode != 0 and not lines
    assert "--full" in r.stderr
    r, lines = _run(["--dry-run", "--full", "--kernel-report", os.devnull, "--steps", "2"])
    assert r.returncode == 0 and len(lines) == 1, r.stderr[-2000:]


def test_bench_child_failure_propagates():
    # a rank count that disagrees with WORLD_SIZE is refused by every rank: the
    # launcher must hand back a non-zero exit code, not swallow it
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--backend", "gloo",
                        "--dry-run"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert r.returncode != 0
