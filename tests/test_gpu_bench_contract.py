"""GPU: bench.py's output contract (one JSON line on stdout with the driver's keys; roofline and cpu_baseline objects
with --full; what a plain run leaves out and what --dump-outputs writes) and __graft_entry__.smoke()."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_json_line_with_the_contract_keys():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--batch", "32",
                        "--full"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "images/sec" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 2
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "bf16" and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - 32 / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-2
    ro = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in ro, k
    assert ro["bound"] == "mfma" and ro["unit"] == "TFLOP/s" and ro["peak"] == 2500.0
    assert abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-3 and 0 < ro["frac"] < 1
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0


def test_plain_bench_run_is_lean_and_dumps_the_last_step(tmp_path):
    """Without --full: the headline keys only (no rooflines, secondary paths or CPU baseline), --steps timed steps, and
    --dump-outputs writes the last timed step's losses (the values the line reports) and E/G/D state as float32 .npy."""
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2", "--batch", "32",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "dtype", "losses", "config"):
        assert k in d, k
    assert d["steps"] == 4 and d["warmup"] == 2 and d["dtype"] == "bf16" and d["config"]["hip_graph"] is True
    assert abs(d["value"] - 32 / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-2
    for k in ("roofline", "cpu_baseline", "parity_path", "dropin_path", "denoise_path", "elided_path"):
        assert k not in d, k
    files = sorted(p.name for p in out_dir.iterdir())
    assert files == ["discriminator_state.npy", "encoder_state.npy", "generator_state.npy", "losses.npy"], files
    assert sum(p.stat().st_size for p in out_dir.iterdir()) <= 64 << 20
    arrs = {f[:-4]: np.load(out_dir / f) for f in files}
    for name, a in arrs.items():
        assert a.dtype == np.float32 and a.ndim == 1 and a.size > 0 and np.isfinite(a).all(), name
    names = ("recon_loss", "kl_loss", "g_loss_adv", "d_loss_1", "d_loss_2")
    np.testing.assert_allclose(arrs["losses"], [d["losses"][n] for n in names], rtol=0, atol=1e-5)


def test_bench_single_rank_rccl_path_keeps_stdout_to_the_json_line():
    """VAEGAN_FORCE_DIST=1: the N > 1 code path (RCCL process group, flat-buffer all-reduces between hipGraph
    segments) with one rank.  RCCL prints a version banner to stdout at communicator creation; bench.py must still
    hand the driver exactly one line."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, VAEGAN_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--batch", "32",
                        "--no-cpu-baseline"], cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["config"]["hip_graph"] is True and d["value"] > 0


def test_graft_entry_smoke():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.smoke()
