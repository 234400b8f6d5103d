"""GPU: bench.py's plain run, --full and --dump-outputs on a small headline
batch. A plain run reports the headline fields and none of the extras; --full
adds the CPU baseline; both write the same output arrays (the inputs depend
on the arguments only), and those arrays are the records the merge returns to
a caller of the engine for the same generated pairs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--n-obj", str(N), "--settle-ms", "20", *args], capture_output=True, text=True, timeout=120,
                       env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_and_full_runs_dump_the_merge_output(gpu, tmp_path):
    import crdts_hip

    plain = _bench("--dump-outputs", str(tmp_path / "a"))
    full = _bench("--full", "--cpu-sample", "2000", "--dump-outputs", str(tmp_path / "b"))
    for r in (plain, full):
        assert r["steps"] == 2 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["value"] > 0
        assert r["unit"] == "objects/s" and r["higher_is_better"] is True and r["dtype"] == "u64"
        assert abs(r["value"] * r["ms_per_step"] * 1e-3 / N - 1) < 1e-9  # objects/s over the timed steps
    assert "cpu_baseline" not in plain and full["cpu_baseline"]["value"] > 0
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == ["out_record_objects.npy", "out_record_sizes.npy",
                                                           "out_records.npy"]
    arr = {}
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and (x == y).all(), n
        arr[n[:-4]] = x
    assert sum(x.nbytes for x in arr.values()) <= 64 << 20
    # the same pairs through the engine: the records a caller receives
    (lb, lo), (rb, ro) = crdts_hip.generate_orswot(N, threads=8)
    L = crdts_hip.OrswotBatch.from_host(lb, lo, 16)
    R = crdts_hip.OrswotBatch.from_host(rb, ro, 16)
    recs = gpu.orswot_merge(L, R).records()
    assert (arr["out_record_objects"] == np.arange(N)).all()
    assert (arr["out_record_sizes"] == [len(r) for r in recs]).all()
    exp = np.frombuffer(b"".join(recs), np.uint32)
    assert arr["out_records"].shape == exp.shape and (arr["out_records"] == exp).all()
