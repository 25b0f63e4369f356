"""bench.py's two kinds of run: a plain run times the steps and prints the headline, nothing else; --full adds the measurements and
checks beside it (the tests that read those -- the self-check against the oracle, the multi-rank lines -- call it with --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
EXTRAS = ("verified", "cpu_baseline", "roofline", "roofline_hbm_kernel", "extension_stage", "incl_pcie", "next_rows")


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}


@pytest.mark.parametrize("args", [["--verify-sample", "1000"], ["--cpu-sample", "5000"], ["--cpu-sample-1t", "100"]])
def test_plain_run_refuses_a_measurement_that_needs_full(args):
    """Asking a plain run for a sample of the CPU baseline or of the self-check is an error (exit 2, before any device work), not a
    line that quietly lacks it."""
    r = subprocess.run([sys.executable, BENCH] + args, env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 2 and "--full" in r.stderr.decode(), r.stderr.decode()[-2000:]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(tmp_path):
    """A plain run on a small workload: the headline fields, the timed steps' own stage times, the dumped regions -- and none of what
    --full measures beside them."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--steps", "2", "--warmup", "1", "--genome-mbp", "40", "--reads-per-gpu", "20000", "--dump-outputs", str(out)],
                       env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    res = json.loads(lines[0])
    assert res["unit"] == "Mreads/s" and res["higher_is_better"] is True and res["dtype"] == "u16" and res["metric"].startswith("Mreads/s")
    assert res["value"] > 0 and res["ms_per_step"] > 0 and res["steps"] == 2 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert abs(res["value"] - 20000 / res["ms_per_step"] / 1e3) < 2e-3 * res["value"] + 2e-3
    assert res["stage_ms"]
    assert [k for k in EXTRAS if k in res] == []
    assert res["stage_ms_isolated"] == {} and res["incl_pcie_value"] is None and res["verified_identical"] is None and res["clock_mhz"] is None
    assert not res["config"]["index_build"].get("verified")
    per_read = np.load(out / "regions_per_read.npy")
    regions = np.load(out / "regions.npy")
    assert per_read.shape == (20000,) and regions.shape == (int(per_read.sum()), 6)
