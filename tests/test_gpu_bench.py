"""bench.py --gpus 2 without a launcher on the one-GPU box:
it starts two rank processes itself, both classify on device 0 (more ranks
than GPUs: round-robin), and the line reports the two ranks that ran."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_self_launched_two_ranks():
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "c2",
                        "--frames", "262144", "--queues", "2", "--steps", "4", "--warmup", "1",
                        "--ramp", "2", "--launch-probe", "3", "--rotate-mib", "32",
                        "--full", "--no-cpu-baseline", "--no-extra"],
                       env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1                     # rank 0's line only
    d = lines[0]
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "replicas2"
    assert d["config"]["rank_devices"] == [0, 0]
    assert d["value"] > 0 and d["steps"] == 4


def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    """A plain run (no --full) prints the headline keys only and, with
    --dump-outputs, writes the last timed step's result sets: per queue the
    decisions and the per-endpoint lists, which must be the stable scatter of
    those decisions."""
    import numpy as np
    from usnetd_amd import lib
    n, nq = 65536 + 321, 2                      # no multiple of the tile; below the dump's sample size
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2",
                        "--frames", str(n), "--queues", str(nq), "--steps", "3", "--warmup", "1",
                        "--ramp", "2", "--rotate-mib", "16", "--dump-outputs", str(tmp_path / "out")],
                       env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = lines[0]
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["full"] is False
    assert d["unit"] == "Mpkts/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    for k in ("roofline", "end_to_end", "cpu_baseline", "c2", "c3", "host_inclusive"):
        assert k not in d
    files = sorted(x.name for x in (tmp_path / "out").iterdir())
    assert files == sorted("q%d_%s.npy" % (j, a) for j in range(nq)
                           for a in ("decisions", "index", "bin_off"))
    for j in range(nq):
        dec, idx, off = (np.load(tmp_path / "out" / ("q%d_%s.npy" % (j, a)))
                         for a in ("decisions", "index", "bin_off"))
        assert dec.dtype == idx.dtype == off.dtype == np.float64
        assert dec.shape == idx.shape == (n,) and off[0] == 0 and off[-1] == n
        n_ep = off.size - 1 - 3
        want = lib.expected_lists(dec.astype(np.uint32), n_ep)
        got = {b: idx[int(off[b]):int(off[b + 1])] for b in range(off.size - 1) if off[b + 1] > off[b]}
        assert sorted(got) == sorted(want)
        assert all(np.array_equal(got[b], want[b]) for b in want)
