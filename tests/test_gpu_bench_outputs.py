"""A plain `bench.py --gpus 1 --steps N --warmup W` run on a reduced workload: one result line with the headline fields and nothing
that --full adds, and --dump-outputs DIR writes the hit lists of the last timed step - the records the line's hits_crc is taken over -
as float arrays; two runs with the same arguments write the same arrays."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--n-seqs", "200000",
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_plain_run_dumps_the_hit_lists_of_its_last_step(tmp_path):
    a, b = _plain(tmp_path / "a"), _plain(tmp_path / "b")
    for line in (a, b):
        assert line["metric"] == "profile-ops/sec" and line["unit"] == "profile-ops/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f32" and line["steps"] == 3 and line["warmup"] == 1
        assert line["value"] > 0 and line["ms_per_step"] > 0
        assert "roofline" not in line and not line["cpu_baseline"] and not [k for k in line if k.startswith("e2e")]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["hits_criterion.npy", "hits_dist.npy", "hits_j.npy", "hits_weight.npy"]
    got = {f: np.load(tmp_path / "a" / f) for f in names}
    seeds, k = a["config"]["seeds_per_step"], a["config"]["top_k"]
    for f, arr in got.items():
        assert arr.shape == (seeds, k) and arr.dtype in (np.float32, np.float64), f
        assert np.array_equal(arr, np.load(tmp_path / "b" / f)), f
    crc = 0   # the line's checksum, taken over the same records as the run took it (ids int32, criteria float32, seed by seed)
    for s in range(seeds):
        crc = zlib.crc32(got["hits_j.npy"][s].astype(np.int32).tobytes(), crc)
        crc = zlib.crc32(got["hits_criterion.npy"][s].astype(np.float32).tobytes(), crc)
    assert crc == a["hits_crc"] == b["hits_crc"]
