"""`bench.py --dump-outputs DIR`: the files hold what the last timed step of a plain run computed -- the forward NTT of the seeded
input column and the inverse of that -- at the seeded sample positions, each word as two exact 32-bit halves in float64; and a plain
run carries no leg, check or baseline beyond the NTT steps (those are `--full`'s)."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _words(a):
    assert a.dtype == np.float64 and a.ndim == 2 and a.shape[1] == 2
    return a[:, 0].astype(np.uint64) | (a[:, 1].astype(np.uint64) << np.uint64(32))


@pytest.mark.gpu
def test_dump_outputs_are_the_timed_steps_outputs(orc, tmp_path):
    sys.path.insert(0, str(ROOT))
    import bench, oracle_lib
    nbits = 21                                                           # 2^21 > DUMP_SAMPLE: the sampled form
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "3", "--warmup", "1", "--nbits", str(nbits), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["legs"] == {} and "cpu_baseline" not in line
    idx = np.load(tmp_path / "sample_index.npy")
    assert idx.dtype == np.float64 and len(idx) == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0)
    idx = idx.astype(np.int64)
    x = oracle_lib.splitmix64_stream(bench.SEED, 1 << nbits)
    assert np.array_equal(_words(np.load(tmp_path / "ntt_inverse.npy")), x[idx])
    assert np.array_equal(_words(np.load(tmp_path / "ntt_forward.npy")), orc.ntt_blocked(x, nbits, False)[idx])
