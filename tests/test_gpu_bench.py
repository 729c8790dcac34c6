"""bench.py's plain run on the GPU: `--steps` timed steps and nothing beside them, and `--dump-outputs`
holding the state those steps left -- checked against the C oracle's run of the same sweeps from the
same lattice start, bit for bit (tolerance: none)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_state(pmc, oracle, tmp_path):
    cps, atoms, warmup, steps = 16, 10_000, 2, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--cps", str(cps), "--atoms",
                        str(atoms), "--steps", str(steps), "--warmup", str(warmup), "--rewarm", "2",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=200)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["metric"] == "MC trial-moves/s (whole node)" and d["unit"] == "trial-moves/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["full"] is False
    assert d["steps"] == steps and d["warmup"] == warmup and d["error_flags"] == 0
    # nothing beside the headline figure on a plain line
    for k in ("roofline", "cpu_baseline", "parity", "energy", "vs_baseline"):
        assert k not in d, k
    # the oracle over the same sweeps: the warm-up ones, then the timed ones with fresh counters
    st = oracle.OracleState(oracle.make_params(cps=cps))
    st.init_lattice(atoms)
    st.run(0, warmup)
    st.stats = oracle.Stats()
    st.run(warmup, steps)
    o = st.stats.as_dict()
    # value and ms_per_step describe the same timed region: trials / (steps x ms_per_step)
    assert d["value"] == pytest.approx(o["trials"] / (steps * d["ms_per_step"] * 1e-3), rel=1e-9)
    assert d["acceptance"] == o["accepted"] / o["trials"]
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["coords", "counts", "counts_sample", "sample_cells", "stats"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["stats"].tolist() == [o["trials"], o["accepted"], o["evaluated"], o["de_fixed"] / 2.0 ** 32]
    assert np.array_equal(got["counts"], st.n)
    cells = got["sample_cells"].astype(np.int64)
    assert np.array_equal(cells, np.arange(cps ** 3))       # a box smaller than the sample: every cell
    want = st.disk.reshape(-1, 3, 16)[cells]
    valid = np.arange(16)[None, None, :] < st.n[cells][:, None, None]
    assert np.array_equal(got["coords"].view(np.uint32), np.where(valid, want, np.float32(0.0)).view(np.uint32))
