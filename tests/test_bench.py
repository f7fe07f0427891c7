"""bench.py's command line: a plain run times the steps only, --full adds the other legs, and
--dump-outputs writes the last timed step's results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float64_arrays(tmp_path):
    r = {"mll": np.arange(6.0).reshape(1, 6), "status": np.zeros((1, 6), dtype=np.int32),
         "mu": np.arange(24, dtype=np.float64).reshape(1, 6, 4)[:, :, ::2]}  # a non-contiguous view
    bench.dump_outputs(str(tmp_path / "a" / "b"), r, 0)
    bench.dump_outputs(str(tmp_path / "a" / "b"), {"mll": r["mll"] + 1}, 3)
    got = sorted(p.name for p in (tmp_path / "a" / "b").iterdir())
    assert got == ["mll.npy", "mll_rank3.npy", "mu.npy", "status.npy"]
    for k, v in r.items():
        a = np.load(tmp_path / "a" / "b" / f"{k}.npy")
        assert a.dtype == np.float64 and a.shape == v.shape
        np.testing.assert_array_equal(a, v)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "b" / "mll_rank3.npy"), r["mll"] + 1)


def test_workload_is_the_same_from_call_to_call():
    a = bench.make_workload(1, 0, 1)[1:]
    b = bench.make_workload(1, 0, 1)[1:]
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_what_they_computed(tmp_path):
    """One plain run at one trial (6 slots): the result line has the headline fields and none of the
    --full legs, and the dumped arrays are bit for bit what the timed path returns for the seeded
    workload."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--trials", "1", "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["fit_ok"] is True
    assert d["unit"] == "fits/s" and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] - 6 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    for k in ("roofline", "roofline_parts", "kernels_ms_per_step", "cpu_baseline", "pred_mean_max_err", "optimise"):
        assert d[k] is None, k
    for leg in ("per-kernel", "optimiser leg", "CPU baseline"):
        assert leg not in p.stderr

    import gprx
    from gprx import shard

    trs, X, Y, T, XT = bench.make_workload(1, 0, 1)
    ctx = gprx.Context(0)
    rb = shard.RankBatch(trs, ctx=ctx)
    try:
        ref = rb.evaluate(T.reshape(rb.n, bench.G, -1))
    finally:
        rb.close()
        ctx.close()
    assert sorted(f.name for f in (tmp_path / "out").iterdir()) == sorted(f"{k}.npy" for k in ref)
    for k, v in ref.items():
        a = np.load(tmp_path / "out" / f"{k}.npy")
        assert a.dtype == np.float64 and a.shape == np.asarray(v).shape, k
        np.testing.assert_array_equal(a, np.asarray(v, dtype=np.float64), err_msg=k)
