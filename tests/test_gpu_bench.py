"""bench.py on a Matrix Market file (round-3 verdict item 2): reader -> own symbolic phase -> timed numeric factorization; the flop
count of the line must be the compiled reference's for the same matrix (fixture), and the CPU leg runs the reference on that file."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _bench(args, env=None, timeout=600):
    out = subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT,
                         env=env or dict(os.environ))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("name,cpu", [("epb1", True), ("cvxqp3", False)])
def test_bench_on_a_matrix_market_file(tmp_path, name, cpu):
    sys.path.insert(0, str(ROOT))
    import bench
    from stmmqr_testlib import load_golden, scalar
    g0 = load_golden(name)
    p = tmp_path / f"{name}.mtx"
    bench._write_mtx(p, int(g0["A_m"][0]), int(g0["A_n"][0]), g0["A_p"], g0["A_i"], g0["A_x"])
    d = _bench(["--matrix", str(p), "--steps", "2", "--warmup", "1", "--full"] + ([] if cpu else ["--no-cpu"]))
    assert d["config"]["flops_per_step"] == scalar(g0, "flopcount")
    assert d["config"]["retries"] == 0 and d["value"] > 0 and "Matrix Market file" in d["config"]["workload"]
    assert d["config"]["matrix_file"]["n1cols"] == scalar(g0, "n1cols")
    if cpu and (ROOT / "oracle" / "_ref" / "refdump").exists():
        cb = d["cpu_baseline"]
        assert cb["kind"] == "reference" and cb["flops_match_device"] is True
        assert cb["legs"][0]["best_of"] == 3


def test_data_dir_replaces_the_standin(tmp_path):
    """xenon1 / sme3Dc / 3D_51448_3D are read from $STMMQR_DATA_DIR when present (stand-in otherwise).  A small file
    under the real name stands for the absent matrix here: the line must say it ran the file, not the stand-in."""
    sys.path.insert(0, str(ROOT))
    import bench
    from stmmqr_testlib import load_golden, scalar
    g0 = load_golden("t2d_q9")
    bench._write_mtx(tmp_path / "xenon1.mtx", int(g0["A_m"][0]), int(g0["A_n"][0]), g0["A_p"], g0["A_i"], g0["A_x"])
    d = _bench(["--steps", "1", "--warmup", "1", "--no-cpu"], env=dict(os.environ, STMMQR_DATA_DIR=str(tmp_path)))
    assert d["config"]["flops_per_step"] == scalar(g0, "flopcount")
    assert "xenon1.mtx" in d["config"]["workload"] and "stand-in" not in d["config"]["workload"]


def test_plain_run_and_dump_outputs(tmp_path):
    """A plain run is the headline alone: --steps timed steps, the contract's keys, none of what --full adds.  --dump-outputs
    writes the factors of the last timed step: float64 arrays, at most 64 MB in all, whose integer parts are the compiled
    reference's (the fixture) bit for bit."""
    import numpy as np
    sys.path.insert(0, str(ROOT / "tests"))
    from stmmqr_testlib import load_golden, scalar
    d = _bench(["--workload", "epb1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "f64"
    for k in ("roofline", "cpu_baseline", "f1_resident_factors", "dropin_seam_ms", "large_front"):
        assert k not in d
    files = sorted((tmp_path / "out").glob("*.npy"))
    assert sum(f.stat().st_size for f in files) <= 64 << 20
    out = {f.stem: np.load(f) for f in files}
    assert all(a.dtype == np.float64 for a in out.values())
    g = load_golden("epb1")
    nf = int(scalar(g, "sym_nf"))
    assert out["info"][0] == scalar(g, "num_rank")
    for k, ref in (("Rdead", g["num_Rdead"][:int(scalar(g, "sym_n"))]), ("HPinv", g["num_HPinv"][:int(scalar(g, "sym_m"))]),
                   ("Hm", g["num_Hm"][:nf]), ("Hr", g["num_Hr"][:nf]), ("Rblock_off", g["num_Rblock_off"][:nf])):
        np.testing.assert_array_equal(out[k], ref.astype(np.float64), err_msg=k)
    assert out["R_H_front_sumsq"].shape == (nf,) and np.all(np.isfinite(out["R_H_stack_sample"]))
