"""Driver-contract test for bench.py: the JSON line the round driver
parses must keep its schema (keys, types, units) in both modes."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = {
    "metric": str, "value": (int, float), "unit": str, "n_gpus": int,
    "steps": int, "warmup": int, "ms_per_step": (int, float),
    "higher_is_better": bool, "scaling": str, "dtype": str, "data": str,
    "config": dict,
}


def _run(mode, *extra):
    out = subprocess.run(
        [sys.executable, "bench.py", "--cpu-small", "--steps", "1",
         "--warmup", "0", "--mode", mode, *extra],
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-800:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert lines, f"no JSON line in stdout: {out.stdout[-300:]}"
    return json.loads(lines[-1])

class TestBenchContract:
    def test_train_mode_json(self):
        j = _run("train")
        for k, t in REQUIRED.items():
            assert k in j, f"missing key {k}"
            assert isinstance(j[k], t), (k, type(j[k]))
        assert "vs_baseline" in j  # null allowed (no published baseline)
        assert j["metric"] == "als_ratings_per_sec"
        assert j["unit"] == "ratings/s"
        assert j["n_gpus"] == 1 and j["steps"] == 1
        assert j["scaling"] == "weak" and j["data"] == "synthetic"
        assert j["value"] > 0 and j["ms_per_step"] > 0
        # whole-job aggregate consistency: value = nnz / sec_per_iter
        cfg = j["config"]
        assert abs(j["value"] - cfg["global_batch"] /
                   (j["ms_per_step"] / 1e3)) / j["value"] < 1e-6
        assert cfg["parallelism"] == "dp1"

    def test_serve_mode_json(self):
        j = _run("serve")
        assert j["metric"] == "serving_queries_per_sec"
        assert j["unit"] == "queries/s"
        assert j["value"] > 0
        assert j["config"]["topk"] == 20

    def test_dump_outputs_train(self, tmp_path):
        """--dump-outputs writes the last step's factors as float .npy
        files, identical from run to run; --full keeps the result line."""
        import numpy as np
        dumps = []
        for name, extra in (("a", ()), ("b", ("--full",))):
            d = tmp_path / name
            j = _run("train", "--dump-outputs", str(d), *extra)
            assert j["metric"] == "als_ratings_per_sec" and j["steps"] == 1
            dumps.append({p.name: np.load(p) for p in d.glob("*.npy")})
        a, b = dumps
        assert set(a) == {"user_factors.npy", "user_factors_rows.npy",
                          "item_factors.npy", "item_factors_rows.npy"}
        assert a["user_factors.npy"].shape == (2000, 64)
        assert a["item_factors.npy"].shape == (1000, 64)
        assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
        for k, v in a.items():
            assert v.dtype in (np.float32, np.float64), (k, v.dtype)
            assert np.isfinite(v).all(), k
            assert np.array_equal(v, b[k]), k

    def test_dump_outputs_serve(self, tmp_path):
        import numpy as np
        _run("serve", "--dump-outputs", str(tmp_path))
        v = np.load(tmp_path / "topk_values.npy")
        i = np.load(tmp_path / "topk_indices.npy")
        assert v.shape == i.shape == (4096, 20)
        assert v.dtype == np.float32 and i.dtype == np.float64
        assert (np.diff(v, axis=1) <= 0).all()  # best first
        assert ((i >= -1) & (i < 1000)).all()

    def test_sample_rows_fixed(self):
        import bench
        a = bench.sample_rows(1_000_000, 1000, 7)
        assert len(a) == len(set(a.tolist())) == 1000
        assert (a[1:] > a[:-1]).all() and a[-1] < 1_000_000
        assert (a == bench.sample_rows(1_000_000, 1000, 7)).all()
        assert (bench.sample_rows(10, 1000, 7) == list(range(10))).all()
