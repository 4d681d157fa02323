"""bench.py --dump-outputs DIR: what the timed entry point returned in its last step, written as DIR/<name>.npy so that two
builds can be compared output for output.  CPU part: the sampled factor positions, the size bound, the step count; GPU part
(-m gpu): two runs of the 1-GPU line on the same arguments dump the same bits, and the dump is the factorisation the
logpdf came from (checked against a NumPy Cholesky of the same seeded problem)."""
import json
import math

import numpy as np
import pytest

import bench_configs as bc
from test_bench_cli import _bench


def test_factor_sample_positions_are_seeded_and_in_the_lower_triangle():
    import bench
    i, j = bench.factor_sample_positions(1000, k=5000)
    i2, j2 = bench.factor_sample_positions(1000, k=5000)
    assert np.array_equal(i, i2) and np.array_equal(j, j2)
    assert (i >= j).all() and j.min() >= 0 and i.max() < 1000
    assert (np.diff(j * 1000 + i) >= 0).all()                       # sorted by column, then row


def test_the_dump_of_every_device_resident_line_fits_its_bound():
    import bench
    n_max = max(N for kind, N, D in bc.CONFIGS.values() if kind != "elbo")
    assert 8 * (1 + 2 * n_max + bench.DUMP_FACTOR_SAMPLE) <= bench.DUMP_LIMIT_BYTES


def test_write_outputs_refuses_more_than_the_bound(tmp_path):
    import bench
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "d"), {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1)})
    assert not (tmp_path / "d").exists()


@pytest.mark.parametrize("steps", ["0", "-1"])
def test_steps_below_one_is_refused(steps):
    r = _bench("--steps", steps, "--config", "c1", "--cpu-sample", "0")
    assert r.returncode == 2 and "--steps" in r.stderr and r.stdout.strip() == ""


@pytest.mark.gpu
def test_dump_outputs_repeat_bit_for_bit_and_are_the_factorisation(tmp_path):
    lines = []
    for d in ("a", "b"):
        r = _bench("--gpus", "1", "--config", "c1", "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--no-host-api",
                   "--dump-outputs", str(tmp_path / d))
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert lines[0]["steps"] == 2
    names = ["factor_diag", "factor_sample", "logpdf", "solved_row"]
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == [n + ".npy" for n in names]
    got = {}
    for n in names:
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert a.dtype == np.float64 and np.array_equal(a, b), n
        got[n] = a
    assert got["logpdf"].tolist() == [lines[0]["logpdf"]]

    import bench
    kind, N, D = bc.CONFIGS["c1"]
    assert kind == "se"
    X, y = bc.make_inputs(N, D)
    Xs = X / math.sqrt(D)
    sq = (Xs * Xs).sum(0)
    K = np.exp(-0.5 * np.maximum(sq[:, None] + sq[None, :] - 2.0 * Xs.T @ Xs, 0.0)) + bc.SIGMA2 * np.eye(N)
    Lr = np.linalg.cholesky(K)
    i, j = bench.factor_sample_positions(N)
    assert got["factor_sample"].shape == i.shape and got["factor_diag"].shape == (N,) == got["solved_row"].shape
    np.testing.assert_allclose(got["factor_diag"], np.diag(Lr), rtol=1e-9)
    np.testing.assert_allclose(got["factor_sample"], Lr[i, j], rtol=0, atol=1e-9)
    np.testing.assert_allclose(got["solved_row"], np.linalg.solve(Lr, y), rtol=0, atol=1e-7)
    lp = -0.5 * (N * math.log(2 * math.pi) + 2 * np.log(got["factor_diag"]).sum() + (got["solved_row"] ** 2).sum())
    assert abs(lp - got["logpdf"][0]) < 1e-10 * abs(got["logpdf"][0])
