"""bench.py as it is run for every change: a plain `--gpus 1 --steps N --warmup W` run prints one JSON
line with the headline figure and nothing that takes runs of its own, and `--dump-outputs DIR` writes
outputs of the timed step that are the same from run to run, whatever N and W are."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def two_runs(tmp_path_factory):
    """Two plain runs, one after the other (two processes sharing the GPU reorder each other's atomic
    reductions), with different numbers of steps, each dumping its outputs."""
    base = tmp_path_factory.mktemp("bench")
    runs = []
    for n in (3, 5):
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(n),
                            "--warmup", "2", "--dump-outputs", str(base / f"dump{n}")],
                           capture_output=True, text=True, timeout=120)
        runs.append((n, r.returncode, r.stdout, r.stderr, base / f"dump{n}"))
    return runs


def test_plain_run_result_line(two_runs):
    for n, rc, out, err, _ in two_runs:
        assert rc == 0, err[-2000:]
        lines = out.splitlines()
        assert len(lines) == 1, out[:500]
        res = json.loads(lines[0])
        assert res["unit"] == "frames/s" and res["higher_is_better"] is True and res["dtype"] == "bf16"
        assert (res["steps"], res["warmup"], res["n_gpus"]) == (n, 2, 1)
        assert res["ms_per_step"] > 0 and res["value"] == pytest.approx(8 * 1e3 / res["ms_per_step"], rel=1e-3)
        assert not {"roofline", "roofline_bwd", "cpu_baseline"} & set(res)  # measured with --full only


def test_dumped_outputs_are_the_same_from_run_to_run(two_runs):
    """One step from the initial state: the loss to the fp32 reduction's rounding (the bound
    test_gpu_captured_step sets between a replay and an eager step), each gradient to one bf16 rounding
    flipped by the reordered fp32 sums of the atomic weight-gradient reductions (spacing <= 2^-7 |g|)."""
    dumps = []
    for _, rc, _, err, d in two_runs:
        assert rc == 0, err[-2000:]
        assert sorted(os.listdir(d)) == ["grads.npy", "loss.npy"]
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64e6
        dumps.append({n: np.load(d / f"{n}.npy") for n in ("loss", "grads")})
    a, b = dumps
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for x in dumps for v in x.values())
    assert a["loss"].shape == () and a["grads"].shape == b["grads"].shape and np.abs(a["grads"]).max() > 0
    d = np.abs(a["grads"].astype(np.float64) - b["grads"])
    print(f"loss {a['loss']} {b['loss']} grads: max |g| {np.abs(a['grads']).max():.3e} max diff {d.max():.3e} "
          f"differing {int((d > 0).sum())} of {d.size}")
    np.testing.assert_allclose(a["loss"], b["loss"], rtol=1e-5, atol=1e-6)
    assert (d <= 2.0 ** -7 * np.abs(a["grads"]) + 1e-6 * np.abs(a["grads"]).max()).all()
    assert np.linalg.norm(d) <= 1e-3 * np.linalg.norm(a["grads"])
