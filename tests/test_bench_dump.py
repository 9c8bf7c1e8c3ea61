"""CPU: what `bench.py --dump-outputs` writes (float32, a fixed seeded sample of an output above the size cap) and the refusal of a run
without timed steps."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    x = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    bench.dump_outputs(str(tmp_path / "a"), "latents", x)
    a = np.load(tmp_path / "a" / "latents.npy")
    assert a.dtype == np.float32 and a.shape == (2, 3, 4) and np.array_equal(a, x.float().numpy())

    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 100)
    big = torch.arange(1000, dtype=torch.float32)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), "latents", big)
    b, c = np.load(tmp_path / "b" / "latents_sample.npy"), np.load(tmp_path / "c" / "latents_sample.npy")
    assert not (tmp_path / "b" / "latents.npy").exists()
    assert b.dtype == np.float32 and b.shape == (100,) and np.array_equal(b, c)          # the same elements in every run
    assert np.all(np.diff(b) > 0)                                                          # distinct elements, in flat-index order


def test_zero_steps_is_refused():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0"], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode != 0 and "--steps 0" in out.stderr and "{" not in out.stdout
