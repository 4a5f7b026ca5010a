"""bench.py --dump-outputs: what a step returned goes to DIR/<name>.npy as float32 / float64, an
output above its share of the size limit as a fixed seeded sample (host only, no GPU)."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_names_dtypes_and_values(tmp_path):
    ctx = torch.arange(24, dtype=torch.float32).reshape(1, 6, 4).requires_grad_(True)
    sel = [torch.tensor([3, 1, 2]), torch.tensor([5, 0, 4])]
    out = {"context": ctx, "selected_tokens": sel, "loss": torch.tensor(0.25), "visibility": None,
           "pair": (torch.zeros(2, dtype=torch.float64), torch.ones(3, dtype=torch.bool))}
    bench.dump_outputs(str(tmp_path / "d"), out)
    got = _load(str(tmp_path / "d"))
    assert sorted(got) == ["context", "loss", "pair_0", "pair_1", "selected_tokens"]
    assert got["context"].dtype == np.float32 and np.array_equal(got["context"], ctx.detach().numpy())
    assert got["selected_tokens"].dtype == np.float64                     # integers: exact in float64
    assert np.array_equal(got["selected_tokens"], [[3, 1, 2], [5, 0, 4]])
    assert got["loss"].dtype == np.float32 and got["loss"].shape == () and got["loss"] == 0.25
    assert got["pair_0"].dtype == np.float64 and got["pair_1"].dtype == np.float64


def test_dump_samples_large_outputs_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    big = torch.arange(10000, dtype=torch.float32).reshape(100, 100)
    small = torch.arange(10, dtype=torch.float32)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), {"big": big, "small": small})
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(v.nbytes for v in a.values()) <= 4096
    assert np.array_equal(a["small"], small.numpy())                      # under its share: whole
    assert a["big"].shape == (512,) and np.array_equal(a["big"], b["big"])   # the same sample every run
    assert len(np.unique(a["big"])) == 512 and np.all(np.diff(a["big"]) > 0)  # distinct elements, in order
