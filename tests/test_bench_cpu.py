"""bench.py's --dump-outputs writer on host tensors: names, exact dtype conversion, the 64 MB budget and its seeded sample."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _total(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_names_and_exact_dtypes(tmp_path):
    g = torch.Generator().manual_seed(0)
    atlas = torch.rand((64, 64, 3), generator=g)
    faces = torch.randint(0, 1 << 30, (50, 3), generator=g, dtype=torch.int64)
    mask = torch.rand((1, 64, 64, 1), generator=g) > 0.5
    full = (torch.rand((20, 3), generator=g), None, faces, None, atlas, mask)       # colorize_one_mesh's 6-tuple
    info = bench.dump_outputs(full, str(tmp_path / "one"))
    assert sorted(os.listdir(tmp_path / "one")) == ["atlas.npy", "faces.npy", "mask.npy", "vertices.npy"]
    assert info["faces"]["dtype"] == "float64" and info["mask"]["dtype"] == "float32" and not any(v["sampled"] for v in info.values())
    assert np.array_equal(np.load(tmp_path / "one" / "faces.npy"), faces.numpy().astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "one" / "mask.npy"), mask.numpy().astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "one" / "atlas.npy"), atlas.numpy())
    bench.dump_outputs([atlas, atlas * 2], str(tmp_path / "list"))                   # colorize_meshes_batched / ShapeGraphs: atlases
    assert sorted(os.listdir(tmp_path / "list")) == ["shape0_atlas.npy", "shape1_atlas.npy"]
    assert np.array_equal(np.load(tmp_path / "list" / "shape1_atlas.npy"), (atlas * 2).numpy())


def test_dump_stays_within_the_budget_with_a_fixed_sample(tmp_path):
    big = [torch.full((1024, 1024, 3), float(i)) + torch.arange(1024 * 1024 * 3, dtype=torch.float32).reshape(1024, 1024, 3)
           for i in range(6)]                                                         # 75.5 MB as float32
    info = bench.dump_outputs(big, str(tmp_path / "a"))
    assert all(v["sampled"] for v in info.values())
    assert _total(tmp_path / "a") <= bench.DUMP_BUDGET_BYTES
    bench.dump_outputs(big, str(tmp_path / "b"))
    for f in os.listdir(tmp_path / "a"):
        a = np.load(tmp_path / "a" / f)
        assert np.array_equal(a, np.load(tmp_path / "b" / f))                         # the same sample every run
        assert np.all(np.diff(a) > 0)                                                 # sorted flat indices of the original
    small = [torch.zeros((1024, 1024, 3)) for _ in range(4)]                           # the default bench step: written whole
    info = bench.dump_outputs(small, str(tmp_path / "c"))
    assert not any(v["sampled"] for v in info.values()) and _total(tmp_path / "c") <= bench.DUMP_BUDGET_BYTES
