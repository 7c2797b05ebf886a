"""bench.py --dump-outputs on CPU tensors: the full stack when it fits the limit, the same seeded sample of every layer past it."""
import os

import numpy as np
import torch

import bench


def _outs(L, M, N):
    g = torch.Generator().manual_seed(1)
    return [torch.randn(M, N, generator=g).half() for _ in range(L)]


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_writes_every_layer_in_float32(tmp_path):
    outs = _outs(64, 1, 4096)
    assert bench.dump_outputs(outs, str(tmp_path)) == {"out": [64, 1, 4096]}
    assert sorted(os.listdir(tmp_path)) == ["out.npy"]
    a = np.load(tmp_path / "out.npy")
    assert a.dtype == np.float32 and np.array_equal(a, torch.stack(outs).float().numpy())


def test_dump_past_the_limit_is_a_fixed_sample_within_it(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    outs = _outs(8, 256, 512)  # 4 MiB as float32
    info = bench.dump_outputs(outs, str(tmp_path / "a"))
    assert info["of"] == [8, 256, 512] and sorted(os.listdir(tmp_path / "a")) == ["out_sample.npy", "out_sample_index.npy"]
    assert _size(tmp_path / "a") <= bench.DUMP_LIMIT_BYTES
    v, i = np.load(tmp_path / "a" / "out_sample.npy"), np.load(tmp_path / "a" / "out_sample_index.npy")
    assert v.dtype == np.float32 and i.dtype == np.float64 and v.shape == (8, i.size) and i.size > 0
    assert np.all(np.diff(i) > 0)
    assert np.array_equal(v, torch.stack(outs).float().reshape(8, -1).numpy()[:, i.astype(np.int64)])
    bench.dump_outputs(outs, str(tmp_path / "b"))
    assert np.array_equal(np.load(tmp_path / "b" / "out_sample_index.npy"), i)


def test_dump_replaces_an_earlier_dump_of_another_shape(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    bench.dump_outputs(_outs(8, 256, 512), str(tmp_path))
    bench.dump_outputs(_outs(2, 1, 64), str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["out.npy"]
