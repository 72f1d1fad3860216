"""`bench.py --dump-outputs`: what the last timed step computed lands as float32 .npy files, cut to a fixed sample when the
arrays exceed the size limit (host-side logic on CPU tensors; the GPU run is tests/test_bench_dump_gpu.py)."""
import os
import types

import numpy as np
import torch

import bench


class _Ema:
    def average(self, p):
        return p * 0.5


def _model(sizes):
    g = torch.Generator().manual_seed(3)
    ps = [torch.randn(n, generator=g) for n in sizes]
    return types.SimpleNamespace(gen_params=ps[:2], disc_params=ps[2:], ema=_Ema())


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_output_as_float32(tmp_path):
    m = _model([10, 20, 30])
    last = {"distance": torch.tensor(0.25), "entropy": torch.tensor(-1.5, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path), m, last)
    out = _read(tmp_path)
    assert set(out) == {"distance", "entropy", "generator_weights", "critic_weights", "generator_ema_weights"}
    assert all(v.dtype == np.float32 for v in out.values())
    assert out["distance"].tolist() == [0.25] and out["entropy"].tolist() == [-1.5]
    np.testing.assert_array_equal(out["generator_weights"], torch.cat(m.gen_params).numpy())
    np.testing.assert_array_equal(out["critic_weights"], m.disc_params[0].numpy())
    np.testing.assert_array_equal(out["generator_ema_weights"], torch.cat(m.gen_params).numpy() * 0.5)


def test_dump_over_the_limit_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    m = _model([1000, 1000, 3000])
    last = {"distance": torch.tensor(1.0), "entropy": torch.tensor(2.0)}
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), m, last)
    bench.dump_outputs(str(b), m, last)
    ra, rb = _read(a), _read(b)
    assert sum(v.nbytes for v in ra.values()) <= 4096
    assert ra["distance"].tolist() == [1.0] and ra["entropy"].tolist() == [2.0]
    for k in ra:
        np.testing.assert_array_equal(ra[k], rb[k])
    full = m.disc_params[0].numpy()
    assert 0 < ra["critic_weights"].size < full.size
    assert np.isin(ra["critic_weights"], full).all()
