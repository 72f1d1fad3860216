"""GPU: train.main on the device-resident uint8 data path (utils/data.py, csrc/data.hip).

  * `--dataset cifar10 --data_on_device` feeds `OTGAN.step` the same bits as the default host path, step for step, so the
    printed distances and the final parameters are equal too (steps are run-to-run deterministic:
    tests/test_train_main_gpu.py::test_resumed_step_is_bit_identical);
  * the downsampled-ImageNet layout and a .npy file train both models at 64 x 64, and 64 x 64 data feeds a 32 x 32 model
    through the box-downsample; the batches are those of tests/data_ref.py for the permutation, offsets and flips the
    loop chose;
  * fid.dataset_stats over a DeviceDataset equals dataset_stats over the float array of the same images."""
import functools
import re

import numpy as np
import pytest
import torch

import data_ref as R
import inception_graphs as G
from otgan_amd.utils import data as D
from otgan_amd.utils import fid, inception_net, tfgraph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL_BOX = 1.2e-7          # tests/test_data_gpu.py: one ulp of a quotient in [1, 2); bit equality is expected


@pytest.fixture
def recorded_steps(monkeypatch):
    """Every `x_data` handed to OTGAN.step, cloned."""
    from otgan_amd.trainer import OTGAN
    rec, orig = [], OTGAN.step

    def step(self, x, *a, **k):
        rec.append(x.detach().clone())
        return orig(self, x, *a, **k)

    monkeypatch.setattr(OTGAN, "step", step)
    return rec


@pytest.fixture
def recorded_requests(monkeypatch):
    """(permutation, offsets, B, flip) of every DeviceDataset.batch call."""
    rec, orig = [], D.DeviceDataset.batch

    def batch(self, offsets, B, flip=None):
        rec.append((self.perm.cpu().numpy().copy(), list(offsets), B, None if flip is None else flip.cpu().numpy().copy()))
        return orig(self, offsets, B, flip)

    monkeypatch.setattr(D.DeviceDataset, "batch", batch)
    return rec


def _distances(out):
    """The numbers of the 'Iteration ...' lines without the wall-clock field."""
    return [re.sub(r"time = \d+s, ", "", l) for l in out.splitlines() if l.startswith("Iteration")]


def _tensors(sd, prefix=""):
    for k, v in sd.items():
        if torch.is_tensor(v):
            yield prefix + k, v
        elif isinstance(v, dict):
            yield from _tensors(v, prefix + k + "/")


def test_host_path_and_device_path_feed_the_same_bits(tmp_path, capsys, recorded_steps):
    from otgan_amd import train
    root = R.write_cifar(tmp_path / "data", R.images(64, 32, seed=21))
    common = ["--data_dir", root, "--nr_gpu", "2", "--batch_size", "8", "--nr_sinkhorn_iter", "5", "--max_steps", "4",
              "--sinkhorn_lambda", "100", "--nr_gen_per_disc", "2", "--seed", "5"]
    runs = []
    for extra in ([], ["--data_on_device"]):
        del recorded_steps[:]
        m = train.main(common + extra + ["--save_dir", str(tmp_path / ("run%d" % len(runs)))])
        out = capsys.readouterr().out
        runs.append((list(recorded_steps), _distances(out), dict(_tensors(m.state_dict()))))
    (xa, da, pa), (xb, db, pb) = runs
    assert len(xa) == len(xb) == 4 and xa[0].shape == (16, 32, 32, 3)
    for i in range(4):
        assert torch.equal(xa[i], xb[i]), "step %d" % i
    assert not torch.equal(xa[0], xa[1])                                         # (different steps are different batches)
    assert len(da) == 1 and "train distance before gen" in da[0] and "nan" not in da[0]
    assert da == db
    assert pa.keys() == pb.keys() and len(pa) > 10
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k


def _check_recorded(x, S, steps, requests, nr_batches, B, tol):
    assert len(steps) == len(requests) > 0
    differ = 0
    for t, (got, (perm, offs, b, flip)) in enumerate(zip(steps, requests)):
        assert b == B and offs == [(t % nr_batches + s * nr_batches) * B for s in range(2)]      # train.py:209-211
        assert sorted(perm.tolist()) == list(range(x.shape[0])) and flip is not None and flip.shape == (2 * B,)
        want = torch.from_numpy(R.batch(x, S, offs, B, perm, flip)).to(DEV)
        assert got.shape == want.shape and float((got - want).abs().max()) <= tol
        differ += int((got != want).sum())
    return differ


@pytest.mark.parametrize("size", [64, 32])
def test_imagenet64_layout_trains_dcgan(tmp_path, capsys, recorded_steps, recorded_requests, size):
    from otgan_amd import train
    x = R.images(32, 64, seed=22)
    root = R.write_imagenet64(tmp_path / "inet", x, files=2)
    m = train.main(["--model", "dcgan", "--image_size", str(size), "--dataset", "imagenet64", "--data_dir", root,
                    "--nr_gpu", "2", "--batch_size", "8", "--nr_sinkhorn_iter", "5", "--sinkhorn_lambda", "100",
                    "--max_steps", "2", "--nr_gen_per_disc", "1", "--save_dir", str(tmp_path / "run")])
    out = capsys.readouterr().out
    assert m.step_counter == 2
    d = _distances(out)
    assert len(d) == 1 and "nan" not in d[0] and "inf" not in d[0]
    vals = [float(v) for v in re.findall(r"= (-?[0-9.]+(?:e-?\d+)?)", d[0])]
    assert len(vals) == 3 and np.isfinite(vals).all()
    differ = _check_recorded(x, size, recorded_steps, recorded_requests, 2, 8, 0.0 if size == 64 else TOL_BOX)
    print("imagenet64 -> %d: %d elements of 2 batches not identical to data_ref" % (size, differ))
    flips = np.concatenate([r[3] for r in recorded_requests])
    assert 0 < int(flips.sum()) < flips.size                                     # the coin of train.py:163-170 was thrown


def test_npy_file_trains_densenet_at_64(tmp_path, capsys, recorded_steps, recorded_requests):
    from otgan_amd import train
    x = R.images(32, 64, seed=22)
    np.save(tmp_path / "images.npy", x)
    m = train.main(["--model", "densenet", "--image_size", "64", "--dataset", "npy", "--data_dir", str(tmp_path / "images.npy"),
                    "--nr_gpu", "2", "--batch_size", "4", "--nr_sinkhorn_iter", "5", "--sinkhorn_lambda", "100",
                    "--max_steps", "1", "--save_dir", str(tmp_path / "run")])
    try:
        assert m.step_counter == 1
        assert "nan" not in _distances(capsys.readouterr().out)[0].split("before disc")[1].split(",")[0]
        assert _check_recorded(x, 64, recorded_steps, recorded_requests, 4, 4, 0.0) == 0
    finally:
        m.close()


def test_image_size_the_data_cannot_feed_fails_before_the_model(tmp_path, monkeypatch):
    from otgan_amd import train, trainer
    np.save(tmp_path / "images.npy", R.images(8, 64, seed=1))

    def no_model(*a, **k):
        raise AssertionError("the model was built")

    monkeypatch.setattr(trainer.OTGAN, "__init__", no_model)
    with pytest.raises(ValueError, match="cannot feed --image_size 48"):
        train.main(["--dataset", "npy", "--data_dir", str(tmp_path / "images.npy"), "--image_size", "48",
                    "--nr_gpu", "2", "--batch_size", "2", "--save_dir", str(tmp_path / "run")])


def test_synthetic_store_and_data_dependent_init(tmp_path, capsys, recorded_steps):
    """--synthetic --data_on_device: a uint8 store of --synthetic_size images at --image_size (what tools/bench_input.py uses);
    --data_dependent_init takes its batch from the store."""
    from otgan_amd import train
    m = train.main(["--synthetic", "--synthetic_size", "32", "--data_on_device", "--data_dependent_init", "--nr_gpu", "2",
                    "--batch_size", "8", "--nr_sinkhorn_iter", "5", "--sinkhorn_lambda", "100", "--max_steps", "2",
                    "--save_dir", str(tmp_path / "run")])
    assert m.step_counter == 2 and len(recorded_steps) == 2
    x = recorded_steps[0]
    assert x.shape == (16, 32, 32, 3) and x.dtype == torch.float32
    assert bool(torch.isin(x, torch.from_numpy(R.lut()).to(DEV)).all())          # every value is a table entry
    assert "nan" not in _distances(capsys.readouterr().out)[0]


@functools.lru_cache(maxsize=None)
def _net():
    _, data = G.narrow_graph()
    return inception_net.InceptionNet(inception_net.lower(tfgraph.parse_graph(data)), DEV)


def test_fid_statistics_from_the_store_equal_those_from_the_float_array():
    net = _net()
    u8 = G.images(50, seed=4).astype(np.uint8)
    floats = R.convert(u8, 32)
    mu_h, sigma_h, n_h = fid.dataset_stats(net, floats)
    ds = D.DeviceDataset(u8, DEV, 32)
    mu_d, sigma_d, n_d = fid.dataset_stats(net, ds)
    assert n_h == n_d == 50 and np.array_equal(mu_h, mu_d) and np.array_equal(sigma_h, sigma_d)
    mu_4, _, n_4 = fid.dataset_stats(net, ds.head(20))                            # --fid_real_samples
    assert n_4 == 20 and np.array_equal(mu_4, fid.dataset_stats(net, floats[:20])[0])
