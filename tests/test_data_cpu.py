"""CPU: the loaders of utils/data.py on files written into tmp_path, every ValueError they and DeviceDataset's host-side
checks promise, and the new command-line flags (--dataset, --data_on_device).  No device is touched."""
import numpy as np
import pytest

import data_ref as R
from otgan_amd.utils import data as D


def test_cifar10_equals_load_cifar_after_the_table(tmp_path):
    from otgan_amd import train
    x = R.images(20, 32, seed=1)
    root = R.write_cifar(tmp_path, x)
    u8 = D.load_u8("cifar10", root)
    assert u8.dtype == np.uint8 and u8.shape == (20, 32, 32, 3) and u8.flags.c_contiguous
    assert np.array_equal(u8, x)
    want = train.load_cifar(root)
    got = R.lut()[u8]
    assert got.dtype == np.float32 and np.array_equal(got, want)              # bit for bit: no NaN in either
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("npz", [False, True])
def test_imagenet64_pickle_and_npz(tmp_path, npz):
    x = R.images(6, 64, seed=2)
    x[3, :, :, 0], x[3, :, :, 1], x[3, :, :, 2] = 10, 20, 30                     # planar -> NHWC: channels that differ
    x[3, 5, 9] = (1, 2, 3)
    root = R.write_imagenet64(tmp_path / "inet", x, files=2, npz=npz)
    u8 = D.load_u8("imagenet64", root)
    assert u8.dtype == np.uint8 and u8.shape == (6, 64, 64, 3)
    assert tuple(u8[3, 0, 0]) == (10, 20, 30) and tuple(u8[3, 5, 9]) == (1, 2, 3) and tuple(u8[3, 9, 5]) == (10, 20, 30)
    assert np.array_equal(u8, x)


def test_imagenet64_validation_split_and_missing_files(tmp_path):
    import pickle
    x = R.images(3, 64, seed=3)
    with open(tmp_path / "val_data", "wb") as f:
        pickle.dump({"data": R.planar(x), "labels": [1, 2, 3]}, f)
    assert np.array_equal(D.load_u8("imagenet64", str(tmp_path), subset="test"), x)
    with pytest.raises(FileNotFoundError):
        D.load_u8("imagenet64", str(tmp_path))                                   # no train_data_batch_*
    with open(tmp_path / "train_data_batch_1", "wb") as f:
        pickle.dump({"data": R.planar(x)[:, :3072]}, f)                          # 32 x 32 rows in a 64 x 64 layout
    with pytest.raises(ValueError, match=r"uint8 3x3072"):
        D.load_u8("imagenet64", str(tmp_path))


def test_imagenet64_says_what_it_found_and_warns_of_a_partial_set(tmp_path, capsys):
    import warnings
    x = R.images(20, 64, seed=4)
    part = R.write_imagenet64(tmp_path / "part", x[:4], files=2)
    with pytest.warns(UserWarning, match=r"only 2 of train_data_batch_1 \.\.\. train_data_batch_10 .* 4 images"):
        D.load_u8("imagenet64", part)
    assert "2 of 10 batch files" in capsys.readouterr().out
    whole = R.write_imagenet64(tmp_path / "whole", x, files=10)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.array_equal(D.load_u8("imagenet64", whole), x)
    assert "10 of 10 batch files" in capsys.readouterr().out and "20 images" not in capsys.readouterr().err


def test_npy_is_memory_mapped_and_npz_keys(tmp_path):
    x = R.images(5, 16, seed=4)
    np.save(tmp_path / "a.npy", x)
    a = D.load_u8("npy", str(tmp_path / "a.npy"))
    assert isinstance(a, np.memmap) and not a.flags.writeable and np.array_equal(a, x)
    for key in ("images", "data"):
        np.savez(tmp_path / ("b_%s.npz" % key), **{key: x, "labels": np.arange(5)})
        assert np.array_equal(D.load_u8("npy", str(tmp_path / ("b_%s.npz" % key))), x)
    np.savez(tmp_path / "c.npz", pictures=x)
    with pytest.raises(ValueError, match="pictures"):
        D.load_u8("npy", str(tmp_path / "c.npz"))


@pytest.mark.parametrize("arr,says", [
    (np.zeros((4, 16, 16, 3), np.float32), r"float32 4x16x16x3"),               # dtype
    (np.zeros((4, 16, 16), np.uint8), r"uint8 4x16x16"),                         # rank
    (np.zeros((4, 16, 12, 3), np.uint8), r"uint8 4x16x12x3"),                    # not square
    (np.zeros((4, 16, 16, 4), np.uint8), r"uint8 4x16x16x4"),                    # not RGB
])
def test_npy_rejects_anything_but_square_uint8_rgb(tmp_path, arr, says):
    np.save(tmp_path / "bad.npy", arr)
    with pytest.raises(ValueError, match=says):
        D.load_u8("npy", str(tmp_path / "bad.npy"))
    with pytest.raises(ValueError, match=says):
        D.DeviceDataset(arr, "cuda:0", 16)                                       # checked before the device is touched


def test_unknown_dataset_name():
    with pytest.raises(ValueError, match="cifar10, imagenet64, npy"):
        D.load_u8("lsun", "/nowhere")


def test_image_size_the_data_cannot_feed():
    assert D.feedable_sizes(64) == [64, 32, 16] and D.feedable_sizes(32) == [32, 16, 8] and D.feedable_sizes(6) == []
    assert D.feedable_sizes(20) == [20] and D.feedable_sizes(24) == [24, 12]
    assert D.check_image_size(64, 64) == 1 and D.check_image_size(64, 32) == 2 and D.check_image_size(128, 32) == 4
    with pytest.raises(ValueError, match=r"64 x 64 data cannot feed --image_size 48: it feeds 64 \| 32 \| 16"):
        D.check_image_size(64, 48)
    with pytest.raises(ValueError, match="--image_size 64"):                     # no up-sampling
        D.check_image_size(32, 64)
    with pytest.raises(ValueError, match="--image_size 48"):                     # DeviceDataset says it before any device work
        D.DeviceDataset(np.zeros((2, 64, 64, 3), np.uint8), "cuda:0", 48)


def test_permutation_range_is_checked_on_the_host():
    p = D.check_permutation(np.array([3, 0, 6, 6], np.int64), 7)
    assert p.dtype == np.int32 and p.tolist() == [3, 0, 6, 6]                    # repeats are allowed: a gather
    with pytest.raises(ValueError, match=r"3 \.\.\. 7 leave the store's 0 \.\.\. 6"):
        D.check_permutation(np.array([3, 7]), 7)
    with pytest.raises(ValueError, match=r"-1 \.\.\. 2"):
        D.check_permutation(np.array([2, -1]), 7)
    with pytest.raises(ValueError):
        D.check_permutation(np.array([0.0, 1.0]), 7)
    with pytest.raises(ValueError):
        D.check_permutation(np.zeros((2, 2), np.int64), 7)
    with pytest.raises(ValueError):
        D.check_permutation(np.zeros(0, np.int64), 7)


def test_new_flags_and_their_trainer_defaults():
    from otgan_amd.train import build_parser, uses_device_data
    from otgan_amd.trainer import default_args
    ns = build_parser().parse_args([])
    d = default_args()
    assert ns.dataset == "cifar10" == d.dataset and ns.data_on_device is False and d.data_on_device is False
    assert not uses_device_data(ns) and not uses_device_data(d)                 # an old command line: the host path
    assert uses_device_data(build_parser().parse_args(["--data_on_device"]))
    for name in ("imagenet64", "npy"):
        ns = build_parser().parse_args(["--dataset", name])
        assert ns.data_on_device is False and uses_device_data(ns)              # no host-float path on purpose
    assert not uses_device_data(build_parser().parse_args(["--synthetic"]))
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--dataset", "lsun"])
