"""numpy restatement of `otgan_batch_from_u8_f32` (include/otgan_layers.h; csrc/data.hip) and small fixtures in the on-disk
layouts `utils.data.load_u8` reads.  Shared by tests/test_data_cpu.py, test_data_gpu.py and test_data_train_gpu.py."""
import os
import pickle

import numpy as np


def lut():
    """The table the host passes: the very expression of train.load_cifar (train.py:158)."""
    return np.arange(256, dtype=np.float32) / 127.5 - 1.


def convert(u8, S):
    """uint8 [n, H, H, 3] -> float32 [n, S, S, 3]: the table at H == S, else the exact integer sum of every f x f box,
    then (float)sum / (127.5f f f) - 1.0f in fp32 (127.5 f f is 510 or 2040: exact)."""
    n, H = u8.shape[0], u8.shape[1]
    f = H // S
    assert u8.dtype == np.uint8 and u8.shape == (n, f * S, f * S, 3) and f in (1, 2, 4) and S % 4 == 0
    if f == 1:
        return lut()[u8]
    s = u8.reshape(n, S, f, S, f, 3).astype(np.int64).sum(axis=(2, 4))
    return s.astype(np.float32) / np.float32(127.5 * f * f) - np.float32(1.0)


def batch(store, S, offsets, B, perm=None, flip=None):
    """Row s * B + k = image (perm[offsets[s] + k] | offsets[s] + k), converted, mirrored in x where flip[s * B + k].
    (Mirroring the output equals reading the box at (f y, f (S - 1 - x)): the boxes tile the line.)"""
    idx = np.concatenate([np.arange(o, o + B) for o in offsets])
    if perm is not None:
        idx = np.asarray(perm)[idx]
    out = convert(store[idx], S)
    if flip is not None:
        m = np.asarray(flip).astype(bool)
        out[m] = out[m][:, :, ::-1]
    return out


def images(n, side, seed=0):
    """uint8 [n, side, side, 3] with every byte value present, no left-right symmetry and three different channels."""
    rng = np.random.RandomState(seed)
    x = rng.randint(0, 256, size=(n, side, side, 3)).astype(np.uint8)
    x.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    return x


def planar(x):
    """NHWC uint8 -> the [n, 3 H W] channel-planar rows of the CIFAR / downsampled-ImageNet pickles."""
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2)).reshape(x.shape[0], -1)


def write_cifar(root, x):
    """x: uint8 [n >= 5, 32, 32, 3] -> <root>/cifar-10-python/cifar-10-batches-py/data_batch_1 ... 5 (in order, about equal)."""
    d = os.path.join(str(root), "cifar-10-python", "cifar-10-batches-py")
    os.makedirs(d)
    for i, part in enumerate(np.array_split(x, 5)):
        with open(os.path.join(d, "data_batch_%d" % (i + 1)), "wb") as f:
            pickle.dump({"data": planar(part), "labels": [0] * part.shape[0]}, f)
    return str(root)


def write_imagenet64(root, x, files=2, npz=False):
    """x: uint8 [n, 64, 64, 3] -> <root>/train_data_batch_1 ... `files` (pickles with data / labels / mean, or .npz)."""
    os.makedirs(str(root), exist_ok=True)
    per = x.shape[0] // files
    assert per * files == x.shape[0]
    for i in range(files):
        e = {"data": planar(x[i * per:(i + 1) * per]), "labels": list(range(1, per + 1)), "mean": np.zeros(12288)}
        path = os.path.join(str(root), "train_data_batch_%d" % (i + 1))
        if npz:
            np.savez(path + ".npz", **{k: np.asarray(v) for k, v in e.items()})
        else:
            with open(path, "wb") as f:
                pickle.dump(e, f)
    return str(root)
