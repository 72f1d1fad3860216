"""Training data as a device-resident uint8 store (train.py --data_on_device, --dataset imagenet64 | npy).

The reference keeps the whole set as float32 on the host and, per step, gathers a batch by the epoch's permutation,
copies it to the device and flips it there (train.py:158,163-170,209-211).  Here the set is uploaded ONCE as uint8 NHWC
(CIFAR-10: 154 MB; ImageNet 64 x 64: 15.7 GB, where float32 on the host would be 63 GB) and one launch per step
(csrc/data.hip, `otgan_batch_from_u8_f32`) produces the step's float32 batch: gather, flip, uint8 -> [-1, 1], and an
integer box-downsample by 2 or 4 when the stored images are larger than the model's.  Nothing goes through the host.

    load_u8(dataset, data_dir, subset)     -> uint8 [n, H, W, 3] (numpy; a memory map for .npy files)
    DeviceDataset(u8, device, image_size)  -> the store, the conversion table and the epoch's permutation on the device
    load_labels(dataset, data_dir, subset) -> int64 [n] class labels of the same images, or None (utils/probe.py; never fed
                                              to training)

The table is `np.arange(256, dtype=np.float32) / 127.5 - 1.`, the expression train.load_cifar applies to the same bytes,
so at equal sizes the device path returns the host path's bits.
"""
import copy
import os
import pickle
import warnings

import numpy as np

DATASETS = ("cifar10", "imagenet64", "npy")
FACTORS = (1, 2, 4)                 # stored side / image_size the kernel takes (otgan_layers.h)
CHUNK_BYTES = 256 << 20             # largest single host -> device copy of the upload


def _check_u8_images(a, what):
    """uint8 [n, H, W, 3] with H = W, or a ValueError that names what was found."""
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3 or a.shape[1] != a.shape[2] or a.shape[0] < 1:
        raise ValueError("%s: expected uint8 images [n, H, W, 3] with H = W, found %s %s"
                         % (what, a.dtype, "x".join(str(d) for d in a.shape) or "scalar"))
    return a


def _planar_rows_to_nhwc(rows, side, what):
    """[n, 3 * side * side] channel-planar uint8 rows (the CIFAR / downsampled-ImageNet pickles) -> NHWC."""
    rows = np.asarray(rows)
    if rows.dtype != np.uint8 or rows.ndim != 2 or rows.shape[1] != 3 * side * side:
        raise ValueError("%s: expected uint8 rows [n, %d], found %s %s"
                         % (what, 3 * side * side, rows.dtype, "x".join(str(d) for d in rows.shape) or "scalar"))
    return rows.reshape(-1, 3, side, side).transpose(0, 2, 3, 1)


def _load_pickle_or_npz(path, key="data"):
    """`path` (a pickle holding a dict) or `path`.npz, whichever exists -> the array under `key`; None when neither does."""
    if os.path.exists(path):
        with open(path, "rb") as fo:
            return pickle.load(fo, encoding="latin1")[key]
    if os.path.exists(path + ".npz"):
        with np.load(path + ".npz") as f:
            return f[key]
    return None


def load_u8(dataset, data_dir, subset="train"):
    """uint8 [n, H, W, 3] of

    cifar10     <data_dir>/cifar-10-python/cifar-10-batches-py/data_batch_1 ... 5 | test_batch: the layout train.load_cifar
                reads (reference data/cifar10_data.py:40-53); 32 x 32
    imagenet64  the downsampled-ImageNet batches directly under <data_dir>: train_data_batch_1 ... 10 (those that are there,
                at least one; the count is printed, and fewer than 10 warn that this is a part of the set) | val_data for
                subset 'test'; pickles, or .npz files of the same names, whose `data` is uint8 [n, 12288], channel-planar like
                CIFAR; labels and `mean` are ignored; 64 x 64
    npy         data_dir IS a .npy file (opened as a read-only memory map) or an .npz file (key `images` or `data`) holding
                uint8 [n, H, W, 3] with H = W
    No download, no decoding."""
    if dataset == "cifar10":
        d = os.path.join(data_dir, "cifar-10-python", "cifar-10-batches-py")
        files = ["data_batch_%d" % i for i in range(1, 6)] if subset == "train" else ["test_batch"]
        xs = []
        for f in files:
            with open(os.path.join(d, f), "rb") as fo:
                e = pickle.load(fo, encoding="latin1")
            xs.append(_planar_rows_to_nhwc(e["data"], 32, os.path.join(d, f)))
        return np.ascontiguousarray(np.concatenate(xs, 0))
    if dataset == "imagenet64":
        files = ["train_data_batch_%d" % i for i in range(1, 11)] if subset == "train" else ["val_data"]
        xs = []
        for f in files:
            rows = _load_pickle_or_npz(os.path.join(data_dir, f))
            if rows is not None:
                xs.append(_planar_rows_to_nhwc(rows, 64, os.path.join(data_dir, f)))
        if not xs:
            raise FileNotFoundError("no %s (pickle or .npz) under %s" % (" ... ".join(files[::max(len(files) - 1, 1)]), data_dir))
        n = sum(x.shape[0] for x in xs)
        print("imagenet64 %s: %d of %d batch files under %s, %d images" % (subset, len(xs), len(files), data_dir, n))
        if len(xs) < len(files):
            warnings.warn("imagenet64: only %d of %s are under %s: training on %d images, a part of the set"
                          % (len(xs), " ... ".join(files[::len(files) - 1]), data_dir, n))
        return np.ascontiguousarray(np.concatenate(xs, 0))
    if dataset == "npy":
        if data_dir.endswith(".npz"):
            with np.load(data_dir) as f:
                keys = [k for k in ("images", "data") if k in f.files]
                if not keys:
                    raise ValueError("%s: no key `images` or `data` (it holds %s)" % (data_dir, ", ".join(f.files) or "nothing"))
                a = f[keys[0]]
        else:
            a = np.load(data_dir, mmap_mode="r")
        return _check_u8_images(a, data_dir)
    raise ValueError("--dataset %r: one of %s" % (dataset, ", ".join(DATASETS)))


def load_labels(dataset, data_dir, subset="train"):
    """int64 [n]: the class labels of the images `load_u8(dataset, data_dir, subset)` returns, in its order, or None when
    the files carry none (utils/probe.py scores features by them; training never reads them).

    cifar10     key `labels` of data_batch_1 ... 5 | test_batch
    imagenet64  key `labels` of the train batches that are there | val_data, as stored
    npy         key `labels` of an .npz; a bare .npy has none
    The row count must equal the image count of the same subset: a ValueError names both otherwise."""
    def checked(labels, images, where):
        labels = np.asarray(labels).reshape(-1).astype(np.int64)
        if labels.shape[0] != images:
            raise ValueError("%s: %d labels for %d images" % (where, labels.shape[0], images))
        return labels

    if dataset == "cifar10":
        d = os.path.join(data_dir, "cifar-10-python", "cifar-10-batches-py")
        files = ["data_batch_%d" % i for i in range(1, 6)] if subset == "train" else ["test_batch"]
        labels, images = [], 0
        for f in files:
            with open(os.path.join(d, f), "rb") as fo:
                e = pickle.load(fo, encoding="latin1")
            if "labels" not in e:
                return None
            labels.append(np.asarray(e["labels"]).reshape(-1))
            images += np.asarray(e["data"]).shape[0]
        return checked(np.concatenate(labels), images, d)
    if dataset == "imagenet64":
        files = ["train_data_batch_%d" % i for i in range(1, 11)] if subset == "train" else ["val_data"]
        labels, images = [], 0
        for f in files:
            path = os.path.join(data_dir, f)          # each file is opened once: a train batch is 1.2 GB unpickled
            if os.path.exists(path):
                with open(path, "rb") as fo:
                    e = pickle.load(fo, encoding="latin1")
                got, n = e.get("labels"), np.asarray(e["data"]).shape[0]
            elif os.path.exists(path + ".npz"):
                with np.load(path + ".npz") as e:
                    got, n = (e["labels"] if "labels" in e.files else None), e["data"].shape[0]
            else:
                continue
            if got is None:
                return None
            labels.append(np.asarray(got).reshape(-1))
            images += n
        if not labels:
            raise FileNotFoundError("no %s (pickle or .npz) under %s" % (" ... ".join(files[::max(len(files) - 1, 1)]), data_dir))
        return checked(np.concatenate(labels), images, data_dir)
    if dataset == "npy":
        if not data_dir.endswith(".npz"):
            return None
        with np.load(data_dir) as f:
            if "labels" not in f.files:
                return None
            keys = [k for k in ("images", "data") if k in f.files]
            if not keys:
                raise ValueError("%s: no key `images` or `data` (it holds %s)" % (data_dir, ", ".join(f.files) or "nothing"))
            return checked(f["labels"], f[keys[0]].shape[0], data_dir)
    raise ValueError("--dataset %r: one of %s" % (dataset, ", ".join(DATASETS)))


def feedable_sizes(side):
    """The image sizes a store of `side` x `side` images can feed: side / 1, 2, 4 where that is a whole multiple of 4."""
    return [side // f for f in FACTORS if side % f == 0 and (side // f) % 4 == 0 and side // f > 0]


def check_image_size(side, image_size):
    ok = feedable_sizes(side)
    if image_size not in ok:
        raise ValueError("%d x %d data cannot feed --image_size %d: it feeds %s (the stored side divided by 1, 2 or 4)"
                         % (side, side, image_size, " | ".join(str(s) for s in ok) or "no size"))
    return side // image_size


def check_permutation(inds, n):
    """The host-side check of set_permutation: a 1-D integer array with 0 <= min and max < n -> int32 copy.  The kernel
    trusts these values."""
    inds = np.asarray(inds)
    if inds.ndim != 1 or inds.size == 0 or inds.dtype.kind not in "iu":
        raise ValueError("a permutation is a non-empty 1-D integer array, found %s %s" % (inds.dtype, inds.shape))
    lo, hi = int(inds.min()), int(inds.max())
    if lo < 0 or hi >= n:
        raise ValueError("permutation values %d ... %d leave the store's 0 ... %d" % (lo, hi, n - 1))
    return inds.astype(np.int32)


class DeviceDataset:
    """uint8 [n, H, W, 3] on the device + the 256-entry conversion table + the current permutation (int32).

    batch(offsets, B, flip) -> float32 [len(offsets) * B, S, S, 3]: row s * B + k is image perm[offsets[s] + k], flipped where
                               flip[s * B + k]
    rows(lo, hi)            -> images lo ... hi - 1 in storage order, unflipped (init batch, FID statistics)
    `shape` is that of the float set the model sees, (n, S, S, 3), so code that reads `trainx.shape[0]` takes either."""

    def __init__(self, u8, device, image_size, chunk_bytes=CHUNK_BYTES):
        import torch
        _check_u8_images(u8, "DeviceDataset")
        self.factor = check_image_size(u8.shape[1], int(image_size))          # before anything touches the device
        if u8.shape[0] >= 2 ** 31:
            raise ValueError("%d images: the permutation is int32" % u8.shape[0])
        self.device = torch.device(device)
        if self.device.type != "cuda":
            from .. import _lib
            raise _lib.OtganError("DeviceDataset lives on a CUDA (MI355X) device; there is no CPU fallback")
        self.n, self.side, self.image_size = int(u8.shape[0]), int(u8.shape[1]), int(image_size)
        self.shape = (self.n, self.image_size, self.image_size, 3)
        self.store = torch.empty(u8.shape, dtype=torch.uint8, device=self.device)
        # bounded pieces: whole images (at least one) are copied into C order on the host, whether the source is pageable, a
        # memory map or a non-contiguous view of one, and go up in copies of at most chunk_bytes: no staging buffer of the
        # size of the set
        image_bytes, step = 3 * self.side * self.side, max(int(chunk_bytes), 1)
        per = max(step // image_bytes, 1)
        flat_dst = self.store.view(-1)
        for i in range(0, self.n, per):
            piece = np.array(u8[i:i + per], order="C").reshape(-1)
            for j in range(0, piece.shape[0], step):
                at = i * image_bytes + j
                flat_dst[at:at + min(step, piece.shape[0] - j)].copy_(torch.from_numpy(piece[j:j + step]))
        self.lut = torch.from_numpy(np.arange(256, dtype=np.float32) / 127.5 - 1.).to(self.device)    # train.py:158
        self.perm = None

    def __len__(self):
        return self.n

    def head(self, n):
        """The first n images as a dataset of their own (shares the store and the table; --fid_real_samples).  It starts without
        a permutation: the parent's may point past its n images, and one set on it is checked against its own n."""
        d = copy.copy(self)
        d.perm = None
        d.n = min(int(n), self.n)
        d.shape = (d.n,) + self.shape[1:]
        return d

    def set_permutation(self, inds):
        import torch
        self.perm = torch.from_numpy(check_permutation(inds, self.n)).to(self.device)

    def batch(self, offsets, B, flip=None):
        from .. import ops
        return ops.batch_from_u8(self.store, offsets, B, self.image_size, self.lut, perm=self.perm, flip=flip)

    def rows(self, lo, hi):
        import torch
        from .. import ops
        if not 0 <= lo <= hi <= self.n:
            raise IndexError("rows %d ... %d of %d" % (lo, hi, self.n))
        if hi == lo:
            return torch.empty(0, self.image_size, self.image_size, 3, dtype=torch.float32, device=self.device)
        return ops.batch_from_u8(self.store, [lo], hi - lo, self.image_size, self.lut)
