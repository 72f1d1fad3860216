"""The k-NN probe without a GPU: the vote of utils/probe.py and the numpy restatement (tests/probe_ref.py) on cases worked
out by hand, deliberately wrong implementations that must fail a comparison, and utils.data.load_labels on tiny files."""
import pickle

import numpy as np
import pytest
import torch

import probe_ref
from otgan_amd.utils import data as udata
from otgan_amd.utils import probe

# rows of ranked neighbour labels and the class each predicts
VOTES = [([2, 1, 1, 2], 2),          # two against two: the class of the first-ranked member
         ([1, 2, 2, 1], 1),
         ([3, 1, 1, 0], 1),          # a plain majority, wherever it ranks
         ([0, 4, 4, 4], 4),
         ([5, -1, -1, -1], 5),       # empty slots do not vote
         ([7, 6, -1, -1], 7),
         ([6, 7, 7, -1], 7),
         ([-1, -1, -1, -1], -1),     # no neighbour: -1, never correct
         ([0, 0, 0, 0], 0)]


def test_vote_by_hand():
    lab = np.array([r for r, _ in VOTES], np.int64)
    want = np.array([p for _, p in VOTES], np.int64)
    assert np.array_equal(probe_ref.vote(lab), want)
    assert np.array_equal(probe.vote(torch.from_numpy(lab)).numpy(), want)
    assert np.array_equal(probe.vote(torch.from_numpy(lab[:, :1])).numpy(), lab[:, 0])       # 1-NN: the first neighbour
    assert probe.vote(torch.empty(0, 4, dtype=torch.int64)).shape == (0,)
    with pytest.raises(ValueError):
        probe.vote(torch.zeros(3, 4, dtype=torch.int32))


def test_vote_matches_reference_on_random_rows():
    rng = np.random.default_rng(0)
    for k in range(1, 9):
        lab = rng.integers(-1, 4, (200, k)).astype(np.int64)
        # empty slots trail the filled ones in a real result; anywhere is handled the same way
        assert np.array_equal(probe.vote(torch.from_numpy(lab)).numpy(), probe_ref.vote(lab))


def test_reference_topk_order_and_self_exclusion():
    y = np.array([[1.0, 0], [0, 1.0], [1.0, 0], [-1.0, 0], [1.0, 0]])
    idx, sc = probe_ref.topk(y[:1], y, 4)
    assert idx.tolist() == [[0, 2, 4, 1]] and sc.tolist() == [[1.0, 1.0, 1.0, 0.0]]          # ties: the smaller column first
    idx, sc = probe_ref.topk(y[:2], y, 8, self0=0)
    assert idx.tolist() == [[2, 4, 1, 3, -1, -1, -1, -1], [0, 2, 3, 4, -1, -1, -1, -1]]       # own column skipped, slots left empty
    assert np.isneginf(sc[0, 4:]).all() and sc[0, 3] == -1.0                                  # the most negative column is still there
    idx, sc = probe_ref.topk(y, y[:0], 2)
    assert (idx == -1).all() and np.isneginf(sc).all()


def test_accuracy_by_hand():
    bank = np.array([[1.0, 0], [0.9, 0.1], [0, 1.0], [0.1, 0.9], [0.6, 0.8]])
    labels = [0, 0, 1, 1, 1]
    q = np.array([[1.0, 0.05], [0.05, 1.0], [0.8, 0.6]])
    # the third query's neighbours are rows 4, 0, 1 (0.96, 0.80, 0.78): labels 1, 0, 0 -- the vote says 0, the first says 1
    assert probe_ref.accuracy(bank, labels, q, [0, 1, 0], 3) == (3, 2, 3)
    assert probe_ref.accuracy(bank, labels, q, [0, 1, 1], 3) == (2, 3, 3)
    assert probe_ref.accuracy(bank, labels, q, [0, 1, 1], 1) == (3, 3, 3)
    # leave one out: a row is never its own neighbour -- with distinct labels per row nothing can be right
    assert probe_ref.accuracy(bank, [0, 1, 2, 3, 4], None, None, 1, leave_one_out=True) == (0, 0, 5)
    assert probe_ref.accuracy(bank, labels, None, None, 1, leave_one_out=True) == (5, 5, 5)   # (with its own column every row would be right for any labels)
    # an empty bank: every row predicts -1
    assert probe_ref.accuracy(bank[:0], [], q, [0, 1, 0], 3) == (0, 0, 3)


def _wrong_vote_larger_label(neigh):
    """ties to the larger label instead of the higher rank"""
    out = []
    for row in np.asarray(neigh):
        labs = [l for l in row if l >= 0]
        out.append(max(labs, key=lambda l: (labs.count(l), l)) if labs else -1)
    return np.array(out, np.int64)


def _wrong_vote_ignores_rank(neigh):
    """ties to the smaller label: np.bincount(...).argmax()"""
    out = []
    for row in np.asarray(neigh):
        labs = [l for l in row if l >= 0]
        out.append(int(np.bincount(labs).argmax()) if labs else -1)
    return np.array(out, np.int64)


def _wrong_topk_larger_index(q, y, k, self0=-1):
    """equal scores by the LARGER column first"""
    d = np.asarray(q, np.float64) @ np.asarray(y, np.float64).T
    return np.stack([np.lexsort((-np.arange(d.shape[1]), -row))[:k] for row in d]).astype(np.int32)


def _wrong_topk_keeps_self(q, y, k, self0=-1):
    return probe_ref.topk(q, y, k, -1)[0]


def test_wrong_implementations_fail():
    lab = np.array([r for r, _ in VOTES], np.int64)
    want = probe_ref.vote(lab)
    assert not np.array_equal(_wrong_vote_larger_label(lab), want)
    assert not np.array_equal(_wrong_vote_ignores_rank(lab), want)
    y = np.array([[1.0, 0], [0, 1.0], [1.0, 0], [-1.0, 0], [1.0, 0]])
    assert not np.array_equal(_wrong_topk_larger_index(y[:1], y, 3), probe_ref.topk(y[:1], y, 3)[0])
    assert not np.array_equal(_wrong_topk_keeps_self(y, y, 2, 0), probe_ref.topk(y, y, 2, 0)[0])


def test_check_neighbours():
    assert probe.check_neighbours(5, 6) == 5 and probe.check_neighbours(1) == 1 and probe.check_neighbours(8) == 8
    for k in (0, 9):
        with pytest.raises(ValueError):
            probe.check_neighbours(k)
    with pytest.raises(ValueError):
        probe.check_neighbours(5, 5)


def test_flags_defaults_and_start_up_errors():
    from otgan_amd import train, trainer
    want = dict(probe_every=0, probe_neighbours=5, probe_train_samples=5000, probe_test_samples=1000)
    parsed, defaults = train.build_parser().parse_args([]), trainer.default_args()
    for name, value in want.items():
        assert getattr(parsed, name) == value and getattr(defaults, name) == value
    got = train.build_parser().parse_args("--probe_every 50 --probe_neighbours 3 --probe_train_samples 7 --probe_test_samples 9".split())
    assert (got.probe_every, got.probe_neighbours, got.probe_train_samples, got.probe_test_samples) == (50, 3, 7, 9)
    for k in ("0", "9"):                       # at start-up: before a device, a file or a rank is touched
        with pytest.raises(ValueError, match="--probe_neighbours"):
            train.main(["--synthetic", "--nr_gpu", "2", "--probe_every", "1", "--probe_neighbours", k])
    for flag in want:
        assert "--" + flag in train.__doc__


# ---------------------------------------------------------------- load_labels
def _cifar_dir(tmp_path, per=3, labels=True, test_labels=None):
    d = tmp_path / "cifar-10-python" / "cifar-10-batches-py"
    d.mkdir(parents=True)
    rng = np.random.default_rng(1)
    for n, f in enumerate(["data_batch_%d" % i for i in range(1, 6)] + ["test_batch"]):
        e = {"data": rng.integers(0, 256, (per, 3072), dtype=np.uint8)}
        if labels:
            e["labels"] = [(n * per + i) % 10 for i in range(per)]
        if f == "test_batch" and test_labels is not None:
            e["labels"] = test_labels
        with open(d / f, "wb") as fo:
            pickle.dump(e, fo)
    return str(tmp_path)


def test_load_labels_cifar(tmp_path):
    root = _cifar_dir(tmp_path)
    tr, te = udata.load_labels("cifar10", root), udata.load_labels("cifar10", root, "test")
    assert tr.dtype == np.int64 and tr.tolist() == [i % 10 for i in range(15)] and te.tolist() == [5, 6, 7]
    assert tr.shape[0] == udata.load_u8("cifar10", root).shape[0] and te.shape[0] == udata.load_u8("cifar10", root, "test").shape[0]


def test_load_labels_cifar_without_labels_and_mismatch(tmp_path):
    assert udata.load_labels("cifar10", _cifar_dir(tmp_path / "a", labels=False)) is None
    root = _cifar_dir(tmp_path / "b", test_labels=[1, 2])
    with pytest.raises(ValueError, match="2 labels for 3 images"):
        udata.load_labels("cifar10", root, "test")


def test_load_labels_imagenet64(tmp_path):
    rng = np.random.default_rng(2)
    for f, n, first in (("train_data_batch_1", 2, 1), ("train_data_batch_3", 3, 500), ("val_data", 2, 1000)):
        np.savez(tmp_path / (f + ".npz"), data=rng.integers(0, 256, (n, 12288), dtype=np.uint8), labels=np.arange(first, first + n))
    with pytest.warns(UserWarning):
        assert udata.load_u8("imagenet64", str(tmp_path)).shape[0] == 5
    assert udata.load_labels("imagenet64", str(tmp_path)).tolist() == [1, 2, 500, 501, 502]            # as stored (1-based)
    assert udata.load_labels("imagenet64", str(tmp_path), "test").tolist() == [1000, 1001]
    np.savez(tmp_path / "val_data.npz", data=rng.integers(0, 256, (2, 12288), dtype=np.uint8))
    assert udata.load_labels("imagenet64", str(tmp_path), "test") is None
    np.savez(tmp_path / "val_data.npz", data=rng.integers(0, 256, (2, 12288), dtype=np.uint8), labels=np.arange(3))
    with pytest.raises(ValueError, match="3 labels for 2 images"):
        udata.load_labels("imagenet64", str(tmp_path), "test")


def test_load_labels_npy(tmp_path):
    im = np.zeros((4, 8, 8, 3), np.uint8)
    np.save(tmp_path / "bare.npy", im)
    np.savez(tmp_path / "with.npz", images=im, labels=np.array([3, 1, 2, 0], np.uint8))
    np.savez(tmp_path / "without.npz", images=im)
    np.savez(tmp_path / "short.npz", images=im, labels=np.arange(3))
    assert udata.load_labels("npy", str(tmp_path / "bare.npy")) is None
    assert udata.load_labels("npy", str(tmp_path / "without.npz")) is None
    got = udata.load_labels("npy", str(tmp_path / "with.npz"))
    assert got.dtype == np.int64 and got.tolist() == [3, 1, 2, 0]
    with pytest.raises(ValueError, match="3 labels for 4 images"):
        udata.load_labels("npy", str(tmp_path / "short.npz"))
    with pytest.raises(ValueError):
        udata.load_labels("mnist", str(tmp_path))
