"""GPU: `otgan_batch_from_u8_f32` (csrc/data.hip) and utils.data.DeviceDataset against the numpy restatement in
tests/data_ref.py.

Bars.  f = 1 is a table lookup: bit equality (torch.equal).  f = 2, 4: the box sum is an exact integer below 2^24, its
conversion to fp32 is exact, the library is built without fast-math so the fp32 division is correctly rounded and a
quotient followed by a subtraction cannot contract: bit equality is EXPECTED; the test allows an absolute 1.2e-7 -- one
ulp of a quotient in [1, 2), the largest the quotient sum / (127.5 f f) in [0, 2] gets -- and prints how many elements
were not identical.
Every output buffer has two sentinel rows in front and behind and, where the pitch is wider than a row, sentinel padding:
all of it must come back untouched."""
import ctypes

import numpy as np
import pytest
import torch

import data_ref as R
from otgan_amd import _lib, ops
from otgan_amd.utils import data as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 777.0
TOL_BOX = 1.2e-7

# 2 shards x B = 3: 6 rows, no multiple of any workgroup size; offsets (1, 4) into a 7-long permutation that repeats an index
# and holds both 0 and n - 1
N, B, OFFSETS = 7, 3, (1, 4)
PERM = np.array([3, 6, 0, 2, 6, 5, 1], np.int32)
FLIPS = {"mixed": np.array([1, 0, 0, 1, 1, 0], np.uint8), "zero": np.zeros(6, np.uint8), "null": None}


def _lut():
    return torch.from_numpy(R.lut()).to(DEV)


def _run(store, S, offsets, B, perm, flip, pad=0):
    """-> (out [rows, S, S, 3] view, whole sentinel buffer [rows + 4, ldo])"""
    rows, row = len(offsets) * B, 3 * S * S
    buf = torch.full((rows + 4, row + pad), SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[2:2 + rows, :row].unflatten(1, (S, S, 3))
    got = ops.batch_from_u8(torch.as_tensor(store, device=DEV), list(offsets), B, S, _lut(),
                            perm=None if perm is None else torch.as_tensor(perm, device=DEV),
                            flip=None if flip is None else torch.as_tensor(flip, device=DEV), out=out)
    assert got.data_ptr() == out.data_ptr()
    return out, buf


def _untouched(buf, rows, row):
    assert bool((buf[:2] == SENTINEL).all()) and bool((buf[2 + rows:] == SENTINEL).all()), "rows beside the output were written"
    assert bool((buf[:, row:] == SENTINEL).all()), "the pitch padding was written"


@pytest.mark.parametrize("flip", list(FLIPS))
@pytest.mark.parametrize("use_perm", [True, False])
@pytest.mark.parametrize("S", [4, 32, 64])
def test_table_path_is_bit_identical(S, use_perm, flip):
    store = R.images(N, S, seed=S)
    perm = PERM if use_perm else None
    for pad in (0, 8):                                                           # ldo == row, ldo > row
        out, buf = _run(store, S, OFFSETS, B, perm, FLIPS[flip], pad)
        want = torch.from_numpy(R.batch(store, S, OFFSETS, B, perm, FLIPS[flip])).to(DEV)
        assert torch.equal(out, want)
        _untouched(buf, 2 * B, 3 * S * S)


def test_a_bool_flip_mask_is_taken_as_it_is():
    store = R.images(N, 32, seed=5)
    flip = torch.as_tensor(FLIPS["mixed"], device=DEV) != 0
    got = ops.batch_from_u8(torch.as_tensor(store, device=DEV), list(OFFSETS), B, 32, _lut(),
                            perm=torch.as_tensor(PERM, device=DEV), flip=flip)
    assert torch.equal(got, torch.from_numpy(R.batch(store, 32, OFFSETS, B, PERM, FLIPS["mixed"])).to(DEV))


@pytest.mark.parametrize("flip", list(FLIPS))
@pytest.mark.parametrize("use_perm", [True, False])
@pytest.mark.parametrize("H,S", [(64, 32), (128, 32), (16, 4), (8, 4)])
def test_box_downsample(H, S, use_perm, flip):
    store = R.images(N, H, seed=H + S)
    store[2] = 255                                                               # the largest sums: out = +1 exactly
    store[5] = 0
    perm = PERM if use_perm else None
    out, buf = _run(store, S, OFFSETS, B, perm, FLIPS[flip], pad=4)
    want = torch.from_numpy(R.batch(store, S, OFFSETS, B, perm, FLIPS[flip])).to(DEV)
    differ = int((out != want).sum())
    worst = float((out - want).abs().max())
    print("box %d -> %d, perm %s, flip %s: %d of %d elements not identical, largest difference %.3g"
          % (H, S, use_perm, flip, differ, want.numel(), worst))
    assert worst <= TOL_BOX
    _untouched(buf, 2 * B, 3 * S * S)


def test_offsets_past_two_to_the_32_bytes():
    """image 349 526 of a 64 x 64 store starts past byte 2^32: the last image of a 349 530-image store and image 0."""
    n = 349530
    assert (n - 1) * 64 * 64 * 3 > 2 ** 32
    store = torch.empty(n, 64, 64, 3, dtype=torch.uint8, device=DEV)             # 4.3 GB, never filled
    two = R.images(2, 64, seed=9)
    store[n - 1].copy_(torch.from_numpy(two[0]))
    store[0].copy_(torch.from_numpy(two[1]))
    perm = torch.tensor([n - 1, 0], dtype=torch.int32, device=DEV)
    got = ops.batch_from_u8(store, [0], 2, 64, _lut(), perm=perm)
    assert torch.equal(got, torch.from_numpy(R.convert(two, 64)).to(DEV))
    got = ops.batch_from_u8(store, [n - 1], 1, 64, _lut())                       # and without a permutation
    assert torch.equal(got, torch.from_numpy(R.convert(two[:1], 64)).to(DEV))
    del store


def _rc(store, S, offsets, B, perm, out, ldo=None):
    off = (ctypes.c_long * len(offsets))(*offsets)
    return _lib.lib().otgan_batch_from_u8_f32(store.data_ptr(), store.shape[0], store.shape[1], store.shape[2], _lib.ptr(perm),
                                              perm.numel() if perm is not None else 0, ctypes.cast(off, ctypes.c_void_p),
                                              len(offsets), B, None, _lut().data_ptr(), S, out.data_ptr(),
                                              3 * S * S if ldo is None else ldo, _lib.stream_ptr())


def test_argument_errors_are_rejected_before_any_launch():
    store = torch.zeros(7, 4, 4, 3, dtype=torch.uint8, device=DEV)
    perm = torch.arange(7, dtype=torch.int32, device=DEV)
    out = torch.full((33 * 8, 48), SENTINEL, device=DEV)
    last = lambda: _lib.lib().otgan_last_error().decode()
    assert _rc(store, 4, [0, 4], 3, perm, out) == 0                              # rows 0 - 2 and 4 - 6: the last legal shard
    torch.cuda.synchronize()
    out.fill_(SENTINEL)
    assert _rc(store, 4, [0, 5], 3, perm, out) == -1                             # 5 + 3 > 7
    assert "shard 1" in last() and "permutation" in last()
    assert _rc(store, 4, [0, 5], 3, None, out) == -1 and "the store" in last()
    assert _rc(store, 4, [-1], 3, perm, out) == -1
    assert _rc(store, 4, [0] * 33, 1, perm, out) == -1 and "33 shards" in last()
    assert _rc(store, 4, [0] * 32, 1, perm, out) == 0                            # (32 is the limit)
    torch.cuda.synchronize()
    out.fill_(SENTINEL)
    s12 = torch.zeros(7, 12, 12, 3, dtype=torch.uint8, device=DEV)
    assert _rc(s12, 4, [0], 3, None, out) == -1 and "factor" in last()           # f = 3
    s6 = torch.zeros(7, 6, 6, 3, dtype=torch.uint8, device=DEV)
    assert _rc(s6, 6, [0], 3, None, torch.full((8, 108), SENTINEL, device=DEV)) == -1 and "multiple of 4" in last()   # S = 6
    s8x4 = torch.zeros(7, 8, 4, 3, dtype=torch.uint8, device=DEV)
    assert _rc(s8x4, 4, [0], 3, None, out) == -1                                 # f differs in the two directions
    assert _rc(store, 8, [0], 3, None, out) == -1                                # no up-sampling
    assert _rc(store, 4, [0], 3, None, out, ldo=44) == -1 and "ldo" in last()    # ldo < row
    assert _rc(store, 4, [0], 3, None, out, ldo=50) == -1                        # ldo % 4
    assert _rc(store, 4, [0], 0, None, out) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(_lib.OtganError, match="code -1.*shard 1"):               # through the wrapper: the code and the message
        ops.batch_from_u8(store, [0, 5], 3, 4, _lut(), perm=perm)
    with pytest.raises(_lib.OtganError):
        ops.batch_from_u8(store.cpu(), [0], 3, 4, _lut())                        # no CPU fallback


def test_device_dataset_rows_batch_and_chunked_upload():
    u8 = R.images(11, 32, seed=12)
    ds = D.DeviceDataset(u8, DEV, 32)
    small = D.DeviceDataset(u8, DEV, 32, chunk_bytes=1024)                       # 33 copies of 1 KB
    assert torch.equal(ds.store, torch.from_numpy(u8).to(DEV)) and torch.equal(small.store, ds.store)
    assert torch.equal(D.DeviceDataset(u8, DEV, 32, chunk_bytes=1000).store, ds.store)      # a partial last copy
    assert ds.shape == (11, 32, 32, 3) and len(ds) == 11
    assert torch.equal(ds.lut, _lut())
    r = ds.rows(2, 9)
    assert torch.equal(r, torch.from_numpy(R.convert(u8[2:9], 32)).to(DEV))
    ds.set_permutation(np.arange(11))
    assert torch.equal(ds.batch([2], 7, torch.zeros(7, dtype=torch.bool, device=DEV)), r)
    assert torch.equal(ds.batch([2], 7), r)
    assert torch.equal(ds.rows(2, 9), r)                                         # rows ignores the permutation ...
    ds.set_permutation(np.arange(11)[::-1].copy())
    assert torch.equal(ds.rows(2, 9), r)
    assert torch.equal(ds.batch([0, 4], 2), torch.from_numpy(R.convert(u8[[10, 9, 6, 5]], 32)).to(DEV))
    assert ds.rows(3, 3).shape == (0, 32, 32, 3)
    with pytest.raises(ValueError):
        ds.set_permutation(np.array([0, 11]))
    with pytest.raises(IndexError):
        ds.rows(5, 12)
    h = ds.head(4)
    assert h.shape == (4, 32, 32, 3) and h.store.data_ptr() == ds.store.data_ptr()
    half = D.DeviceDataset(u8, DEV, 16)                                          # the same store feeds 16 x 16 through the box path
    assert float((half.rows(0, 11) - torch.from_numpy(R.convert(u8, 16)).to(DEV)).abs().max()) <= TOL_BOX


def test_head_starts_without_the_parents_permutation():
    u8 = R.images(11, 16, seed=13)
    ds = D.DeviceDataset(u8, DEV, 16)
    ds.set_permutation(np.arange(11)[::-1].copy())                               # points past a 4-image head
    h = ds.head(4)
    assert h.perm is None and ds.perm is not None
    assert torch.equal(h.batch([1], 3), ds.rows(1, 4))                           # storage order, not the parent's order
    with pytest.raises(ValueError):
        h.set_permutation(np.array([0, 4]))                                      # checked against the head's own n
    h.set_permutation(np.array([3, 0]))
    assert torch.equal(h.batch([0], 2), torch.from_numpy(R.convert(u8[[3, 0]], 16)).to(DEV))
    assert torch.equal(ds.batch([0], 2), torch.from_numpy(R.convert(u8[[10, 9]], 16)).to(DEV))    # the parent keeps its own


def test_upload_of_a_non_contiguous_source_in_pieces():
    base = R.images(9, 16, seed=14)
    for view in (base[:, :, ::-1], base[::2], base.transpose(0, 2, 1, 3)):       # mirrored, strided, transposed: none C-contiguous
        assert not view.flags.c_contiguous
        want = torch.from_numpy(np.ascontiguousarray(view)).to(DEV)
        for chunk in (D.CHUNK_BYTES, 2 * 768 + 100, 500):                        # one piece; pieces of two images; copies inside an image
            assert torch.equal(D.DeviceDataset(view, DEV, 16, chunk_bytes=chunk).store, want)


def test_wrapper_names_caller_errors():
    store = torch.as_tensor(R.images(N, 4, seed=15), device=DEV)
    lut, perm = _lut(), torch.as_tensor(PERM, device=DEV)
    ok = lambda **k: ops.batch_from_u8(store, [0], 3, 4, k.pop("lut", lut), **k)
    ok(perm=perm, flip=torch.zeros(3, dtype=torch.bool, device=DEV), out=torch.empty(3, 4, 4, 3, device=DEV))
    for match, kw in (("perm", dict(perm=perm.long())), ("perm", dict(perm=perm.cpu())), ("perm", dict(perm=perm[::2])),
                      ("out", dict(out=torch.empty(2, 4, 4, 3, device=DEV))),
                      ("out", dict(out=torch.empty(3, 4, 4, 3, dtype=torch.float64, device=DEV))),
                      ("out", dict(out=torch.empty(3, 4, 4, 6, device=DEV)[..., ::2])),
                      ("flip", dict(flip=torch.zeros(4, dtype=torch.bool, device=DEV))),
                      ("flip", dict(flip=torch.zeros(3, device=DEV))),
                      ("lut", dict(lut=lut[:255])), ("lut", dict(lut=lut.double()))):
        with pytest.raises(_lib.OtganError, match="batch_from_u8: " + match):
            ok(**kw)
