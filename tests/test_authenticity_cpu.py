"""CPU: the numpy reference of the authenticity score on hand-made cases, the score's definition, the new flags, the CUDA-only
contract of `nearest`, and the new symbols in header, library and ctypes table."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import authenticity_ref as R
from conftest import ROOT


def _images(rng, n, D=48):
    return rng.integers(0, 256, (n, D), dtype=np.uint8)


def test_reference_finds_a_planted_copy():
    rng = np.random.default_rng(0)
    bank = _images(rng, 12)
    q = _images(rng, 3)
    q[1] = bank[7]
    q[2] = bank[4]
    q[2, 5] = q[2, 5] + 1 if q[2, 5] < 255 else 254
    index, dist = R.nearest(q, bank, 2)
    assert (index[1, 0], dist[1, 0]) == (7, 0) and (index[2, 0], dist[2, 0]) == (4, 1)
    assert dist[0, 0] > 0 and (dist[:, 0] <= dist[:, 1]).all()
    d = R.distances(q, bank)
    assert d[0, 3] == ((q[0].astype(int) - bank[3].astype(int)) ** 2).sum() and d.dtype == np.int64


def test_reference_tie_goes_to_the_smaller_column_and_short_banks_pad():
    bank = np.zeros((5, 16), np.uint8)
    bank[1, 0], bank[3, 0] = 3, 3          # columns 1 and 3 at distance 9, the rest at 0
    q = np.zeros((1, 16), np.uint8)
    index, dist = R.nearest(q, bank, 8)
    assert index[0].tolist() == [0, 2, 4, 1, 3, -1, -1, -1] and dist[0].tolist() == [0, 0, 0, 9, 9, -1, -1, -1]
    index, dist = R.nearest(q, bank, 2, self0=0)      # row 0 skips column 0
    assert index[0].tolist() == [2, 4]
    index, dist = R.nearest(q, bank, 2, self0=7)      # self0 + i >= ny: nothing is excluded
    assert index[0].tolist() == [0, 2]


def test_reference_radii_with_a_duplicated_bank_row():
    rng = np.random.default_rng(1)
    bank = _images(rng, 9)
    bank[6] = bank[2]
    r = R.radii(bank)
    assert r[2] == 0 and r[6] == 0 and (np.delete(r, [2, 6]) > 0).all()
    d = R.distances(bank, bank)
    np.fill_diagonal(d, np.iinfo(np.int64).max)
    assert np.array_equal(r, d.min(axis=1))


def test_score_on_four_points():
    """Bank radii (10, 4, 0); four queries: nearest row 0 at 11 (> 10: authentic), row 0 at 10 (not: equal), row 1 at 0 (an
    exact copy, not authentic), row 2 at 1 (> 0: authentic).  Sorted distances 0, 1, 10, 11: lower median = element 1 = 1."""
    from otgan_amd.utils import authenticity
    radii = np.array([10, 4, 0], np.int64)
    index1 = np.array([0, 0, 1, 2], np.int32)
    dist1 = np.array([11, 10, 0, 1], np.int64)
    assert R.score(index1, dist1, radii) == (2, 1, 1)
    got = authenticity.score(torch.from_numpy(index1), torch.from_numpy(dist1), torch.from_numpy(radii))
    assert got == (2, 1, 1) and all(type(v) is int for v in got)
    assert authenticity.score(torch.from_numpy(index1[:3]), torch.from_numpy(dist1[:3]), torch.from_numpy(radii)) == (1, 1, 10)
    assert authenticity.rms(3072 * 4, 3072) == 2.0


def test_sheet_layout_against_the_reference():
    from otgan_amd.utils import authenticity
    rng = np.random.default_rng(2)
    gen = rng.integers(0, 255, (5, 4, 4, 3), dtype=np.uint8)
    bank = rng.integers(0, 255, (6, 4, 4, 3), dtype=np.uint8)
    index = np.array([[0, 1], [2, -1], [3, 4], [5, 0], [1, 2]], np.int32)
    dist = np.array([[7, 9], [3, -1], [7, 8], [1, 2], [50, 60]], np.int64)
    want = R.sheet(gen, bank, index, dist, rows=3)
    assert want.shape == (3 * 5 + 1, 3 * 5 + 1, 3) and want.dtype == np.uint8
    assert np.array_equal(want[1:5, 1:5], gen[3]) and np.array_equal(want[6:10, 6:10], bank[2])
    assert np.array_equal(want[11:15, 1:5], gen[0])                      # 7 = 7: the smaller sample first
    assert (want[6:10, 11:15] == 255).all() and (want[0] == 255).all() and (want[:, 5] == 255).all()
    for g, b in ((gen, bank), (torch.from_numpy(gen), torch.from_numpy(bank))):
        got = authenticity.sheet(g, b, torch.from_numpy(index), torch.from_numpy(dist), rows=3)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert authenticity.sheet(gen, bank, index, dist).shape[0] == 5 * 5 + 1          # rows is cut to the samples


def test_flags_parse_and_defaults_leave_the_rest():
    from otgan_amd import train
    new = {"authenticity_samples": 0, "authenticity_neighbours": 3, "authenticity_train_samples": 50000}
    base = vars(train.build_parser().parse_args([]))
    for k, v in new.items():
        assert base[k] == v
    args = vars(train.build_parser().parse_args(["--authenticity_samples", "10000", "--authenticity_neighbours", "8",
                                                  "--authenticity_train_samples", "123"]))
    assert (args["authenticity_samples"], args["authenticity_neighbours"], args["authenticity_train_samples"]) == (10000, 8, 123)
    assert {k: v for k, v in args.items() if k not in new} == {k: v for k, v in base.items() if k not in new}
    from otgan_amd.utils import authenticity
    for k in (0, 9):
        with pytest.raises(ValueError):
            authenticity.check_neighbours(k)


def test_nearest_has_no_cpu_fallback():
    from otgan_amd import _lib
    from otgan_amd.utils import authenticity
    x = torch.zeros(4, 16, dtype=torch.uint8)
    with pytest.raises(_lib.OtganError):
        authenticity.nearest(x, x, 1)
    with pytest.raises(_lib.OtganError):
        authenticity.radii(x)


def test_header_library_and_binding_agree_on_the_new_symbols():
    from otgan_amd import _lib
    txt = open(os.path.join(ROOT, "include", "otgan_layers.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("otgan_nn_u8_workspace_bytes", 3), ("otgan_nn_u8", 14)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
        assert hasattr(L, name)
    assert _lib.SIGNATURES["otgan_nn_u8_workspace_bytes"][0] is ctypes.c_size_t
    # the overflow bounds are stated where the contract is
    assert "3 196 108 800" in txt and "805 306 368" in txt
    # the workspace query needs no device: keys per split and row, then the norms
    ws = _lib.lib().otgan_nn_u8_workspace_bytes
    assert ws(0, 5, 1) == 0 and ws(5, 0, 1) == 0 and ws(5, 5, 0) == 0 and ws(5, 5, 9) == 0
    assert ws(3, 5, 2) == 8 * 3 * 2 + 4 * 8
    assert ws(3, 600, 2) >= 2 * 8 * 3 * 2 + 4 * 603
