"""The host side of the Kernel Inception Distance (otgan_amd/utils/kid.py) without a device: the subset draws, the unbiased
estimator against the brute-force fp64 restatement (tests/kid_ref.py), the command-line flags and their trainer defaults,
and the start-up check of the subset size."""
import numpy as np
import pytest

import kid_ref
from otgan_amd.utils import kid


def test_subset_indices_shape_dtype_and_distinct_rows():
    t = kid.subset_indices(50, 20, 6, seed=3, side=0)
    assert t.shape == (6, 20) and t.dtype == np.int32
    assert t.min() >= 0 and t.max() < 50
    for row in t:
        assert len(set(row.tolist())) == 20
    # all n rows: a permutation
    assert sorted(kid.subset_indices(9, 9, 1, 0, 0)[0].tolist()) == list(range(9))
    assert kid.subset_indices(50, 20, 0, 3, 0).shape == (0, 20)


def test_subset_indices_depend_on_seed_side_and_subset_only():
    a = kid.subset_indices(100, 30, 5, seed=7, side=0)
    assert np.array_equal(a, kid.subset_indices(100, 30, 5, seed=7, side=0))
    # the draw of subset b is numpy's documented generator seeded with [seed, side, b], whatever the table around it
    assert np.array_equal(a[3], np.random.default_rng([7, 0, 3]).choice(100, 30, replace=False))
    assert np.array_equal(a[:3], kid.subset_indices(100, 30, 3, seed=7, side=0))
    assert not np.array_equal(a, kid.subset_indices(100, 30, 5, seed=7, side=1))
    assert not np.array_equal(a, kid.subset_indices(100, 30, 5, seed=8, side=0))
    assert all(not np.array_equal(a[i], a[j]) for i in range(5) for j in range(i))


@pytest.mark.parametrize("first,step", [(0, 2), (1, 2), (2, 3), (4, 5), (5, 5)])
def test_subset_indices_first_step_are_rows_of_the_full_table(first, step):
    full = kid.subset_indices(64, 16, 5, seed=1, side=1)
    part = kid.subset_indices(64, 16, 5, seed=1, side=1, first=first, step=step)
    assert part.dtype == np.int32 and part.shape == (len(range(first, 5, step)), 16)
    assert np.array_equal(part, full[first::step])


def test_subset_indices_rejects_more_rows_than_there_are():
    with pytest.raises(ValueError):
        kid.subset_indices(10, 11, 2, 0, 0)


def _brute_force_mmd2(X, Y):
    """Element by element, no Gram matrix: the definition."""
    m, C = X.shape
    k = lambda a, b: (float(np.dot(a, b)) / C + 1.0) ** 3
    sxx = sum(k(X[i], X[j]) for i in range(m) for j in range(m) if i != j)
    syy = sum(k(Y[i], Y[j]) for i in range(m) for j in range(m) if i != j)
    sxy = sum(k(X[i], Y[j]) for i in range(m) for j in range(m))
    return sxx / (m * (m - 1)) + syy / (m * (m - 1)) - 2.0 * sxy / (m * m)


def test_mmd2_from_sums_against_brute_force():
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((13, 8)), rng.standard_normal((13, 8)) + 0.5
    sums = kid_ref.kernel_sums(X, Y)
    ref = _brute_force_mmd2(X, Y)
    got = kid.mmd2_from_sums(sums, 13)
    assert ref > 0.1 and abs(got - ref) <= 1e-12 * kid_ref.scale(sums, 13)
    assert got == pytest.approx(kid_ref.mmd2(sums, 13), rel=1e-15)
    # a table of subsets at once, numpy and torch
    import torch
    table = np.stack([sums, 2 * sums])
    assert np.allclose(kid.mmd2_from_sums(table, 13), [got, 2 * got], rtol=1e-15)
    assert torch.allclose(kid.mmd2_from_sums(torch.as_tensor(table), 13), torch.as_tensor([got, 2 * got], dtype=torch.float64))
    with pytest.raises(ValueError):
        kid.mmd2_from_sums(sums, 1)


def test_mmd2_of_two_halves_of_one_distribution_is_negative_and_not_clipped():
    """The unbiased estimator of a zero distance scatters around zero: of 20 splits of one sample some are negative, and
    the value comes back as it is."""
    vals = []
    for seed in range(20):
        z = np.random.default_rng(seed).standard_normal((40, 8))
        X, Y = z[:20], z[20:]
        v = kid.mmd2_from_sums(kid_ref.kernel_sums(X, Y), 20)
        assert v == pytest.approx(_brute_force_mmd2(X, Y), abs=1e-12)
        vals.append(v)
    assert min(vals) < -1e-3 and max(vals) > 0.0, vals
    assert abs(np.mean(vals)) < 3.0 * np.std(vals) / np.sqrt(len(vals)) + 1e-3       # unbiased: the mean is near zero


def test_parser_has_the_kid_flags():
    from otgan_amd.train import build_parser
    ns = build_parser().parse_args([])
    assert (ns.kid_subsets, ns.kid_subset_size, ns.kid_real_samples) == (0, 1000, 0)
    assert all(type(v) is int for v in (ns.kid_subsets, ns.kid_subset_size, ns.kid_real_samples))
    ns = build_parser().parse_args(["--kid_subsets", "100", "--kid_subset_size", "500", "--kid_real_samples", "10000"])
    assert (ns.kid_subsets, ns.kid_subset_size, ns.kid_real_samples) == (100, 500, 10000)


def test_trainer_defaults_have_the_kid_flags():
    from otgan_amd.trainer import default_args
    d = default_args()
    assert (d.kid_subsets, d.kid_subset_size, d.kid_real_samples) == (0, 1000, 0)


def test_effective_subset_size():
    assert kid.effective_subset_size(1000, 50000, 50000) == 1000
    assert kid.effective_subset_size(1000, 20, 48) == 20                 # the generated rows bind
    assert kid.effective_subset_size(1000, 5000, 300) == 300             # the real rows bind
    # two ranks: shares of 48 and 47 generated rows (the hook's `mine`), 48 real rows each
    assert kid.effective_subset_size(1000, 95, 96, world=2) == 47
    assert kid.effective_subset_size(1000, 96, 95, world=2) == 47
    assert kid.effective_subset_size(32, 95, 96, world=2) == 32
    for bad in ((1, 100, 100, 1), (1000, 1, 100, 1), (1000, 100, 1, 1), (1000, 3, 100, 2), (1000, 100, 3, 2)):
        with pytest.raises(ValueError) as e:
            kid.effective_subset_size(*bad)
        assert "at least 2 rows" in str(e.value) and str(bad[0]) in str(e.value)


def test_no_cpu_fallback():
    import torch
    from otgan_amd import _lib
    idx = np.zeros((1, 2), np.int32)
    with pytest.raises(_lib.OtganError):
        kid.kid_sums(torch.zeros(4, 8), idx, torch.zeros(4, 8), idx)
    with pytest.raises(_lib.OtganError):
        kid.FeatureBank(4, 8, "cpu")
