"""Precision, recall, density and coverage without a GPU: the brute-force reference (tests/pr_ref.py) on cases worked out
by hand, the command-line surface, the K / row-count rule and the notice for a classifier without pool_3."""
from types import SimpleNamespace

import numpy as np
import pytest

import pr_ref
from otgan_amd.utils import pr


def test_identical_sets_give_one_everywhere():
    rng = np.random.default_rng(0)
    S = rng.standard_normal((12, 6))
    p, r, d, c = pr_ref.values(S, S.copy(), 3)
    assert (p, r, c) == (1.0, 1.0, 1.0) and d >= 1.0                    # a ball holds its centre and its K neighbours
    # 4 points at equal spacing on a line with K = 3: every ball reaches all of the set, density 4 / 3 ... and with the
    # rows far from one another in pairs, K = 1: a ball holds its centre and the partner, density 2 / 1
    line = np.arange(4.0)[:, None]
    assert pr_ref.values(line, line, 3) == (1.0, 1.0, 4 / 3, 1.0)
    pairs = np.array([[0.0], [1.0], [100.0], [101.0]])
    assert pr_ref.values(pairs, pairs, 1) == (1.0, 1.0, 2.0, 1.0)
    # (with <= the K-th neighbour lies ON the sphere and counts, so without ties a set against itself has density
    # (K + 1) / K, not 1: the ball holds its centre as well)
    assert d == 4 / 3


def test_far_apart_sets_give_zero_everywhere():
    rng = np.random.default_rng(1)
    G, R = rng.uniform(0, 1, (9, 4)), rng.uniform(0, 1, (7, 4)) + 100.0
    assert pr_ref.values(G, R, 3) == (0.0, 0.0, 0.0, 0.0)
    assert pr_ref.counts(G, R, 3) == (0, 0, 0, 0, 9, 7)


def test_hand_computed_line():
    """On a line: G = {0, 1, 2}, R = {1.5, 2.5, 10}, K = 1.  Radii (squared): G 1, 1, 1; R 1, 1, 56.25.
    d2(g, r): 0 -> 2.25, 6.25, 100; 1 -> 0.25, 2.25, 81; 2 -> 0.25, 0.25, 64.
    precision: g = 0 is in no real ball (2.25 > 1, 6.25 > 1, 100 > 56.25), g = 1 and g = 2 are: 2 / 3.
    density: balls holding g = 1: one (r = 1.5), g = 2: two: 3 / (1 * 3) = 1.
    recall: r = 1.5 is within 1 of g = 1 and g = 2, r = 2.5 of g = 2, r = 10 of none: 2 / 3.
    coverage: nearest g of r = 1.5 at 0.25 <= 1, of 2.5 at 0.25 <= 1, of 10 at 64 > 56.25: 2 / 3."""
    G, R = np.array([[0.0], [1.0], [2.0]]), np.array([[1.5], [2.5], [10.0]])
    assert np.array_equal(pr_ref.radii(G, 1), [1.0, 1.0, 1.0]) and np.array_equal(pr_ref.radii(R, 1), [1.0, 1.0, 56.25])
    assert pr_ref.counts(G, R, 1) == (2, 2, 3, 2, 3, 3)
    assert pr_ref.values(G, R, 1) == (2 / 3, 2 / 3, 1.0, 2 / 3)


def test_repeated_rows_have_radius_zero_by_position():
    S = np.array([[1.0, 2.0], [5.0, 5.0], [1.0, 2.0], [1.0, 2.0], [9.0, 0.0]])
    r1, r2, r3 = pr_ref.radii(S, 1), pr_ref.radii(S, 2), pr_ref.radii(S, 3)
    assert r1[0] == r1[2] == r1[3] == 0.0 and r2[0] == r2[2] == r2[3] == 0.0       # two copies besides the row itself
    assert r3[0] == 25.0 and r1[1] == 25.0                                          # then the nearest other row
    near, inside = pr_ref.knn(S, S, 3, self0=-1, thresh=np.zeros(5))
    assert np.array_equal(near[0], [0.0, 0.0, 0.0]) and list(inside) == [3, 1, 3, 3, 1]
    # fewer columns than k: +inf behind the ones there are
    near, _ = pr_ref.knn(S[:3], S[:3], 3, self0=0)
    assert np.isinf(near[:, 2]).all() and np.isfinite(near[:, :2]).all()
    # a row range of the bank, the multi-rank pattern: the rows' own columns start at self0
    assert np.array_equal(pr_ref.knn(S[2:4], S, 2, self0=2)[0], np.sort(pr_ref.dist2(S, S), axis=1)[2:4, 1:3])


def test_error_bound_covers_the_expanded_form_in_fp64():
    rng = np.random.default_rng(2)
    A = (np.abs(rng.standard_normal((20, 100))) * 3 + 1).astype(np.float32)
    B = (np.abs(rng.standard_normal((30, 100))) * 3 + 1).astype(np.float32)
    a, b = A.astype(np.float64), B.astype(np.float64)
    expanded = np.maximum(0.0, ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]) - 2.0 * (a @ b.T))
    assert (np.abs(expanded - pr_ref.dist2(A, B)) <= pr_ref.error_bound(A, B)).all()
    assert pr_ref.error_bound(A, B).max() < 1e-9 * pr_ref.dist2(A, B).min()          # and is far below the distances


def test_values_are_quotients_of_the_counts():
    assert pr.values_from_counts([2, 2, 3, 2, 3, 3], 1) == (2 / 3, 2 / 3, 1.0, 2 / 3)
    assert pr.values_from_counts([10, 5, 45, 7, 20, 10], 3) == (0.5, 0.5, 0.75, 0.7)


def test_parser_and_trainer_defaults_have_the_flags():
    from otgan_amd.train import build_parser
    from otgan_amd.trainer import default_args
    ns = build_parser().parse_args([])
    assert (ns.pr_neighbours, ns.pr_real_samples) == (0, 0)
    ns = build_parser().parse_args(["--pr_neighbours", "3", "--pr_real_samples", "10000"])
    assert (ns.pr_neighbours, ns.pr_real_samples) == (3, 10000)
    d = default_args()
    assert (d.pr_neighbours, d.pr_real_samples) == (0, 0)


def test_neighbour_rule():
    assert pr.check_neighbours(3, 50000, 50000) == 3
    assert pr.check_neighbours(3, 4, 96) == 3 and pr.check_neighbours(8, 9, 9) == 8
    with pytest.raises(ValueError, match="more than 3 rows"):
        pr.check_neighbours(3, 3, 96)                                   # a generated row has only 2 others
    with pytest.raises(ValueError, match="more than 3 rows"):
        pr.check_neighbours(3, 96, 2)
    with pytest.raises(ValueError, match="between 1 and 8"):
        pr.check_neighbours(9, 96, 96)
    with pytest.raises(ValueError, match="between 1 and 8"):
        pr.check_neighbours(0, 96, 96)


def test_real_state_is_skipped_with_a_classifier_without_pool3(capsys):
    from otgan_amd.train import real_pr_state
    args = SimpleNamespace(pr_neighbours=3, pr_real_samples=0, eval_samples=20)
    trainx = np.zeros((48, 32, 32, 3), np.float32)
    assert real_pr_state(args, object(), trainx, 0, 1) == {}
    assert real_pr_state(args, None, trainx, 1, 2) == {}                # said by rank 0 only
    out = capsys.readouterr().out
    assert out.count("precision and recall need the 2015 Inception graph") == 1 and out.count("skipped") == 1


def test_no_cpu_fallback():
    import torch
    from otgan_amd import _lib
    x = torch.zeros(4, 8)
    with pytest.raises(_lib.OtganError, match="no CPU fallback"):
        pr.knn(x, x, 1)
