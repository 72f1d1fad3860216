"""CPU: the host half of the Frechet Inception Distance (utils/fid.py) -- the eigh-based distance against
scipy.linalg.sqrtm and against closed forms, the finalisation of the moments against numpy, the stats file format,
and the two command-line flags."""
import numpy as np
import pytest

from otgan_amd.utils import fid


def _spd(rng, C, n=None):
    """A random covariance: full rank from a C x C factor, or np.cov of n rows (rank n - 1 when n <= C)."""
    a = rng.standard_normal((n or 4 * C, C)) * rng.uniform(0.2, 2.0, C)
    return np.cov(a, rowvar=False), a.mean(0)


def _sqrtm_distance(mu1, s1, mu2, s2):
    from scipy import linalg
    covmean = linalg.sqrtm(s1 @ s2)
    if isinstance(covmean, tuple):
        covmean = covmean[0]
    d = mu1 - mu2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(covmean.real))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_frechet_distance_against_sqrtm_full_rank(seed):
    rng = np.random.default_rng(seed)
    s1, mu1 = _spd(rng, 64)
    s2, mu2 = _spd(rng, 64)
    got, ref = fid.frechet_distance(mu1, s1, mu2, s2), _sqrtm_distance(mu1, s1, mu2, s2)
    print("full rank: eigh %.15g sqrtm %.15g relative difference %.2e" % (got, ref, abs(got - ref) / ref))
    assert abs(got - ref) <= 1e-9 * abs(ref)


def test_frechet_distance_closed_form_for_diagonal_covariances():
    rng = np.random.default_rng(3)
    a, b = rng.uniform(0.1, 4.0, 48), rng.uniform(0.1, 4.0, 48)
    a[5], b[9] = 0.0, 0.0                                   # a dead channel on either side
    mu1, mu2 = rng.standard_normal(48), rng.standard_normal(48)
    ref = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum() + ((mu1 - mu2) ** 2).sum()
    assert fid.frechet_distance(mu1, np.diag(a), mu2, np.diag(b)) == pytest.approx(ref, rel=1e-12)


def test_distance_of_a_distribution_to_itself_is_zero():
    # (full rank: a null direction's eigenvalue of R sigma R is rounding noise of size eps * lambda_max^2, and its
    # square root, sqrt(eps) * lambda_max, is what a rank-deficient pair is held to in the next test)
    rng = np.random.default_rng(4)
    for C in (16, 64):
        s, mu = _spd(rng, C)
        assert abs(fid.frechet_distance(mu, s, mu, s)) <= 1e-8 * np.trace(s)


def test_rank_deficient_pair_is_real_and_finite():
    # pool_3-like magnitudes (non-negative features below ~1): both methods carry rounding noise of about
    # sqrt(eps) * lambda_max = 1.5e-8 * lambda_max per null direction (the square root of an eigenvalue that is noise of
    # size eps * lambda_max^2), so an absolute bar belongs to a scale; 20 rows in 40 channels leave 21 null directions
    rng = np.random.default_rng(5)

    def stats():
        a = np.abs(rng.standard_normal((20, 40))) * rng.uniform(0.05, 0.5, 40)
        return np.cov(a, rowvar=False), a.mean(0)
    s1, mu1 = stats()
    s2, mu2 = stats()
    assert np.linalg.matrix_rank(s1) == 19 and np.linalg.matrix_rank(s2) == 19
    got = fid.frechet_distance(mu1, s1, mu2, s2)
    ref = _sqrtm_distance(mu1, s1, mu2, s2)
    print("rank deficient (20 rows, 40 channels): eigh %.15g sqrtm %.15g difference %.2e" % (got, ref, abs(got - ref)))
    assert isinstance(got, float) and np.isfinite(got)
    assert abs(got - ref) <= 1e-7


def test_dead_channels_do_not_turn_rounding_noise_into_error():
    """Channels that are exactly zero in both sets (dead ReLUs) are null directions of both covariances.  One-pass
    moments in any summation order and the two-pass np.cov differ by rounding only (1e-16), and d^2 must agree at the
    1e-9 the device accumulator is held to against host moments -- not at the sqrt of the noise."""
    rng = np.random.default_rng(8)
    dead = [5, 17, 33]

    def feats(shift):
        a = np.abs(rng.standard_normal((96, 40))) * rng.uniform(0.05, 0.5, 40) + shift * rng.uniform(0.0, 0.3, 40)
        a[:, dead] = 0.0
        return a.astype(np.float32).astype(np.float64)
    a, b = feats(0.0), feats(1.0)
    ref = fid.frechet_distance(a.mean(0), np.cov(a, rowvar=False), b.mean(0), np.cov(b, rowvar=False))
    worst = 0.0
    for _ in range(20):
        pa, pb = a[rng.permutation(96)], b[rng.permutation(96)]
        got = fid.frechet_distance(*fid.stats_from_moments(96, pa.sum(0), pa.T @ pa),
                                   *fid.stats_from_moments(96, pb.sum(0), pb.T @ pb))
        worst = max(worst, abs(got - ref) / ref)
    print("dead channels: d^2 %.12g, worst relative spread over summation orders %.2e" % (ref, worst))
    assert worst <= 1e-9


def test_stats_from_moments_against_numpy():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((300, 24)) * 3.0 + rng.uniform(-2, 2, 24)
    mu, sigma = fid.stats_from_moments(x.shape[0], x.sum(0), x.T @ x)
    np.testing.assert_allclose(mu, np.mean(x, 0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(sigma, np.cov(x, rowvar=False), rtol=1e-12, atol=1e-12)
    for n in (0, 1):
        with pytest.raises(ValueError):
            fid.stats_from_moments(n, x[:n].sum(0), x[:n].T @ x[:n])


def test_stats_file_round_trip_and_channel_mismatch(tmp_path):
    rng = np.random.default_rng(7)
    s, mu = _spd(rng, 12)
    path = str(tmp_path / "stats.npz")
    fid.save_stats(path, mu, s, 48)
    with np.load(path) as f:
        assert set(f.files) == {"mu", "sigma", "n"}
        assert f["mu"].dtype == np.float64 and f["sigma"].dtype == np.float64 and f["sigma"].shape == (12, 12)
    mu2, s2, n = fid.load_stats(path, 12)
    assert n == 48 and np.array_equal(mu2, mu) and np.array_equal(s2, s)
    # a circulated file has no `n`
    other = str(tmp_path / "circulated.npz")
    np.savez(other, mu=mu, sigma=s)
    assert fid.load_stats(other, 12)[2] == 0
    with pytest.raises(ValueError) as e:
        fid.load_stats(path, 2048)
    assert "12" in str(e.value) and "2048" in str(e.value)


def test_flags_and_their_trainer_defaults():
    from otgan_amd.train import build_parser
    from otgan_amd.trainer import default_args
    ns = build_parser().parse_args([])
    assert ns.fid_stats == "" and ns.fid_real_samples == 0
    d = default_args()
    assert d.fid_stats == "" and d.fid_real_samples == 0
    ns = build_parser().parse_args(["--fid_stats", "a.npz", "--fid_real_samples", "1000"])
    assert ns.fid_stats == "a.npz" and ns.fid_real_samples == 1000


def test_accumulator_has_no_cpu_path():
    from otgan_amd import _lib
    with pytest.raises(_lib.OtganError):
        fid.MomentAccumulator(8, "cpu")
