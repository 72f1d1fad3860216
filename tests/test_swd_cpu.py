"""CPU: the fp64 restatement of the sliced Wasserstein distance (tests/swd_ref.py) against scipy and against its own invariants,
and the host side of utils/swd.py: quantisation, positions, directions, the flags and the new symbols."""
import os
import re

import numpy as np
import pytest
import torch

import swd_ref as R
from conftest import ROOT


def _images(seed, n, S):
    return np.random.RandomState(seed).randint(0, 256, (n, S, S, 3)).astype(np.uint8)


@pytest.mark.parametrize("S", [16, 32, 64])
def test_reference_pyramid_against_scipy(S):
    """The border rule is scipy's mode='mirror'; down and up as the issue states them."""
    ndi = pytest.importorskip("scipy.ndimage")
    img = _images(S, 2, S)
    L = R.levels(S)
    pyr = [img.astype(np.float64)]
    k = R.G[None, :, :, None]
    for i in range(1, L):
        pyr.append(ndi.convolve(pyr[i - 1], k, mode="mirror")[:, ::2, ::2])
        z = np.zeros_like(pyr[i - 1])
        z[:, ::2, ::2] = pyr[i]
        pyr[i - 1] = pyr[i - 1] - ndi.convolve(z, 4.0 * k, mode="mirror")
    got = R.pyramid(img)
    assert len(got) == L == {16: 1, 32: 2, 64: 3}[S]
    for l in range(L):
        assert got[l].shape == (2, S >> l, S >> l, 3)
        err = np.abs(got[l] - pyr[l]).max()
        print("S %d level %d: %.3g" % (S, l, err))
        assert err <= 1e-12


def test_unsupported_sizes_are_value_errors():
    from otgan_amd.utils import swd
    for S in (8, 24, 48, 128):
        with pytest.raises(ValueError):
            R.levels(S)
        with pytest.raises(ValueError):
            swd.levels(S)
    assert [swd.levels(S) for S in (16, 32, 64)] == [1, 2, 3]


def _setup(S, n=6, P=5, nd=7, seed=0):
    from otgan_amd.utils import swd
    g = torch.Generator().manual_seed(seed)
    pa, pb = swd.positions(n, S, P, g).numpy(), swd.positions(n, S, P, g).numpy()
    d = swd.directions(1, nd, g).numpy()
    return pa, pb, d


@pytest.mark.parametrize("S", [16, 32])
def test_reference_distance_of_a_set_with_itself_is_zero(S):
    A = _images(1, 6, S)
    pa, _, d = _setup(S)
    assert np.all(R.distance(A, A, pa, pa, d) == 0.0)
    B = _images(2, 6, S)
    assert np.all(R.distance(A, B, pa, pa, d) > 0.0)


@pytest.mark.parametrize("S", [16, 32, 64])
def test_reference_distance_ignores_a_constant_offset(S):
    """A constant added to every pixel of one set leaves the Laplacian levels as they are (the taps sum to 1) and moves the
    Gaussian 16 x 16 level by that constant, which the normalisation removes: every level's distance unchanged to 1e-9."""
    A = _images(3, 6, S) // 2
    B = _images(4, 6, S) // 2
    pa, pb, d = _setup(S)
    base = R.distance(A, B, pa, pb, d)
    moved = R.distance(A, (B + 37).astype(np.uint8), pa, pb, d)
    print(S, base, np.abs(moved - base).max())
    assert np.abs(moved - base).max() <= 1e-9


def test_quantise():
    from otgan_amd.utils import swd
    k = np.arange(0, 255)
    ties = -1.0 + (2.0 * k + 1.0) / 255.0
    for x in (ties, ties.astype(np.float32)):
        want = np.clip(np.rint(127.5 * (x + 1.0)), 0, 255).astype(np.uint8)
        assert np.array_equal(swd.quantise(x), want)
        got = swd.quantise(torch.from_numpy(x))
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
        assert np.all((want == k) | (want == k + 1))
    # the one tie that is exact in binary: 127.5 -> 128 (half to even), and 0.5 -> 0, 1.5 -> 2 in the rule itself
    assert int(swd.quantise(torch.tensor([0.0]))[0]) == 128 and int(swd.quantise(np.array([0.0]))[0]) == 128
    assert torch.round(torch.tensor([0.5, 1.5, 2.5])).tolist() == [0.0, 2.0, 2.0]
    x = torch.tensor([-3.0, -1.0 - 1e-3, -1.0, 1.0, 1.0 + 1e-3, 7.0])
    assert swd.quantise(x).tolist() == [0, 0, 0, 255, 255, 255]
    assert swd.quantise(x.numpy()).tolist() == [0, 0, 0, 255, 255, 255]
    u8 = torch.arange(256, dtype=torch.float32)
    assert torch.equal(swd.quantise(u8 / 127.5 - 1.0), u8.to(torch.uint8))      # the stored bytes come back


@pytest.mark.parametrize("S", [16, 32, 64])
def test_positions_and_directions(S):
    from otgan_amd.utils import swd
    g = torch.Generator().manual_seed(5)
    pos = swd.positions(40, S, 16, g)
    L = swd.levels(S)
    assert pos.dtype == torch.int32 and tuple(pos.shape) == (L, 40, 16, 2)
    for l in range(L):
        assert int(pos[l].min()) == 0 and int(pos[l].max()) == (S >> l) - 7      # inside, and both ends are reached
    again = swd.positions(40, S, 16, torch.Generator().manual_seed(5))
    assert torch.equal(pos, again)
    d = swd.directions(3, 4, g)
    assert d.dtype == torch.float32 and tuple(d.shape) == (12, 147)
    assert torch.allclose(d.double().norm(dim=1), torch.ones(12, dtype=torch.float64), atol=1e-6)


def test_flags_parse_and_default_to_off():
    from otgan_amd.train import build_parser
    from otgan_amd.trainer import default_args
    ns = build_parser().parse_args([])
    assert (ns.swd_samples, ns.swd_patches, ns.swd_dirs, ns.swd_repeats) == (0, 128, 128, 4)
    d = default_args()
    assert (d.swd_samples, d.swd_patches, d.swd_dirs, d.swd_repeats) == (0, 128, 128, 4)
    ns = build_parser().parse_args(["--swd_samples", "16384", "--swd_patches", "8", "--swd_dirs", "4", "--swd_repeats", "2"])
    assert (ns.swd_samples, ns.swd_patches, ns.swd_dirs, ns.swd_repeats) == (16384, 8, 4, 2)


def test_symbols_are_declared_and_bound():
    from otgan_amd import _lib
    txt = open(os.path.join(ROOT, "include", "otgan_layers.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("otgan_swd_levels", "otgan_swd_pyramid_u8", "otgan_swd_workspace_bytes", "otgan_swd_channel_stats_u8",
                 "otgan_swd_project_u8", "otgan_swd_row_l1_f64"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.SIGNATURES, name
    L = _lib.lib()
    assert [L.otgan_swd_levels(S) for S in (16, 32, 64, 48, 128)] == [1, 2, 3, 0, 0]
    assert L.otgan_swd_workspace_bytes(7, 64, 128) == 7 * 3 * 6 * 8


def test_no_cpu_fallback():
    from otgan_amd import _lib
    from otgan_amd.utils import swd
    img = torch.zeros(2, 16, 16, 3, dtype=torch.uint8)
    g = torch.Generator().manual_seed(0)
    with pytest.raises(_lib.OtganError):
        swd.SwdReal(img, swd.positions(2, 16, 3, g), swd.directions(1, 2, g))
