"""CPU: the host side of --augment (utils/augment.py, the flag), the yardstick of the GPU tests (tests/augment_ref.py) checked
against itself in fp64, and the argument errors of otgan_augment_fwd_f32 / _bwd_f32, which return before any launch."""
import ctypes

import pytest
import torch

import augment_ref as R


def test_parse_policy():
    from otgan_amd.utils import augment as A
    assert A.parse_policy("") == 0
    assert A.parse_policy("color") == 1 and A.parse_policy("translation") == 2 and A.parse_policy("cutout") == 4
    assert A.parse_policy("color,translation,cutout") == 7            # DiffAugment's own spelling
    assert A.parse_policy("cutout,color") == 5 and A.parse_policy("translation, cutout") == 6
    assert A.parse_policy("color,color") == 1
    assert A.policy_names(5) == ["color", "cutout"] and A.policy_names(0) == []
    for bad in ("colour", "color,flip", "Color", "color;cutout"):
        with pytest.raises(ValueError) as e:
            A.parse_policy(bad)
        assert all(n in str(e.value) for n in ("color", "translation", "cutout"))
    from otgan_amd import ops
    assert (ops.AUG_COLOR, ops.AUG_TRANSLATION, ops.AUG_CUTOUT) == (A.POLICIES["color"], A.POLICIES["translation"], A.POLICIES["cutout"])
    assert (R.COLOR, R.TRANSLATION, R.CUTOUT) == (ops.AUG_COLOR, ops.AUG_TRANSLATION, ops.AUG_CUTOUT)


def test_flag_default_is_off():
    from otgan_amd import train
    from otgan_amd.trainer import default_args
    assert train.build_parser().parse_args([]).augment == ""
    assert train.build_parser().parse_args(["--augment", "color,cutout"]).augment == "color,cutout"
    assert default_args().augment == ""
    assert "--augment" in train.__doc__


def test_unknown_policy_name_is_an_error_before_any_device_work():
    from otgan_amd import train
    with pytest.raises(ValueError, match="--augment.*valid names"):
        train.main(["--synthetic", "--augment", "color,rotate"])


def test_reference_parameters():
    """The derivation at the ends of [0, 1): the clamps, the zero shift, windows half outside."""
    u = R.edge_rows(torch.Generator().manual_seed(0))
    for S, Rr in ((4, 1), (8, 1), (32, 4), (64, 8)):
        p = R.params(u, S, 7)
        h = S // 4
        assert p["tx"].tolist()[:5] == [-Rr, Rr, 0, -Rr, Rr] and p["ty"].tolist()[:5] == [-Rr, Rr, 0, Rr, -Rr]
        assert (p["wx0"][0], p["wx1"][0], p["wy0"][0], p["wy1"][0]) == (0, h, 0, h)
        assert (p["wx0"][1], p["wx1"][1], p["wy0"][1], p["wy1"][1]) == (S - h, S, S - h, S)
        assert (p["wx0"][5], p["wx1"][5], p["wy0"][5], p["wy1"][5]) == (0, h, S - h, S)
        assert float(p["b"][0]) == -0.5 and float(p["ks"][0]) == 0.0 and float(p["kc"][0]) == 0.5
        q = R.params(u, S, 0)
        assert not any(q[k].any() for k in ("tx", "ty", "wx1", "wy1", "b")) and bool((q["ks"] == 1).all())


@pytest.mark.parametrize("S", [4, 8, 32])
@pytest.mark.parametrize("policy", range(8))
def test_reference_adjoint_identity(S, policy):
    """<T x - T 0, y> = <x, T^T y> in fp64 to 1e-12 relative, T^T from the stated backward formulas: T is affine (the
    brightness offset b is its constant term T 0 and has no transpose term), so the identity holds for its linear part.
    Autograd of `apply` gives the same T^T y."""
    g = torch.Generator().manual_seed(100 * S + policy)
    u = torch.cat([R.edge_rows(g), torch.rand(3, 8, generator=g)])
    rows = u.shape[0]
    x = (torch.rand(rows, S, S, 3, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    y = torch.rand(rows, S, S, 3, generator=g, dtype=torch.float64) * 2 - 1
    Tx = R.apply(x, u, policy)
    lin = Tx.detach() - R.apply(torch.zeros_like(y), u, policy)
    Tty = R.transpose(y, u, policy)
    for r in range(rows):       # per image: T acts on each alone
        lhs, rhs = float((lin[r] * y[r]).sum()), float((x[r].detach() * Tty[r]).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (r, lhs, rhs)
    (auto,) = torch.autograd.grad(Tx, x, y)
    assert float((auto - Tty).abs().max()) <= 1e-14


def test_library_argument_errors():
    """Invalid arguments return OTGAN_ERR_INVALID with a message before any launch (so this runs without a device)."""
    from otgan_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    a = (ctypes.addressof(buf) + 15) & ~15             # a 16-byte aligned non-null address; never dereferenced
    x, y, u = a, a + 64, a + 128
    for fn in (L.otgan_augment_fwd_f32, L.otgan_augment_bwd_f32):
        bad = [(x, 1, 6, u, 7, y), (x, 1, 0, u, 7, y), (x, 1, -4, u, 7, y), (x, 1, 68, u, 7, y),      # S
               (None, 1, 8, u, 7, y), (x, 1, 8, None, 7, y), (x, 1, 8, u, 7, None),                   # null pointers
               (x, -1, 8, u, 7, y),                                                                    # negative rows
               (x, 1, 8, u, 8, y), (x, 1, 8, u, -1, y),                                                # policy outside the mask
               (x + 4, 1, 8, u, 7, y), (x, 1, 8, u, 7, y + 8), (x, 1, 8, u, 7, x)]                     # alignment, in place
        for args in bad:
            assert fn(*args, None) == -1, args
            with pytest.raises(_lib.OtganError, match="augment_(fwd|bwd): "):       # the library's own message
                _lib.check(-1, "call")
        assert fn(x, 0, 8, u, 7, y, None) == 0           # nothing to do: no launch
