"""GPU: the augmentation kernels (csrc/augment.hip: otgan_augment_fwd_f32 / _bwd_f32) and ops.augment against the fp64
restatement of include/otgan_layers.h in tests/augment_ref.py.

Accuracy bound 1e-5 absolute, forward and backward, derived and not measured: inputs and upstream gradients lie in [-1, 1], so the
intermediates stay below 12 (forward: |v1| <= 1.5, |v2| <= 4.5, |v3| <= 10.5) and below 6 (backward); about 8 fp32 roundings of
6e-8 relative at those magnitudes give about 6e-6, and the fixed-order mean of 3 S^2 <= 12288 elements adds less than 2e-6.
The worst case is printed by every case (pytest -s); measured on an MI355X: 7.0e-7 forward, 3.1e-7 backward (both at S = 64),
below a third of the bound."""
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu

BOUND = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _windows(pool, rows):
    """Calls of `rows` rows each that together present every row of the pool (the last one wraps around)."""
    n = pool.shape[0]
    return [torch.arange(s, s + rows) % n for s in range(0, n, rows)]


@pytest.mark.parametrize("rows", [1, 3, 7])
@pytest.mark.parametrize("S", [4, 8, 32, 64])
def test_forward_backward_against_fp64(dev, S, rows):
    """All 8 policies at this S and row count; the rows of u are augment_ref.edge_rows (every slot 0, every slot 1 - 2^-24, zero
    shift, shifts of +-R, cutout centres at 0 and S), presented `rows` at a time.  Per policy: max |error| <= 1e-5 both ways;
    without the colour bit every element has the bits of its source or is +0.0f (policy 0: a bit-exact copy); and the adjoint
    identity <T x - T 0, dy> = <x, T^T dy> holds on the DEVICE outputs, accumulated in fp64, to 1e-5 relative -- relative to
    |T x - T 0| |dy| and |x| |T^T dy| (2-norms), the dot-product test's usual scale: the two inner products are sums of thousands
    of terms of both signs and can cancel to nearly nothing (at S = 8 one policy's sum is 0.09 from terms that add up to 60 in
    magnitude), so their own size says nothing about the accuracy of the terms."""
    from otgan_amd import ops
    g = torch.Generator().manual_seed(1000 * S + rows)
    pool = R.edge_rows(g)
    worst_f = worst_b = worst_adj = 0.0
    for policy in range(8):
        lhs = rhs = nl = nd = nx = nt = 0.0
        for pick in _windows(pool, rows):
            u = pool[pick].contiguous()
            x = torch.rand(rows, S, S, 3, generator=g) * 2 - 1
            dy = torch.rand(rows, S, S, 3, generator=g) * 2 - 1
            y = ops.augment(x.to(dev), u.to(dev), policy)
            dx = ops.augment_transpose(dy.to(dev), u.to(dev), policy)
            y0 = ops.augment(torch.zeros_like(x).to(dev), u.to(dev), policy)
            assert y.shape == x.shape and y.dtype == torch.float32 and ops.amax_of(y) is None
            y, dx, y0 = y.cpu(), dx.cpu(), y0.cpu()
            worst_f = max(worst_f, float((y.double() - R.apply(x.double(), u, policy)).abs().max()))
            worst_b = max(worst_b, float((dx.double() - R.transpose(dy.double(), u, policy)).abs().max()))
            if not policy & R.COLOR:
                # the restatement only gathers and selects here: in fp32 it is the expected bit pattern, zeros are +0.0f
                assert torch.equal(_bits(y), _bits(R.apply(x, u, policy))), (policy, "forward bits")
                assert torch.equal(_bits(dx), _bits(R.transpose(dy, u, policy))), (policy, "backward bits")
            if policy == 0:
                assert torch.equal(_bits(y), _bits(x)) and torch.equal(_bits(dx), _bits(dy))
            lhs += float(((y.double() - y0.double()) * dy.double()).sum())
            rhs += float((x.double() * dx.double()).sum())
            nl, nd = nl + float((y.double() - y0.double()).pow(2).sum()), nd + float(dy.double().pow(2).sum())
            nx, nt = nx + float(x.double().pow(2).sum()), nt + float(dx.double().pow(2).sum())
        adj = abs(lhs - rhs) / max((nl * nd) ** 0.5, (nx * nt) ** 0.5)
        worst_adj = max(worst_adj, adj)
        assert adj <= 1e-5, (policy, lhs, rhs)
    print("S %d rows %d: worst forward error %.3g, backward %.3g (bound %.0e), adjoint %.3g" % (S, rows, worst_f, worst_b, BOUND, worst_adj))
    assert worst_f <= BOUND and worst_b <= BOUND, (worst_f, worst_b)


@pytest.mark.parametrize("S", [4, 32, 64])
def test_deterministic_and_position_independent(dev, S):
    """The same image and row of u give the same bits at row 0 of a 1-row call, at row 5 of a 7-row call and in a second call,
    forward and backward, for every policy with a per-image reduction in it and without."""
    from otgan_amd import ops
    g = torch.Generator().manual_seed(S)
    x7 = (torch.rand(7, S, S, 3, generator=g) * 2 - 1).to(dev)
    u7 = torch.rand(7, 8, generator=g).to(dev)
    x1, u1 = x7[5:6].clone(), u7[5:6].clone()
    for policy in (7, 1, 6):
        for fn in (ops.augment, ops.augment_transpose):
            a = fn(x1, u1, policy)
            b = fn(x7, u7, policy)
            c = fn(x7, u7, policy)
            assert torch.equal(_bits(a[0]), _bits(b[5])), (policy, fn.__name__)
            assert torch.equal(_bits(b), _bits(c)), (policy, fn.__name__)


def test_autograd(dev):
    from otgan_amd import ops
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(3, 32, 32, 3, generator=g) * 2 - 1).to(dev)
    u = torch.rand(3, 8, generator=g).to(dev)
    dy = (torch.rand(3, 32, 32, 3, generator=g) * 2 - 1).to(dev)
    y = ops.augment(x, u, 7)
    assert y.grad_fn is None and not y.requires_grad          # no node: the backward kernel cannot launch
    xg = x.clone().requires_grad_(True)
    yg = ops.augment(xg, u, 7)
    assert yg.grad_fn is not None and torch.equal(_bits(yg.detach()), _bits(y))
    yg.backward(dy)
    assert torch.equal(_bits(xg.grad), _bits(ops.augment_transpose(dy, u, 7)))
    # a non-contiguous upstream gradient and input are taken as their values
    xt = x.transpose(1, 2).contiguous().transpose(1, 2)
    assert not xt.is_contiguous() and torch.equal(ops.augment(xt, u, 7), y)


def test_wrapper_errors(dev):
    from otgan_amd import _lib, ops
    x = torch.zeros(2, 8, 8, 3, device=dev)
    u = torch.zeros(2, 8, device=dev)
    for bad in (lambda: ops.augment(x.cpu(), u.cpu(), 7), lambda: ops.augment(x, u[:1], 7), lambda: ops.augment(x.double(), u, 7),
                lambda: ops.augment(x[:, :6], u, 7), lambda: ops.augment(x, u, 8),
                lambda: ops.augment(torch.zeros(2, 6, 6, 3, device=dev), u, 7)):
        with pytest.raises(_lib.OtganError):
            bad()
