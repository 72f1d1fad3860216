"""The augmentation T of include/otgan_layers.h (otgan_augment_fwd_f32 / _bwd_f32) restated in PyTorch on the host: the yardstick of
tests/test_augment_*.py.  The per-image parameters are derived in fp32 exactly as the header states them, so that the integer
shifts and windows agree with the kernels'; everything after that runs in the dtype of the input (fp64 in the tests).
`apply` is differentiable by autograd; `transpose` states the backward formulas on their own."""
import torch

COLOR, TRANSLATION, CUTOUT = 1, 2, 4


def params(u, S, policy):
    """u: [rows, 8] uniforms.  -> dict of per-image b, ks, kc (fp32) and tx, ty, wx0, wx1, wy0, wy1 (int64)."""
    u = u.detach().cpu().to(torch.float32)
    rows = u.shape[0]
    zf, zi = torch.zeros(rows, dtype=torch.float32), torch.zeros(rows, dtype=torch.int64)
    p = dict(b=zf, ks=zf + 1, kc=zf + 1, tx=zi, ty=zi, wx0=zi, wx1=zi, wy0=zi, wy1=zi)
    if policy & COLOR:
        p.update(b=u[:, 0] - 0.5, ks=2.0 * u[:, 1], kc=u[:, 2] + 0.5)
    if policy & TRANSLATION:
        R = (S + 4) // 8
        shift = lambda v: torch.clamp((v * float(2 * R + 1)).to(torch.int64), max=2 * R) - R      # (fp32 product, truncated)
        p.update(tx=shift(u[:, 3]), ty=shift(u[:, 4]))
    if policy & CUTOUT:
        h = (S // 2) // 2
        centre = lambda v: torch.clamp((v * float(S + 1)).to(torch.int64), max=S)
        ox, oy = centre(u[:, 5]), centre(u[:, 6])
        p.update(wx0=(ox - h).clamp(min=0), wx1=(ox + h).clamp(max=S), wy0=(oy - h).clamp(min=0), wy1=(oy + h).clamp(max=S))
    return p


def _grid(S):
    i = torch.arange(S)
    return i[None, :, None], i[None, None, :]          # yy [1, S, 1], xx [1, 1, S]


def _col(v):
    return v[:, None, None]


def _gather(v, sy, sx, keep):
    """v[r, sy, sx] where keep, else +0: [rows, S, S, 3]."""
    S = v.shape[1]
    r = torch.arange(v.shape[0])[:, None, None]
    g = v[r, sy.clamp(0, S - 1).expand(-1, S, S), sx.clamp(0, S - 1).expand(-1, S, S)]
    return torch.where(keep[..., None], g, torch.zeros((), dtype=v.dtype))


def apply(x, u, policy):
    """T(x): x [rows, S, S, 3] (a CPU tensor of any float dtype), u [rows, 8]."""
    S = x.shape[1]
    p = params(u, S, policy)
    v = x
    if policy & COLOR:
        b, ks, kc = (p[k].to(x.dtype)[:, None, None, None] for k in ("b", "ks", "kc"))
        v1 = x + b
        m = v1.sum(3, keepdim=True) / 3
        v2 = (v1 - m) * ks + m
        mu = x.sum((1, 2, 3), keepdim=True) / (3 * S * S) + b
        v = (v2 - mu) * kc + mu
    yy, xx = _grid(S)
    sy, sx = yy - _col(p["ty"]), xx - _col(p["tx"])
    cut = (yy >= _col(p["wy0"])) & (yy < _col(p["wy1"])) & (xx >= _col(p["wx0"])) & (xx < _col(p["wx1"]))
    keep = (sy >= 0) & (sy < S) & (sx >= 0) & (sx < S) & ~cut
    if not policy & (TRANSLATION | CUTOUT):
        return v if policy else x.clone()
    return _gather(v, sy, sx, keep)


def transpose(dy, u, policy):
    """T^T dy by the backward formulas of the header (not by autograd)."""
    S = dy.shape[1]
    p = params(u, S, policy)
    yy, xx = _grid(S)
    oy, ox = yy + _col(p["ty"]), xx + _col(p["tx"])          # the output position input pixel (yy, xx) lands on
    cut = (oy >= _col(p["wy0"])) & (oy < _col(p["wy1"])) & (ox >= _col(p["wx0"])) & (ox < _col(p["wx1"]))
    keep = (oy >= 0) & (oy < S) & (ox >= 0) & (ox < S) & ~cut
    e = _gather(dy, oy, ox, keep)
    if not policy & COLOR:
        return e
    ks, kc = (p[k].to(dy.dtype)[:, None, None, None] for k in ("ks", "kc"))
    e2 = kc * e + (1 - kc) * (e.sum((1, 2, 3), keepdim=True) / (3 * S * S))
    return ks * e2 + (1 - ks) * (e2.sum(3, keepdim=True) / 3)


HI = 1.0 - 2.0 ** -24        # the largest fp32 below 1


def edge_rows(gen):
    """[7, 8] rows of u that reach every clamp and edge of the parameter derivation: every slot 0 (shift -R, -R; cutout centre
    at 0, 0: three quarters of the window outside); every slot 1 - 2^-24 (the clamps: shift +R, +R; centre at S, S); a zero shift
    (u3 = u4 = 0.5); shifts (-R, +R) and (+R, -R); cutout centres (0, S) and (S, 0); the other slots random."""
    u = torch.rand(7, 8, generator=gen)
    u[0] = 0.0
    u[1] = HI
    u[2, 3:5] = 0.5
    u[3, 3], u[3, 4] = 0.0, HI
    u[4, 3], u[4, 4] = HI, 0.0
    u[5, 5], u[5, 6] = 0.0, HI
    u[6, 5], u[6, 6] = HI, 0.0
    return u.to(torch.float32)
