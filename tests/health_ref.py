"""Plain numpy / Python restatement of every definition behind --health_every (utils/health.py, csrc/health.hip): what the
tests compare the kernels and the host layer against.  fp64 throughout; sums that are the subject of a check use math.fsum
(`_sum`)."""
import math

import numpy as np


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0x7fffffff)


def _sum(terms):
    """The sum of non-negative fp64 terms, correctly rounded (math.fsum).  Past 2^16 terms -- whole networks, where fsum's
    Python loop takes seconds -- numpy's pairwise sum in the 64-bit significand of the x86 long double: its own error, about
    log2(n) 2^-64 relative, is 2^-11 / n of the (n + 1) 2^-53 the sums are held to."""
    if terms.size <= 1 << 16 or np.finfo(np.longdouble).nmant < 63:
        return math.fsum(terms)
    return float(np.sum(terms, dtype=np.longdouble))


def tensor_health(x, ref=None):
    """x, ref: float32 arrays of one size -> (out [6] float64, hist [256] int64) as include/otgan_layers.h states them."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    b = _bits(x)
    finite = b < 0x7f800000
    zero = b == 0
    xd = x[finite].astype(np.float64)
    out = np.zeros(6, np.float64)
    out[0] = _sum(xd * xd)                       # exact products
    out[1] = np.abs(xd).max() if xd.size else 0.0
    if ref is not None:
        r = np.ascontiguousarray(ref, np.float32).reshape(-1)
        assert r.size == x.size
        both = finite & (_bits(r) < 0x7f800000)
        d = x[both].astype(np.float64) - r[both].astype(np.float64)
        out[2] = _sum(d * d)
        out[3] = np.abs(d).max() if d.size else 0.0
    out[4] = int(zero.sum())
    out[5] = int((~finite).sum())
    hist = np.bincount((b[finite & ~zero] >> 23).astype(np.int64), minlength=256).astype(np.int64)
    return out, hist


def sum_bound(n, want):
    """worst case of an fp64 sum of n non-negative exact terms in any order"""
    return (n + 1) * 2.0 ** -53 * want


def plan_marginals(plan):
    """plan: float32 [n, m] -> [4] float64: max and mean of |r_i - 1|, max and mean of |c_j - n / m|"""
    p = np.asarray(plan, np.float32).astype(np.float64)
    n, m = p.shape
    r, c = np.abs(p.sum(1) - 1.0), np.abs(p.sum(0) - n / m)
    return np.array([r.max(), r.mean(), c.max(), c.mean()])


def marginals_bound(n, m):
    return (n + m + 4) * 2.0 ** -53 * max(1.0, n / m)


def below(hist, bits):
    hist = [int(c) for c in hist]
    occupied = [b for b, c in enumerate(hist) if c]
    if not occupied:
        return 0.0
    top = occupied[-1]
    return sum(c for b, c in enumerate(hist) if top - b >= bits) / sum(hist)


def kind(step, period):
    return "disc" if step % period == 0 else "gen"


def partner(anchor, period):
    """the first step after `anchor` of the other kind"""
    s = anchor + 1
    while kind(s, period) == kind(anchor, period):
        s += 1
    return s


def reported(steps, every, period):
    """the reported steps below `steps`, by the definition: the multiples of `every` and each one's partner"""
    out = set()
    for a in range(0, steps, every):
        out.add(a)
        if period >= 2 and partner(a, period) < steps:
            out.add(partner(a, period))
    return sorted(out)


def record(step, kind_, names, grads, params_before=None, params_after=None):
    """the numeric part of a record from host arrays: per variable and in total"""
    vars_, g2, p2, u2, b11, b22, nz, nonf = {}, [], [], [], 0, 0, 0, 0
    for i, name in enumerate(names):
        go, gh = tensor_health(grads[i])
        tot = int(gh.sum())
        v = {"n": int(np.asarray(grads[i]).size), "grad_norm": math.sqrt(go[0]), "grad_amax": float(go[1]), "grad_zero": int(go[4]),
             "grad_nonfinite": int(go[5]), "grad_below_11": below(gh, 11), "grad_below_22": below(gh, 22)}
        b11 += round(below(gh, 11) * tot)
        b22 += round(below(gh, 22) * tot)
        nz += tot
        nonf += int(go[5])
        g2.append(go[0])
        if params_after is not None:
            po, _ = tensor_health(params_after[i], params_before[i])
            v.update(param_norm=math.sqrt(po[0]), param_amax=float(po[1]), update_norm=math.sqrt(po[2]), update_amax=float(po[3]))
            p2.append(po[0])
            u2.append(po[2])
        vars_[name] = v
    rec = {"step": step, "kind": kind_, "grad_norm": math.sqrt(math.fsum(g2)), "grad_nonfinite": nonf,
           "grad_below_11": b11 / nz if nz else 0.0, "grad_below_22": b22 / nz if nz else 0.0, "vars": vars_}
    if params_after is not None:
        rec["param_norm"], rec["update_norm"] = math.sqrt(math.fsum(p2)), math.sqrt(math.fsum(u2))
        rec["update_ratio"] = rec["update_norm"] / rec["param_norm"]
    return rec
