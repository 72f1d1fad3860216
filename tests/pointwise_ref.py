"""References and comparison helpers for the memory-bound kernels (csrc/pointwise.hip, the absmax reduction of
csrc/winograd.hip, the batched copies).  No GPU and no library: tests/test_pointwise_ref_cpu.py exercises everything here
on the host, tests/test_pointwise_edges_gpu.py holds the kernels to it.

Three techniques:
  * integer-exact reductions -- `int_valued` inputs make every fp32 partial sum of a reduction exact in ANY order, so a sum
    is compared with `==`: one dropped row, one pitch column read, and the result differs;
  * planted extrema -- `plant` puts the maximum at the position a kernel is most likely to miss (last quad of an unrolled
    region, first of a tail, last column of a pitched row); max is order-free, so the record is compared with `==`;
  * guarded buffers -- `guarded` hands out a payload view inside a buffer pre-filled with a NaN bit pattern: a stray write
    shows in `assert_guards_intact`, a stray read poisons the result.

fp64 references are restatements of the operation in torch, gradients through torch.autograd on the fp64 forward.  The
float32 emulations of the optimiser steps round every operation once, in the order pointwise.hip writes them, with no
fused multiply-add."""
import numpy as np
import torch

SENTINEL_BITS = 0x7FC5A5A5      # a quiet NaN with a payload: never produced by arithmetic
POISON_BITS = 0x7FC1BEEF        # the fill of INPUT buffers: another NaN, so that a pitch column copied onto a guard shows
GUARD = 64                      # floats in front of and behind every guarded payload (at least)
AMAX_RECORD_FLOATS, AMAX_SUB, AMAX_SUB_STRIDE = 512, 16, 32      # csrc/common.h: amax records


def _np(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def _f64(a):
    return torch.as_tensor(_np(a)).double()


# ------------------------------------------------------------------------------------------------ comparison helpers
def assert_bits_equal(got, ref, what=""):
    """Equal as bit patterns (int32 view): NaN payloads and the sign of zero count."""
    g = np.ascontiguousarray(_np(got), dtype=np.float32)
    r = np.ascontiguousarray(_np(ref), dtype=np.float32)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    diff = g.view(np.int32) != r.view(np.int32)
    if diff.any():
        idx = tuple(int(i) for i in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} elements differ in their bits; first at {idx}: "
                             f"got {g[idx]!r} ({g.view(np.uint32)[idx]:#010x}), expected {r[idx]!r} ({r.view(np.uint32)[idx]:#010x})")


def assert_close_elementwise(got, ref, scale, tol, what=""):
    """|got - ref| <= tol * scale for EVERY element (scale broadcasts against ref); a non-finite `got` fails.  Where the
    scale is 0 the element must equal the reference.  Returns the worst ratio |err| / (tol * scale)."""
    g = _np(got).astype(np.float64)
    r = _np(ref).astype(np.float64)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    s = np.broadcast_to(np.abs(_np(scale).astype(np.float64)), r.shape)
    err = np.abs(g - r)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(s > 0, err / (tol * s), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(g), ratio, np.inf)
    if ratio.size == 0:
        return 0.0
    flat = int(np.argmax(ratio))
    worst = float(ratio.reshape(-1)[flat])
    if not worst <= 1.0:
        idx = tuple(int(i) for i in np.unravel_index(flat, r.shape))
        raise AssertionError(f"{what}: worst |err| / (tol * scale) = {worst:.3g} at {idx}: got {g[idx]!r}, expected {r[idx]!r}, "
                             f"scale {s[idx]!r}, tol {tol:g}")
    return worst


class Guarded:
    """`view`: the payload (shape `shape`, rows `pitch` floats apart) inside `buf`, which is sentinel everywhere else."""

    def __init__(self, buf, view, start, rows, cols, pitch, bits):
        self.buf, self.view, self.start, self.rows, self.cols, self.pitch, self.bits = buf, view, start, rows, cols, pitch, bits

    def payload_mask(self):
        m = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        m.as_strided((self.rows, self.cols), (self.pitch, 1), self.start).fill_(True)
        return m


def guarded(shape, pitch=None, lead=0, device="cpu", bits=SENTINEL_BITS):
    """A float32 payload of `shape` whose rows (all dimensions but the last, flattened) lie `pitch` floats apart
    (default: dense), inside a larger buffer filled with SENTINEL_BITS: GUARD + lead floats in front, the pitch columns
    of every row, and at least GUARD floats behind.  `lead` shifts the payload: lead = 1 makes it a 4-byte-aligned view
    of a live allocation, lead = 8 a column offset.  The payload itself starts out as sentinel too.  Buffers a kernel
    READS are filled with bits = POISON_BITS instead."""
    shape = tuple(int(d) for d in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    cols = shape[-1]
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    pitch = cols if pitch is None else int(pitch)
    assert pitch >= cols and rows >= 1 and cols >= 1
    start = GUARD + int(lead)
    buf = torch.empty(start + rows * pitch + GUARD, dtype=torch.float32, device=device)
    buf.view(torch.int32).fill_(bits)
    strides, s = [1], pitch
    for d in reversed(shape[1:-1] if len(shape) > 1 else ()):
        strides.insert(0, s)
        s *= d
    if len(shape) > 1:
        strides.insert(0, s)
    view = buf.as_strided(shape, tuple(strides), start)
    return Guarded(buf, view, start, rows, cols, pitch, bits)


def assert_guards_intact(g, what=""):
    """Every float of g.buf outside the payload still holds the sentinel bit pattern."""
    bad = (g.buf.view(torch.int32) != g.bits) & ~g.payload_mask()
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        where = "in front of the payload" if i < g.start else (
            "behind the payload" if i >= g.start + g.rows * g.pitch - (g.pitch - g.cols) else
            f"in a pitch column (row {(i - g.start) // g.pitch}, column {(i - g.start) % g.pitch})")
        raise AssertionError(f"{what}: {int(bad.sum())} guard floats overwritten; first at buffer index {i}, {where}: "
                             f"{float(g.buf[i])!r}")


def plant(t, index, value):
    """Put `value` at `index` (a tuple, or a flat index into the logical shape) of the array / tensor `t`."""
    if not isinstance(index, tuple):
        index = tuple(int(i) for i in np.unravel_index(int(index), tuple(t.shape)))
    t[index] = value
    return index


def int_valued(shape, lo, hi, gen):
    """float32 tensor of integers drawn uniformly from [lo, hi]: sums of fewer than 2^24 / max(|lo|, |hi|) of them are
    exact in fp32 whatever the order."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).to(torch.float32)


def record_value(rec):
    """Value of an amax record (csrc/common.h): the largest of its 16 sub-slots as BIT PATTERNS of non-negative floats
    (NaN sorts above infinity), as an np.float32."""
    r = np.ascontiguousarray(_np(rec), dtype=np.float32).reshape(-1)
    assert r.size == AMAX_RECORD_FLOATS
    bits = r.view(np.uint32)[::AMAX_SUB_STRIDE] & np.uint32(0x7FFFFFFF)
    return np.array([bits.max()], dtype=np.uint32).view(np.float32)[0]


def amax_exact(x):
    """max |x| as an np.float32; NaN if any element is NaN."""
    a = np.abs(_np(x).astype(np.float32))
    return np.float32(np.nan) if np.isnan(a).any() else np.float32(a.max() if a.size else 0.0)


def ulp_distance(got, ref):
    """Element-wise distance in units of the last place (finite float32 values)."""
    def key(a):
        i = np.ascontiguousarray(_np(a), dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(got) - key(ref))


# ------------------------------------------------------------------------------------------------ launch geometry
def _cdiv(a, b):
    return -(-a // b)


def colreduce_geometry(rows, cols):
    """(row chunks, rows per chunk) of the two-stage column reductions (pointwise.hip: colreduce / otgan_glu_bwd_colsum_f32)."""
    nchunk = max(1, min(_cdiv(1024, _cdiv(cols, 64)), 256, _cdiv(rows, 64)))
    return nchunk, _cdiv(rows, nchunk)


def colsum_chain_length(rows, cols, vec=True):
    """Longest sequential addition chain behind one output of a column reduction: a lane's rows of a chunk (16 row lanes in
    the float4 kernels, 4 in the scalar one), the 16 row lanes in LDS, a finishing lane's chunks (4 lanes share them) and
    the last four-term tree."""
    nchunk, per = colreduce_geometry(rows, cols)
    return _cdiv(per, 16 if vec else 4) + 16 + _cdiv(nchunk, 4) + 4


def grid_wrap_elements(per_thread=4):
    """Elements after which a `grid_for(n, per_thread)` launch stops growing: 4096 blocks x 256 threads x per_thread."""
    return 4096 * 256 * per_thread


def absmax_geometry(rows, C, ld):
    """Quads, blocks and grid stride of absmax_kernel (winograd.hip: op_scales), and the quad indices at the seam of its
    8-way unrolled sweep: (n4, blocks, stride, last quad of the unrolled region or None, first quad of the tail or None)."""
    n4 = rows * (C // 4)
    blocks = max(1, min(256, _cdiv(n4, 256 * 8)))
    stride = blocks * 256
    i = np.arange(stride, dtype=np.int64)
    iters = np.zeros(stride, dtype=np.int64)
    if ld == C or rows == 1:
        room = n4 - 7 * stride - 1 - i
        iters = np.where(room >= 0, room // (8 * stride) + 1, 0)
    done = iters > 0
    last_unrolled = int((i + 7 * stride + 8 * stride * (iters - 1))[done].max()) if done.any() else None
    tail = i + 8 * stride * iters
    first_tail = int(tail[tail < n4].min()) if (tail < n4).any() else None
    return n4, blocks, stride, last_unrolled, first_tail


# ------------------------------------------------------------------------------------------------ fp64 references
def colsum_exact(a):
    """Column sums of an integer-valued [rows, cols] array, in int64."""
    a = _np(a)
    ai = a.astype(np.int64)
    assert (ai == a).all()
    return ai.sum(0)


def glu_fwd(x):
    a, l = torch.chunk(_f64(x), 2, -1)
    return a * torch.sigmoid(l)


def glu_bwd(x, dy):
    x64 = _f64(x).requires_grad_(True)
    a, l = torch.chunk(x64, 2, -1)
    (dx,) = torch.autograd.grad(a * torch.sigmoid(l), x64, _f64(dy))
    return dx


def tanh_fwd(x):
    return torch.tanh(_f64(x))


def tanh_bwd(x, dy):
    x64 = _f64(x).requires_grad_(True)
    (dx,) = torch.autograd.grad(torch.tanh(x64), x64, _f64(dy))
    return dx


def feature_head_fwd(x):
    """x [N, HW, C] -> (f [N, HW * 2C], norm [N]): concat([relu(x), relu(-x)], channel), flatten, divide by the L2 norm."""
    x64 = _f64(x)
    u = torch.cat([torch.relu(x64), torch.relu(-x64)], -1).reshape(x64.shape[0], -1)
    norm = torch.sqrt((u * u).sum(1))
    return u / norm[:, None], norm


def feature_head_bwd(x, df):
    x64 = _f64(x).requires_grad_(True)
    u = torch.cat([torch.relu(x64), torch.relu(-x64)], -1).reshape(x64.shape[0], -1)
    f = u / torch.sqrt((u * u).sum(1, keepdim=True))
    (dx,) = torch.autograd.grad(f, x64, _f64(df))
    return dx


def weight_norm_fwd(V, g):
    """V [K, Cout], g [Cout] -> (w, inv): inv = rsqrt(max(sum_k V^2, 1e-12)), w = V * g * inv."""
    V64, g64 = _f64(V), _f64(g)
    inv = torch.rsqrt(torch.clamp((V64 * V64).sum(0), min=1e-12))
    return V64 * (g64 * inv), inv


def weight_norm_bwd(V, g, dw):
    V64, g64 = _f64(V).requires_grad_(True), _f64(g).requires_grad_(True)
    w = V64 * (g64 * torch.rsqrt(torch.clamp((V64 * V64).sum(0), min=1e-12)))
    dV, dg = torch.autograd.grad(w, [V64, g64], _f64(dw))
    return dV, dg


def adam64(p, g, v, mg, lr, mom1, mom2, c1, c2):
    """One Adam step of the reference in fp64 (epsilon inside the square root); v may be None when mom1 == 0."""
    p, g, mg = (_np(a).astype(np.float64) for a in (p, g, mg))
    if mom1 > 0:
        v = mom1 * _np(v).astype(np.float64) + (1.0 - mom1) * g
        vhat = v / c1
    else:
        vhat = g
    mg = mom2 * mg + (1.0 - mom2) * g * g
    return p - lr * (vhat / np.sqrt(mg / c2 + 1e-8)), v, mg


def adamax64(p, g, v, mg, lr, mom1, mom2):
    p, g, mg = (_np(a).astype(np.float64) for a in (p, g, mg))
    vt = g
    if mom1 > 0:
        v = mom1 * _np(v).astype(np.float64) + (1.0 - mom1) * g
        vt = v
    mg = np.maximum(mom2 * mg + 1e-8, np.abs(g))
    return p - lr * (vt / mg), v, mg


def nesterov64(p, g, v, lr, mom1):
    p, g, v = (_np(a).astype(np.float64) for a in (p, g, v))
    vn = mom1 * v - lr * g
    return p - mom1 * v + (1.0 + mom1) * vn, vn


def ema64(sh, p, decay):
    return decay * _np(sh).astype(np.float64) + (1.0 - decay) * _np(p).astype(np.float64)


# ------------------------------------------------------------------------------------------------ float32 emulations
_f = np.float32


def fma_f32(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in the 64-bit mantissa of np.longdouble, the sum
    is rounded there and once more to float32 (a double rounding needs a tie in bit 40: it does not occur in a test)."""
    ld = np.longdouble
    return (np.asarray(a, dtype=_f).astype(ld) * np.asarray(b, dtype=_f).astype(ld) + np.asarray(c, dtype=_f).astype(ld)).astype(_f)


def _arr(a):
    return np.ascontiguousarray(_np(a), dtype=_f)


def adam_f32(p, g, v, mg, lr, mom1, mom2, c1, c2, fused=None):
    """adam_elem of pointwise.hip, one rounding per operation.  `fused` ("v", "mg" or "p") contracts that one expression
    into a fused multiply-add -- the wrong implementation the bit-exact comparison has to catch."""
    p, g, mg = _arr(p), _arr(g), _arr(mg)
    lr_, m1, o1, m2, o2 = _f(lr), _f(mom1), _f(1.0 - mom1), _f(mom2), _f(1.0 - mom2)
    c1, c2 = _f(c1), _f(c2)
    if m1 > 0:
        v = _arr(v)
        v = fma_f32(m1, v, o1 * g) if fused == "v" else m1 * v + o1 * g
        vhat = v / c1
    else:
        vhat = g
    t = o2 * g * g
    mg = fma_f32(m2, mg, t) if fused == "mg" else m2 * mg + t
    q = vhat / np.sqrt(mg / c2 + _f(1e-8))
    pn = fma_f32(-lr_, q, p) if fused == "p" else p - lr_ * q
    assert pn.dtype == _f and mg.dtype == _f
    return pn, v, mg


def ema_f32(sh, p, decay):
    """ema_elem: decay * shadow + (1 - decay) * p."""
    return _f(decay) * _arr(sh) + _f(1.0 - decay) * _arr(p)


def adamax_f32(p, g, v, mg, lr, mom1, mom2):
    p, g, mg = _arr(p), _arr(g), _arr(mg)
    m1, o1 = _f(mom1), _f(1.0 - mom1)
    vt = g
    if m1 > 0:
        v = m1 * _arr(v) + o1 * g
        vt = v
    mg = np.maximum(_f(mom2) * mg + _f(1e-8), np.abs(g))
    return p - _f(lr) * (vt / mg), v, mg


def nesterov_f32(p, g, v, lr, mom1):
    p, g, v = _arr(p), _arr(g), _arr(v)
    m1, opm = _f(mom1), _f(1.0 + mom1)
    vn = m1 * v - _f(lr) * g
    return p - m1 * v + opm * vn, vn


def optimiser_gradient(n, gen):
    """randn * 10 ** uniform(-6, 3): nine decades, so that every branch of the rounding is met."""
    return (torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * 9.0 - 6.0)).to(torch.float32)


def int_sum_bound(rows, max_abs, unit=1.0):
    """Largest |partial sum| of `rows` values bounded by max_abs, in units of `unit` (the common divisor of the values): below
    2^24 every partial sum is an fp32 number."""
    return rows * max_abs / unit
