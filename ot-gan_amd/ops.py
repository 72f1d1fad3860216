"""torch.autograd plumbing around the HIP layer kernels (include/otgan_layers.h).

Every Function launches hand-written gfx950 kernels through the C ABI on the current
PyTorch stream; PyTorch only owns the device memory and the backward graph.  There is no
fallback: CPU tensors raise OtganError.
"""
import ctypes
import os
import sys
import weakref
from collections import OrderedDict

import torch

from . import _lib
from ._lib_layers import ConvDesc, WnBwdLayer, WnFwdLayer

ACT = {None: 0, "none": 0, "crelu": 1, "celu": 2, "elu": 3, "relu": 4}
DOUBLED = (1, 2)

_ws = {}


class _NullCtx:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NULL_CTX = _NullCtx()


def workspace(nbytes, device):
    """Grow-only scratch buffer per (device, stream) -- the caller-provided workspace of the C ABI.
    Kernels of one stream run in order, so one buffer per stream is race-free; two trainers driving
    different streams get different buffers."""
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(max(nbytes, 1 << 20)), dtype=torch.uint8, device=device)
        _ws[key] = buf
    return buf


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.OtganError("otgan_amd ops need CUDA (MI355X) tensors; there is no CPU fallback")


_map_cache = {}


def channel_maps(segs, preact, device):
    """Device tables for a *list* input (reference nn.py:198,200 interleaves per element:
    [x0,-x0,x1,-x1,...]).  Returns (cmap, inv) int32 tensors, or (None, None) when the default
    single-tensor ordering applies."""
    segs = tuple(int(s) for s in segs)
    if preact not in DOUBLED or len(segs) <= 1:
        return None, None
    key = (segs, device)
    hit = _map_cache.get(key)
    if hit is not None:
        return hit
    C = sum(segs)
    cmap, invp, invn = [], [0] * C, [0] * C
    off = 0
    for s in segs:
        base = len(cmap)
        cmap += [off + i for i in range(s)]
        cmap += [(off + i) | (1 << 31) for i in range(s)]
        for i in range(s):
            invp[off + i] = base + i
            invn[off + i] = base + s + i
        off += s
    # int32 with the sign bit as the "negate" flag
    cm = torch.tensor([c - (1 << 32) if c >= (1 << 31) else c for c in cmap], dtype=torch.int32,
                      device=device)
    inv = torch.tensor(invp + invn, dtype=torch.int32, device=device)
    _map_cache[key] = (cm, inv)
    return cm, inv


def make_desc(x, C, upsample, kh, kw, stride, cout, ldy, y_coff, preact, segs=None):
    N, H, W, ldx = x.shape
    quads = 1 if all(int(s) % 4 == 0 for s in (segs or (C,))) else 0
    return ConvDesc(N, H, W, C, ldx, 1 if upsample else 0, kh, kw, stride, cout, ldy, y_coff, preact, quads)


def out_hw(H, W, upsample, stride):
    Hin, Win = (H * 2, W * 2) if upsample else (H, W)
    return -(-Hin // stride), -(-Win // stride)


# ------------------------------------------------------------------------------- weight cache
# Normalised (and, for upsampling layers, folded) weights depend only on (V, g); the critic
# runs two or three forward passes per step on the same parameters.  Entries are keyed by the
# parameter object and validated by (global epoch, tensor versions): the optimiser / EMA kernels
# write parameters through raw pointers, so they bump `weights_epoch` explicitly.
weights_epoch = 0          # global: bumped when anything may have changed (checkpoint load, tests)
_storage_epoch = {}        # per storage: bumped by the optimiser / EMA kernels that write into it
_wcache = OrderedDict()    # id(V) -> (V, g, token, value), least recently used first
_WCACHE_MAX = 1024         # > 2 networks x (live + EMA) x ~160 layers (DenseNet); entries are evicted one by one


def bump_weights_epoch(t=None):
    """Invalidate cached normalised weights: of the storage `t` lives in, or (no argument) all."""
    global weights_epoch
    if t is None:
        weights_epoch += 1
    else:
        key = t.untyped_storage().data_ptr()
        _storage_epoch[key] = _storage_epoch.get(key, 0) + 1


def _epoch_of(t):
    return _storage_epoch.get(t.untyped_storage().data_ptr(), 0)


def _token(V, g):
    return (weights_epoch, _epoch_of(V), _epoch_of(g), V._version, g._version)


def cached_weights(V, g, compute):
    key = id(V)
    token = _token(V, g)
    hit = _wcache.get(key)
    if hit is not None and hit[0] is V and hit[1] is g and hit[2] == token:
        _wcache.move_to_end(key)
        return hit[3]
    val = compute()
    _wcache[key] = (V, g, token, val)      # holding V keeps id(V) from being reused
    _wcache.move_to_end(key)
    while len(_wcache) > _WCACHE_MAX:      # evict the least recently used entry only
        _wcache.popitem(last=False)
    return val


def weights_in(t):
    """The weight-cache entries of the parameters in `t`'s storage and the dense-block operands made from them, as they
    stand: a snapshot for reinstate_weights() (trainer.GraphedSteps keeps the ones its "gen1" capture made)."""
    key = t.untyped_storage().data_ptr()
    ents = [(k, e[0], e[1], e[3]) for k, e in _wcache.items() if e[0].untyped_storage().data_ptr() == key]
    mine = {id(e[3][0]) for e in ents}
    blocks = [(k, e) for k, e in _block_cache.items() if e[0] and all(id(w) in mine for w in e[0])]
    return ents, blocks


def forget_weights(t):
    """Drop the cache entries of the parameters in `t`'s storage (a trainer that is closed: its entries -- normalised
    weights and Winograd filters, 100+ MB for a wide layer -- would otherwise stay until 1024 newer entries evict them)."""
    ents, blocks = weights_in(t)
    for k, *_ in ents:
        _wcache.pop(k, None)
    for k, _e in blocks:
        _block_cache.pop(k, None)


def forget_stream(stream):
    """Drop the workspace of a stream that is no longer used."""
    for key in [k for k in _ws if k[1] == stream.cuda_stream]:
        del _ws[key]


def forget_side_events():
    """A step capture has ended (trainer.GraphedSteps): drop the events that ordered input-gradient filters made on the side
    stream (Conv2dFunction.forward) before their use.  An event recorded inside a capture has no meaning outside it, and
    nothing outside needs one: a replay, like an eager step, joins the side stream before its stream runs anything else."""
    for e in _wcache.values():
        if isinstance(e[3][-1], dict):
            e[3][-1].pop("bwd_event", None)


def reinstate_weights(snap):
    """Make the entries of a weights_in() snapshot the caches' again, valid at the current epochs: for a caller that has just
    recomputed every tensor they hold from the current weights (a replay of the graph that made them)."""
    ents, blocks = snap
    for k, V, g, val in ents:
        _wcache[k] = (V, g, _token(V, g), val)
        _wcache.move_to_end(k)
    for k, e in blocks:
        _block_cache[k] = e
        _block_cache.move_to_end(k)
    while len(_wcache) > _WCACHE_MAX:
        _wcache.popitem(last=False)
    while len(_block_cache) > 64:
        _block_cache.popitem(last=False)


# ------------------------------------------------------------------------------- raw launchers
def weightnorm_fwd(V2d, g):
    """V2d: [K, Cout] view of the HWIO direction tensor.  Returns (w, wT, inv_norm); w and wT carry the amax record of
    the normalised weights (the Winograd filter operands are scaled by it: prepare_filters)."""
    K, Cout = V2d.shape
    w = torch.empty_like(V2d)
    wT = torch.empty((Cout, K), dtype=V2d.dtype, device=V2d.device)
    inv = torch.empty(Cout, dtype=V2d.dtype, device=V2d.device)
    rec = amax_slot(V2d.device)
    _lib.check(_lib.lib().otgan_weightnorm_fwd_amax_f32(V2d.data_ptr(), g.data_ptr(), K, Cout,
                                                        w.data_ptr(), wT.data_ptr(), inv.data_ptr(), rec.data_ptr(),
                                                        _lib.stream_ptr()), "weightnorm_fwd")
    tag_amax(w, rec)
    tag_amax(wT, rec)
    return w, wT, inv


# Layers whose forward AND input-gradient passes take Winograd filters made from un-folded weights: both filter operands
# straight from (V, g * inv_norm); the normalised copies w / wT are never written (Conv2dFunction.forward).  False: through
# weightnorm_fwd, as every other layer (same bits; tests/test_filters_from_raw_gpu.py compares the two).
FILTERS_FROM_RAW = True


def weightnorm_scale(V2d, g):
    """Weight norm without the normalised weights.  Returns (scale, inv_norm): scale = g * inv_norm [Cout] stands in for
    w = V2d * scale -- it carries the amax record of that w and, as "raw", V2d itself; prepare_filters() makes the filters
    from the pair."""
    K, Cout = V2d.shape
    L = _lib.lib()
    inv = torch.empty(Cout, dtype=V2d.dtype, device=V2d.device)
    scale = torch.empty(Cout, dtype=V2d.dtype, device=V2d.device)
    rec = amax_slot(V2d.device)
    n = L.otgan_weightnorm_scale_scratch_floats(K, Cout)
    scratch = torch.empty(n, dtype=torch.float32, device=V2d.device)
    _lib.check(L.otgan_weightnorm_scale_amax_f32(V2d.data_ptr(), g.data_ptr(), K, Cout, inv.data_ptr(), scale.data_ptr(),
                                                 rec.data_ptr(), scratch.data_ptr(), n, _lib.stream_ptr()),
               "weightnorm_scale")
    tag_amax(scale, rec)
    leave(scale, "raw", V2d)
    return scale, inv


def weightnorm_bwd(V2d, g, inv, dw):
    K, Cout = V2d.shape
    dV = torch.empty_like(V2d)
    dg = torch.empty_like(g)
    scratch = torch.empty(Cout, dtype=V2d.dtype, device=V2d.device)
    _lib.check(_lib.lib().otgan_weightnorm_bwd_f32(V2d.data_ptr(), g.data_ptr(), inv.data_ptr(),
                                                   dw.data_ptr(), K, Cout, dV.data_ptr(),
                                                   dg.data_ptr(), scratch.data_ptr(),
                                                   _lib.stream_ptr()), "weightnorm_bwd")
    return dV, dg


def colsum(a2d_ptr, rows, cols, lda, device):
    out = torch.empty(cols, dtype=torch.float32, device=device)
    scratch = torch.empty(256 * cols, dtype=torch.float32, device=device)
    _lib.check(_lib.lib().otgan_colsum_f32(a2d_ptr, rows, cols, lda, out.data_ptr(),
                                           scratch.data_ptr(), _lib.stream_ptr()), "colsum")
    return out


# Per-launch fields of `otgan_conv_desc`: what ONE launch reads or writes beside its geometry (N ... list_quads, list_width).
# A descriptor that is kept -- in a ctx, in a dense-block plan -- holds geometry only; every launcher works on a private copy
# of the descriptor it is given, with the fields of its keyword arguments filled in.
_LAUNCH_POINTERS = ("x_amax", "dy_amax", "w_amax", "y_amax_out", "dx_amax_out", "glu_out", "glu_amax_out", "x_operand")
_LAUNCH_INTS = ("ldy", "y_accumulate")


def launch_desc(desc, **fields):
    """A private copy of `desc` with the given per-launch fields set: tensors (None: a null pointer) for the records, the
    gated product and the kept operand, `(records, count)` for x_amax / dy_amax with consecutive records, integers for ldy
    (the channel stride of dy in a backward launch) and y_accumulate.  Fields that are not named keep what `desc` holds.
    A launch and the queries that decide about it (amax_fused, otgan_conv2d_glu_fused, filter / operand bytes) take the
    same copy."""
    d = ConvDesc.from_buffer_copy(desc)
    for name, v in fields.items():
        if name in _LAUNCH_INTS:
            setattr(d, name, int(v))
        elif name in _LAUNCH_POINTERS:
            if isinstance(v, tuple):
                v, count = v
                assert name in ("x_amax", "dy_amax"), name      # the two that may be `count` consecutive records
                setattr(d, name + "_count", int(count))
            setattr(d, name, _lib.ptr(v))
        else:
            raise TypeError(f"{name} is not a per-launch field of otgan_conv_desc")
    return d


def conv_fwd_raw(desc, x, cmap, wT, bias, y, filters=None, **fields):
    L = _lib.lib()
    desc = launch_desc(desc, **fields)
    need = L.otgan_conv2d_workspace_bytes(ctypes.byref(desc), 0)
    ws = workspace(need, x.device)
    _lib.check(L.otgan_conv2d_fwd_pf_f32(ctypes.byref(desc), x.data_ptr(), _lib.ptr(cmap),
                                         wT.data_ptr(), _lib.ptr(filters), _lib.ptr(bias), y.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "conv2d_fwd")


def conv_dgrad_raw(desc, dy, w, x, inv, dx, lddx, accumulate, filters=None, **fields):
    L = _lib.lib()
    desc = launch_desc(desc, **fields)
    need = L.otgan_conv2d_workspace_bytes(ctypes.byref(desc), 1)
    ws = workspace(need, dy.device)
    _lib.check(L.otgan_conv2d_dgrad_pf_f32(ctypes.byref(desc), dy.data_ptr(), w.data_ptr(), _lib.ptr(filters),
                                           _lib.ptr(x), _lib.ptr(inv), dx.data_ptr(), lddx,
                                           1 if accumulate else 0, ws.data_ptr(), ws.numel(),
                                           _lib.stream_ptr()), "conv2d_dgrad")


def absmax_record(t):
    """amax record (otgan_layers.h: otgan_absmax_f32) of a contiguous NHWC tensor: AMAX_RECORD_FLOATS floats on its device, value =
    max |t|.  The Winograd passes scale their two-piece fp16 operands by it; computing it here, once per tensor,
    lets forward + wgrad (x) and dgrad + wgrad (dy) share one reduction."""
    rec = torch.empty(AMAX_RECORD_FLOATS, dtype=torch.float32, device=t.device)
    C = t.shape[-1]
    _lib.check(_lib.lib().otgan_absmax_f32(t.data_ptr(), t.numel() // C, C, C, rec.data_ptr(), _lib.stream_ptr()),
               "absmax")
    return rec


# ---- amax records written by the kernel that PRODUCES a tensor (otgan_layers.h: y_amax_out / dx_amax_out) -------------
# A Winograd layer scales its fp16 GEMM operands by the largest magnitude of the tensor they are a transform of.  The
# record used to come from one more pass over the tensor (absmax_record: 20 launches, 0.33 ms of a DCGAN step); now the
# kernel that writes the tensor -- GLU forward / backward, the output transforms of the strided layers, the RGB-in
# layer, the feature head's backward -- leaves it in a zeroed slot, and the tensor carries the slot to its consumer
# (hand-offs, below; a tensor that arrives without one, e.g. through a view or from outside, is reduced as before).
AMAX_RECORD_FLOATS = 512     # otgan_layers.h: OTGAN_AMAX_RECORD_FLOATS
_AMAX_SLOTS = 256
_amax_pool = {}       # device -> [zeroed [slots, AMAX_RECORD_FLOATS] tensor, next free slot]
# Constants (they were OTGAN_* environment switches while each mechanism was being A/B-ed; the measurements are in
# DESIGN / docs/history).  Tests that compare a mechanism with its predecessor patch the attribute in-process.
_GRAD_INPLACE = True      # DenseBlockFunction.backward walks ONE gradient buffer
DENSE_SPLIT = True        # dense blocks: block input and finished halves through wide Winograd convolutions (_split_block_plan)
# growth chains of 64-pixel-wide blocks on the two-scaled-fp16-piece kernels (True) or on the fp32 / three-piece kernels (False).
# Decided by an A/B of one whole block, forward + backward (128 images, C0 = 32, L = 16): h2 10.53 ms against 15.18 ms, medians
# of 7 alternating runs, the old route's runs 0.05 ms apart (profiles/densenet64_growth_ab.txt)
DENSE_H2_AT_64 = True
DENSE_GROUP = None        # growth outputs per wide convolution; None = half the block


# ---- hand-offs: values that ride on a tensor from the autograd node that produced it to the one that consumes it ------
# One attribute, (version, {kind: value}): the amax record ("amax"), the column sums ("colsum", GluFunction.backward -> the
# bias gradient of the convolution in front) and the gated product ("glu", Conv2dFunction.forward with glu_hint ->
# GluFunction.forward) of the tensor as it stood at that version.  The rule, stated once:
#   * the stamp catches what torch writes: any in-place op bumps the counter and everything left on the tensor is stale;
#   * the library writes through raw pointers, which the counter does not see: code that lets it write into a tensor it did
#     not allocate calls forget() (DenseBlockFunction.backward, when it walks the incoming gradient in place);
#   * a view shares its base's counter but not its attribute: a value does not follow a view (carry_amax does that), and an
#     in-place write to the base or to a sibling view makes it stale -- read before you write (ExtendChannelsFunction).
_HANDOFF = "_otgan_handoff"


def leave(t, kind, value):
    """Leave `value` on `t` for its consumer, valid while `t` stays at its current version.  Kinds left at the same
    version stay; what was left at an older one is discarded."""
    tag = getattr(t, _HANDOFF, None)
    if tag is None or tag[0] != t._version:
        tag = (t._version, {})
        setattr(t, _HANDOFF, tag)
    tag[1][kind] = value
    return t


def take(t, kind, remove=False):
    """What leave() left on `t` under `kind`, or None: nothing there, or the tensor was modified since."""
    tag = getattr(t, _HANDOFF, None)
    if tag is None:
        return None
    if tag[0] != t._version:
        delattr(t, _HANDOFF)         # stale: nobody can use it any more
        return None
    return tag[1].pop(kind, None) if remove else tag[1].get(kind)


def forget(t):
    """Drop everything left on `t` (a raw-pointer write is about to change it, or has)."""
    if hasattr(t, _HANDOFF):
        delattr(t, _HANDOFF)


def colsum_of(t):
    """Column sums of `t` left by its producer (GluFunction.backward), or None."""
    return take(t, "colsum")


def amax_slot(device):
    """A zeroed amax record (one launch zeroes 256 of them).  The pool is shared by the streams of a step (trainer.py runs two
    chains of a step on a second stream): a stream other than the one that zeroed the pool waits for that launch."""
    ent = _amax_pool.get(device)
    cur = torch.cuda.current_stream(device)
    if ent is None or ent[1] >= _AMAX_SLOTS:
        pool = torch.zeros((_AMAX_SLOTS, AMAX_RECORD_FLOATS), dtype=torch.float32, device=device)
        ent = [pool, 0, cur.cuda_stream, cur.record_event(), set()]
        _amax_pool[device] = ent
    elif cur.cuda_stream != ent[2] and cur.cuda_stream not in ent[4]:
        cur.wait_event(ent[3])
        ent[0].record_stream(cur)
        ent[4].add(cur.cuda_stream)
    rec = ent[0][ent[1]]
    ent[1] += 1
    return rec


def amax_slots(device, n):
    """n CONSECUTIVE zeroed records ([n, AMAX_RECORD_FLOATS]) from the pool: the record arrays of a dense block's passes
    (one row per layer) without a zeroing launch each."""
    if n > _AMAX_SLOTS:
        return torch.zeros((n, AMAX_RECORD_FLOATS), dtype=torch.float32, device=device)
    ent = _amax_pool.get(device)
    if ent is not None and ent[1] + n > _AMAX_SLOTS:
        ent[1] = _AMAX_SLOTS                      # not enough left in this pool: the next draw opens a new one
    first = amax_slot(device)                     # (opens / joins the pool; takes slot ent[1] - 1)
    ent = _amax_pool[device]
    i0 = ent[1] - 1
    ent[1] = i0 + n
    return ent[0][i0:i0 + n]


def reset_amax_pool():
    """Forget the current pool of zeroed records: the next amax_slot() allocates (and zeroes) a new one.  A step captured in
    a hipGraph calls this at the start of the capture, so that the pool's zeroing is part of the graph and every replay starts
    from zeroed records, and at its end, so that eager code never draws from a pool a replay re-zeroes."""
    _amax_pool.clear()


def tag_amax(t, rec):
    """`t` was just written by a kernel that max-accumulated |t| into rec[0]."""
    return leave(t, "amax", rec)


def amax_of(t):
    """The producer's amax record of `t`, or None (no record, or the tensor was modified since)."""
    return take(t, "amax")


def carry_amax(dst, src):
    """`dst` holds the same values as `src` (a view / reshape): the record still describes it."""
    rec = amax_of(src)
    if rec is not None:
        tag_amax(dst, rec)
    return dst


def amax_fused(desc, which):
    return bool(_lib.lib().otgan_conv2d_amax_fused(ctypes.byref(desc), which))


def shared_x_operand(desc, device):
    """Buffer for `otgan_conv_desc::x_operand` (the forward pass leaves its transformed input there, the weight
    gradient of the same x reads it back instead of transforming x again), or None when the layer's two passes do not
    share an operand.  Sets the field of the descriptor it is given: a launch_desc() copy, not one that is kept."""
    nbytes = _lib.lib().otgan_conv2d_operand_bytes(ctypes.byref(desc))
    if not nbytes:
        return None
    buf = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
    desc.x_operand = buf.data_ptr()
    return buf


def prepare_filters(desc, which, w, **fields):
    """Winograd-domain filters of a layer's forward (which=0, from wT) or dgrad (which=1, from w) pass, or None
    when the pass does not run as a Winograd GEMM (otgan_layers.h).  w_amax is the record `w` carries unless given.
    `w` may be the scale of weightnorm_scale(): the filters then come from the raw V it carries, same bits."""
    L = _lib.lib()
    # left by weightnorm_fwd on the un-folded w / wT (folded weights are another tensor: no record, the kernel reduces them)
    fields.setdefault("w_amax", amax_of(w))
    desc = launch_desc(desc, **fields)
    nbytes = L.otgan_conv2d_filter_bytes(ctypes.byref(desc), which)
    if not nbytes:
        return None
    buf = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=w.device)
    raw = take(w, "raw")
    if raw is not None:
        _lib.check(L.otgan_conv2d_prepare_filters_raw_f32(ctypes.byref(desc), which, raw.data_ptr(), w.data_ptr(),
                                                          buf.data_ptr(), buf.numel() * 4, _lib.stream_ptr()),
                   "prepare_filters_raw")
        return buf
    _lib.check(L.otgan_conv2d_prepare_filters_f32(ctypes.byref(desc), which, w.data_ptr(), buf.data_ptr(),
                                                  buf.numel() * 4, _lib.stream_ptr()), "prepare_filters")
    return buf


def conv_wgrad_raw(desc, x, cmap, dy, dw, **fields):
    L = _lib.lib()
    desc = launch_desc(desc, **fields)
    need = L.otgan_conv2d_workspace_bytes(ctypes.byref(desc), 2)
    ws = workspace(need, dy.device)
    _lib.check(L.otgan_conv2d_wgrad_f32(ctypes.byref(desc), x.data_ptr(), _lib.ptr(cmap),
                                        dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel(),
                                        _lib.stream_ptr()), "conv2d_wgrad")


def fold_weights(desc, w):
    """(weff, weffT) of an upsampling layer that the library folds (otgan_layers.h); `w` is HWIO."""
    nfold = _lib.lib().otgan_conv2d_folded_weight_elems(ctypes.byref(desc))
    weff = torch.empty(nfold, dtype=w.dtype, device=w.device)
    weffT = torch.empty(nfold, dtype=w.dtype, device=w.device)
    _lib.check(_lib.lib().otgan_conv2d_fold_weights_f32(ctypes.byref(desc), w.data_ptr(), weff.data_ptr(),
                                                        weffT.data_ptr(), _lib.stream_ptr()), "fold_weights")
    return weff, weffT


# ------------------------------------------------------------------------------- second stream for weight gradients
# A layer's weight-gradient chain (adjoint transform of dy, t-leading GEMM, adjoint filter transform, weight-norm backward) feeds
# nothing but the optimiser, while its input-gradient chain is what the next layer's backward waits for.  With a side stream set
# (trainer.py: single-process runs), Conv2dFunction.backward issues the weight-gradient chain there: the two chains alternate
# HBM-bound transforms and matrix-bound GEMMs, and on one in-order stream every kernel also waits for the previous one's last
# workgroup -- on two streams each chain's kernels start in the other's tails.  Same kernels, same arguments, same results.
# The caller joins the side stream before it reads the gradients (ops.join_side_stream).
SIDE_STREAM = None
# Variables whose weight gradient this backward pass has already produced on the side stream.  A variable used by TWO nodes of one
# graph (weight sharing, the critic called twice under grad) has its gradients accumulated by the autograd engine on the MAIN
# stream as soon as the second node returns: that node therefore makes the main stream wait for the side stream before it hands
# its gradients back (today's models use every variable once per graph, so the wait never happens).
_SIDE_SEEN = set()


def join_side_stream(tensors=()):
    """Make the current stream wait for the side stream's work and tell the allocator that `tensors` (allocated there) are
    used here from now on."""
    _SIDE_SEEN.clear()
    if SIDE_STREAM is None:
        return
    cur = torch.cuda.current_stream()
    cur.wait_stream(SIDE_STREAM)
    for t in tensors:
        if t is not None and t.is_cuda:
            t.record_stream(cur)


# The gated product a convolution wrote for the glu() that follows it (glu_hint) rides on the convolution's output (the
# "glu" hand-off) until GluFunction.forward claims it.  A caller that passes the hint and then never applies glu to that very
# tensor would keep the product alive as long as the output: the next convolution's forward pass drops it.
_PENDING_GLU = [None]


def _drop_unclaimed_glu():
    ref = _PENDING_GLU[0]
    if ref is not None:
        t = ref()
        if t is not None:
            take(t, "glu", remove=True)
        _PENDING_GLU[0] = None


# ------------------------------------------------------------------------------- conv2d / dense
# Test instrumentation (tests/test_dist_gpu.py): a list here makes every layer with a ReLU-type pre-activation and the feature
# head append the sign pattern of its input (a CPU bool tensor per call, in call order).  Two fp32 evaluations of one step
# agree to rounding EXCEPT where a pre-activation that is zero to rounding lands on different sides: the unit's gradient then
# switches branches (CReLU: [relu(x), relu(-x)], nn.py:198-200) -- counting those units separates arithmetic from flips.
SIGN_TRACE = None


def _trace_signs(x):
    if SIGN_TRACE is not None:
        SIGN_TRACE.append((x.detach() > 0).cpu())


class Conv2dFunction(torch.autograd.Function):
    """y = conv2d(preact(upsample(x)), g*V/||V||) + b     (reference nn.py:327-338).

    x: [N,H,W,C] NHWC (C may be the concatenation of a list, `segs` gives the element sizes);
    V: [KH,KW,Cin_eff,Cout]; g, b: [Cout]."""

    @staticmethod
    def forward(ctx, x, V, g, b, stride, upsample, preact, segs, glu_hint=False, grow=0):
        _need_cuda(x, V, g, b)
        _drop_unclaimed_glu()
        x = x.contiguous()
        if preact in (1, 4):
            _trace_signs(x)
        N, H, W, C = x.shape
        # a dense layer passes its [Cin_eff, Cout] variable as is (a 1x1 filter): the weight cache is keyed by
        # the parameter OBJECT, so a fresh .view() per call would miss every time and pin a new entry
        KH, KW, Cin_eff, Cout = V.shape if V.dim() == 4 else (1, 1) + tuple(V.shape)
        if Cin_eff != C * (2 if preact in DOUBLED else 1):
            raise ValueError(f"weight expects {Cin_eff} effective input channels, input gives "
                             f"{C * (2 if preact in DOUBLED else 1)}")
        V2d = V.contiguous().view(KH * KW * Cin_eff, Cout)
        OH, OW = out_hw(H, W, upsample, stride)
        grow = int(grow) if (grow and Cout % 4 == 0 and not glu_hint and _GROW_IN_PLACE) else 0
        if grow:
            # the caller appends `grow` channels next (a dense block, nn.dense_block): the output is the channel prefix of a
            # buffer with room for them (ldy of the conv ABI) -- the block grows there in place instead of copying its input
            full = torch.empty((N, OH, OW, Cout + grow), dtype=x.dtype, device=x.device)
            full._otgan_grow = True
            y = full[..., :Cout]
        else:
            y = torch.empty((N, OH, OW, Cout), dtype=x.dtype, device=x.device)
        desc = make_desc(x, C, upsample, KH, KW, stride, Cout, Cout + grow, 0, preact,
                         segs if (segs and not upsample) else None)
        # with upsample the reference concatenates the list BEFORE the pre-activation
        # (nn.py:235-237), so the doubled ordering is [x_all, -x_all], not per element
        cmap, inv = channel_maps(segs if (segs and not upsample) else (C,), preact, x.device)
        nfold = _lib.lib().otgan_conv2d_folded_weight_elems(ctypes.byref(desc))

        def has(which):
            return _lib.lib().otgan_conv2d_filter_bytes(ctypes.byref(desc), which) > 0

        # Winograd passes of a folded layer take filters made from the UN-folded weights (which = 2 forward,
        # 3 dgrad: no fold pass at all); a layer may have only the forward one (3x3 on an upsampled input)
        unf_f = bool(nfold) and has(2)
        unf_b = bool(nfold) and has(3)
        # THIS call's forward and input-gradient passes both run on prepared filters and read no weights (a list input, a
        # misaligned operand or a geometry off the Winograd passes sends a strided layer to the implicit GEMM, which does)
        raw_ok = (FILTERS_FROM_RAW and cmap is None and ((unf_f and unf_b) if nfold else (has(0) and has(1))) and
                  all(t is None or t.data_ptr() % 16 == 0 for t in (x, V2d, b)))

        def compute(raw=raw_ok):
            if raw:
                # the filters come from (V, g * inv_norm) and the normalised copies are never written.  `scale` takes their
                # place in the entry (it carries w's record)
                scale, inv_norm = weightnorm_scale(V2d, g)
                return scale, scale, inv_norm, {"fwd": prepare_filters(desc, 2 if nfold else 0, scale), "bwd": None,
                                                "bwd_done": False, "bwd_which": 3 if nfold else 1, "raw": scale}
            w, wT, inv_norm = weightnorm_fwd(V2d, g)
            wd = w                       # operand of dgrad
            if nfold and not (unf_f and unf_b):
                # conv o upsample == four parity-class convs with pre-summed taps (otgan_layers.h)
                wd_f, wT_f = fold_weights(desc, w)
                if not unf_b:
                    wd = wd_f
                if not unf_f:
                    wT = wT_f
            # Winograd-domain filters live as long as the normalised weights (the critic's survive the five
            # generator steps between its updates); the dgrad ones are made by the first backward that needs them.
            return wd, wT, inv_norm, {"fwd": prepare_filters(desc, 2 if unf_f else 0, wT), "bwd": None,
                                      "bwd_done": False, "bwd_which": 3 if unf_b else 1}

        wd, wT, inv_norm, filt = cached_weights(V, g, compute)
        if "raw" in filt and not raw_ok:
            # the entry (keyed by the parameter alone) was made by a call whose passes read no weights; this one's may:
            # it gets normalised weights of its own, and the entry stays for the calls it serves
            wd, wT, inv_norm, filt = compute(False)
        # left by the weight-norm kernel (same values in w and wT); the implicit-GEMM passes' two-piece fp16 loop scales the
        # weights by it (else it reduces them itself)
        ctx.w_rec = amax_of(wT)
        ctx.x_rec = None
        if filt["fwd"] is not None and x.is_contiguous() and C % 4 == 0:
            # Winograd passes: the record x's producer left (else one reduction of x), for the forward pass now and
            # the weight gradient later
            ctx.x_rec = amax_of(x)
            if ctx.x_rec is None:
                ctx.x_rec = absmax_record(x)
        # the forward launch: the weights' record and the record of x -- the Winograd passes' own, else what x's producer
        # left (the implicit-GEMM passes scale their two-piece operands by it, else they reduce x; the backward launches
        # do not get that one)
        fwd = launch_desc(desc, w_amax=ctx.w_rec, x_amax=ctx.x_rec if ctx.x_rec is not None else amax_of(x))
        # 288 GB of HBM: keep the transformed input of the Winograd passes for the weight gradient (0.15-0.6 GB a layer)
        ctx.x_op = None
        if (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]) and cmap is None and filt["fwd"] is not None:
            ctx.x_op = shared_x_operand(fwd, x.device)
        y_rec = y_glu = glu_rec = None
        if amax_fused(fwd, 0):
            y_rec = amax_slot(x.device)          # the kernel that writes y also leaves max |y| (for the next layer)
        if glu_hint and cmap is None and _lib.lib().otgan_conv2d_glu_fused(ctypes.byref(fwd)):
            # the caller applies a gated linear unit to y next (models/dcgan.py:50): the kernel that writes y leaves the
            # gated product (and its amax record) too; GluFunction.forward picks it up instead of reading y again
            y_glu = torch.empty((N, OH, OW, Cout // 2), dtype=x.dtype, device=x.device)
            glu_rec = amax_slot(x.device)
        # (an entry without normalised weights: with `filters` the pass reads none; V2d is a valid pointer of w's size)
        conv_fwd_raw(fwd, x, cmap, V2d if "raw" in filt else wT, b, y, filt["fwd"], y_amax_out=y_rec, glu_out=y_glu,
                     glu_amax_out=glu_rec)
        if y_glu is not None:
            leave(y, "glu", tag_amax(y_glu, glu_rec))
            _PENDING_GLU[0] = weakref.ref(y)
        if y_rec is not None:
            tag_amax(y, y_rec)
        if (SIDE_STREAM is not None and ctx.needs_input_grad[0] and not filt["bwd_done"] and
                _lib.lib().otgan_conv2d_filter_bytes(ctypes.byref(desc), filt["bwd_which"]) > 0):
            # the input-gradient pass will want its Winograd-domain filters (a function of the weights alone): made now on the
            # side stream, under this forward pass, instead of on the backward pass's critical path
            cur = torch.cuda.current_stream()
            SIDE_STREAM.wait_stream(cur)                 # (the normalised weights were written on this stream)
            # (an entry without normalised weights: this launch reads the PARAMETER V on the side stream, not a snapshot.
            # Whoever writes V next must have joined the side stream: the backward pass waits for bwd_event, and a step joins
            # before its optimiser runs (join_side_stream).  A caller that runs forward passes only under grad mode and then
            # updates V through raw pointers has to join as well.)
            with torch.cuda.stream(SIDE_STREAM):
                filt["bwd"], filt["bwd_done"] = prepare_filters(desc, filt["bwd_which"], wd), True
                filt["bwd_event"] = SIDE_STREAM.record_event()
            wd.record_stream(SIDE_STREAM)
        ctx.save_for_backward(x, V2d, g, wd, inv_norm)
        ctx.filt = filt
        ctx.desc, ctx.cmap, ctx.inv = desc, cmap, inv
        ctx.vshape = V.shape
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, V2d, g, w, inv_norm = ctx.saved_tensors
        # dy may be the channel prefix of a dense block's gradient buffer (DenseBlockFunction.backward hands it on without a
        # copy): read in place through the ABI's channel stride.  Anything else is made contiguous.
        ld = channel_prefix_stride(dy)
        if ld is None:
            dy = carry_amax(dy.contiguous(), dy)
            if "raw" in ctx.filt and dy.data_ptr() % 16:
                # (a misaligned dy would send a strided layer's input gradient off the Winograd pass, to one that reads weights)
                dy = carry_amax(dy.clone(), dy)
            ld = dy.shape[-1]
        dx = dV = dg = db = None
        dy_rec = None
        if ctx.x_rec is not None and dy.shape[-1] % 4 == 0:
            dy_rec = amax_of(dy)              # left by dy's producer, else reduced here; shared by dgrad and wgrad
            if dy_rec is None:
                dy_rec = (absmax_record(dy) if dy.is_contiguous() else
                          absmax_record_strided(dy.data_ptr(), dy.numel() // dy.shape[-1], dy.shape[-1], ld, dy.device))
        # what every launch of this pass sees: dy's channel stride in place of y's, and the records / kept operand of the
        # forward pass again
        desc = launch_desc(ctx.desc, ldy=ld, w_amax=ctx.w_rec, x_amax=ctx.x_rec, x_operand=ctx.x_op, dy_amax=dy_rec)
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            filt = ctx.filt
            if "raw" in filt:
                # no normalised weights in this entry: the filters come from (V, scale) -- also the ones a later step makes on a
                # cache hit -- and the pass, which reads none with `filters`, gets V2d as its weight pointer
                src, w = filt["raw"], V2d
            else:
                src = w
            if not filt["bwd_done"]:
                filt["bwd"], filt["bwd_done"] = prepare_filters(desc, filt["bwd_which"], src), True
            elif filt.get("bwd_event") is not None:
                # made on the side stream during a forward pass: this stream waits for that launch (once is enough, but the
                # wait is free when the event has long completed) and the buffer is in use here from now on
                torch.cuda.current_stream().wait_event(filt["bwd_event"])
                if filt["bwd"] is not None:
                    filt["bwd"].record_stream(torch.cuda.current_stream())
            dx_rec = None
            # (a list input keeps a layer off the Winograd passes; the implicit-GEMM epilogue writes every real channel
            # once whatever the channel map, round 4)
            if amax_fused(desc, 1) and (ctx.inv is None or filt["bwd"] is None):
                dx_rec = amax_slot(x.device)
            conv_dgrad_raw(desc, dy, w, x, ctx.inv, dx, x.shape[3], False, filt["bwd"], dx_amax_out=dx_rec)
            if dx_rec is not None:
                tag_amax(dx, dx_rec)
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        need_b = ctx.has_b and ctx.needs_input_grad[3]
        side = SIDE_STREAM if (need_w or need_b) else None
        if side is not None:
            # fork: everything dy depends on is enqueued on the current stream
            side.wait_stream(torch.cuda.current_stream())
            for t in (dy, x, ctx.x_op, dy_rec, ctx.x_rec):
                if t is not None:
                    t.record_stream(side)        # (dy and the kept operand are freed when this node is: not before the side stream is done)
        with (torch.cuda.stream(side) if side is not None else _NULL_CTX):
            if need_w:
                dw = torch.empty_like(V2d)
                conv_wgrad_raw(desc, x, ctx.cmap, dy, dw)
                dV2d, dg = weightnorm_bwd(V2d, g, inv_norm, dw)
                dV = dV2d.view(ctx.vshape)
            if need_b:
                db = colsum_of(dy)
                if db is None:
                    rows = dy.numel() // dy.shape[-1]
                    db = colsum(dy.data_ptr(), rows, dy.shape[-1], ld, dy.device)
        if side is not None:
            key = V2d.untyped_storage().data_ptr() + V2d.storage_offset()
            if key in _SIDE_SEEN:       # second use of this variable in one pass: the engine will add the two gradients on the main stream
                torch.cuda.current_stream().wait_stream(side)
            _SIDE_SEEN.add(key)
        return dx, dV, dg, db, None, None, None, None, None, None


def conv2d_op(x, V, g, b, stride=1, upsample=False, preact=0, segs=None, glu_hint=False, grow=0):
    """glu_hint: the caller feeds the result to glu() next -- where the library can, the layer's output kernel also
    writes the gated product and glu() takes it from there (same values; the hint changes nothing else).
    grow: the caller appends that many channels next (nn.dense_block): the result is the channel prefix of a buffer with
    room for them, same values."""
    return Conv2dFunction.apply(x, V, g, b, int(stride), bool(upsample), int(preact),
                                tuple(segs) if segs else None, bool(glu_hint), int(grow))


def channel_prefix_stride(t):
    """ld when `t` [N,H,W,C] is a channel slice of a contiguous [N,H,W,ld] buffer that the kernels can read in place
    (16-byte aligned, ld % 4 == 0), else None (also for contiguous tensors: nothing to do)."""
    if t.dim() != 4 or t.is_contiguous():
        return None
    N, H, W, C = t.shape
    ld = t.stride(2)
    if (t.stride(3) != 1 or ld < C or ld % 4 or C % 4 or t.stride(1) != W * ld or t.stride(0) != H * W * ld
            or t.data_ptr() % 16):
        return None
    return int(ld)


def grown_buffer(x, Ctot, claim=False):
    """The [N,H,W,Ctot] buffer a convolution with `grow` allocated around its output `x` (its channel prefix), or None."""
    base = x._base if x.dim() == 4 else None
    if base is None or not getattr(base, "_otgan_grow", False) or not base.is_contiguous():
        return None
    N, H, W, C = x.shape
    if tuple(base.shape) != (N, H, W, Ctot) or x.data_ptr() != base.data_ptr() or channel_prefix_stride(x) != Ctot:
        return None
    if claim:
        base._otgan_grow = False       # one block grows in a buffer
    return base


def dense_op(x, V, g, b, preact=0, segs=None):
    """x: [N, Cin]; V: [Cin_eff, Cout]  (reference nn.py:314-325) -- a 1x1 conv on a 1x1 image."""
    N, C = x.shape
    y = Conv2dFunction.apply(x.view(N, 1, 1, C), V, g, b, 1, False,
                             int(preact), tuple(segs) if segs else None)
    return y.view(N, -1)


def absmax_record_strided(t_ptr, rows, C, ld, device):
    """amax record of a channel slice [rows][C] (row stride ld floats) of a larger NHWC buffer."""
    rec = torch.empty(AMAX_RECORD_FLOATS, dtype=torch.float32, device=device)
    _lib.check(_lib.lib().otgan_absmax_f32(t_ptr, rows, C, ld, rec.data_ptr(), _lib.stream_ptr()), "absmax")
    return rec


def _input_row_order(segs0, preact, device):
    """Effective-channel rows of the block input inside a growth layer's weight tensor, in the order the
    single-tensor convolution kernels use ([act(x_all), act(-x_all)]): the reference interleaves per list element
    ([x0, -x0, x1, -x1, ...], nn.py:198-200).  None = already in that order."""
    segs0 = tuple(int(c) for c in segs0)
    if preact not in DOUBLED or len(segs0) <= 1:
        return None
    key = ("rows", segs0, device)
    hit = _map_cache.get(key)
    if hit is None:
        pos, neg, off = [], [], 0
        for c in segs0:
            pos += [2 * off + i for i in range(c)]
            neg += [2 * off + c + i for i in range(c)]
            off += c
        hit = torch.tensor(pos + neg, dtype=torch.int64, device=device)
        _map_cache[key] = hit
    return hit


def _aligned16(*ts):
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


def weightnorm_fwd_block(V2ds, gs):
    """weightnorm_fwd of every 16-output layer of a dense block in ONE launch (otgan_weightnorm_fwd_batched16_f32);
    the results are views of three block-wide buffers.  Returns [(w, wT, inv_norm)] per layer."""
    L = len(V2ds)
    Ks = [int(v.shape[0]) for v in V2ds]
    dev, dt = V2ds[0].device, V2ds[0].dtype
    w_all = torch.empty(sum(Ks) * 16, dtype=dt, device=dev)
    wT_all = torch.empty(sum(Ks) * 16, dtype=dt, device=dev)
    inv_all = torch.empty(L * 16, dtype=dt, device=dev)
    arr = (WnFwdLayer * L)()
    out, off = [], 0
    wp, tp, ip = w_all.data_ptr(), wT_all.data_ptr(), inv_all.data_ptr()
    for k in range(L):
        n = Ks[k] * 16
        a = arr[k]
        a.V, a.g, a.K = V2ds[k].data_ptr(), gs[k].data_ptr(), Ks[k]
        a.w, a.wT, a.inv = wp + 4 * off, tp + 4 * off, ip + 64 * k
        out.append((w_all[off:off + n].view(Ks[k], 16), wT_all[off:off + n].view(16, Ks[k]), inv_all[16 * k:16 * k + 16]))
        off += n
    _lib.check(_lib.lib().otgan_weightnorm_fwd_batched16_f32(arr, L, _lib.stream_ptr()), "weightnorm_fwd_batched")
    return out


def weightnorm_bwd_block(V2ds, gs, invs, parts):
    """weightnorm_bwd of every 16-output layer of a dense block in ONE launch.  parts[k]: up to three
    (tensor_or_pointer, perm, nrows, rstride) pieces of layer k's weight gradient (otgan_layers.h: otgan_wn_part).
    Returns ([dV2d_k], [dg_k])."""
    L = len(V2ds)
    Ks = [int(v.shape[0]) for v in V2ds]
    dev, dt = V2ds[0].device, V2ds[0].dtype
    dV_all = torch.empty(sum(Ks) * 16, dtype=dt, device=dev)
    dg_all = torch.empty(L * 16, dtype=dt, device=dev)
    arr = (WnBwdLayer * L)()
    dVs, dgs, off = [], [], 0
    vp, gp = dV_all.data_ptr(), dg_all.data_ptr()
    for k in range(L):
        n = Ks[k] * 16
        a = arr[k]
        a.V, a.g, a.inv = V2ds[k].data_ptr(), gs[k].data_ptr(), invs[k].data_ptr()
        a.dV, a.dg = vp + 4 * off, gp + 64 * k
        a.taps = 9
        a.Ceff = Ks[k] // 9
        for i, (ptr, perm, nrows, rstride) in enumerate(parts[k]):
            q = a.part[i]
            q.p, q.perm, q.nrows, q.rstride = ptr, (perm.data_ptr() if perm is not None else None), nrows, rstride
        dVs.append(dV_all[off:off + n].view(Ks[k], 16))
        dgs.append(dg_all[16 * k:16 * k + 16])
        off += n
    _lib.check(_lib.lib().otgan_weightnorm_bwd_batched16_f32(arr, L, _lib.stream_ptr()), "weightnorm_bwd_batched")
    return dVs, dgs


def _row_order_back(order):
    """int32 inverse of `_input_row_order`: position, in the single-tensor order, of every row of the reference's
    per-element order (None stays None)."""
    if order is None:
        return None
    key = ("back", order.data_ptr())
    hit = _map_cache.get(key)
    if hit is None:
        back = torch.empty_like(order)
        back[order] = torch.arange(order.numel(), device=order.device)
        hit = (order, back.to(torch.int32))      # holding `order` keeps its data_ptr from being reused
        _map_cache[key] = hit
    return hit[1]


_block_cache = OrderedDict()   # id(V of layer 0) -> (per-layer normalised weights it was made from, value)
DENSE16_MAX_BATCH = 16         # otgan_layers.h: OTGAN_DENSE16_MAX_BATCH (chain layers per otgan_dense16_prepare_* call)
DENSE16_MAX_CHAIN = 17         # slices per otgan_dense16_chain_{fwd,bwd}_f32 call (conv.hip)


def _wide_operands(per_layer, layers, row0, nrows, order, F, desc):
    """One wide 3x3 convolution gathered from a dense block: rows [row0, row0 + nrows) of the normalised weights of
    `layers` (the effective channels of one finished channel group), side by side.  w [9*nrows][len(layers)*F],
    wT [len(layers)*F][9*nrows], rows re-ordered to the single-tensor order when `order` is given."""
    layers = list(layers)
    nl = len(layers)
    n = nl * F
    ref = per_layer[layers[0]][0]
    w = torch.empty((9 * nrows, n), dtype=ref.dtype, device=ref.device)
    wT = torch.empty((n, 9 * nrows), dtype=ref.dtype, device=ref.device)
    map32 = None
    if order is not None:
        key = ("rows32", order.data_ptr())
        hit = _map_cache.get(key)
        if hit is None:
            hit = (order, order.to(torch.int32))      # holding `order` keeps its data_ptr from being reused
            _map_cache[key] = hit
        map32 = hit[1]
    # two launches (otgan_gather3d_batched_f32: one segment per layer) instead of a cat, an index_select and their copies
    # per operand -- 0.33 ms of framework kernels per DenseNet step before round 6; same values, bit for bit
    segs_w, segs_t = [], []
    for j, k in enumerate(layers):
        w_k, wT_k = per_layer[k][0], per_layer[k][1]
        assert w_k.is_contiguous() and wT_k.is_contiguous()
        ceff = w_k.shape[0] // 9
        assert row0 + nrows <= ceff
        # w_k [9][ceff][F] -> w [9][nrows][nl F] at column j F;  wT_k [F 9][ceff] -> wT [nl F 9][nrows] at row j F 9
        segs_w.append((w_k.data_ptr(), w.data_ptr() + 4 * j * F, 9, ceff * F, F, nrows * n, n))
        segs_t.append((wT_k.data_ptr(), wT.data_ptr() + 4 * j * F * 9 * nrows, F * 9, ceff, 1, nrows, 1))
    # the first gather also leaves the amax record of the gathered weights (w and wT hold the same elements): the filter
    # transforms of the wide convolution take it from there instead of reducing the weights again (15 launches per DenseNet step)
    rec = amax_slot(ref.device)
    gather3d_batched(segs_w, nrows, F, row0, map32, rec)
    gather3d_batched(segs_t, nrows, 1, row0, map32)
    tag_amax(w, rec)
    tag_amax(wT, rec)
    return {"w": w, "wT": wT, "fwd": prepare_filters(desc, 0, wT), "bwd": None, "bwd_done": False}


def _split_block_weights(Vs, per_layer, plan, F):
    """Operands of a dense block computed as "wide convolutions of finished channel groups + short growth chains"
    (DenseBlockFunction): per wide convolution the gathered weights and their Winograd-domain filters, per layer the
    rows of its own chain as contiguous tensors.  Cached for as long as the per-layer normalised weights are.  The operands
    are functions of the weights and of the cut, not of the batch (the Winograd filters depend on the channel counts
    alone, and which convolutions take the Winograd path does not depend on N): the entry is shared by every batch size
    with the same cut -- the critic's blocks run on nb images in a generator step and on 2 nb in a critic step, and a
    critic step reads the operands that the generator step before it made (trainer.GraphedSteps: the "gen1" graph's)."""
    key = id(Vs[0])
    ws = [pl[0] for pl in per_layer]
    hit = _block_cache.get(key)
    cut = plan["key"][1:]             # (N, ...): everything but the batch
    if hit is not None and len(hit[0]) == len(ws) and all(a is b for a, b in zip(hit[0], ws)) and hit[2] == cut:
        _block_cache.move_to_end(key)
        return hit[1]
    L = len(per_layer)
    val = {"wide": [_wide_operands(per_layer, range(wd["d0"], L), wd["row0"], wd["nrows"], wd["order"], F, wd["desc"])
                    for wd in plan["wide"]],
           "w_g": [None] * L, "wT_g": [None] * L}
    # every layer's own-chain rows (rows r0 .. of each of the 9 taps) as contiguous tensors: two flat buffers carved
    # into the layers' slices, filled by ONE batched strided copy (28 slices per 16-layer block; as framework copies these
    # were 100 of the DenseNet step's launches)
    own = [k for k in range(L) if plan["own_len"][k]]
    if own:
        dev, dt = per_layer[own[0]][0].device, per_layer[own[0]][0].dtype
        sizes = [9 * (per_layer[k][0].shape[0] // 9 - plan["own_row0"][k]) * F for k in own]
        flat_w = torch.empty(sum(sizes), dtype=dt, device=dev)
        flat_wT = torch.empty(sum(sizes), dtype=dt, device=dev)
        segs, off = [], 0
        for k, sz in zip(own, sizes):
            r0 = plan["own_row0"][k]
            ceff = per_layer[k][0].shape[0] // 9
            n_own = ceff - r0
            w_k, wT_k = per_layer[k][0], per_layer[k][1]
            assert w_k.is_contiguous() and wT_k.is_contiguous()
            val["w_g"][k] = flat_w[off:off + sz].view(9 * n_own, F)
            val["wT_g"][k] = flat_wT[off:off + sz].view(F, 9 * n_own)
            # w [9][ceff][F] -> [9][n_own][F]: 9 rows of n_own * F floats;  wT [F * 9][ceff] -> [F * 9][n_own]
            segs.append((w_k.data_ptr() + 4 * r0 * F, val["w_g"][k].data_ptr(), 9, n_own * F, ceff * F, n_own * F))
            segs.append((wT_k.data_ptr() + 4 * r0, val["wT_g"][k].data_ptr(), 9 * F, n_own, ceff, n_own))
            off += sz
        copy2d_batched(segs)
        val["_own_flat"] = (flat_w, flat_wT)
        val["h2"] = [None] * L
        if plan.get("h2"):
            # the chain weights pre-split into two scaled fp16 pieces in MFMA fragment order: one launch per block and
            # weight update (otgan_dense16_prepare_filters_f32)
            lib = _lib.lib()
            nsl = [plan["own_len"][k] for k in own]
            fbytes = [int(lib.otgan_dense16_filter_bytes(n)) for n in nsl]
            flat_q = torch.empty(sum(fbytes), dtype=torch.uint8, device=dev)
            off = 0
            for k, nb in zip(own, fbytes):
                val["h2"][k] = flat_q[off:off + nb]
                off += nb
            n = len(own)
            pw = (ctypes.c_void_p * n)(*[val["wT_g"][k].data_ptr() for k in own])
            pn = (ctypes.c_int * n)(*nsl)
            pf = (ctypes.c_void_p * n)(*[val["h2"][k].data_ptr() for k in own])
            _lib.check(lib.otgan_dense16_prepare_filters_f32(ctypes.cast(pw, ctypes.c_void_p), ctypes.cast(pn, ctypes.c_void_p),
                                                              ctypes.cast(pf, ctypes.c_void_p), n, _lib.stream_ptr()),
                       "dense16_prepare_filters")
            val["_h2_flat"] = flat_q
    _block_cache[key] = (ws, val, cut)
    while len(_block_cache) > 64:
        _block_cache.popitem(last=False)
    return val


def _split_block_plan(N, H, W, C0, L, F, segs0, preact, device):
    """How a dense block is cut (None: not at all).  The pre-activation of layer k is linear in act(every earlier
    channel), so the share of a FINISHED channel group in all later layers is one 3x3 convolution group -> (later
    layers) * F, wide enough for the Winograd F(4x4,3x3) passes:
      * the block input (C0 channels) into all L layers, before the chain starts;
      * every group of `DENSE_GROUP` (default L/2: the first half into the second half) consecutive growth outputs
        into all layers after the group, once its last layer is done -- as long as the library takes that convolution
        on its Winograd path.
    What stays on the 16-output growth kernels is each layer's chain inside its own group."""
    if not DENSE_SPLIT or F != 16 or L < 2 or any(int(c) % 4 for c in segs0):
        return None
    mult = 2 if preact in DOUBLED else 1
    Ctot = C0 + L * F
    lib = _lib.lib()
    desc_in = ConvDesc(N, H, W, C0, Ctot, 0, 3, 3, 1, L * F, Ctot, C0, preact, 1)
    if not lib.otgan_conv2d_filter_bytes(ctypes.byref(desc_in), 0):
        return None
    wide = [{"desc": desc_in, "x_off": 0, "C": C0, "d0": 0, "row0": 0, "nrows": C0 * mult,
             "order": _input_row_order(segs0, preact, device), "accumulate": 0, "after": -1}]
    # measured on the DenseNet step (L = 16): halves 51.9 ms, groups of four 52.9 (with 64-column convolutions allowed
    # 53.5), pairs 60.7, block input only 58.2 -- a wide convolution with K = 128 is bound by its transforms
    group = (L + 1) // 2 if DENSE_GROUP is None else int(DENSE_GROUP)
    g0 = [0] * L          # growth outputs [0, g0[k]) reach layer k through wide convolutions
    for s0 in range(0, L, group) if group > 0 else ():
        s1 = min(s0 + group, L)
        if s1 >= L:
            break
        n = s1 - s0
        desc = ConvDesc(N, H, W, n * F, Ctot, 0, 3, 3, 1, (L - s1) * F, Ctot, C0 + s1 * F, preact, 1)
        if not lib.otgan_conv2d_filter_bytes(ctypes.byref(desc), 0):
            break         # later groups feed fewer layers still
        wide.append({"desc": desc, "x_off": C0 + s0 * F, "C": n * F, "d0": s1, "row0": (C0 + s0 * F) * mult,
                     "nrows": n * F * mult, "order": _input_row_order((F,) * n, preact, device), "accumulate": 1,
                     "after": s1 - 1})
        for k in range(s1, L):
            g0[k] = s1
    for wd in wide:
        wd["back"] = _row_order_back(wd["order"])
    # the chains on the two-scaled-fp16-piece kernel (CReLU, 16-channel list elements; otgan_layers.h: list_width)
    probe = ConvDesc(N, H, W, F, Ctot, 0, 3, 3, 1, F, Ctot, C0, preact, 1)
    probe.list_width = F
    h2 = bool(lib.otgan_dense16_h2_ok(ctypes.byref(launch_desc(probe, y_accumulate=1)))) and (W != 64 or DENSE_H2_AT_64)
    # the library prepares at most OTGAN_DENSE16_MAX_BATCH chain layers per call (forward and by-slice backward filters) and
    # a chain call takes at most 17 slices per group: longer blocks / groups (layers_per_block > 18 at the default grouping)
    # keep the fp32 growth kernels
    own_len = [k - g0[k] for k in range(L)]
    starts = sorted({wd["d0"] for wd in wide}) + [L]
    if sum(1 for n in own_len if n) > DENSE16_MAX_BATCH or max(b - a for a, b in zip(starts[:-1], starts[1:])) > DENSE16_MAX_CHAIN:
        h2 = False
    return {"wide": wide, "g0": g0, "own_len": own_len, "h2": h2,
            "own_row0": [(C0 + g0[k] * F) * mult for k in range(L)],
            "key": (N, H, W, C0, L, F, tuple(segs0), preact, tuple(g0), h2)}


def _calibrate_backward_arg_refs():
    """sys.getrefcount of the gradient argument inside a custom Function's backward when nothing but the engine and the
    call hold it (a CPU mini-graph; the count is a property of the interpreter / torch build, 6 on Python 3.10 + torch 2.10)."""
    seen = []

    class _Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2

        @staticmethod
        def backward(ctx, dy):
            seen.append(sys.getrefcount(dy))
            return dy

    with torch.enable_grad():
        x = torch.zeros(2, requires_grad=True)
        (_Probe.apply(x) * 3).sum().backward()
    return seen[0]


_BACKWARD_ARG_REFS = _calibrate_backward_arg_refs()
# False (tests): convolutions ignore `grow`, dense blocks copy their input into their own buffer as before round 5
_GROW_IN_PLACE = True


class DenseBlockFunction(torch.autograd.Function):
    """L weight-normalised convolutions that each read the concatenation of everything before
    them and append `F` channels (reference models/densenet.py:11-16: `x.append(conv2d(x, F))`).

    The block grows IN PLACE: one [N,H,W,C0+L*F] buffer, layer k reads channels [0, Ck) through
    the channel map of its list segmentation and writes channels [Ck, Ck+F) (ldy / y_coff of
    the conv ABI).  The backward pass walks the layers in reverse over one gradient buffer:
    layer k's dy is a channel slice of it and its dgrad accumulates into channels [0, Ck).
    No concatenation copies, no per-layer activation tensors.

    Finished channel groups are taken out of the chain (`_split_block_plan`): every layer's pre-activation is linear
    in act(earlier channels), so the block input's share of ALL L layers is one 3x3 convolution C0 -> L*F written
    straight into channels [C0, Ctot) of the buffer, and the finished first half of the growth outputs enters the second
    half of the layers through one more (L/2)*F -> (L/2)*F convolution added onto them -- GEMMs wide enough for the
    Winograd F(4x4,3x3) passes on the split-precision engine (2.25 instead of 9 products per output); layer k then
    only adds the convolution of the growth outputs of its own group (`y_accumulate`).  Backward mirrors it: the
    growth layers' dgrad / wgrad see their own group only, each wide convolution takes one dgrad and one wgrad
    against the finished gradient of the channels it wrote.  Same sums in a different order; chosen when the
    library routes the wide convolutions to its Winograd path (the module constants DENSE_SPLIT = False: never,
    DENSE_GROUP = n: groups of n, 0: the block input only).

    args: x0 [N,H,W,C0] (concatenated initial list), then V_k, g_k, b_k for every layer."""

    @staticmethod
    def forward(ctx, x0, segs0, ksize, preact, *params):
        _need_cuda(x0)
        L = len(params) // 3
        N, H, W, C0 = x0.shape
        F = params[0].shape[-1]
        Ctot = C0 + L * F
        buf = grown_buffer(x0, Ctot, claim=True)      # the producing convolution left room (conv2d_op grow): no copy
        if buf is None:
            buf = torch.empty((N, H, W, Ctot), dtype=x0.dtype, device=x0.device)
            buf[..., :C0].copy_(x0)
        mult = 2 if preact in DOUBLED else 1
        saved, descs, maps, per_layer = [], [], [], []
        segs = list(segs0)
        V2ds = []
        for k in range(L):
            V = params[3 * k]
            assert tuple(V.shape) == (ksize, ksize, (C0 + k * F) * mult, F), (V.shape, C0 + k * F, mult)
            V2ds.append(V.contiguous().view(-1, F))
        gs = list(params[1::3])
        ctx.batched = F == 16 and ksize == 3 and _aligned16(*V2ds, *gs)     # one weight-norm launch per block and pass
        batch = []

        def normalised(k):
            # all layers of the block in one launch the first time any of them misses the cache
            if ctx.batched:
                if not batch:
                    batch.extend(weightnorm_fwd_block(V2ds, gs))
                return batch[k]
            return weightnorm_fwd(V2ds[k], gs[k])

        for k in range(L):
            per_layer.append(cached_weights(params[3 * k], gs[k], lambda k=k: normalised(k)))
            saved += [V2ds[k], gs[k], per_layer[k][0], per_layer[k][2]]
        ctx.vshapes = [p.shape for p in params[0::3]]
        ctx.L, ctx.C0, ctx.F = L, C0, F

        plan = None
        if ksize == 3 and all(p is not None for p in params[2::3]):
            plan = _split_block_plan(N, H, W, C0, L, F, segs0, preact, x0.device)
        ctx.plan = plan
        if plan is not None:
            sw = _split_block_weights(params[0::3], per_layer, plan, F)
            # the L biases side by side, kept with the block's operands: rebuilt with them after a weight update (the optimiser
            # kernels bump the storage epoch that invalidates `sw`), or when a torch op touched a bias (version counters)
            bkey = tuple((id(b), b._version) for b in params[2::3])
            if sw.get("bias_key") != bkey:
                sw["bias_all"], sw["bias_key"] = torch.cat([b.detach() for b in params[2::3]]), bkey
            bias_all = sw["bias_all"]
            rows = N * H * W
            wides = plan["wide"]
            # what the wide convolutions' backward launches get again: the record(s) of their input, their kept operand
            ctx.x_recs, ctx.x_ops = [None] * len(wides), [None] * len(wides)
            # amax records without extra passes: every kernel that writes growth channels -- the wide convolutions (the
            # second one adds onto the first) and the 16-output kernels of the chains -- leaves the largest magnitude of the
            # values it writes in a record (layout below); the block's output carries max(record of x0, all of them) for
            # the transition that reads the whole buffer.
            rec_x0 = amax_of(x0)
            # round 4: ONE zeroed array of records per block.  Group i (the layers between two wide convolutions) owns
            # rows [gbase(i), gbase(i + 1)): first the record of the sums the group's wide convolution leaves in the
            # growth channels it writes (W_i: bounds every slice a layer of the group finishes without a chain kernel,
            # and the partial sums of the others), then one record per layer of the group, written by the chain kernel
            # that finishes the layer's slice.  A chain kernel reads rows [gbase, gbase + 1 + j) -- consecutive records,
            # otgan_conv_desc::x_amax_count -- as the bound of the slices it multiplies (the two-scaled-fp16-piece
            # kernel needs it; records are only ever read by launches after their writers: deterministic).
            gbase = [wd["d0"] + i for i, wd in enumerate(wides)] + [L + len(wides)]
            gidx = {wd["d0"]: i for i, wd in enumerate(wides)}
            R = amax_slots(buf.device, L + len(wides))

            def wide_fwd(i):
                wd, ops_ = wides[i], sw["wide"][i]
                src = buf[..., wd["x_off"]:]       # channel slice: same rows, pointer advanced by x_off floats
                if i == 0 and rec_x0 is not None:
                    x_amax = (rec_x0, 1)
                elif i > 0:
                    # the finished slices of the group that feeds this convolution: its rows of R as they are
                    # (otgan_conv_desc::x_amax_count consecutive records; until round 4 an amax over them: one launch)
                    x_amax = (R[gbase[i - 1]:gbase[i]], gbase[i] - gbase[i - 1])
                else:
                    x_amax = (absmax_record_strided(src.data_ptr(), rows, wd["C"], Ctot, buf.device), 1)
                ctx.x_recs[i] = x_amax
                desc = launch_desc(wd["desc"], x_amax=x_amax, y_accumulate=wd["accumulate"], y_amax_out=R[gbase[i]])
                if any(ctx.needs_input_grad[4:]):
                    ctx.x_ops[i] = shared_x_operand(desc, buf.device)    # read back by this convolution's wgrad
                conv_fwd_raw(desc, src, None, ops_["wT"], None if wd["accumulate"] else bias_all, buf, ops_["fwd"])

            def chain_desc(n_own, k):
                desc = ConvDesc(N, H, W, n_own * F, Ctot, 0, ksize, ksize, 1, F, Ctot, C0 + k * F, preact, 1)
                desc.list_width = F
                return desc

            wide_fwd(0)
            chain_h2 = plan.get("h2") and all(sw["h2"][k] is not None for k in range(L) if plan["own_len"][k])
            if chain_h2:
                # every group's chain in one library call (otgan_dense16_chain_fwd_f32: its layers' launches back to back)
                lib = _lib.lib()
                for gi, wd in enumerate(wides):
                    d0, d1 = wd["d0"], (wides[gi + 1]["d0"] if gi + 1 < len(wides) else L)
                    if gi > 0:
                        wide_fwd(gi)        # (the group that feeds this one is finished)
                    if d1 - d0 >= 2:
                        pf = (ctypes.c_void_p * (d1 - d0 - 1))(*[sw["h2"][k].data_ptr() for k in range(d0 + 1, d1)])
                        _lib.check(lib.otgan_dense16_chain_fwd_f32(N, H, W, d1 - d0, buf.data_ptr() + 4 * (C0 + d0 * F), Ctot,
                                                                   ctypes.cast(pf, ctypes.c_void_p), R[gbase[gi]].data_ptr(),
                                                                   _lib.stream_ptr()), "dense16_chain_fwd")
                for k in range(L):      # descriptors / maps of the chain layers (their weight gradients use them)
                    n_own = plan["own_len"][k]
                    descs.append(chain_desc(n_own, k) if n_own else None)
                    maps.append(channel_maps((F,) * n_own, preact, x0.device) if n_own else (None, None))
            for k in range(L) if not chain_h2 else ():
                n_own = plan["own_len"][k]
                desc = cmap = inv = None
                if n_own:
                    g0 = plan["g0"][k]
                    gi = gidx[g0]
                    desc = chain_desc(n_own, k)
                    cmap, inv = channel_maps((F,) * n_own, preact, x0.device)
                    conv_fwd_raw(desc, buf[..., C0 + g0 * F:], cmap, sw["wT_g"][k], None, buf, sw["h2"][k], y_accumulate=1,
                                 x_amax=(R[gbase[gi]], 1 + n_own), y_amax_out=R[gbase[gi] + 1 + n_own])
                descs.append(desc)
                maps.append((cmap, inv))
                for i, wd in enumerate(wides):
                    if wd["after"] == k:       # the group that ends with layer k is finished
                        wide_fwd(i)
            ctx.sw = sw
            ctx.save_for_backward(buf, *saved)
            ctx.descs, ctx.maps = descs, maps
            ctx.fwd_recs = (R, gbase, gidx)      # read again by the chains' weight gradients
            # ctx.x_recs[0]: the producer's record of x0, or the reduction wide_fwd(0) made
            tag_amax(buf, torch.maximum(ctx.x_recs[0][0], R.amax(0)))
            return buf

        for k in range(L):
            b = params[3 * k + 2]
            Ck = C0 + k * F
            desc = ConvDesc(N, H, W, Ck, Ctot, 0, ksize, ksize, 1, F, Ctot, Ck, preact,
                            1 if all(s % 4 == 0 for s in segs) else 0)
            cmap, inv = channel_maps(tuple(segs), preact, x0.device)
            conv_fwd_raw(desc, buf, cmap, per_layer[k][1], b, buf)
            descs.append(desc)
            maps.append((cmap, inv))
            segs.append(F)
        ctx.save_for_backward(buf, *saved)
        ctx.descs, ctx.maps = descs, maps
        return buf

    @staticmethod
    def backward(ctx, dbuf):
        # gradient w.r.t. the whole concatenation; the earlier slices' gradients are accumulated into it.  The incoming
        # tensor itself is used when nothing else can see it -- contiguous and referenced only by the engine and this call
        # (a gradient that a torch op hands to two nodes at once, e.g. of `block_a + block_b`, has more references) --
        # instead of a copy of the whole buffer per block and pass (0.5 ms of a DenseNet step).
        # `_use_count` counts references to the C++ tensor, not Python references to its wrapper: a gradient that a tensor
        # hook (register_hook) or an upstream custom Function has kept alive shows up in sys.getrefcount only.
        # Both are checked, the second against the count an un-retained gradient has inside a custom backward in this
        # interpreter / torch build (calibrated at import): a retained gradient is copied, never overwritten.
        if (_GRAD_INPLACE and dbuf.is_contiguous() and hasattr(dbuf, "_use_count") and dbuf._use_count() <= 2 and
                sys.getrefcount(dbuf) <= _BACKWARD_ARG_REFS):
            G = dbuf
        else:
            G = dbuf.contiguous().clone()
        try:
            return DenseBlockFunction._backward_impl(ctx, dbuf, G)
        finally:
            if G is dbuf:
                forget(dbuf)      # the raw kernels wrote into the incoming tensor (hand-offs: the rule above leave())

    @staticmethod
    def _backward_impl(ctx, dbuf, G):
        buf, *saved = ctx.saved_tensors
        L, C0, F = ctx.L, ctx.C0, ctx.F
        N, H, W, Ctot = buf.shape
        need_w = any(ctx.needs_input_grad[4:])
        grads = [None] * (3 * L)
        rows = N * H * W
        plan = ctx.plan
        if plan is not None and plan.get("h2") and ctx.batched and len(plan["wide"]) <= 2:
            grads = _backward_by_slice(ctx, buf, saved, G, dbuf, need_w)
            dx0 = _block_input_grad(G, C0) if ctx.needs_input_grad[0] else None
            if dx0 is not None and C0 % 4 == 0:
                tag_amax(dx0, ctx.dx0_rec)
            return (dx0, None, None, None, *grads)
        if plan is not None:
            sw = ctx.sw
            dw_g = [None] * L
            dw_wide = [None] * len(plan["wide"])

            def wide_bwd(i, need_dx):
                # channels [C0 + d0*F, Ctot) of G are final here: one reduction of them for the two passes
                d0 = plan["wide"][i]["d0"]
                dy_rec = absmax_record_strided(G.data_ptr() + 4 * (C0 + d0 * F), rows, (L - d0) * F, Ctot, G.device)
                dw_wide[i] = _wide_bwd(ctx, buf, G, i, need_w, need_dx, dy_rec)

            for k in reversed(range(L)):
                for i in reversed(range(1, len(plan["wide"]))):
                    if plan["wide"][i]["after"] == k:
                        wide_bwd(i, True)
                if plan["own_len"][k]:
                    desc = ctx.descs[k]
                    cmap, inv = ctx.maps[k]
                    off = C0 + plan["g0"][k] * F
                    if need_w:
                        dw_g[k] = torch.empty_like(sw["w_g"][k])
                        conv_wgrad_raw(desc, buf[..., off:], cmap, G, dw_g[k])
                    # d/d(growth outputs of the layer's own half) accumulates into their channels of G
                    conv_dgrad_raw(desc, G, sw["w_g"][k], buf[..., off:], inv, G[..., off:], Ctot, True)
            wide_bwd(0, ctx.needs_input_grad[0])
            if need_w and ctx.batched and len(plan["wide"]) <= 2:
                _block_weight_grads(ctx, saved, grads, dw_g, dw_wide)
            elif need_w:
                for k in range(L):
                    V2d, g, w, inv_norm = saved[4 * k:4 * k + 4]
                    parts = []
                    for i, wd in enumerate(plan["wide"]):
                        if wd["d0"] <= k:
                            dwi = dw_wide[i].view(9, wd["nrows"], L - wd["d0"], F)
                            if wd["back"] is not None:
                                dwi = dwi.index_select(1, wd["back"].long())
                            parts.append(dwi[:, :, k - wd["d0"], :])
                    if dw_g[k] is not None:
                        parts.append(dw_g[k].view(9, -1, F))
                    dw = torch.cat(parts, dim=1) if len(parts) > 1 else parts[0].contiguous()
                    dV2d, dg = weightnorm_bwd(V2d, g, inv_norm, dw.view(-1, F))
                    grads[3 * k:3 * k + 2] = [dV2d.view(ctx.vshapes[k]), dg]
        else:
            dws = [None] * L
            for k in reversed(range(L)):
                V2d, g, w, inv_norm = saved[4 * k:4 * k + 4]
                desc = ctx.descs[k]
                cmap, inv = ctx.maps[k]
                if need_w:
                    dws[k] = torch.empty_like(V2d)
                    conv_wgrad_raw(desc, buf, cmap, G, dws[k])
                    if not ctx.batched:
                        dV2d, dg = weightnorm_bwd(V2d, g, inv_norm, dws[k])
                        grads[3 * k:3 * k + 2] = [dV2d.view(ctx.vshapes[k]), dg]
                # d/d(inputs of layer k) accumulates into the first Ck channels of G
                conv_dgrad_raw(desc, G, w, buf, inv, G, Ctot, True)
            if need_w and ctx.batched:
                _block_weight_grads(ctx, saved, grads, dws)
        if need_w:
            _block_bias_grads(ctx, G, grads)
        dx0 = _block_input_grad(G, C0) if ctx.needs_input_grad[0] else None
        return (dx0, None, None, None, *grads)


def _wide_bwd(ctx, buf, G, i, need_w, need_dx, dy_amax, dx_amax_out=None, wgrad_stream=None):
    """Backward of wide convolution i of a split block, once the gradient of the channels it wrote ([C0 + d0*F, Ctot) of G)
    is final: its weight gradient (returned: [9][nrows][layers d0 ..][F], rows in the convolution's own order; issued under
    `wgrad_stream()` when given) and, with need_dx, its input gradient added into G.  dy_amax bounds those channels of G,
    dx_amax_out receives the largest magnitude the input gradient writes; the record(s) of the input and the kept operand are
    the forward launch's (ctx.x_recs, ctx.x_ops)."""
    wd, ops_ = ctx.plan["wide"][i], ctx.sw["wide"][i]
    src, gsrc = buf[..., wd["x_off"]:], G[..., wd["x_off"]:]
    desc = launch_desc(wd["desc"], x_amax=ctx.x_recs[i], x_operand=ctx.x_ops[i], dy_amax=dy_amax)
    dw = None
    if need_w:
        with (wgrad_stream() if wgrad_stream is not None else _NULL_CTX):
            dw = torch.empty_like(ops_["w"])
            conv_wgrad_raw(desc, src, None, G, dw)
    if need_dx:
        if not ops_["bwd_done"]:
            ops_["bwd"], ops_["bwd_done"] = prepare_filters(desc, 1, ops_["w"]), True
        conv_dgrad_raw(desc, G, ops_["w"], src, None, gsrc, G.shape[-1], True, ops_["bwd"], dx_amax_out=dx_amax_out)
    return dw


def _block_weight_grads(ctx, saved, grads, dw_g, dw_wide=()):
    """grads[3 k], grads[3 k + 1] (dV, dg) of every layer of a dense block from the pieces of its weight gradient where the
    passes left them -- a column slice of each wide convolution's dw, in that convolution's row order, then the layer's own
    chain (dw_g[k]; the whole gradient when the block is not split) -- in one launch (weightnorm_bwd_block)."""
    L, F = ctx.L, ctx.F
    parts = []
    for k in range(L):
        pk = []
        for wd, dw in zip(ctx.plan["wide"] if dw_wide else (), dw_wide):
            if wd["d0"] <= k:
                pk.append((dw.data_ptr() + 4 * (k - wd["d0"]) * F, wd["back"], wd["nrows"], (L - wd["d0"]) * F))
        if dw_g[k] is not None:
            pk.append((dw_g[k].data_ptr(), None, dw_g[k].shape[0] // 9, F))
        parts.append(pk)
    dVs, dgs = weightnorm_bwd_block(saved[0::4], saved[1::4], saved[3::4], parts)
    for k in range(L):
        grads[3 * k:3 * k + 2] = [dVs[k].view(ctx.vshapes[k]), dgs[k]]


def _block_bias_grads(ctx, G, grads):
    """grads[3 k + 2] of every layer of a dense block.  Layer k's output gradient G[..., Ck:Ck+F] is final once the layers
    after it have been processed, and no earlier layer writes there: all L bias gradients are the column sums of the
    finished G -- one reduction instead of L."""
    L, C0, F = ctx.L, ctx.C0, ctx.F
    Ctot = G.shape[-1]
    db_all = colsum(G.data_ptr() + 4 * C0, G.numel() // Ctot, L * F, Ctot, G.device)
    for k in range(L):
        grads[3 * k + 2] = db_all[k * F:(k + 1) * F]


def _block_input_grad(G, C0):
    """Gradient of a dense block's input = channels [0, C0) of its finished gradient buffer: handed on as a VIEW when the
    kernels of the layer in front can read it through a channel stride (Conv2dFunction.backward: channel_prefix_stride),
    else as a copy (round 5: one copy of the block input's gradient per block and pass less)."""
    v = G[..., :C0]
    return v if channel_prefix_stride(v) is not None else v.contiguous()


def _dense16_bwd_filters(sw, plan, L, F, device):
    """Prepared weights of the by-slice input gradient (otgan_dense16_prepare_bwd_filters_f32): per output slice c one
    buffer holding the pairs (c, k), k = the later layers of c's group.  Cached with the block's forward operands."""
    hit = sw.get("h2_bwd")
    if hit is not None:
        return hit
    from ._lib_layers import Dense16BwdPair
    lib = _lib.lib()
    starts = [wd["d0"] for wd in plan["wide"]] + [L]
    gend = {}
    for a, b in zip(starts[:-1], starts[1:]):
        for c in range(a, b):
            gend[c] = b
    nsl = {c: gend[c] - 1 - c for c in range(L) if gend[c] - 1 - c >= 1}
    sizes = {c: int(lib.otgan_dense16_bwd_filter_bytes(n)) for c, n in nsl.items()}
    flat = torch.empty(sum(sizes.values()), dtype=torch.uint8, device=device)
    out, off, pairs = {}, 0, []
    for c in sorted(nsl):
        out[c] = flat[off:off + sizes[c]]
        off += sizes[c]
        for j in range(nsl[c]):
            k = c + 1 + j
            pairs.append(Dense16BwdPair(sw["w_g"][k].data_ptr(), sw["h2"][k].data_ptr(), out[c].data_ptr(),
                                        plan["own_len"][k], c - plan["g0"][k], j))
    allf = [sw["h2"][k] for k in range(L) if sw["h2"][k] is not None]
    if pairs:
        arr = (Dense16BwdPair * len(pairs))(*pairs)
        pf = (ctypes.c_void_p * len(allf))(*[t.data_ptr() for t in allf])
        _lib.check(lib.otgan_dense16_prepare_bwd_filters_f32(ctypes.cast(arr, ctypes.c_void_p), len(pairs),
                                                              ctypes.cast(pf, ctypes.c_void_p), len(allf), _lib.stream_ptr()),
                   "dense16_prepare_bwd_filters")
    res = {"flat": flat, "slice": out, "nsl": nsl}
    sw["h2_bwd"] = res
    return res


def _backward_by_slice(ctx, buf, saved, G, dbuf, need_w):
    """Backward of a split dense block whose chains run on the two-scaled-fp16-piece kernels (plan["h2"]): the input
    gradient of the chains is gathered per SLICE, last slice first (otgan_dense16_bwd_slice_f32: one read-modify-write of
    each slice instead of one per (layer, earlier slice) pair), and every kernel that adds into the gradient buffer leaves
    the largest magnitude it wrote in a record -- no reduction passes over slices of the buffer (round 3: two per block).
    Returns the list of parameter gradients (grads[3 k + 2], the biases, included)."""
    L, C0, F = ctx.L, ctx.C0, ctx.F
    N, H, W, Ctot = buf.shape
    plan, sw = ctx.plan, ctx.sw
    lib = _lib.lib()
    grads = [None] * (3 * L)
    dw_g = [None] * L
    wides = plan["wide"]
    dw_wide = [None] * len(wides)
    bw = _dense16_bwd_filters(sw, plan, L, F, buf.device)
    # records: Rc bounds the incoming gradient and everything the wide convolutions' input gradients add; RS[c] what the
    # slice kernel of slice c leaves.  A reader takes the maximum of Rc and the rows of the slices it reads.
    # One array: rows [0, L) = RS, row L = Rc -- a reader of the slices from d0 on passes rows [d0, L] as they are
    # (otgan_conv_desc::dy_amax_count consecutive records; until round 4 an amax over the rows and a maximum with Rc: two launches).
    tag = amax_of(dbuf)
    RR = amax_slots(buf.device, L + 1)
    RS, Rc = RR[:L], RR[L]
    Rc.copy_(tag if tag is not None else absmax_record(G))
    R0 = amax_slot(buf.device)
    ctx.dx0_rec = R0
    gptr, bptr = G.data_ptr(), buf.data_ptr()
    # weight-gradient work on the side stream (SIDE_STREAM, see Conv2dFunction.backward): every weight gradient of the block
    # reads slices of G that are FINAL when it is issued and writes its own tensors, so it can run under the input-gradient
    # kernels that follow on this stream (they add into OTHER channels of G)
    side = SIDE_STREAM if need_w else None
    if side is not None:
        for t in [G, buf, RR, R0, ctx.fwd_recs[0]] + [t for t in ctx.x_ops if t is not None]:
            t.record_stream(side)

    def wgrad_stream():
        if side is None:
            return _NULL_CTX
        side.wait_stream(torch.cuda.current_stream())      # (what the weight gradient reads is enqueued on this stream)
        return torch.cuda.stream(side)

    def wide_bwd(i, need_dx):
        # the slices from d0 on and the incoming bound: rows [d0, L] of RR as they are.  i = 0 writes the block input's
        # gradient (sums onto the incoming one): its own record, handed to the layer in front of the block with dx0
        # (round 4: that layer reduced the tensor itself)
        d0 = wides[i]["d0"]
        dw_wide[i] = _wide_bwd(ctx, buf, G, i, need_w, need_dx, (RR[d0], L + 1 - d0), Rc if i > 0 else R0, wgrad_stream)

    starts = [wd["d0"] for wd in wides] + [L]
    for gi in reversed(range(len(wides))):
        d0, d1 = starts[gi], starts[gi + 1]
        if gi + 1 < len(wides):
            wide_bwd(gi + 1, True)       # the later groups are final: their share in this group's slices
        if d1 - d0 >= 2:
            # slices d1 - 2 .. d0, last first, in one library call (otgan_dense16_chain_bwd_f32)
            pf = (ctypes.c_void_p * (d1 - d0 - 1))(*[bw["slice"][c].data_ptr() for c in range(d0, d1 - 1)])
            off0 = 4 * (C0 + d0 * F)
            _lib.check(lib.otgan_dense16_chain_bwd_f32(N, H, W, d1 - d0, gptr + off0, Ctot, bptr + off0, Ctot,
                                                       ctypes.cast(pf, ctypes.c_void_p), Rc.data_ptr(), RS[d0].data_ptr(),
                                                       _lib.stream_ptr()), "dense16_chain_bwd")
        # the gradients of the group's slices are final: the chain weight gradients of its layers
        for c in reversed(range(d0, d1)):
            if need_w and plan["own_len"][c]:
                desc = ctx.descs[c]
                cmap, _inv = ctx.maps[c]
                off = C0 + plan["g0"][c] * F
                # records of the slices the layer read (the rows its forward kernel read) and of its output gradient (the
                # slices' rows from c on and the incoming bound): the kernel runs on the fp16 matrix pipe (round 4)
                R, gbase, gidx = ctx.fwd_recs
                with wgrad_stream():
                    dw_g[c] = torch.empty_like(sw["w_g"][c])
                    conv_wgrad_raw(desc, buf[..., off:], cmap, G, dw_g[c], dy_amax=(RR[c], L + 1 - c),
                                   x_amax=(R[gbase[gidx[plan["g0"][c]]]], 1 + plan["own_len"][c]))
    wide_bwd(0, ctx.needs_input_grad[0])
    if need_w:
        assert ctx.batched and len(wides) <= 2
        with wgrad_stream():
            _block_weight_grads(ctx, saved, grads, dw_g, dw_wide)
            _block_bias_grads(ctx, G, grads)
    return grads


def dense_block_op(x0, segs0, params, ksize=3, preact=1):
    flat = [t for p in params for t in p]
    return DenseBlockFunction.apply(x0, tuple(segs0), int(ksize), int(preact), *flat)


# ------------------------------------------------------------------------------- pointwise
class GluFunction(torch.autograd.Function):
    """x: [..., 2C] -> x[..., :C] * sigmoid(x[..., C:])   (models/dcgan.py:35-36)."""

    @staticmethod
    def forward(ctx, x):
        _need_cuda(x)
        x = x.contiguous()
        C2 = x.shape[-1]
        rows = x.numel() // C2
        pre = take(x, "glu", remove=True)
        if pre is not None:
            # the layer that produced x already wrote the gated product (Conv2dFunction, glu_hint)
            _PENDING_GLU[0] = None
            ctx.save_for_backward(x)
            return pre
        y = torch.empty(x.shape[:-1] + (C2 // 2,), dtype=x.dtype, device=x.device)
        # the library writes a record from its float4 kernel only (C % 4 == 0, 16-byte aligned x and y); a contiguous view at
        # an odd storage offset takes the scalar kernel and y goes on without one: its consumer reduces it (absmax_record)
        rec = amax_slot(x.device) if (C2 // 2) % 4 == 0 and _aligned16(x, y) else None
        _lib.check(_lib.lib().otgan_glu_fwd_amax_f32(x.data_ptr(), rows, C2 // 2, y.data_ptr(), _lib.ptr(rec),
                                                     _lib.stream_ptr()), "glu_fwd")
        if rec is not None:
            tag_amax(y, rec)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        C2 = x.shape[-1]
        dx = torch.empty_like(x)
        if (C2 // 2) % 4 == 0 and _aligned16(x, dy, dx):
            rec = amax_slot(x.device)
            # dx is the output gradient of the convolution in front of the GLU: leave its column sums (that layer's
            # bias gradient) with it instead of reading dx once more there
            cs = torch.empty(C2, dtype=x.dtype, device=x.device)
            scratch = torch.empty(256 * C2, dtype=x.dtype, device=x.device)
            _lib.check(_lib.lib().otgan_glu_bwd_colsum_f32(x.data_ptr(), dy.data_ptr(), x.numel() // C2, C2 // 2,
                                                           dx.data_ptr(), rec.data_ptr(), cs.data_ptr(), scratch.data_ptr(),
                                                           _lib.stream_ptr()), "glu_bwd_colsum")
            leave(dx, "colsum", cs)
            tag_amax(dx, rec)
        else:
            # scalar kernel (C % 4 != 0, or a misaligned contiguous view): dx carries neither; the convolution in front reduces
            # its bias gradient and its record itself
            _lib.check(_lib.lib().otgan_glu_bwd_amax_f32(x.data_ptr(), dy.data_ptr(), x.numel() // C2,
                                                         C2 // 2, dx.data_ptr(), None, _lib.stream_ptr()), "glu_bwd")
        return dx


class TanhFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _need_cuda(x)
        x = x.contiguous()
        y = torch.empty_like(x)
        _lib.check(_lib.lib().otgan_tanh_fwd_f32(x.data_ptr(), x.numel(), y.data_ptr(),
                                                 _lib.stream_ptr()), "tanh_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(y)
        _lib.check(_lib.lib().otgan_tanh_bwd_f32(y.data_ptr(), dy.data_ptr(), y.numel(),
                                                 dx.data_ptr(), _lib.stream_ptr()), "tanh_bwd")
        return dx


class FeatureHeadFunction(torch.autograd.Function):
    """[N,H,W,C] -> [N, H*W*2C]: concat([relu(x), relu(-x)], channel), flatten, L2-normalise
    (models/dcgan.py:16-19, models/densenet.py:37-42; no epsilon)."""

    @staticmethod
    def forward(ctx, x):
        _need_cuda(x)
        x = x.contiguous()
        _trace_signs(x)
        N, H, W, C = x.shape
        f = torch.empty((N, H * W * 2 * C), dtype=x.dtype, device=x.device)
        norm = torch.empty(N, dtype=x.dtype, device=x.device)
        _lib.check(_lib.lib().otgan_feature_head_fwd_f32(x.data_ptr(), N, H * W, C, f.data_ptr(),
                                                         norm.data_ptr(), _lib.stream_ptr()), "head_fwd")
        ctx.save_for_backward(x, f, norm)
        return f

    @staticmethod
    def backward(ctx, df):
        x, f, norm = ctx.saved_tensors
        df = df.contiguous()
        N, H, W, C = x.shape
        dx = torch.empty_like(x)
        rec = amax_slot(x.device) if C % 4 == 0 else None
        _lib.check(_lib.lib().otgan_feature_head_bwd_amax_f32(x.data_ptr(), f.data_ptr(), norm.data_ptr(),
                                                              df.data_ptr(), N, H * W, C, dx.data_ptr(), _lib.ptr(rec),
                                                              _lib.stream_ptr()), "head_bwd")
        if rec is not None:
            tag_amax(dx, rec)
        return dx


class ConcatChannelsFunction(torch.autograd.Function):
    """torch.cat(xs, dim = 3) of NHWC tensors that carries amax records both ways (round 4): the result is tagged with the
    maximum of its elements' records (elements without one -- the 16-channel noise inputs of the DenseNet generator,
    models/densenet.py:60-73 -- are reduced, they are small), and every piece of the gradient with the gradient's own
    record: a bound of a channel subset is all a consumer's power-of-two scale needs.  Without this the dense block
    behind the cat reduced its block input, and the layer in front of it its output gradient, once per step each."""

    @staticmethod
    def forward(ctx, *xs):
        ctx.widths = [int(t.shape[-1]) for t in xs]
        y = torch.cat(xs, 3)
        if all(w % 4 == 0 for w in ctx.widths) and any(amax_of(t) is not None for t in xs):
            recs = [amax_of(t) if amax_of(t) is not None else absmax_record(t.contiguous()) for t in xs]
            rec = recs[0]
            for r in recs[1:]:
                rec = torch.maximum(rec, r)
            tag_amax(y, rec)
        return y

    @staticmethod
    def backward(ctx, dy):
        rec = amax_of(dy)
        outs = []
        for piece in dy.split(ctx.widths, 3):
            piece = piece.contiguous()
            if rec is not None:
                tag_amax(piece, rec)
            outs.append(piece)
        return tuple(outs)


def concat_channels(xs):
    return ConcatChannelsFunction.apply(*xs)


class ExtendChannelsFunction(torch.autograd.Function):
    """[x, *others] concatenated along the channels IN the buffer a convolution with `grow` allocated around x (round 5):
    the other elements (the 16-channel noise inputs of the DenseNet generator, models/densenet.py:60-73) are copied behind
    x, the result is the channel prefix [0, C0) of that buffer -- x itself is not copied, and its gradient is handed back
    as a view of the incoming one.  Records as in ConcatChannelsFunction."""

    @staticmethod
    def forward(ctx, Ctot, x, *others):
        base = grown_buffer(x, Ctot)
        assert base is not None
        ctx.widths = [int(t.shape[-1]) for t in (x,) + others]
        # read before you write (hand-offs): x is a view of `base`, the in-place copies below make what it carries stale
        # (the record was never carried and the block reduced its input again)
        rec = amax_of(x) if all(w % 4 == 0 for w in ctx.widths) else None
        if rec is not None:
            for t in others:
                r = amax_of(t)
                rec = torch.maximum(rec, r if r is not None else absmax_record(t.contiguous()))
        off = ctx.widths[0]
        for t in others:
            base[..., off:off + t.shape[-1]].copy_(t)
            off += t.shape[-1]
        y = base[..., :off]
        if rec is not None:
            tag_amax(y, rec)
        return y

    @staticmethod
    def backward(ctx, dy):
        rec = amax_of(dy)
        outs, off = [], 0
        for i, w in enumerate(ctx.widths):
            piece = dy[..., off:off + w]
            off += w
            if not ctx.needs_input_grad[1 + i]:
                outs.append(None)
                continue
            if i > 0 or channel_prefix_stride(piece) is None:
                piece = piece.contiguous()
            if rec is not None:
                tag_amax(piece, rec)
            outs.append(piece)
        return (None, *outs)


def extend_channels(xs, Ctot):
    """concat_channels(xs) inside the grown buffer of xs[0] when there is one with Ctot channels, else None."""
    if grown_buffer(xs[0], Ctot) is None or any(t.shape[:3] != xs[0].shape[:3] for t in xs[1:]):
        return None
    return ExtendChannelsFunction.apply(int(Ctot), *xs)


glu = GluFunction.apply
tanh = TanhFunction.apply
feature_head = FeatureHeadFunction.apply


# ------------------------------------------------------------------------------- optimiser steps
def adam_step(p, grad, v, mg, lr, mom1, mom2, t, coef=None):
    bump_weights_epoch(p)
    _lib.check(_lib.lib().otgan_adam_step_coef_f32(p.data_ptr(), grad.data_ptr(), _lib.ptr(v), mg.data_ptr(),
                                                   p.numel(), float(lr), float(mom1), float(mom2),
                                                   float(t), _lib.ptr(coef), _lib.stream_ptr()), "adam_step")


ADAM_MAX_SEGMENTS = 32      # otgan_layers.h: OTGAN_ADAM_MAX_SEGMENTS


def adam_coefficients(mom1, mom2, t):
    """(1 - mom1^t, 1 - mom2^t) as the library's Adam entries evaluate them (fp32; host only, no launch)."""
    out = (ctypes.c_float * 2)()
    _lib.lib().otgan_adam_coefficients(float(mom1), float(mom2), float(t), ctypes.cast(out, ctypes.c_void_p))
    return float(out[0]), float(out[1])


def adam_step_gather(p_flat, grads, offsets, v, mg, lr, mom1, mom2, t, ema_shadow=None, ema_decay=0.0, coef=None):
    """Adam on a flat parameter buffer from per-variable gradient tensors (no concatenation); optionally the EMA of the
    updated parameters in the same launch (otgan_adam_step_gather_f32).  coef: a device tensor [2] holding the step's
    bias corrections (adam_coefficients) -- read by the kernel instead of being derived from `t` on the host, so that a
    captured launch can be replayed for later steps (trainer.GraphedSteps)."""
    n = len(grads)
    bump_weights_epoch(p_flat)
    if ema_shadow is not None:
        bump_weights_epoch(ema_shadow)
    gp = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads])
    off = (ctypes.c_long * (n + 1))(*offsets)
    _lib.check(_lib.lib().otgan_adam_step_gather_coef_f32(p_flat.data_ptr(), ctypes.cast(gp, ctypes.c_void_p),
                                                          ctypes.cast(off, ctypes.c_void_p), n, _lib.ptr(v), mg.data_ptr(),
                                                          float(lr), float(mom1), float(mom2), float(t), _lib.ptr(coef),
                                                          _lib.ptr(ema_shadow), float(ema_decay), _lib.stream_ptr()),
               "adam_step_gather")


COPY2D_MAX_SEGMENTS = 64   # include/otgan_layers.h


def copy2d_batched(segs):
    """Strided 2-D copies in one launch (otgan_copy2d_batched_f32): segs = [(src_ptr, dst_ptr, rows, cols, src_ld, dst_ld)],
    element units, at most COPY2D_MAX_SEGMENTS per launch (longer lists take several)."""
    for i0 in range(0, len(segs), COPY2D_MAX_SEGMENTS):
        part = segs[i0:i0 + COPY2D_MAX_SEGMENTS]
        n = len(part)
        src = (ctypes.c_void_p * n)(*[q[0] for q in part])
        dst = (ctypes.c_void_p * n)(*[q[1] for q in part])
        rows = (ctypes.c_int * n)(*[q[2] for q in part])
        cols = (ctypes.c_int * n)(*[q[3] for q in part])
        sld = (ctypes.c_long * n)(*[q[4] for q in part])
        dld = (ctypes.c_long * n)(*[q[5] for q in part])
        cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
        _lib.check(_lib.lib().otgan_copy2d_batched_f32(cast(src), cast(dst), cast(rows), cast(cols), cast(sld), cast(dld), n,
                                                       _lib.stream_ptr()), "copy2d_batched")


GATHER3D_MAX_SEGMENTS = 32   # include/otgan_layers.h


def gather3d_batched(segs, n1, n2, base1=0, map1=None, amax_out=None):
    """Strided 3-D copies with a gathered middle index in one launch (otgan_gather3d_batched_f32): segs = [(src_ptr, dst_ptr, n0,
    src_stride0, src_stride1, dst_stride0, dst_stride1)], element units; map1: int32 device tensor of n1 indices or None."""
    assert map1 is None or (map1.dtype == torch.int32 and map1.numel() == n1 and map1.is_contiguous())
    assert amax_out is None or len(segs) <= GATHER3D_MAX_SEGMENTS
    for i0 in range(0, len(segs), GATHER3D_MAX_SEGMENTS):
        part = segs[i0:i0 + GATHER3D_MAX_SEGMENTS]
        n = len(part)
        cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
        arr = lambda ty, i: cast((ty * n)(*[q[i] for q in part]))
        _lib.check(_lib.lib().otgan_gather3d_batched_f32(arr(ctypes.c_void_p, 0), arr(ctypes.c_void_p, 1), arr(ctypes.c_int, 2),
                                                         int(n1), int(n2), arr(ctypes.c_long, 3), arr(ctypes.c_long, 4),
                                                         arr(ctypes.c_long, 5), arr(ctypes.c_long, 6), int(base1),
                                                         _lib.ptr(map1), _lib.ptr(amax_out), n, _lib.stream_ptr()),
                   "gather3d_batched")


def adamax_step(p, grad, v, mg, lr, mom1, mom2):
    bump_weights_epoch(p)
    _lib.check(_lib.lib().otgan_adamax_step_f32(p.data_ptr(), grad.data_ptr(), _lib.ptr(v),
                                                mg.data_ptr(), p.numel(), float(lr), float(mom1),
                                                float(mom2), _lib.stream_ptr()), "adamax_step")


def nesterov_step(p, grad, v, lr, mom1):
    bump_weights_epoch(p)
    _lib.check(_lib.lib().otgan_nesterov_step_f32(p.data_ptr(), grad.data_ptr(), v.data_ptr(),
                                                  p.numel(), float(lr), float(mom1),
                                                  _lib.stream_ptr()), "nesterov_step")


def ema_update(shadow, p, decay):
    bump_weights_epoch(shadow)
    _lib.check(_lib.lib().otgan_ema_update_f32(shadow.data_ptr(), p.data_ptr(), p.numel(),
                                               float(decay), _lib.stream_ptr()), "ema_update")


BATCH_U8_MAX_SHARDS = 32   # include/otgan_layers.h


def batch_from_u8(store, offsets, B, S, lut, perm=None, flip=None, out=None):
    """The step's float32 batch from a device-resident uint8 store in one launch (otgan_batch_from_u8_f32): store uint8
    [n, SH, SW, 3]; row s * B + k of the result is image perm[offsets[s] + k] (offsets[s] + k without a permutation), flipped
    horizontally where flip[s * B + k] (bool / uint8, optional), through the 256-entry table `lut` (SH == S) or box-downsampled by
    SH / S in {2, 4}.  `out`: a float32 [len(offsets) * B, S, S, 3] tensor whose images are contiguous and whose row stride is the
    pitch (a row slice of a wider buffer); allocated when None.  Geometry errors come back as OtganError from the library."""
    if not (store.is_cuda and store.dtype == torch.uint8 and store.dim() == 4 and store.shape[3] == 3 and store.is_contiguous()):
        raise _lib.OtganError("batch_from_u8 takes a contiguous CUDA (MI355X) uint8 [n, H, W, 3] store; there is no CPU fallback")
    rows = len(offsets) * int(B)
    if out is None:
        out = torch.empty(rows, S, S, 3, dtype=torch.float32, device=store.device)
    if not (out.dtype == torch.float32 and out.shape == (rows, S, S, 3) and out[:1].is_contiguous() and out.device == store.device):
        raise _lib.OtganError("batch_from_u8: out must be float32 [%d, %d, %d, 3] on %s with contiguous images, found %s %s on %s"
                              % (rows, S, S, store.device, out.dtype, tuple(out.shape), out.device))
    if perm is not None and not (perm.dtype == torch.int32 and perm.dim() == 1 and perm.is_contiguous()
                                 and perm.device == store.device):
        raise _lib.OtganError("batch_from_u8: perm must be a contiguous 1-D int32 tensor on %s, found %s %s on %s"
                              % (store.device, perm.dtype, tuple(perm.shape), perm.device))
    if flip is not None:
        if flip.dtype == torch.bool and flip.is_contiguous():
            flip = flip.view(torch.uint8)      # a bool tensor stores one byte 0 / 1 per element
        if not (flip.dtype == torch.uint8 and flip.numel() == rows and flip.is_contiguous() and flip.device == store.device):
            raise _lib.OtganError("batch_from_u8: flip must be %d contiguous bool / uint8 values on %s, found %s %s on %s"
                                  % (rows, store.device, flip.dtype, tuple(flip.shape), flip.device))
    if not (lut.dtype == torch.float32 and lut.numel() == 256 and lut.is_contiguous() and lut.device == store.device):
        raise _lib.OtganError("batch_from_u8: lut must be 256 contiguous float32 values on %s, found %s %s on %s"
                              % (store.device, lut.dtype, tuple(lut.shape), lut.device))
    off = (ctypes.c_long * len(offsets))(*[int(o) for o in offsets])
    with torch.cuda.device(store.device):
        _lib.check(_lib.lib().otgan_batch_from_u8_f32(store.data_ptr(), store.shape[0], store.shape[1], store.shape[2],
                                                      _lib.ptr(perm), perm.numel() if perm is not None else 0,
                                                      ctypes.cast(off, ctypes.c_void_p), len(offsets), int(B), _lib.ptr(flip),
                                                      lut.data_ptr(), int(S), out.data_ptr(), out.stride(0) if rows > 1 else 3 * S * S,
                                                      _lib.stream_ptr()), "batch_from_u8")
    return out


AUG_COLOR, AUG_TRANSLATION, AUG_CUTOUT = 1, 2, 4      # include/otgan_layers.h: OTGAN_AUG_*


def _augment_launch(fn, name, src, u, policy):
    """One launch of otgan_augment_{fwd,bwd}_f32 on the current stream: src [rows, S, S, 3] fp32 -> a new tensor of its shape."""
    _need_cuda(src, u)
    src = src.contiguous()
    if not (src.dtype == torch.float32 and src.dim() == 4 and src.shape[1] == src.shape[2] and src.shape[3] == 3):
        raise _lib.OtganError("%s takes float32 [rows, S, S, 3] images, found %s %s" % (name, src.dtype, tuple(src.shape)))
    rows, S = src.shape[0], src.shape[1]
    if not (u.dtype == torch.float32 and tuple(u.shape) == (rows, 8) and u.is_contiguous() and u.device == src.device):
        raise _lib.OtganError("%s: u must be contiguous float32 [%d, 8] on %s, found %s %s on %s"
                              % (name, rows, src.device, u.dtype, tuple(u.shape), u.device))
    out = torch.empty_like(src)
    with torch.cuda.device(src.device):
        _lib.check(fn(src.data_ptr(), rows, S, u.data_ptr(), int(policy), out.data_ptr(), _lib.stream_ptr()), name)
    return out


class AugmentFunction(torch.autograd.Function):
    """y = T(x): colour / translation / cutout per image from its row of uniforms `u` (otgan_augment_fwd_f32; the formulas are
    in include/otgan_layers.h), dx = T^T dy (otgan_augment_bwd_f32).  T is affine in x, so the backward pass needs u and the
    policy only.  The output carries no amax record: its consumer reduces it, as it does the data batch."""

    @staticmethod
    def forward(ctx, x, u, policy):
        ctx.policy = int(policy)
        ctx.save_for_backward(u)
        return _augment_launch(_lib.lib().otgan_augment_fwd_f32, "augment_fwd", x, u, policy)

    @staticmethod
    def backward(ctx, dy):
        (u,) = ctx.saved_tensors
        return augment_transpose(dy, u, ctx.policy), None, None


def augment(x, u, policy):
    """T(x) for a batch x [rows, S, S, 3] in fp32, u [rows, 8] uniforms in [0, 1), policy a mask of AUG_COLOR | AUG_TRANSLATION
    | AUG_CUTOUT (utils/augment.parse_policy).  One launch; the backward launch exists only where x needs a gradient (autograd
    builds no node otherwise: the critic step never runs it)."""
    return AugmentFunction.apply(x, u, policy)


def augment_transpose(dy, u, policy):
    """T^T dy: the backward launch of `augment` on its own (no autograd)."""
    return _augment_launch(_lib.lib().otgan_augment_bwd_f32, "augment_bwd", dy, u, policy)


SWD_DESC = 147             # 7 x 7 x 3 values of a patch descriptor (include/otgan_layers.h)


def swd_levels(S):
    """Pyramid levels of S x S images, log2(S / 16) + 1; a ValueError for any S but 16, 32 and 64."""
    L = _lib.lib().otgan_swd_levels(int(S))
    if L == 0:
        raise ValueError("the sliced Wasserstein pyramid is defined for images of 16, 32 and 64 pixels a side, not %d" % S)
    return L


def _swd_images(img, name):
    if not (torch.is_tensor(img) and img.is_cuda):
        raise _lib.OtganError("%s takes CUDA (MI355X) tensors; there is no CPU fallback" % name)
    if not (img.dtype == torch.uint8 and img.dim() == 4 and img.shape[1] == img.shape[2] and img.shape[3] == 3):
        raise ValueError("%s takes uint8 [n, S, S, 3] images, found %s %s" % (name, img.dtype, tuple(img.shape)))
    L = swd_levels(img.shape[1])
    return img.contiguous(), img.shape[0], img.shape[1], L


def _swd_positions(pos, L, n, name, device):
    if not (torch.is_tensor(pos) and pos.is_cuda and pos.device == device):
        raise _lib.OtganError("%s takes its positions as a CUDA (MI355X) tensor on %s; there is no CPU fallback" % (name, device))
    if not (pos.dtype == torch.int32 and pos.dim() == 4 and tuple(pos.shape[:2]) == (L, n) and pos.shape[2] >= 1
            and pos.shape[3] == 2):
        raise ValueError("%s: positions must be int32 [%d, %d, P, 2], found %s %s" % (name, L, n, pos.dtype, tuple(pos.shape)))
    return pos.contiguous(), pos.shape[2]


def swd_pyramid(img, level):
    """Level `level` of the Laplacian pyramid of uint8 images [n, S, S, 3] -> fp32 [n, S_l, S_l, 3] (otgan_swd_pyramid_u8)."""
    img, n, S, L = _swd_images(img, "swd_pyramid")
    if not 0 <= level < L:
        raise ValueError("swd_pyramid: level %d of %d" % (level, L))
    out = torch.empty(n, S >> level, S >> level, 3, dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        _lib.check(_lib.lib().otgan_swd_pyramid_u8(img.data_ptr(), n, S, int(level), out.data_ptr(), _lib.stream_ptr()), "swd_pyramid")
    return out


def swd_channel_stats(img, pos):
    """(mean, inv_std), fp32 [L, 3] each: the per-level, per-channel statistics of the patch descriptors of uint8 images
    [n, S, S, 3] at positions int32 [L, n, P, 2] (otgan_swd_channel_stats_u8).  No host synchronisation."""
    img, n, S, L = _swd_images(img, "swd_channel_stats")
    if n == 0:
        raise ValueError("swd_channel_stats: statistics of no image")
    pos, P = _swd_positions(pos, L, n, "swd_channel_stats", img.device)
    mean = torch.empty(L, 3, dtype=torch.float32, device=img.device)
    inv_std = torch.empty(L, 3, dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        nbytes = _lib.lib().otgan_swd_workspace_bytes(n, S, P)
        ws = workspace(nbytes, img.device)
        _lib.check(_lib.lib().otgan_swd_channel_stats_u8(img.data_ptr(), n, S, pos.data_ptr(), P, mean.data_ptr(), inv_std.data_ptr(),
                                                         ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "swd_channel_stats")
    return mean, inv_std


def swd_project(img, pos, level, mean, inv_std, dirs, out=None, col0=0):
    """Projections of the normalised patch descriptors of level `level` on `dirs` fp32 [nd, 147] (otgan_swd_project_u8):
    out[j, col0 + i P + p], out fp32 [nd, ld] with ld >= col0 + n P (allocated [nd, n P] when None).  Columns outside
    [col0, col0 + n P) are not touched."""
    img, n, S, L = _swd_images(img, "swd_project")
    pos, P = _swd_positions(pos, L, n, "swd_project", img.device)
    if not 0 <= level < L:
        raise ValueError("swd_project: level %d of %d" % (level, L))
    _need_cuda(mean, inv_std, dirs, out)
    for t, name in ((mean, "mean"), (inv_std, "inv_std")):
        if not (t.dtype == torch.float32 and tuple(t.shape) == (L, 3) and t.is_contiguous() and t.device == img.device):
            raise ValueError("swd_project: %s must be contiguous float32 [%d, 3] on %s, found %s %s" % (name, L, img.device, t.dtype, tuple(t.shape)))
    if not (dirs.dtype == torch.float32 and dirs.dim() == 2 and dirs.shape[1] == SWD_DESC and dirs.is_contiguous()
            and dirs.device == img.device):
        raise ValueError("swd_project: dirs must be contiguous float32 [nd, %d] on %s, found %s %s" % (SWD_DESC, img.device, dirs.dtype, tuple(dirs.shape)))
    nd = dirs.shape[0]
    if out is None:
        out = torch.empty(nd, col0 + n * P, dtype=torch.float32, device=img.device)
    if not (out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == nd and out.shape[1] >= col0 + n * P and col0 >= 0
            and out.device == img.device and (out.stride(1) == 1 or out.shape[1] == 1) and (nd <= 1 or out.stride(0) >= out.shape[1])):
        raise ValueError("swd_project: out must be float32 [%d, >= %d] on %s with unit column stride, found %s %s"
                         % (nd, col0 + n * P, img.device, out.dtype, tuple(out.shape)))
    ldp = out.stride(0) if nd > 1 else out.shape[1]
    with torch.cuda.device(img.device):
        _lib.check(_lib.lib().otgan_swd_project_u8(img.data_ptr(), n, S, pos.data_ptr(), P, int(level), mean.data_ptr(),
                                                   inv_std.data_ptr(), dirs.data_ptr(), nd, out.data_ptr() + 4 * int(col0),
                                                   ldp, _lib.stream_ptr()), "swd_project")
    return out


def swd_row_l1(a, b):
    """fp64 [rows]: mean over the columns of |a - b| for fp32 [rows, m] a, b with unit column stride (otgan_swd_row_l1_f64)."""
    _need_cuda(a, b)
    if not (torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == torch.float32 and b.dtype == torch.float32 and a.dim() == 2
            and a.shape == b.shape and a.shape[1] >= 1 and a.device == b.device):
        raise ValueError("swd_row_l1 takes two float32 [rows, m] tensors of one shape and device")
    if a.stride(1) != 1 or a.stride(0) < a.shape[1]:
        a = a.contiguous()
    if b.stride(1) != 1 or b.stride(0) < b.shape[1]:
        b = b.contiguous()
    out = torch.empty(a.shape[0], dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().otgan_swd_row_l1_f64(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), a.shape[0], a.shape[1],
                                                   out.data_ptr(), _lib.stream_ptr()), "swd_row_l1")
    return out


NN_U8_MAX_K, NN_U8_MAX_D = 8, 49152


def _nn_u8_rows(x, name):
    """x as otgan_nn_u8 reads it: uint8 CUDA [n, D] (or [n, S, S, 3], flattened) in 16-byte pieces of a row; a column slice
    of a wider buffer passes its row stride on, anything that cannot be read that way is copied."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.OtganError("nn_u8 takes CUDA (MI355X) uint8 tensors; there is no CPU fallback")
    if x.dtype != torch.uint8 or x.dim() not in (2, 4) or (x.dim() == 4 and (x.shape[1] != x.shape[2] or x.shape[3] != 3)):
        raise ValueError("nn_u8: %s must be uint8 [n, D] or [n, S, S, 3], found %s %s" % (name, x.dtype, tuple(x.shape)))
    if x.dim() == 4:
        x = x.contiguous().view(x.shape[0], -1)
    D = x.shape[1]
    if D % 16 or not 16 <= D <= NN_U8_MAX_D:
        raise ValueError("nn_u8: %s has rows of %d values; a multiple of 16 in 16 ... %d" % (name, D, NN_U8_MAX_D))
    if x.stride(1) != 1 or x.stride(0) < D or x.stride(0) % 16 or x.data_ptr() % 16:
        x = x.contiguous()
    return x


def nn_u8(q, y, k, self0=-1):
    """(index int32 [nq, k], dist int64 [nq, k]): per row of q the rows of y with the k smallest squared Euclidean distances
    over the raw uint8 values, by distance ascending, equal distances by the smaller row first; (-1, -1) where fewer were
    counted.  Row self0 + i of y is skipped for row i of q (self0 = -1: none).  Exact integers from the int8 matrix pipe
    (otgan_nn_u8); q, y: uint8 CUDA [n, D] or [n, S, S, 3]."""
    q, y = _nn_u8_rows(q, "q"), _nn_u8_rows(y, "y")
    if q.shape[1] != y.shape[1] or q.device != y.device:
        raise ValueError("nn_u8: q %s and y %s must have the same row length and device" % (tuple(q.shape), tuple(y.shape)))
    k, self0 = int(k), int(self0)
    if not 1 <= k <= NN_U8_MAX_K:
        raise ValueError("nn_u8: %d neighbours: between 1 and %d" % (k, NN_U8_MAX_K))
    if self0 < -1:
        raise ValueError("nn_u8: self0 %d >= -1" % self0)
    nq, ny, D = q.shape[0], y.shape[0], q.shape[1]
    index = torch.empty(nq, k, dtype=torch.int32, device=q.device)
    dist = torch.empty(nq, k, dtype=torch.int64, device=q.device)
    if nq == 0:
        return index, dist
    L = _lib.lib()
    with torch.cuda.device(q.device):
        nbytes = L.otgan_nn_u8_workspace_bytes(nq, ny, k)
        ws = workspace(nbytes, q.device)
        _lib.check(L.otgan_nn_u8(nq, ny, D, q.data_ptr(), q.stride(0) if nq > 1 else D, y.data_ptr() if ny else None,
                                 y.stride(0) if ny > 1 else D, k, self0, index.data_ptr(), dist.data_ptr(), ws.data_ptr(),
                                 ws.numel(), _lib.stream_ptr()), "nn_u8")
    return index, dist


HEALTH_CHUNK, HEALTH_MAX_SEGMENTS = 2048, 64      # otgan_layers.h: OTGAN_HEALTH_CHUNK, OTGAN_HEALTH_MAX_SEGMENTS


def tensor_health(tensors, refs=None):
    """(out float64 [nseg, 6], hist int64 [nseg, 256]) of a list of float32 CUDA tensors, one segment each
    (otgan_tensor_health_f32): per segment sum x^2, max |x|, sum (x - ref)^2, max |x - ref|, the count of exact zeros and the
    count of non-finite elements, and one count per finite non-zero element in the bucket of its biased fp32 exponent.  `refs`:
    None, or a list as long as `tensors` of tensors of the same sizes, entries may be None (slots 2 and 3 are then 0).  The
    results of a segment do not depend on the other segments, on alignment or on the call.  No host synchronisation."""
    tensors = list(tensors)
    refs = None if refs is None else list(refs)
    if refs is not None and len(refs) != len(tensors):
        raise ValueError("tensor_health: %d tensors and %d refs" % (len(tensors), len(refs)))
    _need_cuda(*tensors)
    if refs is not None:
        _need_cuda(*refs)
    if not tensors:
        raise ValueError("tensor_health: no tensor (the device of the result is the tensors')")
    dev = tensors[0].device
    xs, rs = [], []
    for i, t in enumerate(tensors):
        r = None if refs is None else refs[i]
        for u, what in ((t, "tensor"), (r, "ref")):
            if u is not None and not (torch.is_tensor(u) and u.dtype == torch.float32 and u.device == dev):
                raise ValueError("tensor_health: %s %d must be a float32 tensor on %s" % (what, i, dev))
        if r is not None and r.numel() != t.numel():
            raise ValueError("tensor_health: tensor %d has %d elements, its ref %d" % (i, t.numel(), r.numel()))
        xs.append(t.detach().contiguous())
        rs.append(None if r is None else r.detach().contiguous())
    nseg = len(xs)
    out = torch.empty(nseg, 6, dtype=torch.float64, device=dev)
    hist = torch.empty(nseg, 256, dtype=torch.int64, device=dev)
    arr = ctypes.c_void_p * nseg
    X = arr(*[x.data_ptr() if x.numel() else None for x in xs])
    R = None if refs is None else arr(*[r.data_ptr() if r is not None and r.numel() else None for r in rs])
    n = (ctypes.c_long * nseg)(*[x.numel() for x in xs])
    L = _lib.lib()
    with torch.cuda.device(dev):
        nbytes = L.otgan_tensor_health_workspace_bytes(ctypes.cast(n, ctypes.c_void_p), nseg)
        ws = workspace(nbytes, dev)
        _lib.check(L.otgan_tensor_health_f32(ctypes.cast(X, ctypes.c_void_p), None if R is None else ctypes.cast(R, ctypes.c_void_p),
                                             ctypes.cast(n, ctypes.c_void_p), nseg, out.data_ptr(), hist.data_ptr(), ws.data_ptr(),
                                             ws.numel(), _lib.stream_ptr()), "tensor_health")
    return out, hist


def plan_marginals(plan):
    """float64 [P, 4]: max_i |r_i - 1|, mean_i |r_i - 1|, max_j |c_j - n/m|, mean_j |c_j - n/m| of the row sums r and column
    sums c of float32 CUDA plans [P, n, m] (or [n, m]) with unit column stride; a row pitch above m is passed on
    (otgan_plan_marginals_f32).  No host synchronisation."""
    _need_cuda(plan)
    if not (torch.is_tensor(plan) and plan.dtype == torch.float32 and plan.dim() in (2, 3)):
        raise ValueError("plan_marginals takes float32 plans [P, n, m] or [n, m]")
    if plan.dim() == 2:
        plan = plan.unsqueeze(0)
    P, n, m = plan.shape
    if n < 1 or m < 1:
        raise ValueError("plan_marginals: empty plans %s" % (tuple(plan.shape),))
    ldp = plan.stride(1) if n > 1 else m
    if not ((m == 1 or plan.stride(2) == 1) and ldp >= m and (P == 1 or plan.stride(0) == n * ldp)):
        plan = plan.contiguous()
        ldp = m
    out = torch.empty(P, 4, dtype=torch.float64, device=plan.device)
    if P == 0:
        return out
    L = _lib.lib()
    with torch.cuda.device(plan.device):
        nbytes = L.otgan_plan_marginals_workspace_bytes(P, n, m)
        ws = workspace(nbytes, plan.device)
        _lib.check(L.otgan_plan_marginals_f32(plan.data_ptr(), P, n, m, ldp, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _lib.stream_ptr()), "plan_marginals")
    return out
