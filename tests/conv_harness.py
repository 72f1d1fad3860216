"""The buffers and the calls of the convolution route tests (tests/test_conv_routes_gpu.py, tests/test_conv_sparse_gpu.py): every
operand in one flat allocation with guard floats around it (Pitched, Flat), a workspace between guard bytes (Workspace), and
the three passes of one table case of tests/conv_routes.py through the C ABI (Call).  Importing needs neither a GPU nor the
library; making a Call does."""
import ctypes

import pytest
import torch

import conv_routes as R

SENT = 0x7FC0BEEF        # a NaN bit pattern no kernel produces


class Pitched:
    """GUARD floats, `off` floats, [rows, pitch] floats, GUARD floats in one allocation; the call gets the row block.  `fill`:
    a finite value for inputs (a kernel may read inside the buffer and mask), None = the sentinel for outputs."""

    def __init__(self, rows, width, pitch, first, off, dev, fill=None):
        self.rows, self.width, self.pitch, self.first, self.off = rows, width, pitch, first, off
        n = 2 * R.GUARD + off + rows * pitch
        if fill is None:
            self.buf = torch.full((n,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
        else:
            self.buf = torch.full((n,), fill, dtype=torch.float32, device=dev)
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + 4 * (R.GUARD + off)

    def valid(self, t=None):
        t = self.buf if t is None else t
        a = R.GUARD + self.off
        return t[a:a + self.rows * self.pitch].view(self.rows, self.pitch)[:, self.first:self.first + self.width]

    def put(self, x):
        self.valid().copy_(x.reshape(self.rows, self.width))
        return self

    def bits(self):
        return self.buf.view(torch.int32).clone()

    def check_outside(self, before, what):
        """everything but the valid block is what it was before the call, bit for bit"""
        now, was = self.bits(), before.clone()
        mask = torch.ones_like(now, dtype=torch.bool)
        self.valid(mask).fill_(False)
        bad = int((now[mask] != was[mask]).sum())
        assert bad == 0, "%s: %d floats outside the valid block were written (guards / pad channels / offset)" % (what, bad)

    def check_written(self, what):
        v = self.valid().contiguous().view(torch.int32)
        assert not bool((v == SENT).any()), what + ": an element of the valid block was not written"


class Flat(Pitched):
    def __init__(self, n, off, dev, fill=None):
        super().__init__(1, n, n, 0, off, dev, fill)


class Workspace:
    """256 guard bytes, `off` floats, the workspace, 512 tail bytes, all 0xA5"""

    def __init__(self, case, need, dev):
        self.mode, self.need = case["ws"], need
        self.bytes = {"full": need, "short": max(need - 1, 0), "null": 0}[case["ws"]]
        self.off = 4 * case["off"]["ws"]
        self.buf = torch.full((256 + self.off + need + 512,), 0xA5, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = None if case["ws"] == "null" else self.buf.data_ptr() + 256 + self.off

    def check(self, what, untouched=False):
        a = 256 + self.off
        used = 0 if (untouched or self.ptr is None) else self.bytes
        assert bool((self.buf[:a] == 0xA5).all()) and bool((self.buf[a + used:] == 0xA5).all()), what + ": wrote outside its workspace"


def _cdesc(fields, **extra):
    from otgan_amd import _lib_layers
    d = _lib_layers.ConvDesc()
    for k, v in dict(fields, **extra).items():
        setattr(d, k, v)
    return d


def _maps(case, dev):
    """(cmap, inv) int32 device tensors or (None, None): the per-element interleave [x0, -x0, x1, -x1, ...] of a list input
    (include/otgan_layers.h "Channel maps"), or the default ordering written out"""
    if not R.has_cmap(case):
        return None, None
    C, neg = sum(case["segs"]), 1 << 31
    segs = case["segs"] if R.doubled(case["pre"]) else (C,)
    cmap, invp, invn, off = [], [0] * C, [0] * C, 0
    for s in segs:
        base = len(cmap)
        cmap += [off + i for i in range(s)]
        if R.doubled(case["pre"]):
            cmap += [(off + i) | neg for i in range(s)]
        for i in range(s):
            invp[off + i], invn[off + i] = base + i, base + s + i
        off += s
    to32 = lambda v: torch.tensor([c - (1 << 32) if c >= neg else c for c in v], dtype=torch.int32, device=dev)
    return to32(cmap), to32(invp + invn)


class Call:
    """the buffers of one case and the three passes on them; `inp`: the input dict (default: conv_routes.inputs(case))"""

    def __init__(self, case, dev, inp=None):
        from otgan_amd import _lib
        self.case, self.dev, self.L = case, dev, _lib.lib()
        self.stream = _lib.stream_ptr()
        self.check = _lib.check
        self.fields = R.desc_fields(case)
        self.geo = R.make_geo(self.fields)
        self.desc = _cdesc(self.fields)
        L, d, g = self.L, self.fields, self.geo
        inp = self.inp = R.inputs(case) if inp is None else inp
        sh, off = R.shapes(case), case["off"]
        self.x = Pitched(*sh["x"], off["x"], dev, fill=7.0).put(inp["x"].to(dev))
        self.dy = Pitched(*sh["dy"], off["dy"], dev, fill=-3.0).put(inp["dy"].to(dev))
        self.bias = Flat(sh["bias"], off["bias"], dev, fill=5.0).put(inp["bias"].to(dev)) if case["bias"] else None
        self.cmap, self.inv = _maps(case, dev)
        # the weights as each pass takes them: wT [Cout][K] / w [K][Cout], or the folded weffT / weff of a folded layer
        w = inp["w"].to(dev).reshape(-1, d["Cout"]).contiguous()
        wT = w.t().contiguous()
        self.plain = dict(w=w, wT=wT)
        nfold = int(L.otgan_conv2d_folded_weight_elems(ctypes.byref(self.desc)))
        assert (nfold > 0) == g["fold"] and nfold == R.folded_weight_elems(d, g)
        fw, bw = wT, w
        if nfold:
            weff, weffT = torch.empty(nfold, device=dev), torch.empty(nfold, device=dev)
            self.check(L.otgan_conv2d_fold_weights_f32(ctypes.byref(self.desc), w.data_ptr(), weff.data_ptr(), weffT.data_ptr(), self.stream),
                       "fold weights")
            fw, bw = weffT, weff
            self.plain.update(weff=weff, weffT=weffT)
        self.w_fwd = Flat(fw.numel(), off["w"], dev, fill=9.0).put(fw)
        self.w_dg = Flat(bw.numel(), off["w"], dev, fill=9.0).put(bw)
        self.operand = None
        if case["x_operand"]:
            nb = int(L.otgan_conv2d_operand_bytes(ctypes.byref(self.desc)))
            self.operand = torch.zeros(max(nb, 256), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def filters(self, which):
        """the prepared filters of pass `which` (0 forward, 1 input gradient) as the case asks, or None"""
        mode = self.case["filters"]
        if mode is None:
            return None
        idx = which + (2 if mode == "unfolded" else 0)
        nb = int(self.L.otgan_conv2d_filter_bytes(ctypes.byref(self.desc), idx)) if mode != "dummy" else 0
        if nb == 0:
            return torch.zeros(256, dtype=torch.uint8, device=self.dev)      # ignored by the passes that have no such filters
        src = {0: self.plain.get("weffT", self.plain["wT"]), 1: self.plain.get("weff", self.plain["w"]), 2: self.plain["wT"],
               3: self.plain["w"]}[idx]
        buf = torch.zeros(nb, dtype=torch.uint8, device=self.dev)
        self.check(self.L.otgan_conv2d_prepare_filters_f32(ctypes.byref(self.desc), idx, src.data_ptr(), buf.data_ptr(), nb, self.stream),
                   "prepare filters")
        return buf

    def run(self, which, **desc_extra):
        """one pass -> (return code, error text, result tensor or None, FLOP reported, launches); `desc_extra`: further
        fields of the descriptor (amax records)"""
        case, L, dev = self.case, self.L, self.dev
        d, sh, off = self.fields, R.shapes(case), case["off"]
        inp = self.inp
        what = "%s %s" % (case["name"], ("fwd", "dgrad", "wgrad")[which])
        desc = _cdesc(self.fields, x_operand=self.operand.data_ptr() if self.operand is not None else None, **desc_extra)
        need = int(L.otgan_conv2d_workspace_bytes(ctypes.byref(desc), which))
        ws = Workspace(case, need, dev)
        filt = self.filters(which) if which < 2 else None
        if which == 0:
            out = Pitched(*sh["y"], off["y"], dev)
            if case["y_acc"]:
                out.put(inp["y0"].to(dev))
        elif which == 1:
            out = Pitched(*sh["dx"], off["dx"], dev)
            if case["acc"]:
                out.put(inp["dx0"].to(dev))
        else:
            out = Flat(sh["w"], off["dw"], dev)
        ins = [b for b in (self.x, self.dy, self.bias, self.w_fwd, self.w_dg) if b is not None]
        before_in, before_out = [b.bits() for b in ins], out.bits()
        torch.cuda.synchronize()
        L.otgan_prof_enable(1)
        try:
            L.otgan_prof_reset()
            if which == 0:
                rc = L.otgan_conv2d_fwd_pf_f32(ctypes.byref(desc), self.x.ptr, None if self.cmap is None else self.cmap.data_ptr(),
                                               self.w_fwd.ptr, None if filt is None else filt.data_ptr(),
                                               None if self.bias is None else self.bias.ptr, out.ptr, ws.ptr, ws.bytes, self.stream)
            elif which == 1:
                rc = L.otgan_conv2d_dgrad_pf_f32(ctypes.byref(desc), self.dy.ptr, self.w_dg.ptr, None if filt is None else filt.data_ptr(),
                                                 self.x.ptr, None if self.inv is None else self.inv.data_ptr(), out.ptr, R.lddx(case),
                                                 case["acc"], ws.ptr, ws.bytes, self.stream)
            else:
                rc = L.otgan_conv2d_wgrad_f32(ctypes.byref(desc), self.x.ptr, None if self.cmap is None else self.cmap.data_ptr(), self.dy.ptr,
                                              out.ptr, ws.ptr, ws.bytes, self.stream)
            text = L.otgan_last_error().decode() if rc else ""
            try:
                torch.cuda.synchronize()
            except RuntimeError as e:      # a device fault: nothing more is started on this GPU
                pytest.exit("%s: %s" % (what, e), returncode=3)
            prof = (ctypes.c_double * 4)()
            L.otgan_prof_collect(which, prof)
        finally:
            L.otgan_prof_enable(0)
        # inputs, guards, pads and the workspace's surroundings: bit for bit what they were
        for b, was in zip(ins, before_in):
            assert torch.equal(b.bits(), was), what + ": an input buffer was written"
        ws.check(what, untouched=rc != 0)
        if rc != 0:
            assert torch.equal(out.bits(), before_out), what + ": a refused call wrote to its output"
            return rc, text, None, prof[2], prof[0]
        out.check_outside(before_out, what)
        out.check_written(what)
        return rc, text, out.valid().clone(), prof[2], prof[0]
