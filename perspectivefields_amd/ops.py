"""Kernel-level entry points of libpf_hip.so (pf_op_* in include/pf_hip.h) for parity tests
and tuning.  Activations are NHWC float32 torch tensors on a GPU; weights are passed in the
reference's (PyTorch) layouts and packed by the library."""
from __future__ import annotations

import contextlib
import ctypes
import threading

import numpy as np

from .engine import PfError, _check, _stream_ptr, load_library


def _np(a):
    if a is None:
        return None
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _dp(t):
    return t.data_ptr() if t is not None else None


@contextlib.contextmanager
def saturation_watch(limit=65504.0):
    """Switches the saturation watch of the kernel-level entry points on for this thread (pf_op_set_saturation_watch): yields a zeroed uint32 device counter
    (a one-element int32 tensor on the current device) that every pf_op_* launch inside the block adds to when an output leaves `limit`; always off again afterwards."""
    import torch

    lib = load_library()
    counter = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))
    _check(lib.pf_op_set_saturation_watch(counter.data_ptr(), float(limit)), None, "pf_op_set_saturation_watch")
    try:
        yield counter
    finally:
        lib.pf_op_set_saturation_watch(None, 0.0)


# ---- checked outputs: every tensor a pf_op_* launch writes is allocated by _out(); inside checked_outputs() it is poisoned and guard-banded
GUARD_BYTES = 256 * 1024      # on each side of an output: four full 64 KB output tiles (256 x 64 or 128 x 128 fp32, the largest of the tile table); a multiple of 512, so the
                              # output keeps the alignment torch gives the backing buffer
POISON_BYTE = 0xFF            # 0xFFFFFFFF, 0xFFFF: a NaN in fp32, fp16 and bf16 -- an element no kernel wrote fails every comparison downstream
HOLD_LIMIT_BYTES = 1 << 30    # backing buffers a manager keeps before it verifies and releases them early
_checked = threading.local()


def guard_pattern(device):
    """The GUARD_BYTES bytes every guard band holds: byte i = (131 i + 7) mod 256.  Not a constant, so a kernel that stores zeros, the poison or any one value into a
    guard changes it."""
    import torch

    return ((torch.arange(GUARD_BYTES, dtype=torch.int64) * 131 + 7) & 0xFF).to(torch.uint8).to(device)


class _Guarded:
    """one output of _out() under checked_outputs(): `backing` = front guard | `nbytes` output bytes | back guard, all uint8"""

    def __init__(self, label, backing, nbytes):
        self.label, self.backing, self.nbytes = label, backing, nbytes

    def guards(self):
        """(2, GUARD_BYTES) view: row 0 the front guard, row 1 the back guard"""
        return self.backing.as_strided((2, GUARD_BYTES), (GUARD_BYTES + self.nbytes, 1))

    def body(self):
        return self.backing[GUARD_BYTES:GUARD_BYTES + self.nbytes]


class CheckedOutputs:
    """What checked_outputs() yields.  `buffers`: the outputs allocated so far and not yet verified (a _Guarded each, in order)."""

    def __init__(self):
        self.buffers = []
        self.held_bytes = 0
        self.outputs = 0          # allocated since the block was entered
        self._patterns = {}

    def _pattern(self, device):
        if device not in self._patterns:
            self._patterns[device] = guard_pattern(device)
        return self._patterns[device]

    def allocate(self, shape, dtype, device, label, fill, poison):
        import torch

        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(v) for v in shape)
        nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
        if self.held_bytes + nbytes + 2 * GUARD_BYTES > HOLD_LIMIT_BYTES and self.buffers:
            self.verify()         # releases what was held: from here on the allocator may hand those blocks out again (poisoned afresh, guards rewritten)
        g = _Guarded(label, torch.empty(nbytes + 2 * GUARD_BYTES, dtype=torch.uint8, device=device), nbytes)
        g.guards().copy_(self._pattern(device))
        out = g.body().view(dtype).view(shape)
        if poison:
            g.body().fill_(POISON_BYTE)
        elif fill is not None:
            out.fill_(fill)
        self.buffers.append(g)
        self.held_bytes += nbytes + 2 * GUARD_BYTES
        self.outputs += 1
        return out

    def verify(self, release=True):
        """Compares every guard held with the pattern (one device-to-host copy, which synchronises the current stream, for all of them) and lets the buffers go
        (release=False: keeps them, for a caller that launches into the same buffers again).  Raises AssertionError on damage: for each damaged guard the op's label,
        the side, the damaged byte count and the offset of the first damaged byte from the output's first byte (negative in the front guard, >= the output's size in
        the back guard)."""
        import torch

        held = list(self.buffers)
        if release:
            self.buffers, self.held_bytes = [], 0
        if not held:
            return
        bad = torch.stack([g.guards().ne(self._pattern(g.backing.device)).sum(1) for g in held]).cpu()
        if not bool(bad.any()):
            return
        msgs = []
        for g, row in zip(held, bad.tolist()):
            for side, count in enumerate(row):
                if count:
                    first = int(g.guards()[side].ne(self._pattern(g.backing.device)).nonzero()[0])
                    off = first - GUARD_BYTES if side == 0 else g.nbytes + first
                    msgs.append(f"{g.label}: {'front' if side == 0 else 'back'} guard damaged: {count} byte(s), the first at offset {off:+d} from the first byte of the "
                                f"{g.nbytes}-byte output")
        raise AssertionError("store outside an output: " + "; ".join(msgs[:8]) + (f"; ... ({len(msgs)} guards in all)" if len(msgs) > 8 else ""))


@contextlib.contextmanager
def checked_outputs():
    """Inside the block (this thread only) every output the entry points below allocate -- Planes and the copies that cnx_mlp / rb_proj_fc1 update in place included --
    lies between two GUARD_BYTES guard bands holding guard_pattern(), and every byte of a fresh output is POISON_BYTE (NaN in fp32, fp16 and bf16) before the launch: an
    element the kernel does not write stays NaN, a store up to GUARD_BYTES outside the output changes a guard.  Yields the CheckedOutputs that keeps every backing buffer
    alive until the block ends (so no block of the caching allocator comes back holding an earlier launch's result) and compares all guards then, or at `.verify()`:
    AssertionError on damage.  Past HOLD_LIMIT_BYTES it verifies and releases early.  An exception inside the block is not replaced by a guard report.

    Not covered: a store further than GUARD_BYTES away; out-of-bounds READS; the library-owned buffers of the *_bench entries; with iters > 0 the launches repeat into the
    same output, whose contents mean nothing then (the guards still do).  thin128(inplace=True) / mit_attn64(inplace=True) run on a guarded copy that is copied back into
    the caller's tensor: guards only, no poison, and the caller's own allocation is not watched.  The `pn` of conv2d_head and conv2d_g, a caller's tensor written in part, is left where it is.
    Not re-entrant: a second checked_outputs() inside the block raises RuntimeError.  Always off again afterwards."""
    if getattr(_checked, "mgr", None) is not None:
        raise RuntimeError("checked_outputs() is already active on this thread: it does not nest (call .verify() on the active one for an intermediate check)")
    mgr = CheckedOutputs()
    _checked.mgr = mgr
    try:
        yield mgr
    except BaseException:
        mgr.buffers = []
        raise
    finally:
        _checked.mgr = None
    mgr.verify()


def _out(shape, dtype, device, label, fill=None, poison=True):
    """Every output allocation of this module.  Outside checked_outputs(): torch.empty (fill None), torch.zeros (fill 0) or torch.full, nothing else.  Inside: a guarded
    view (CheckedOutputs.allocate): poisoned, or with poison=False holding `fill` (None: left for the caller to copy into)."""
    import torch

    mgr = getattr(_checked, "mgr", None)
    if mgr is not None:
        return mgr.allocate(shape, dtype, device, label, fill, poison)
    if fill is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if fill == 0:
        return torch.zeros(shape, dtype=dtype, device=device)
    return torch.full(shape, fill, dtype=dtype, device=device)


def _checking():
    return getattr(_checked, "mgr", None) is not None


def _out_copy(t, label):
    """a contiguous copy of `t` that a kernel updates in place: t.contiguous().clone(), or inside checked_outputs() the same values between guards"""
    t = t.contiguous()
    if not _checking():
        return t.clone()
    return _out(t.shape, t.dtype, t.device, label, poison=False).copy_(t)


class Planes:
    """An fp32 tensor in one of the engine's split activation formats (include/pf_hip.h): fmt "bf16x3" = three exact bf16
    planes, "f16x2" = the two fp16 planes of the split-f16 scheme.  `plane_elems` carries the format in bit 0."""

    def __init__(self, shape, device, fmt="bf16x3"):
        import torch

        self.shape = tuple(shape)
        self.fmt = fmt
        self.numel = int(np.prod(self.shape))
        stride = (self.numel + 127) // 128 * 128
        self.plane_elems = stride | (1 if fmt == "f16x2" else 0)
        self.data = _out((2 if fmt == "f16x2" else 3) * stride, torch.int16, device, "Planes", fill=0)

    def data_ptr(self):
        return self.data.data_ptr()

    def merge(self):
        """back to fp32: h + m + l (exact) or hi + lo, lo unscaled (the value the split-f16 GEMM works with)."""
        import torch

        lib = load_library()
        y = _out(self.shape, torch.float32, self.data.device, "Planes.merge")
        _check(lib.pf_op_merge_bf16(self.data.device.index, self.data_ptr(), self.plane_elems, self.numel, y.data_ptr(), _stream_ptr()), None, "pf_op_merge_bf16")
        return y


def split_planes(x, fmt="bf16x3"):
    lib = load_library()
    x = x.contiguous()
    pl = Planes(x.shape, x.device, fmt)
    _check(lib.pf_op_split_bf16(x.device.index, x.data_ptr(), x.numel(), pl.data_ptr(), pl.plane_elems, _stream_ptr()), None, "pf_op_split_bf16")
    return pl


def _pl(planes):
    return (planes.data_ptr(), planes.plane_elems) if planes is not None else (None, 0)


def conv2d(x, weight, bias=None, stride=1, pad=0, act=0, res1=None, res2=None, post_relu=False, x2=None, nchw_out=False, tile=-1,
           planes_in=False, planes_out=False, precision=0, planes_fmt="bf16x3", splitk=True):
    """x: (B,H,W,C1) [+ x2: (B,H,W,C2) channel-concat]; weight: (Cout, C1+C2, KH, KW).  Returns (B,Ho,Wo,Cout) or NCHW.
    planes_in: hand the input(s) to the kernel as split-bf16 planes only; planes_out: take the output as planes
    (returned merged back to fp32, which is exact).  precision (split tiles): 0 split-f16 (default parity scheme), 3 exact bf16
    split, 1 bf16x3, 2 bf16.  splitk=False: never contract K in slices (the engine's split-K rule applies otherwise)."""
    import torch

    lib = load_library()
    x = x.contiguous()
    B, H, W, C1 = x.shape
    C2 = 0 if x2 is None else x2.shape[-1]
    w = _np(weight)
    Cout, Cin, KH, KW = w.shape
    if Cin != C1 + C2:
        raise PfError(f"weight Cin {Cin} != {C1}+{C2}")
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    shape = (B, Cout, Ho, Wo) if nchw_out else (B, Ho, Wo, Cout)
    b = _np(bias)
    x2 = x2.contiguous() if x2 is not None else None
    xp = split_planes(x, planes_fmt) if planes_in else None
    x2p = split_planes(x2, planes_fmt) if (planes_in and x2 is not None) else None
    yp = Planes(shape, x.device, planes_fmt) if planes_out else None
    y = None if planes_out else _out(shape, torch.float32, x.device, "conv2d")
    rc = lib.pf_op_conv2d(
        x.device.index, None if planes_in else x.data_ptr(), None if planes_in else _dp(x2), B, H, W, C1, C2, _hp(w), _hp(b),
        Cout, KH, KW, stride, pad, act, _dp(res1), _dp(res2), int(post_relu), int(nchw_out), tile, _dp(y),
        *_pl(xp), *_pl(x2p), *_pl(yp), precision + (0 if splitk else 16), _stream_ptr(),
    )
    _check(rc, None, "pf_op_conv2d")
    return yp.merge() if planes_out else y


def linear(x, weight, bias=None, act=0, res1=None, tile=-1):
    """x: (..., K); weight (N, K) -> (..., N)."""
    K = x.shape[-1]
    rows = x.numel() // K
    w = _np(weight)
    y = conv2d(x.reshape(1, rows, 1, K), w.reshape(w.shape[0], K, 1, 1), bias, act=act,
               res1=None if res1 is None else res1.reshape(1, rows, 1, -1), tile=tile)
    return y.reshape(*x.shape[:-1], w.shape[0])


def linear_ln(x, weight, bias, gamma, beta, eps, act=0, res1=None, tile=-1, precision=0):
    """act(Linear(LayerNorm(x))) + res1 with the LayerNorm fused into the GEMM (pf_op_linear_ln).  x: (..., K); weight (N, K)."""
    import torch

    lib = load_library()
    x = x.contiguous()
    K = x.shape[-1]
    rows = x.numel() // K
    w, b, g, be = _np(weight), _np(bias), _np(gamma), _np(beta)
    N = w.shape[0]
    y = _out((*x.shape[:-1], N), torch.float32, x.device, "linear_ln")
    _check(lib.pf_op_linear_ln(x.device.index, x.data_ptr(), rows, K, _hp(w), _hp(b), _hp(g), _hp(be), float(eps), N, act, _dp(res1), tile, y.data_ptr(), precision,
                               _stream_ptr()), None, "pf_op_linear_ln")
    return y


def rb_linear(x, weight, bias, tokens, gamma=None, beta=None, eps=1e-6, act=0, res=None, iters=0):
    """act(Linear(LayerNorm?(x))) + res in the row-block form (pf_op_rb_linear).  x: (rows, K) with rows = images x tokens; weight (N, K).
    iters > 0: returns the average ms per launch instead."""
    import torch

    lib = load_library()
    x = x.contiguous()
    K = x.shape[-1]
    rows = x.numel() // K
    w, b = _np(weight), _np(bias)
    g, be = (_np(gamma), _np(beta)) if gamma is not None else (None, None)
    N = w.shape[0]
    y = _out((*x.shape[:-1], N), torch.float32, x.device, "rb_linear")
    ms = ctypes.c_float()
    _check(lib.pf_op_rb_linear(x.device.index, x.data_ptr(), rows, tokens, K, _hp(w), _hp(b), _hp(g), _hp(be), float(eps), N,
                               act, _dp(res), y.data_ptr(), iters, ctypes.byref(ms), _stream_ptr()), None, "pf_op_rb_linear")
    return ms.value if iters > 0 else y


def rb_proj_fc1(attn, x, proj_w, proj_b, ln2_g, ln2_b, eps, fc1_w, fc1_b, tokens, iters=0):
    """x1 = x + proj(attn); hidden = fc1(LayerNorm_2(x1)) in one launch (pf_op_rb_proj_fc1).  attn, x: (rows, C) on the GPU, rows = images x tokens, C = 320.
    Returns (x1, hidden); iters > 0: the average ms per launch instead."""
    import torch

    lib = load_library()
    attn = attn.contiguous()
    x1 = _out_copy(x, "rb_proj_fc1 x1")
    rows, C = attn.shape
    hidden = _out((rows, 4 * C), torch.float32, attn.device, "rb_proj_fc1 hidden")
    ms = ctypes.c_float()
    a = [_np(t) for t in (proj_w, proj_b, ln2_g, ln2_b, fc1_w, fc1_b)]
    _check(lib.pf_op_rb_proj_fc1(attn.device.index, attn.data_ptr(), x1.data_ptr(), rows // tokens, tokens, C, _hp(a[0]), _hp(a[1]), _hp(a[2]), _hp(a[3]), float(eps), _hp(a[4]), _hp(a[5]),
                                 hidden.data_ptr(), iters, ctypes.byref(ms), _stream_ptr()), None, "pf_op_rb_proj_fc1")
    return ms.value if iters > 0 else (x1, hidden)


def rb_srkv(x, ln1_g, ln1_b, eps1, sr_w, sr_b, srn_g, srn_b, eps2, kv_w, kv_b, iters=0):
    """Key / value branch of a MiT block with 2 x 2 spatial reduction in one launch (pf_op_rb_srkv).  x: (B, 2 Hr, 2 Wr, C) on the GPU, C = 320.
    Returns kv (B, Hr Wr, 2 C); iters > 0: the average ms per launch instead."""
    import torch

    lib = load_library()
    x = x.contiguous()
    B, H, W, C = x.shape
    kv = _out((B, (H // 2) * (W // 2), 2 * C), torch.float32, x.device, "rb_srkv")
    ms = ctypes.c_float()
    a = [_np(t) for t in (ln1_g, ln1_b, sr_w, sr_b, srn_g, srn_b, kv_w, kv_b)]
    _check(lib.pf_op_rb_srkv(x.device.index, x.data_ptr(), B, H // 2, W // 2, C, _hp(a[0]), _hp(a[1]), float(eps1), _hp(a[2]), _hp(a[3]), _hp(a[4]), _hp(a[5]), float(eps2),
                             _hp(a[6]), _hp(a[7]), kv.data_ptr(), iters, ctypes.byref(ms), _stream_ptr()), None, "pf_op_rb_srkv")
    return ms.value if iters > 0 else kv


def mit_attn64(x, kv, ln_gamma, ln_beta, eps, q_w, q_b, proj_w, proj_b, iters=0, inplace=False):
    """y = x + proj(softmax((LN1(x) Wq^T + bq) K^T / 8) V) for (B, N, 64) token rows and (B, M, 128) keys | values in one launch (attn_block.hip).
    iters > 0: returns (y, avg ms per launch)."""
    lib = load_library()
    x, kv = x.contiguous(), kv.contiguous()
    B, N, C = x.shape
    home = x if (inplace and _checking()) else None   # checked: the in-place launch runs on a guarded copy, which is copied back
    if home is not None:
        x = _out_copy(x, "mit_attn64 in place")
    y = x if inplace else _out(x.shape, x.dtype, x.device, "mit_attn64")
    ms = ctypes.c_float()
    g, b, qw, qb, pw, pb = (_np(t) for t in (ln_gamma, ln_beta, q_w, q_b, proj_w, proj_b))
    _check(lib.pf_op_mit_attn64(x.device.index, x.data_ptr(), kv.data_ptr(), y.data_ptr(), B, N, kv.shape[1], _hp(g), _hp(b), eps, _hp(qw), _hp(qb), _hp(pw), _hp(pb),
                                iters, ctypes.byref(ms), _stream_ptr()), None, "pf_op_mit_attn64")
    if home is not None:
        y = home.copy_(y)
    return (y, ms.value) if iters > 0 else y


def stem7x7(x4, weight, bias, stride, relu=False, ln_gamma=None, ln_beta=None, eps=1e-5, iters=0):
    """conv 7x7 / stride 2 or 4 / pad 3, 3 -> 64 channels (+ ReLU, or + LayerNorm over the 64 channels) on an NHWC4 image (B, H, W, 4) in one launch (stem7.hip).
    iters > 0: returns (y, avg ms per launch)."""
    import torch

    lib = load_library()
    x4 = x4.contiguous()
    B, H, W, _ = x4.shape
    Ho, Wo = (H + 6 - 7) // stride + 1, (W + 6 - 7) // stride + 1
    y = _out((B, Ho, Wo, 64), torch.float32, x4.device, "stem7x7")
    ms = ctypes.c_float()
    w, b = _np(weight), _np(bias)
    g, be = (_np(ln_gamma), _np(ln_beta)) if ln_gamma is not None else (None, None)
    _check(lib.pf_op_stem7x7(x4.device.index, x4.data_ptr(), y.data_ptr(), B, H, W, stride, _hp(w), _hp(b), 1 if relu else 0, _hp(g), _hp(be), float(eps), iters, ctypes.byref(ms),
                             _stream_ptr()), None, "pf_op_stem7x7")
    return (y, ms.value) if iters > 0 else y


def thin128(x, weight, bias, res=None, iters=0, inplace=False):
    """x W^T + b (+ res) for a 128 -> 128 layer over (..., 128) rows in the transposed, register-epilogue form (thin_linear.hip).  inplace: y aliases res.
    iters > 0: returns (y, avg ms per launch)."""
    lib = load_library()
    x = x.contiguous()
    rows = x.numel() // 128
    home = res if (inplace and res is not None and res.is_contiguous() and _checking()) else None   # checked: the in-place launch runs on a guarded copy, which is copied back
    if home is not None:
        res = _out_copy(res, "thin128 in place")
    y = res if (inplace and res is not None) else _out(x.shape, x.dtype, x.device, "thin128")
    ms = ctypes.c_float()
    w, b = _np(weight), _np(bias)
    _check(lib.pf_op_thin128(x.device.index, x.data_ptr(), rows, _hp(w), _hp(b), _dp(res), y.data_ptr(), iters, ctypes.byref(ms), _stream_ptr()), None, "pf_op_thin128")
    if home is not None:
        y = home.copy_(y)
    return (y, ms.value) if iters > 0 else y


def mit_mlp(x, fc1_w, fc1_b, ln_gamma, ln_beta, eps, dw_w, dw_b, fc2_w, fc2_b, iters=0):
    """One MiT block Mlp in one kernel: x + fc2(GELU(dwconv3x3(fc1(LayerNorm(x))))).  x: (B, Hs, Ws, C) on the GPU, C = 64 or 128.
    iters > 0: returns the average ms per launch instead."""
    lib = load_library()
    x = x.contiguous()
    B, Hs, Ws, C = x.shape
    y = _out(x.shape, x.dtype, x.device, "mit_mlp")
    ms = ctypes.c_float()
    a = [_np(v) for v in (fc1_w, fc1_b, ln_gamma, ln_beta, dw_w, dw_b, fc2_w, fc2_b)]
    _check(lib.pf_op_mit_mlp(x.device.index, x.data_ptr(), y.data_ptr(), B, Hs, Ws, C, _hp(a[0]), _hp(a[1]), _hp(a[2]), _hp(a[3]), float(eps), _hp(a[4]), _hp(a[5]), _hp(a[6]), _hp(a[7]),
                             iters, ctypes.byref(ms), _stream_ptr()), None, "pf_op_mit_mlp")
    return ms.value if iters > 0 else y


def cnx_mlp(d, y, w1, b1, ln_gamma, ln_beta, eps, w2, b2, layer_scale, iters=0):
    """One ConvNeXt block MLP in one kernel: returns y + layer_scale * pwconv2(GELU(pwconv1(LayerNorm(d)))) (y is not modified: a copy is
    updated).  d, y: (rows, C) on the GPU, C = 96 or 192 (cnx_mlp.hip), 384 or 768
    (the row-block form, cnx_rb.hip).  iters > 0: returns (result of the first launch is lost) the average ms per launch."""
    lib = load_library()
    d = d.contiguous()
    out = _out_copy(y, "cnx_mlp")
    rows, C = d.shape
    ms = ctypes.c_float()
    a = [_np(v) for v in (w1, b1, ln_gamma, ln_beta, w2, b2, layer_scale)]
    _check(lib.pf_op_cnx_mlp(d.device.index, d.data_ptr(), out.data_ptr(), rows, C, _hp(a[0]), _hp(a[1]), _hp(a[2]), _hp(a[3]), float(eps), _hp(a[4]), _hp(a[5]), _hp(a[6]),
                             iters, ctypes.byref(ms), _stream_ptr()), None, "pf_op_cnx_mlp")
    return ms.value if iters > 0 else out


def layernorm(x, gamma, beta, eps, planes_out=False):
    lib = load_library()
    x = x.contiguous()
    C = x.shape[-1]
    y = None if planes_out else _out(x.shape, x.dtype, x.device, "layernorm")
    yp = Planes(x.shape, x.device) if planes_out else None
    g, b = _np(gamma), _np(beta)
    _check(lib.pf_op_layernorm(x.device.index, x.data_ptr(), _hp(g), _hp(b), _dp(y), x.numel() // C, C, eps, *_pl(yp), _stream_ptr()), None, "pf_op_layernorm")
    return yp.merge() if planes_out else y


def dwconv3x3_gelu(x, weight, bias, planes_out=False, variant=None):
    """variant None: the default path; otherwise an explicit kernel (pf_op_dwconv3x3_bench's ids)."""
    lib = load_library()
    x = x.contiguous()
    B, H, W, C = x.shape
    y = None if planes_out else _out(x.shape, x.dtype, x.device, "dwconv3x3_gelu")
    yp = Planes(x.shape, x.device) if planes_out else None
    w, b = _np(weight), _np(bias)
    if variant is not None:
        _check(lib.pf_op_dwconv3x3_gelu_cfg(x.device.index, x.data_ptr(), _hp(w), _hp(b), _dp(y), B, H, W, C, *_pl(yp), int(variant), _stream_ptr()), None, "pf_op_dwconv3x3_gelu_cfg")
        return yp.merge() if planes_out else y
    _check(lib.pf_op_dwconv3x3_gelu(x.device.index, x.data_ptr(), _hp(w), _hp(b), _dp(y), B, H, W, C, *_pl(yp), _stream_ptr()), None, "pf_op_dwconv3x3_gelu")
    return yp.merge() if planes_out else y


def dwconv7x7(x, weight, bias, variant=None, nc=0, nb=0, th=0):
    """variant None: the default path; 3: column-blocked streaming kernel (nc columns per thread, nb row buffers, strips of th
    rows; 0 = automatic); 2: one column per lane."""
    lib = load_library()
    x = x.contiguous()
    B, H, W, C = x.shape
    y = _out(x.shape, x.dtype, x.device, "dwconv7x7")
    w, b = _np(weight), _np(bias)
    if variant is None:
        _check(lib.pf_op_dwconv7x7(x.device.index, x.data_ptr(), _hp(w), _hp(b), y.data_ptr(), B, H, W, C, _stream_ptr()), None, "pf_op_dwconv7x7")
    else:
        _check(lib.pf_op_dwconv7x7_cfg(x.device.index, x.data_ptr(), _hp(w), _hp(b), y.data_ptr(), B, H, W, C, variant, nc, nb, th, _stream_ptr()), None, "pf_op_dwconv7x7_cfg")
    return y


def dwconv7x7_bench(variant, B, H, W, C, nc=0, nb=0, th=0, iters=10, device=0):
    lib = load_library()
    ms = ctypes.c_float()
    _check(lib.pf_op_dwconv7x7_bench(device, variant, nc, nb, th, B, H, W, C, iters, ctypes.byref(ms)), None, "pf_op_dwconv7x7_bench")
    return ms.value


def sr_attention(q, kv, heads, planes_out=False):
    """q: (B,N,C), kv: (B,M,2C) -> (B,N,C); head_dim 64."""
    lib = load_library()
    q, kv = q.contiguous(), kv.contiguous()
    B, N, C = q.shape
    M = kv.shape[1]
    out = None if planes_out else _out(q.shape, q.dtype, q.device, "sr_attention")
    op = Planes(q.shape, q.device) if planes_out else None
    _check(lib.pf_op_sr_attention(q.device.index, q.data_ptr(), kv.data_ptr(), _dp(out), B, N, M, heads, *_pl(op), _stream_ptr()), None, "pf_op_sr_attention")
    return op.merge() if planes_out else out


def sr_attention_variant(q, kv, heads, variant, iters=0):
    """variant 1: split-f16 MFMA kernel (the forward's default), 0: exact fp32 MFMA.  iters > 0: returns (out, avg ms per launch)."""
    lib = load_library()
    q, kv = q.contiguous(), kv.contiguous()
    B, N, C = q.shape
    out = _out(q.shape, q.dtype, q.device, "sr_attention_variant")
    ms = ctypes.c_float()
    _check(lib.pf_op_sr_attention_variant(q.device.index, variant, q.data_ptr(), kv.data_ptr(), out.data_ptr(), B, N, kv.shape[1], heads, iters,
                                          ctypes.byref(ms), _stream_ptr()), None, "pf_op_sr_attention_variant")
    return (out, ms.value) if iters > 0 else out


def upsample2x(x, planes_out=False):
    import torch

    lib = load_library()
    x = x.contiguous()
    B, H, W, C = x.shape
    shape = (B, 2 * H, 2 * W, C)
    y = None if planes_out else _out(shape, torch.float32, x.device, "upsample2x")
    yp = Planes(shape, x.device) if planes_out else None
    _check(lib.pf_op_upsample2x(x.device.index, x.data_ptr(), _dp(y), B, H, W, C, *_pl(yp), _stream_ptr()), None, "pf_op_upsample2x")
    return yp.merge() if planes_out else y


def conv_tiles():
    lib = load_library()
    return [lib.pf_op_conv_tile_name(i).decode() for i in range(lib.pf_op_num_conv_tiles())]


# ---- the kernels at the two ends of the forward (pf_op_prep_* ... pf_op_conv2d_head in include/pf_hip.h)
def prep_u8(x_u8, mean3, std3):
    """(B,H,W,3) uint8 -> (B,H,W,4) fp32: (x - mean) / std, channel 3 = 0."""
    import torch

    lib = load_library()
    x_u8 = x_u8.contiguous()
    B, H, W, _ = x_u8.shape
    m, s = _np(mean3), _np(std3)
    y = _out((B, H, W, 4), torch.float32, x_u8.device, "prep_u8")
    _check(lib.pf_op_prep_u8(x_u8.device.index, x_u8.data_ptr(), B, H, W, _hp(m), _hp(s), y.data_ptr(), _stream_ptr()), None, "pf_op_prep_u8")
    return y


def prep_f32_nchw(x, mean3, std3):
    """(B,3,H,W) fp32 -> (B,H,W,4) fp32: (x - mean) / std, channel 3 = 0."""
    import torch

    lib = load_library()
    x = x.contiguous()
    B, _, H, W = x.shape
    m, s = _np(mean3), _np(std3)
    y = _out((B, H, W, 4), torch.float32, x.device, "prep_f32_nchw")
    _check(lib.pf_op_prep_f32_nchw(x.device.index, x.data_ptr(), B, H, W, _hp(m), _hp(s), y.data_ptr(), _stream_ptr()), None, "pf_op_prep_f32_nchw")
    return y


def pred_regression(tg, tl, wg, bg, wl, bl, with_pn=True, pn_fill=None):
    """tg, tl: (B,HW,32) -> pg (B,2,HW) normalised, pl (B,HW) clamped, pn (B*HW,4) = (g0, g1, lat, 0) or None."""
    import torch

    lib = load_library()
    tg, tl = tg.contiguous(), tl.contiguous()
    B, HW, _ = tg.shape
    a = [_np(t) for t in (wg, bg, wl, bl)]
    pg = _out((B, 2, HW), torch.float32, tg.device, "pred_regression pg")
    pl = _out((B, HW), torch.float32, tg.device, "pred_regression pl")
    pn = _out((B * HW, 4), torch.float32, tg.device, "pred_regression pn", fill=float("nan") if pn_fill is None else pn_fill, poison=False) if with_pn else None
    _check(lib.pf_op_pred_regression(tg.device.index, tg.data_ptr(), tl.data_ptr(), B, HW, _hp(a[0]), _hp(a[1]), _hp(a[2]), _hp(a[3]), pg.data_ptr(), pl.data_ptr(), _dp(pn),
                                     _stream_ptr()), None, "pf_op_pred_regression")
    return pg, pl, pn


def decode_cls(logit_g, logit_l):
    """logits (B,ng,HW), (B,nl,HW) -> dg (B,2,HW) unit vectors ((0,0) for the last gravity bin), dl (B,HW) degrees."""
    import torch

    lib = load_library()
    logit_g, logit_l = logit_g.contiguous(), logit_l.contiguous()
    B, ng, HW = logit_g.shape
    nl = logit_l.shape[1]
    dg = _out((B, 2, HW), torch.float32, logit_g.device, "decode_cls dg")
    dl = _out((B, HW), torch.float32, logit_g.device, "decode_cls dl")
    _check(lib.pf_op_decode_cls(logit_g.device.index, logit_g.data_ptr(), ng, logit_l.data_ptr(), nl, B, HW, dg.data_ptr(), dl.data_ptr(), _stream_ptr()), None, "pf_op_decode_cls")
    return dg, dl


def nearest_nhwc4(x, Ho, Wo):
    """(B,H,W,4) -> (B,Ho,Wo,4), F.interpolate's default 'nearest'."""
    import torch

    lib = load_library()
    x = x.contiguous()
    B, H, W, _ = x.shape
    y = _out((B, Ho, Wo, 4), torch.float32, x.device, "nearest_nhwc4")
    _check(lib.pf_op_nearest_nhwc4(x.device.index, x.data_ptr(), B, H, W, Ho, Wo, y.data_ptr(), _stream_ptr()), None, "pf_op_nearest_nhwc4")
    return y


def gap_ln_head(x, gamma, beta, eps, head_w, head_b):
    """x: (B,HW,C) -> (B,nout): mean over HW, LayerNorm, Linear."""
    import torch

    lib = load_library()
    x = x.contiguous()
    B, HW, C = x.shape
    g, b, w, hb = (_np(t) for t in (gamma, beta, head_w, head_b))
    nout = w.shape[0]
    y = _out((B, nout), torch.float32, x.device, "gap_ln_head")
    _check(lib.pf_op_gap_ln_head(x.device.index, x.data_ptr(), B, HW, C, _hp(g), _hp(b), float(eps), _hp(w), _hp(hb), nout, y.data_ptr(), _stream_ptr()), None, "pf_op_gap_ln_head")
    return y


def paramnet_scalars(raw, mode):
    """raw: (B,nraw) -> (B,8) (pf_op_paramnet_scalars)."""
    import torch

    lib = load_library()
    raw = raw.contiguous()
    B, nraw = raw.shape
    out = _out((B, 8), torch.float32, raw.device, "paramnet_scalars", fill=float("nan"))
    _check(lib.pf_op_paramnet_scalars(raw.device.index, raw.data_ptr(), B, nraw, int(mode), out.data_ptr(), _stream_ptr()), None, "pf_op_paramnet_scalars")
    return out


def conv2d_head_tiles(B, H, W, Cin, act, head_kind):
    """ids of the conv tiles that can run pf_op_conv2d_head's form (host logic only: no GPU needed)."""
    lib = load_library()
    return [t for t in range(lib.pf_op_num_conv_tiles()) if lib.pf_op_conv2d_head_tile_usable(B, H, W, Cin, act, head_kind, t)]


def conv2d_head(x, weight, bias, act, head_kind, head_w, head_b, tile=-1, pn=None):
    """3x3 / stride 1 / pad 1 conv to 32 channels with the prediction head in its epilogue.  x: (B,H,W,Cin) -> head_out (B,2,H*W) (head_kind 1) or (B,H*W) (head_kind 2);
    pn: optional (B*H*W,4) tensor, partly written in place (head_kind 1: floats 0-1, head_kind 2: floats 2-3 of each row).  A tile that cannot run the form raises."""
    import torch

    lib = load_library()
    x = x.contiguous()
    B, H, W, Cin = x.shape
    w, b, hw, hb = _np(weight), _np(bias), _np(head_w), _np(head_b)
    if w.shape != (32, Cin, 3, 3):
        raise PfError(f"weight shape {w.shape} != (32, {Cin}, 3, 3)")
    out = _out((B, 2, H * W) if head_kind == 1 else (B, H * W), torch.float32, x.device, "conv2d_head")
    _check(lib.pf_op_conv2d_head(x.device.index, x.data_ptr(), B, H, W, Cin, _hp(w), _hp(b), int(act), int(head_kind), _hp(hw), _hp(hb), int(tile), out.data_ptr(), _dp(pn),
                                 _stream_ptr()), None, "pf_op_conv2d_head")
    return out


def conv2d_g_tiles(B, H, W, C1, Cout, K, stride=1, pad=0, act=0, groups=1, ups=False, C2=0, has_table=False, head_kind=0, precision=0):
    """ids of the conv tiles that can run a form of pf_op_conv2d_g (host logic only: no GPU needed).  H, W: the full-resolution size."""
    lib = load_library()
    return [t for t in range(lib.pf_op_num_conv_tiles())
            if lib.pf_op_conv2d_g_tile_usable(B, H, W, C1, C2, Cout, K, K, stride, pad, act, groups, int(ups), int(has_table), head_kind, precision, t)]


def conv2d_g(problems, stride=1, pad=0, act=0, post_relu=False, ups=False, tile=-1, precision=0, splitk=-1, size=None):
    """One grouped launch (pf_op_conv2d_g) of len(problems) = 1 or 2 convs of one shape.  A problem is a dict: x (B,H,W,C1), or with ups (B,H/2,W/2,C1) at half
    resolution; weight (Cout,C1+C2,KH,KW); optional x2 (B,H,W,C2), bias ((Cout,), or (9,Cout): the border-case table), res1, res2, and for a fused head head_kind (1 / 2),
    head_w, head_b and pn ((B*H*W,4), partly written in place; the groups may share one).  splitk: -1 the engine's rule, 0 never, N > 1 that factor.
    size: the full-resolution (H, W) when it is not the one x implies (with ups an odd size, which the entry refuses).
    Returns (outputs, factor): per problem y (B,Ho,Wo,Cout) or the head output ((B,2,Ho*Wo) / (B,Ho*Wo)), and the split-K factor the launch used (1 = none).
    A tile that cannot run the form raises."""
    import torch

    lib = load_library()
    n = len(problems)
    if n not in (1, 2):
        raise PfError("conv2d_g: one or two problems")
    xs = [pr["x"].contiguous() for pr in problems]
    B, Hs, Ws, C1 = xs[0].shape
    H, W = size if size is not None else ((2 * Hs, 2 * Ws) if ups else (Hs, Ws))
    ws = [_np(pr["weight"]) for pr in problems]
    Cout, Cin, KH, KW = ws[0].shape
    C2 = Cin - C1
    x2s = [pr["x2"].contiguous() if pr.get("x2") is not None else None for pr in problems]
    bs = [_np(pr.get("bias")) for pr in problems]
    rows = [9 if (b is not None and b.ndim == 2) else 1 for b in bs]
    kinds = [int(pr.get("head_kind", 0)) for pr in problems]
    hws, hbs = [_np(pr.get("head_w")) for pr in problems], [_np(pr.get("head_b")) for pr in problems]
    for x, w, x2, b, r in zip(xs, ws, x2s, bs, rows):
        if x.shape != xs[0].shape or w.shape != ws[0].shape or (x2 is None) != (C2 == 0) or (x2 is not None and tuple(x2.shape) != (B, H, W, C2)):
            raise PfError("conv2d_g: the problems of one launch share one shape; x2 (B,H,W,C2) exactly when the weight has more input channels than x")
        if b is not None and b.shape != ((9, Cout) if r == 9 else (Cout,)):
            raise PfError(f"conv2d_g: bias shape {b.shape} is neither ({Cout},) nor (9, {Cout})")
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    outs = [_out(((B, 2, Ho * Wo) if k == 1 else (B, Ho * Wo)) if k else (B, Ho, Wo, Cout), torch.float32, xs[0].device, "conv2d_g") for k in kinds]

    def arr(vals, host=False):
        return (ctypes.c_void_p * n)(*[(v.ctypes.data if v is not None else None) if host else _dp(v) for v in vals])

    ints = lambda vals: (ctypes.c_int * n)(*vals)
    used = ctypes.c_int(1)
    rc = lib.pf_op_conv2d_g(
        xs[0].device.index, n, arr(xs), arr(x2s), B, H, W, C1, C2, arr(ws, True), arr(bs, True), ints(rows), Cout, KH, KW, stride, pad, int(act),
        arr([pr.get("res1") for pr in problems]), arr([pr.get("res2") for pr in problems]), int(post_relu), int(ups),
        arr([None if k else o for k, o in zip(kinds, outs)]), ints(kinds), arr(hws, True), arr(hbs, True), arr([o if k else None for k, o in zip(kinds, outs)]),
        arr([pr.get("pn") for pr in problems]), int(tile), int(precision), int(splitk), ctypes.byref(used), _stream_ptr())
    _check(rc, None, "pf_op_conv2d_g")
    return outs, used.value


def conv2d_bench(B, H, W, Cin, Cout, K, stride=1, pad=0, tile=-1, iters=10, device=0, fmt=0, precision=0):
    """Average ms per launch of one conv shape on random data (tuning aid).  fmt 0: fp32 in / out; 1: split-plane
    input; 2: split-plane input and output (the exact bf16 split).  precision: PF_PRECISION_* of the split tiles
    (0 split-f16 default, 3 exact bf16 split, 1 bf16x3, 2 bf16).  Returns -1 when the tile cannot run the format."""
    lib = load_library()
    ms = ctypes.c_float()
    _check(lib.pf_op_conv2d_bench(device, B, H, W, Cin, Cout, K, stride, pad, tile, iters, fmt + 16 * precision, ctypes.byref(ms)), None, "pf_op_conv2d_bench")
    return ms.value


def dwconv3x3_bench(variant, B, H, W, C, iters=10, device=0):
    lib = load_library()
    ms = ctypes.c_float()
    _check(lib.pf_op_dwconv3x3_bench(device, variant, B, H, W, C, iters, ctypes.byref(ms)), None, "pf_op_dwconv3x3_bench")
    return ms.value
