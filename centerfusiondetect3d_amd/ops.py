"""Operator-level host wrappers over the C ABI (include/cf_hip.h).

Each function mirrors one operator the reference dispatches on the hot path (see the header for
the file:line each replaces).  Tensors are torch CUDA(=HIP) tensors used purely as device memory;
activations are NHWC fp32 (a (B,H,W,C) contiguous tensor).  Nothing here falls back to torch ops.
"""
import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import (ACT_NONE, ACT_RELU, ACT_SIGMOID_CLAMP, ACT_RAW_AND_SIGDEPTH, LAYOUT_NHWC, LAYOUT_NCHW)
from .packing import PackedConv, PackedDcn, MX_ROW as packing_MX_ROW


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.CfHipError("libcfhip operators need device tensors (no CPU path)")


DEFAULT_IN_SCALE = 16.0     # activation pre-scale of the f16x3 / mx kernels (cf_f16x3.h: ASCALE); 65504 / 16 = 4094 is where they clamp
F16_MAX = 65504.0


IN_SCALE_KEEP_MIN = 2.0 ** -6   # the default pre-scale is kept down to this max |x| (below, the lo half turns fp16-subnormal)
IN_SCALE_MAX = 2.0 ** 32        # cap of the lower branch: out_scale = 2^-s / in_scale stays a normal fp32
F32_MIN_NORMAL = 2.0 ** -126


def _largest_pow2_scale(a, limit):
    """The largest power of two s with a * s <= limit (a, limit > 0)."""
    import math
    p = math.floor(math.log2(limit / a))
    while a * 2.0 ** (p + 1) <= limit:
        p += 1
    while a * 2.0 ** p > limit:
        p -= 1
    return 2.0 ** p


def in_scale_for_large(absmax, headroom=8.0):
    """The upper branch of `in_scale_for` alone: 16 unless max |x| * 16 comes within a factor 4 of the fp16 limit.  The rule
    of the heads' mx rows (block floating point: no lower-end problem)."""
    a = float(absmax)
    if not (a == a) or a == float("inf"):
        raise _lib.CfHipError("activation range is not finite (NaN / inf in a layer input)")
    if a * DEFAULT_IN_SCALE <= F16_MAX / 4.0:
        return DEFAULT_IN_SCALE
    return _largest_pow2_scale(a, F16_MAX / headroom)


def in_scale_for(absmax, headroom=8.0):
    """The activation pre-scale (a power of two) for a layer whose inputs reach `absmax`: the default 16 while
    2^-6 <= absmax and absmax * 16 leaves a factor 4 to the fp16 limit (and for absmax == 0: an empty map); otherwise the
    largest power of two that keeps absmax * scale <= 65504 / headroom - below 2^-6 that RAISES the scale (capped at 2^32),
    so the lo half of the split stays a normal fp16."""
    a = float(absmax)
    if a == 0.0 or a >= IN_SCALE_KEEP_MIN or not (a == a):
        return in_scale_for_large(a, headroom)
    return min(IN_SCALE_MAX, _largest_pow2_scale(a, F16_MAX / headroom))


def _scaled_out_scale(out_scale, in_scale, what):
    """out_scale of a launch whose activation pre-scale is `in_scale` instead of 16; it must stay a normal fp32."""
    s = out_scale * DEFAULT_IN_SCALE / float(in_scale)
    if out_scale > 0 and not (F32_MIN_NORMAL <= s < float("inf")):
        raise _lib.CfHipError(f"{what}: out_scale {s!r} for in_scale {float(in_scale)!r} is not a normal fp32")
    return s


def conv_args(pc: PackedConv, srcs: Sequence[torch.Tensor], src_strides: Sequence[int], B, H, W,
              out: torch.Tensor, out_stride: int, act=ACT_NONE, residual=None, res_stride=0,
              layout=LAYOUT_NHWC, out2=None, out_offset=0, precise=True, elem_bytes=4, in_scale=None) -> _lib.ConvArgs:
    """Build (and return for reuse) the argument block of one fused convolution.  in_scale (f16x3 kernels): the layer's
    activation pre-scale, a power of two (None = the default 16); out_scale follows it."""
    a = _lib.ConvArgs()
    for i, (s, c) in enumerate(zip(srcs, src_strides)):
        a.src[i] = s.data_ptr()
        a.src_c[i] = c
    a.n_src = len(srcs)
    a.B, a.H, a.W = B, H, W
    a.Ho = (H + 2 * pc.pad - pc.kh) // pc.stride + 1
    a.Wo = (W + 2 * pc.pad - pc.kh) // pc.stride + 1
    a.stride = pc.stride
    a.weight, a.slots, a.bias = pc.weight.data_ptr(), pc.slots.data_ptr(), pc.bias.data_ptr()
    a.K_pad, a.N, a.N_pad = pc.k_pad, pc.n, pc.n_pad
    a.residual = _lib.ptr(residual)
    a.res_stride = res_stride
    a.out = out.data_ptr() + elem_bytes * out_offset
    a.out2 = _lib.ptr(out2)
    a.out_stride, a.out_layout, a.act = out_stride, layout, act
    a.precise = int(bool(precise))
    a.out_scale = float(getattr(pc, "out_scale", 0.0))        # 2^-(s+4): the packer's figure at the default pre-scale
    if in_scale is not None and float(in_scale) != DEFAULT_IN_SCALE:
        a.in_scale = float(in_scale)
        a.out_scale = _scaled_out_scale(a.out_scale, in_scale, "conv_args")
    return a


def absmax(x, out=None):
    """max |x| of an fp32 device tensor (contiguous, or a 2-D row-strided view) as a 1-element device tensor: NaN if any
    element is NaN, inf if any is infinite (cf_absmax_f32).  No host sync."""
    _need_cuda(x)
    if x.dtype != torch.float32:
        raise _lib.CfHipError("absmax: float32 only")
    if x.is_contiguous():
        M, Cc, stride = x.numel() // max(1, x.shape[-1] if x.dim() else 1), (x.shape[-1] if x.dim() else 1), (x.shape[-1] if x.dim() else 1)
        if Cc % 4 or x.data_ptr() % 16:
            M, Cc, stride = 1, x.numel(), x.numel()        # (one long row: the element-wise path)
    elif x.dim() == 2 and x.stride(1) == 1:
        M, Cc, stride = x.shape[0], x.shape[1], x.stride(0)
    else:
        raise _lib.CfHipError("absmax: contiguous tensor or a row-strided 2-D view")
    if out is None:
        out = torch.empty(1, device=x.device, dtype=torch.float32)
    if x.numel() == 0:
        out.zero_()
        return out
    _lib.check(_lib.load().cf_absmax_f32(x.data_ptr(), M, Cc, stride, out.data_ptr(), _lib.stream_ptr()), "cf_absmax_f32")
    return out


def run_conv_f16(a: _lib.ConvArgs, patch=False):
    if patch:
        _lib.check(_lib.load().cf_conv3x3_f16x3(C.byref(a), _lib.stream_ptr()), "cf_conv3x3_f16x3")
    else:
        _lib.check(_lib.load().cf_conv2d_f16x3(C.byref(a), _lib.stream_ptr()), "cf_conv2d_f16x3")


def conv2d_f16x3(pc: PackedConv, srcs, B, H, W, act=ACT_NONE, residual=None, out=None, patch=None, in_scale=None):
    """fp32 NHWC in / out, split-fp16 products (packing.pack_conv_f16).  patch: use the LDS-patch
    3x3 kernel (default: whenever the packing allows it).  in_scale: the activation pre-scale (None = 16)."""
    _need_cuda(*srcs, residual)
    Ho = (H + 2 * pc.pad - pc.kh) // pc.stride + 1
    Wo = (W + 2 * pc.pad - pc.kh) // pc.stride + 1
    if out is None:
        out = torch.empty((B, Ho, Wo, pc.n), device=srcs[0].device, dtype=torch.float32)
    a = conv_args(pc, srcs, [s.shape[-1] for s in srcs], B, H, W, out, out.shape[-1], act, residual,
                  residual.shape[-1] if residual is not None else 0, LAYOUT_NHWC, None, 0, False, in_scale=in_scale)
    run_conv_f16(a, pc.patch if patch is None else patch)
    return out


def group_ptrs(blocks):
    """The host array of argument-block pointers a grouped entry point takes (keep `blocks` alive beside it)."""
    return (C.POINTER(type(blocks[0])) * len(blocks))(*[C.pointer(b) for b in blocks])


def conv3x3_f16x3_grouped(pcs: Sequence[PackedConv], xs, act=ACT_NONE, out=None, in_scales=None):
    """The offset convolutions (N_pad = 32) of up to four same-shape layers on their own inputs as ONE launch
    (cf_conv3x3_f16x3_grouped).  xs: (B,H,W,C) tensors; -> (G,B,H,W,S), S = `out`'s row stride (default 32: the offmask rows
    the DCN reads); group g's rows carry the bits of the ungrouped call on (pcs[g], xs[g]).  in_scales: one activation
    pre-scale per group (None = 16 each)."""
    _need_cuda(*xs, out)
    B, H, W, _ = xs[0].shape
    if out is None:
        out = torch.empty((len(xs), B, H, W, pcs[0].n_pad), device=xs[0].device, dtype=torch.float32)
    S = out.shape[-1]
    blocks = [conv_args(pc, [x], [x.shape[-1]], B, H, W, out[g], S, act, None, 0, LAYOUT_NHWC, None, 0, False,
                        in_scale=None if in_scales is None else in_scales[g])
              for g, (pc, x) in enumerate(zip(pcs, xs))]
    _lib.check(_lib.load().cf_conv3x3_f16x3_grouped(group_ptrs(blocks), len(blocks), _lib.stream_ptr()), "cf_conv3x3_f16x3_grouped")
    return out


def conv3x3_grouped_form(blocks):
    """{WC, WP, WK, NU, T2, CT}: the conv3x3_f16x3_kernel_grouped instantiation cf_conv3x3_f16x3_grouped launches for these
    argument blocks (the launcher's own choice; nothing is launched)."""
    form = (C.c_int32 * 6)()
    _lib.check(_lib.load().cf_conv3x3_grouped_form(group_ptrs(blocks), len(blocks), form), "cf_conv3x3_grouped_form")
    return dict(zip(("WC", "WP", "WK", "NU", "T2", "CT"), form))


CONV3_ENTRIES = {"plain": 0, "root": 1, "proj": 2, "grouped": 3}            # CF_CONV3_ENTRY_*
CONV3_FORM_FIELDS = ("patch", "fused", "WC", "WP", "WK", "RT", "NU", "DB", "MINB", "T2", "CT", "S2", "ROOT", "PROJ", "GRP",
                     "blocks", "grid_y", "threads", "lds", "PR", "tiles_x", "tiles_y", "n_rounds")
DCN_FORM_FIELDS = ("WC", "WP", "RT", "COAL", "CT", "grid_x", "grid_y", "ks", "tiles")


def conv3x3_tile_form(entry, blocks, channels=None):
    """What cf_conv3x3_f16x3 ("plain": one block), cf_conv3x3_root_f16x3 ("root": conv2's block, the Root's, root channels),
    cf_conv3x3_proj_f16x3 ("proj": one block, source channels) or cf_conv3x3_f16x3_grouped ("grouped") would launch for
    these argument blocks, as CONV3_FORM_FIELDS (cf_conv3x3_tile_form: the launchers' own choice; host only, nothing is
    launched).  patch = 0: forwarded to cf_conv2d_f16x3, every form field -1."""
    form = (C.c_int32 * len(CONV3_FORM_FIELDS))()
    ch = None if channels is None else (C.c_int32 * len(channels))(*channels)
    _lib.check(_lib.load().cf_conv3x3_tile_form(CONV3_ENTRIES[entry], group_ptrs(blocks), len(blocks), ch, form), "cf_conv3x3_tile_form")
    return dict(zip(CONV3_FORM_FIELDS, form))


def dcn_v2_f16x3_form(blocks):
    """What cf_dcn_v2_f16x3_grouped (one block: cf_dcn_v2_f16x3) would launch for these argument blocks, as DCN_FORM_FIELDS
    (cf_dcn_v2_f16x3_form: the launchers' own choice; host only, nothing is launched)."""
    form = (C.c_int32 * len(DCN_FORM_FIELDS))()
    _lib.check(_lib.load().cf_dcn_v2_f16x3_form(group_ptrs(blocks), len(blocks), form), "cf_dcn_v2_f16x3_form")
    return dict(zip(DCN_FORM_FIELDS, form))


def dcn_v2_f16x3_grouped(pds: Sequence[PackedDcn], xs, offmask, act=ACT_RELU, k_split=True, in_scales=None):
    """The deformable convolutions of up to four same-shape layers as ONE launch (+ one reduction on K-split maps;
    cf_dcn_v2_f16x3_grouped).  xs: (B,H,W,C) tensors (two groups may share one); offmask (G,B,H,W,S>=27); -> (G,B,H,W,N).
    in_scales: one activation pre-scale per group (None = 16 each)."""
    _need_cuda(*xs, offmask)
    B, H, W, _ = xs[0].shape
    G, pd = len(xs), pds[0]
    out = torch.empty((G, B, H, W, pd.n), device=xs[0].device, dtype=torch.float32)
    ws = None
    if k_split:
        nbytes = _lib.load().cf_dcn_v2_workspace_bytes(B, H, W, pd.c, pd.n_pad)
        ws = torch.empty(G * nbytes, device=xs[0].device, dtype=torch.uint8) if nbytes else None
    blocks = [dcn_args(p_, x, offmask[g], offmask.shape[-1], B, H, W, out[g], pd.n, act, False, workspace=ws,
                       in_scale=None if in_scales is None else in_scales[g])
              for g, (p_, x) in enumerate(zip(pds, xs))]
    _lib.check(_lib.load().cf_dcn_v2_f16x3_grouped(group_ptrs(blocks), G, _lib.stream_ptr()), "cf_dcn_v2_f16x3_grouped")
    return out


def conv3x3_proj_f16x3(pc: PackedConv, t, pooled, act=ACT_RELU, out=None, in_scale=None):
    """BasicBlock conv2 + the Tree's `project` of the pooled level input in ONE launch (cf_conv3x3_proj_f16x3; pc from
    packing.pack_conv_f16(proj=...)): out = act(conv3x3(t) + project(pooled) + biases).  in_scale: ONE activation pre-scale
    for both operands (None = 16)."""
    _need_cuda(t, pooled)
    assert pc.proj_k > 0, "weights packed without a projection"
    B, H, W, _ = t.shape
    if out is None:
        out = torch.empty((B, H, W, pc.n), device=t.device, dtype=torch.float32)
    a = conv_args(pc, [t, pooled], [t.shape[-1], pooled.shape[-1]], B, H, W, out, out.shape[-1], act, None, 0,
                  LAYOUT_NHWC, None, 0, False, in_scale=in_scale)
    ch = (C.c_int32 * 2)(*[int(c) for c in pc.real_cin])
    _lib.check(_lib.load().cf_conv3x3_proj_f16x3(C.byref(a), ch, _lib.stream_ptr()), "cf_conv3x3_proj_f16x3")
    return out


def conv3x3_root_f16x3(pc2: PackedConv, pc_root: PackedConv, t, x1, children=(), act_root=ACT_RELU, x2_out=None,
                       in_scale=None, root_in_scale=None):
    """One-level Tree tail: x2 = ReLU(conv3x3(t) + x1), out = act(Root([x2, x1, *children])) as ONE launch where the shape
    allows (cf_conv3x3_root_f16x3), the two launches otherwise - same bits.  -> (out, x2 buffer: written only on the fallback).
    in_scale / root_in_scale: the activation pre-scales of conv2's input and of the Root's operands (None = 16)."""
    _need_cuda(t, x1, *children)
    B, H, W, _ = t.shape
    x2 = torch.empty((B, H, W, pc2.n), device=t.device, dtype=torch.float32) if x2_out is None else x2_out
    out = torch.empty((B, H, W, pc_root.n), device=t.device, dtype=torch.float32)
    a = conv_args(pc2, [t], [t.shape[-1]], B, H, W, x2, x2.shape[-1], ACT_RELU, x1, x1.shape[-1], LAYOUT_NHWC, None, 0, False,
                  in_scale=in_scale)
    srcs = [x2, x1, *children]
    r = conv_args(pc_root, srcs, [s.shape[-1] for s in srcs], B, H, W, out, out.shape[-1], act_root, None, 0,
                  LAYOUT_NHWC, None, 0, False, in_scale=root_in_scale)
    ch = (C.c_int32 * len(srcs))(*[int(c) for c in pc_root.real_cin])
    _lib.check(_lib.load().cf_conv3x3_root_f16x3(C.byref(a), C.byref(r), ch, _lib.stream_ptr()), "cf_conv3x3_root_f16x3")
    return out, x2


def run_conv(a: _lib.ConvArgs):
    _lib.check(_lib.load().cf_conv2d_fused(C.byref(a), _lib.stream_ptr()), "cf_conv2d_fused")


def conv2d_fused(pc: PackedConv, srcs, B, H, W, act=ACT_NONE, residual=None, layout=LAYOUT_NHWC,
                 out=None, out2=None, precise=True):
    """Convenience form: allocates the output.  srcs: NHWC tensors (B,H,W,Ci)."""
    _need_cuda(*srcs, residual)
    Ho = (H + 2 * pc.pad - pc.kh) // pc.stride + 1
    Wo = (W + 2 * pc.pad - pc.kh) // pc.stride + 1
    dev = srcs[0].device
    if out is None:
        shape = (B, Ho, Wo, pc.n) if layout == LAYOUT_NHWC else (B, pc.n, Ho, Wo)
        out = torch.empty(shape, device=dev, dtype=torch.float32)
    if act == ACT_RAW_AND_SIGDEPTH and out2 is None:
        out2 = torch.empty_like(out)
    a = conv_args(pc, srcs, [s.shape[-1] for s in srcs], B, H, W, out, pc.n, act, residual,
                  residual.shape[-1] if residual is not None else 0, layout, out2, 0, precise)
    run_conv(a)
    return (out, out2) if act == ACT_RAW_AND_SIGDEPTH else out


def split_bf16(x, channels=None, cs=None, out=None):
    """fp32 NHWC (B,H,W,S) -> split-bf16 (B,H,W,2,Cs) stored as a bf16 tensor."""
    _need_cuda(x)
    B, H, W, S = x.shape
    Cc = channels or S
    Cs = cs or ((Cc + 7) // 8) * 8
    if out is None:
        out = torch.empty((B, H, W, 2, Cs), device=x.device, dtype=torch.bfloat16)
    _lib.check(_lib.load().cf_split_bf16(x.data_ptr(), out.data_ptr(), B * H * W, Cc, S, Cs,
                                         _lib.stream_ptr()), "cf_split_bf16")
    return out


def head_tail_args(x, x_stride, B, H, W, heads):
    """The `tail` member of cf_head_fused's argument block (head_fused_args builds the whole block; x / x_stride / c_base are
    not read by the launch).  heads: list of dicts {c_base, w_hidden:[frag tensors], b_hidden:[f32 tensors], w_out, b_out,
    n_out, act, out (NCHW tensor or None), out2}.  Outputs may be patched later (a.out[i] = ptr)."""
    a = _lib.HeadTailArgs()
    a.x, a.x_stride, a.B, a.H, a.W = x.data_ptr(), x_stride, B, H, W
    a.n_heads = len(heads)
    a.n_hidden = len(heads[0]["w_hidden"])
    for i, hd in enumerate(heads):
        assert len(hd["w_hidden"]) == a.n_hidden
        for l, (w, b) in enumerate(zip(hd["w_hidden"], hd["b_hidden"])):
            a.w_hidden[i][l], a.b_hidden[i][l] = w.data_ptr(), b.data_ptr()
        a.w_out[i], a.b_out[i] = hd["w_out"].data_ptr(), hd["b_out"].data_ptr()
        a.out[i] = _lib.ptr(hd.get("out"))
        a.out2[i] = _lib.ptr(hd.get("out2"))
        a.c_base[i], a.n_out[i], a.act[i] = hd["c_base"], hd["n_out"], hd["act"]
    return a


def head_fused_args(srcs, src_strides, slots, k_pad, B, H, W, heads, layout3x3=None):
    """heads: as head_tail_args plus w_first (16x16x32 fragments [16][K_pad/32]..., or the mx operand stream), b_first (256 f32),
    w_out_perm and mfma16.  layout3x3 (default: every head carries w_out_perm): the slots are pack_conv_bf16's canonical order
    for [feat 64 (, pc_hm 8)] sources - what the 2-D patch kernel implies.  cf_head_fused runs layout3x3 = 1 with mfma16 = 1
    only and refuses every other form."""
    f = _lib.HeadFusedArgs()
    t = head_tail_args(srcs[0], 256, B, H, W, [dict(hd, c_base=0) for hd in heads])
    C.memmove(C.byref(f.tail), C.byref(t), C.sizeof(t))
    for i, (s, c) in enumerate(zip(srcs, src_strides)):
        f.src[i], f.src_c[i] = s.data_ptr(), c
    f.n_src = len(srcs)
    f.slots, f.K_pad = (slots.data_ptr() if slots is not None else None), int(k_pad or 0)   # (mx: no slot table)
    for i, hd in enumerate(heads):
        f.w_first[i], f.b_first[i] = hd["w_first"].data_ptr(), hd["b_first"].data_ptr()
        if hd.get("w_out_perm") is not None:
            f.w_out_perm[i] = hd["w_out_perm"].data_ptr()
    f.layout3x3 = int(all(hd.get("w_out_perm") is not None for hd in heads)) if layout3x3 is None else int(layout3x3)
    f.mfma16 = int(all(bool(hd.get("mfma16")) for hd in heads))     # fragments packed for the 16x16x32 shape
    f.mx = int(all(hd.get("first_scale") is not None for hd in heads))   # packing.pack_head_first_mx streams: srcs[0] = mx rows
    if f.mx:
        for i, hd in enumerate(heads):
            f.first_scale[i] = float(hd["first_scale"])
    return f


def pack_feat_mx(feat, out=None, scale=None):
    """feat (..., C >= 64) fp32 NHWC (the first 64 channels are the feature map) -> (..., 272) uint8 rows for
    cf_head_fused with mx = 1 (include/cf_hip.h: cf_pack_feat_mx; scale: the rows' power-of-two pre-scale, None = 16)."""
    _need_cuda(feat)
    assert feat.dtype == torch.float32 and feat.is_contiguous() and feat.shape[-1] >= 64
    M = feat.numel() // feat.shape[-1]
    if out is None:
        out = torch.empty(feat.shape[:-1] + (packing_MX_ROW,), device=feat.device, dtype=torch.uint8)
    _lib.check(_lib.load().cf_pack_feat_mx_scaled(feat.data_ptr(), feat.shape[-1], out.data_ptr(), M,
                                                  float(scale or DEFAULT_IN_SCALE), _lib.stream_ptr()), "cf_pack_feat_mx")
    return out


def run_head_fused(f, tile=None, pc_skip=None):
    """tile = 0 (8 x 16) / 1 (16 x 8), pc_skip = 0 / 1: force that choice of the launcher's (tests and measurement tools; the
    bits depend on neither); None: the launcher's own."""
    if tile is None and pc_skip is None:
        return _lib.check(_lib.load().cf_head_fused(C.byref(f), _lib.stream_ptr()), "cf_head_fused")
    force = lambda v: -1 if v is None else int(v)
    _lib.check(_lib.load().cf_head_fused_with(C.byref(f), force(tile), force(pc_skip), _lib.stream_ptr()), "cf_head_fused_with")


def dcn_args(pd: PackedDcn, x, offmask, om_stride, B, H, W, out, out_stride, act=ACT_RELU,
             precise=True, out_split=None, workspace=None, out_mx=None, in_scale=None, mx_scale=None):
    """in_scale: the activation pre-scale of `x` (f16x3 kernel; None = 16); mx_scale: the pre-scale of the out_mx rows."""
    a = _lib.DcnArgs()
    a.x, a.offmask, a.om_stride = x.data_ptr(), offmask.data_ptr(), om_stride
    a.B, a.H, a.W, a.C = B, H, W, pd.c
    a.weight, a.bias, a.N, a.N_pad = pd.weight.data_ptr(), pd.bias.data_ptr(), pd.n, pd.n_pad
    a.out, a.out_stride, a.act = out.data_ptr(), out_stride, act
    a.precise = int(bool(precise))
    a.out_scale = float(getattr(pd, "out_scale", 0.0))
    if in_scale is not None and float(in_scale) != DEFAULT_IN_SCALE:
        a.in_scale = float(in_scale)
        a.out_scale = _scaled_out_scale(a.out_scale, in_scale, "dcn_args")
    if mx_scale is not None and float(mx_scale) != DEFAULT_IN_SCALE:
        a.mx_scale = float(mx_scale)
    if out_split is not None:            # (B,H,W,2,Cs) bf16: split copy for the head kernels (f16x3 kernel only)
        a.out_split_bf16, a.split_stride = out_split.data_ptr(), out_split.shape[-1]
    if out_mx is not None:               # (B,H,W,272) uint8: the mx rows of the heads' first layer (f16x3 kernel, N = 64)
        a.out_mx = out_mx.data_ptr()
    if workspace is not None:            # K split on small maps (cf_dcn_v2_workspace_bytes)
        a.workspace = workspace.data_ptr()
        a.workspace_bytes = workspace.numel() * workspace.element_size()
    return a


def run_dcn(a: _lib.DcnArgs):
    fn = _lib.load().cf_dcn_v2_f16x3 if a.out_scale > 0 else _lib.load().cf_dcn_v2_fused
    _lib.check(fn(C.byref(a), _lib.stream_ptr()), "cf_dcn_v2")


def dcn_v2_fused(pd: PackedDcn, x, offmask, act=ACT_RELU, precise=True, k_split=True, in_scale=None):
    """x (B,H,W,C) NHWC, offmask (B,H,W,S>=27) NHWC raw conv_offset_mask output.  in_scale (f16x3 packing): the activation
    pre-scale (None = 16)."""
    _need_cuda(x, offmask)
    B, H, W, _ = x.shape
    out = torch.empty((B, H, W, pd.n), device=x.device, dtype=torch.float32)
    ws = None
    if k_split and getattr(pd, "out_scale", 0.0) > 0:
        nbytes = _lib.load().cf_dcn_v2_workspace_bytes(B, H, W, pd.c, pd.n_pad)
        ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8) if nbytes else None
    a = dcn_args(pd, x, offmask, offmask.shape[-1], B, H, W, out, pd.n, act, precise, workspace=ws, in_scale=in_scale)
    run_dcn(a)
    return out


def nchw_to_nhwc(x, out=None, out_offset=0):
    """(B,C,H,W) fp32 -> (B,H,W,S) NHWC, written at channel `out_offset` of `out` (default: a fresh (B,H,W,C))."""
    _need_cuda(x, out)
    B, Cc, H, W = x.shape
    if out is None:
        out = torch.empty((B, H, W, Cc), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().cf_nchw_to_nhwc(x.data_ptr(), out.data_ptr(), B, Cc, H, W, out.shape[-1], out_offset,
                                           _lib.stream_ptr()), "cf_nchw_to_nhwc")
    return out


_DCN_PACKS = {}       # id(weight) -> (weakref to weight, weight stamp, weakref to bias or None, bias stamp, PackedDcn)
_DCN_PACK_KEYS = 64   # LRU bound
_DCN_PACK_LOCK = __import__("threading").Lock()   # (the operator may be called from several host threads)
_DCN_PACK_VERIFY = True


def set_dcn_pack_verify(on=True):
    """`deform_conv2d` keeps the packed form of each weight it has seen.  An in-place write through `weight.data`
    (`w.data.copy_()`, an EMA swap, a hand-written checkpoint load) bumps no version counter autograd can see, so with
    verification ON (the default) every call also compares a 64-bit checksum of the live weight and bias bits with the one
    taken when the entry was packed - one small reduction and one device->host scalar per call.  Turn it off for a serving
    loop whose weights are frozen (and call `clear_dcn_pack_cache()` after any manual write).  -> previous setting."""
    global _DCN_PACK_VERIFY
    prev, _DCN_PACK_VERIFY = _DCN_PACK_VERIFY, bool(on)
    return prev


_DCN_RANGE_CHECK = True


def set_dcn_range_check(on=True):
    """`deform_conv2d` evaluates its products from fp16-split operands after a power-of-two pre-scale of the input (16 by
    default: |input| up to 4094).  With the check ON (the default) every call measures max |input| (cf_absmax_f32, one
    device->host scalar) and picks the pre-scale for it, so any finite fp32 input is accepted as torchvision's operator
    accepts it; a NaN / inf input raises.  OFF: the default pre-scale, no sync - inputs beyond 4094 are then CLAMPED silently;
    only for callers that know their range.  Inside a stream capture the check cannot run (no sync): default pre-scale.
    -> previous setting."""
    global _DCN_RANGE_CHECK
    prev, _DCN_RANGE_CHECK = _DCN_RANGE_CHECK, bool(on)
    return prev


def clear_dcn_pack_cache():
    """Drop every packed weight `deform_conv2d` holds (they are rebuilt on the next call)."""
    with _DCN_PACK_LOCK:
        _DCN_PACKS.clear()


def _stamp(t):
    """what autograd and the allocator can tell about a tensor's contents without reading them"""
    return (t._version, t.data_ptr(), tuple(t.shape), t.dtype)


def _checksum(weight, bias):
    """64-bit sum of the raw bits (order-independent, exact: integer arithmetic) - a device scalar."""
    def bits(t):
        t = t.detach().contiguous()
        return t.view(torch.int32 if t.element_size() == 4 else torch.int16 if t.element_size() == 2 else torch.int64)
    c = bits(weight).sum(dtype=torch.int64)
    if bias is not None:
        c = c * 1000003 + bits(bias).sum(dtype=torch.int64)
    return c


def _packed_dcn(weight, bias, pack=None, verify=True):
    """Pack (split fp16 hi / lo, MFMA fragment order: packing.pack_dcn_f16) ONCE per weight tensor OBJECT and content -
    the reference calls the operator with the same nn.Parameter every forward (dla.py:464-465).  The entry holds weak
    references and is valid only while they still point at the very tensors passed in (a data pointer or an id() alone
    can be reused by another tensor after the first one is freed), their version counter, data pointer, shape and dtype
    are unchanged, and - `set_dcn_pack_verify` - their bits still add up to the checksum taken at packing time.
    `pack` (default packing.pack_dcn_f16): the packer of another layer kind that lives in the same cache - the offset
    convolution of `deform_conv_block` (a weight tensor is one layer's, so the key stays the weight).  verify=False: this call
    trusts the version counters (DLASeg's own nn.Parameters, which only optimizers and load_state_dict write): no checksum, no sync."""
    import weakref
    from . import packing
    with _DCN_PACK_LOCK:
        return _packed_dcn_locked(weight, bias, weakref, packing, pack, verify)


def _packed_dcn_locked(weight, bias, weakref, packing, pack=None, verify=True):
    key = id(weight)
    e = _DCN_PACKS.pop(key, None)
    verify = verify and _DCN_PACK_VERIFY and weight.is_cuda and not torch.cuda.is_current_stream_capturing()
    csum = None
    if e is not None:
        wref, wst, bref, bst, pd, csum0 = e
        same_bias = (bref is None) if bias is None else (bref is not None and bref() is bias and bst == _stamp(bias))
        if not (wref() is weight and wst == _stamp(weight) and same_bias and pd.weight.device == weight.device):
            e = None
        elif verify:
            csum = int(_checksum(weight, bias).item())
            if csum0 is None:
                e = (wref, wst, bref, bst, pd, csum)      # packed during a capture: the checksum is taken now
            elif csum != csum0:
                e = None
    if e is None:
        w = weight.detach().float().cpu()
        b = torch.zeros(w.shape[0]) if bias is None else bias.detach().float().cpu()
        pd = (pack or packing.pack_dcn_f16)(w, b).to(weight.device)
        if verify and csum is None:
            csum = int(_checksum(weight, bias).item())
        e = (weakref.ref(weight), _stamp(weight), None if bias is None else weakref.ref(bias),
             None if bias is None else _stamp(bias), pd, csum if verify else None)
    for k in [k for k, v in _DCN_PACKS.items() if v[0]() is None]:
        del _DCN_PACKS[k]                         # weights that no longer exist: free their packed copies now
    _DCN_PACKS[key] = e                           # re-inserted last: dict order is the LRU order
    while len(_DCN_PACKS) > _DCN_PACK_KEYS:
        _DCN_PACKS.pop(next(iter(_DCN_PACKS)))
    return e[4]


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(e) for e in v)


def _deform_conv2d_forward(input, offset, weight, bias, mask):
    """The forward launches of `deform_conv2d` (arguments already checked) -> (out NCHW, x NHWC, offmask NHWC)."""
    B, Cin, H, W = input.shape
    dev = input.device
    pd = _packed_dcn(weight, bias)
    x = nchw_to_nhwc(input.float().contiguous())
    om = torch.empty((B, H, W, 32), device=dev, dtype=torch.float32)
    nchw_to_nhwc(offset.float().contiguous(), om, 0)
    if mask is None:
        om[..., 18:27] = 1.0
    else:
        nchw_to_nhwc(mask.float().contiguous(), om, 18)
    out = torch.empty((B, H, W, pd.n_pad), device=dev, dtype=torch.float32)     # (any Cout: the row stride is N_pad)
    nbytes = _lib.load().cf_dcn_v2_workspace_bytes(B, H, W, pd.c, pd.n_pad)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
    in_scale = None
    if _DCN_RANGE_CHECK and not torch.cuda.is_current_stream_capturing():
        in_scale = in_scale_for(float(absmax(x).item()))          # (raises on NaN / inf)
    a = dcn_args(pd, x, om, 32, B, H, W, out, pd.n_pad, ACT_NONE, precise=True, workspace=ws, in_scale=in_scale)
    a.mask_activated = 1
    run_dcn(a)
    return nhwc_to_nchw(out, channels=pd.n), x, om


def dcn_bwd_args(gout, x, offmask, weight=None, gx=None, gom=None, gw=None, gbias=None, workspace=None) -> _lib.DcnBwdArgs:
    """The argument block of cf_dcn_v2_bwd_data / cf_dcn_v2_bwd_weight: gout (B,H,W,N), x (B,H,W,C), offmask (B,H,W,32 - the
    mask ACTIVATED), all fp32 NHWC; weight: the raw (N,C,3,3); gx must arrive zeroed."""
    _need_cuda(gout, x, offmask, weight, gx, gom, gw, gbias, workspace)
    for t in (gout, x, offmask, weight, gx, gom, gw, gbias):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.CfHipError("dcn backward: contiguous float32 tensors only")
    a = _lib.DcnBwdArgs()
    a.B, a.H, a.W, a.C = x.shape
    a.N = gout.shape[-1]
    if tuple(gout.shape[:3]) != tuple(x.shape[:3]) or tuple(offmask.shape) != tuple(x.shape[:3]) + (32,):
        raise _lib.CfHipError("dcn backward: gout / x / offmask disagree in shape")
    a.gout, a.x, a.offmask, a.weight = gout.data_ptr(), x.data_ptr(), offmask.data_ptr(), _lib.ptr(weight)
    a.gx, a.gom, a.gw, a.gbias = _lib.ptr(gx), _lib.ptr(gom), _lib.ptr(gw), _lib.ptr(gbias)
    if workspace is not None:
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    return a


def run_dcn_bwd_data(a: _lib.DcnBwdArgs):
    """gx (float atomics) and gom of the deformable convolution (cf_dcn_v2_bwd_data)."""
    _lib.check(_lib.load().cf_dcn_v2_bwd_data(C.byref(a), _lib.stream_ptr()), "cf_dcn_v2_bwd_data")


def run_dcn_bwd_weight(a: _lib.DcnBwdArgs):
    """gw and gbias of the deformable convolution, slab-reduced in a fixed order (cf_dcn_v2_bwd_weight)."""
    _lib.check(_lib.load().cf_dcn_v2_bwd_weight(C.byref(a), _lib.stream_ptr()), "cf_dcn_v2_bwd_weight")


class _DeformConv2dFn(torch.autograd.Function):
    """`deform_conv2d` under autograd: the forward's launches, the NHWC input / offset-mask buffers they built and the raw
    weight saved; backward on cf_dcn_v2_bwd_data / cf_dcn_v2_bwd_weight, only what `needs_input_grad` asks for."""

    @staticmethod
    def forward(ctx, input, offset, weight, bias, mask):
        out, x, om = _deform_conv2d_forward(input, offset, weight, bias, mask)
        w = weight.detach()
        ctx.save_for_backward(x, om, w if w.dtype == torch.float32 and w.is_contiguous() else w.float().contiguous())
        ctx.dtypes = tuple(None if t is None else t.dtype for t in (input, offset, weight, bias, mask))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        x, om, w = ctx.saved_tensors
        need_x, need_off, need_w, need_b, need_m = ctx.needs_input_grad
        B, H, W, Cin = x.shape
        dev = x.device
        gout = nchw_to_nhwc(grad_output.float().contiguous())
        gx = gom = gw = gb = None
        if need_x or need_off or need_m:
            gx = torch.zeros((B, H, W, Cin), device=dev, dtype=torch.float32) if need_x else None
            gom = torch.empty((B, H, W, 32), device=dev, dtype=torch.float32) if (need_off or need_m) else None
            run_dcn_bwd_data(dcn_bwd_args(gout, x, om, weight=w, gx=gx, gom=gom))
        if need_w or need_b:
            gw = torch.empty_like(w) if need_w else None
            gb = torch.empty(w.shape[0], device=dev, dtype=torch.float32) if need_b else None
            nbytes = _lib.load().cf_dcn_v2_bwd_workspace_bytes(B, H, W, Cin, w.shape[0])
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            run_dcn_bwd_weight(dcn_bwd_args(gout, x, om, gw=gw, gbias=gb, workspace=ws))

        def om_channels(first, n):            # channels first .. first + n of gom as an NCHW map
            res = torch.empty((B, n, H, W), device=dev, dtype=torch.float32)
            _lib.check(_lib.load().cf_nhwc_to_nchw(gom.data_ptr() + 4 * first, res.data_ptr(), B, H, W, n, 32,
                                                   _lib.stream_ptr()), "cf_nhwc_to_nchw")
            return res
        cast = lambda g, i: g if g is None or ctx.dtypes[i] == torch.float32 else g.to(ctx.dtypes[i])
        return (cast(nhwc_to_nchw(gx) if need_x else None, 0), cast(om_channels(0, 18) if need_off else None, 1),
                cast(gw, 2), cast(gb, 3), cast(om_channels(18, 9) if need_m else None, 4))


def deform_conv2d(input, offset, weight, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), mask=None):
    """Operator-level drop-in for `torchvision.ops.deform_conv2d` as the reference calls it
    (model/networks/dla.py:461-470) - same signature, same semantics: `input` (B,Cin,H,W),
    `offset` (B,18,H,W) with channel 2k = dy and 2k+1 = dx of tap k = 3i+j, `mask` (B,9,H,W) ALREADY activated (the
    caller's sigmoid; None = unmodulated DCNv1), raw `weight` (Cout,Cin,3,3) and `bias` (Cout) -> (B,Cout,H,W), all
    NCHW fp32 on the device.  `torchvision.ops.deform_conv2d = centerfusiondetect3d_amd.ops.deform_conv2d` lets the
    reference's own `DeformConv` module run on the HIP kernel unchanged.

    What runs: three layout launches (cf_nchw_to_nhwc: input, offset, mask -> the NHWC buffers the kernel reads),
    cf_dcn_v2_f16x3 with `mask_activated`, cf_nhwc_to_nchw.  The module path (DLASeg) never takes this route: there
    the maps stay NHWC and the mask logits go in raw.  Only the configuration the reference uses is implemented -
    3x3, stride 1, padding 1, dilation 1, one group, one offset group, Cin a multiple of 32; anything else raises
    NotImplementedError (no fallback).

    Autograd: the operator is differentiable in all five tensor arguments (input, offset, weight, bias, mask), once
    (no double backward), fp32 only (no autocast).  With grad mode on and at least one of them requiring grad the same
    launches run inside a `torch.autograd.Function` that keeps the NHWC input and offset-mask buffers and the raw weight;
    backward runs cf_dcn_v2_bwd_data (input, offset, mask) and cf_dcn_v2_bwd_weight (weight, bias), each only when
    `needs_input_grad` asks for one of its outputs, on the exact fp32-input MFMA.  The input gradient is summed with float
    atomics and can differ in the last bits from run to run; the weight and bias gradients are slab sums added in a
    fixed order and cannot.  At an integer sampling position the offset gradient is the right-hand derivative, as
    torchvision's is.  The range check and the packed-weight cache behave as in inference: an optimizer's in-place step
    bumps the weight's version, so the next forward packs it again.  Otherwise (no_grad, nothing requiring grad) the
    inference path runs as it always did and the result carries no grad_fn.  The module path (`DLASeg`) does not come
    through here: it trains its heads through `head_stack` and, after `unfreeze_neck`, its neck through `deform_conv_block`,
    which shares this operator's backward kernels and stays NHWC."""
    _need_cuda(input, offset, weight, bias, mask)
    if input.dim() != 4 or weight.dim() != 4:
        raise ValueError("deform_conv2d: input must be (B,Cin,H,W) and weight (Cout,Cin,kh,kw)")
    B, Cin, H, W = input.shape
    Cout, Cw, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or _pair(stride) != (1, 1) or _pair(padding) != (1, 1) or _pair(dilation) != (1, 1):
        raise NotImplementedError("deform_conv2d on the HIP path: 3x3, stride 1, padding 1, dilation 1 only "
                                  "(the one configuration of dla.py:385-472)")
    if Cw != Cin:
        raise NotImplementedError("deform_conv2d on the HIP path: groups == 1 only")
    if Cin % 32:
        raise NotImplementedError(f"deform_conv2d on the HIP path: Cin={Cin} must be a multiple of 32")
    if tuple(offset.shape) != (B, 18, H, W):
        if offset.dim() == 4 and offset.shape[1] % 18 == 0 and offset.shape[1] > 18:
            raise NotImplementedError("deform_conv2d on the HIP path: one offset group only")
        raise ValueError(f"deform_conv2d: offset must be {(B, 18, H, W)}, got {tuple(offset.shape)}")
    if mask is not None and tuple(mask.shape) != (B, 9, H, W):
        raise ValueError(f"deform_conv2d: mask must be {(B, 9, H, W)}, got {tuple(mask.shape)}")
    if bias is not None and tuple(bias.shape) != (Cout,):
        raise ValueError(f"deform_conv2d: bias must be ({Cout},), got {tuple(bias.shape)}")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (input, offset, weight, bias, mask)):
        return _DeformConv2dFn.apply(input, offset, weight, bias, mask)
    return _deform_conv2d_forward(input, offset, weight, bias, mask)[0]


# ---- the criterion (cf_loss_forward / cf_loss_backward) ----
LOSS_L1, LOSS_L1_UNC, LOSS_BINROT, LOSS_BCE = _lib.LOSS_L1, _lib.LOSS_L1_UNC, _lib.LOSS_BINROT, _lib.LOSS_BCE


def _loss_tensor(t, what, dtype, shape):
    _need_cuda(t)
    if t.dtype != dtype:
        raise _lib.CfHipError(f"generic_loss: {what} must be {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise _lib.CfHipError(f"generic_loss: {what} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t.detach().contiguous()


def _loss_map(t, what, shape):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise NotImplementedError(f"generic_loss: {what} must be a float32 map (no autocast, no fp16 / bf16 / float64)")
    return _loss_tensor(t, what, torch.float32, shape)


def _loss_forward(spec, tensors):
    """tensors: [heat, map_0 .. map_{n-1}, unc | None, heat_gt, centers, wh, mask, cls, (target_i, aux_i | None) ...] ->
    the argument block (outputs allocated, gradients unset) and what keeps its pointers alive"""
    n = len(spec["kinds"])
    heat, maps, unc = tensors[0], tensors[1:1 + n], tensors[1 + n]
    heat_gt, centers, wh, mask, cls = tensors[2 + n:7 + n]
    rest = tensors[7 + n:]
    if heat.dim() != 4:
        raise _lib.CfHipError("generic_loss: heatmap must be (B,C,h,w)")
    if n > _lib.CF_LOSS_MAX_HEADS:
        raise _lib.CfHipError(f"generic_loss: at most {_lib.CF_LOSS_MAX_HEADS} heads")
    B, Cc, h, w = heat.shape
    if centers.dim() != 3:
        raise _lib.CfHipError("generic_loss: heatCenters must be (B,M,2)")
    M = centers.shape[1]
    keep = [_loss_map(heat, "heatmap", (B, Cc, h, w)), _loss_tensor(heat_gt, "heatmap target", torch.float32, (B, Cc, h, w)),
            _loss_tensor(centers, "heatCenters", torch.float32, (B, M, 2)), _loss_tensor(wh, "widthHeight", torch.float32, (B, M, 2)),
            _loss_tensor(mask, "mask", torch.float32, (B, M)), _loss_tensor(cls, "classIds", torch.int64, (B, M))]
    a = _lib.LossArgs()
    a.heat, a.heat_gt, a.centers, a.wh, a.mask, a.cls = (t.data_ptr() for t in keep)
    a.B, a.C, a.h, a.w, a.M, a.n_heads = B, Cc, h, w, M, n
    a.out_area, a.heat_weight = float(spec["out_area"]), float(spec["heat_weight"])
    uncc = None if unc is None else _loss_map(unc, "uncertainty", (B, 1, h, w))
    keep.append(uncc)
    for i, (kind, weight) in enumerate(zip(spec["kinds"], spec["weights"])):
        H = a.head[i]
        if maps[i].dim() != 4:
            raise _lib.CfHipError(f"generic_loss: head {i} must be (B,C,h,w)")
        ch = maps[i].shape[1]
        m = _loss_map(maps[i], f"head {i}", (B, ch, h, w))
        target, aux = rest[2 * i], rest[2 * i + 1]
        t = _loss_tensor(target, f"head {i} target", torch.float32, (B, M, 2 if kind == LOSS_BINROT else ch))
        keep += [m, t]
        H.kind, H.channels, H.map, H.target, H.weight = kind, ch, m.data_ptr(), t.data_ptr(), float(weight)
        if kind == LOSS_BINROT:
            x = _loss_tensor(aux, f"head {i} rotbin", torch.int64, (B, M, 2))
            H.rotbin = x.data_ptr()
            keep.append(x)
        elif kind == LOSS_BCE:
            x = _loss_tensor(aux, f"head {i} mask", torch.float32, (B, M, ch))
            H.mask = x.data_ptr()
            keep.append(x)
        elif kind == LOSS_L1_UNC:
            if uncc is None:
                raise _lib.CfHipError("generic_loss: an L1_UNC head needs the uncertainty map")
            H.unc = uncc.data_ptr()
        elif kind != LOSS_L1:
            raise _lib.CfHipError(f"generic_loss: unknown head kind {kind}")
    return a, keep


def _loss_run_forward(spec, tensors):
    a, keep = _loss_forward(spec, tensors)
    dev = tensors[0].device
    n = a.n_heads
    vec = torch.empty(n + 3, device=dev, dtype=torch.float32)
    total = torch.empty((), device=dev, dtype=torch.float32)
    stats = torch.empty(_lib.CF_LOSS_STATS, device=dev, dtype=torch.float32)
    lm = torch.empty((a.B, a.M), device=dev, dtype=torch.bool)
    nbytes = _lib.load().cf_loss_workspace_bytes(a.B, a.C, a.h, a.w)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    a.losses, a.total, a.stats, a.layer_mask = vec.data_ptr(), total.data_ptr(), stats.data_ptr(), lm.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    _lib.check(_lib.load().cf_loss_forward(C.byref(a), _lib.stream_ptr()), "cf_loss_forward")
    return total, vec, lm, stats


class _GenericLossFn(torch.autograd.Function):
    """`generic_loss` under autograd: cf_loss_forward, the maps, the targets and the `stats` block saved; backward on
    cf_loss_backward, a gradient for exactly the maps `needs_input_grad` names, scaled by the incoming gradient on the device."""

    @staticmethod
    def forward(ctx, spec, *tensors):
        total, vec, lm, stats = _loss_run_forward(spec, tensors)
        ctx.spec = spec
        ctx.save_for_backward(stats, *tensors)
        ctx.mark_non_differentiable(vec, lm)
        return total, vec, lm

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gtotal, _gvec, _glm):
        stats, *tensors = ctx.saved_tensors
        spec = ctx.spec
        n = len(spec["kinds"])
        need = ctx.needs_input_grad[1:2 + n + 1]
        a, keep = _loss_forward(spec, tensors)
        dev = stats.device
        go = gtotal.detach().to(torch.float32).contiguous()
        a.stats, a.grad_out = stats.data_ptr(), go.data_ptr()
        grads = [None] * len(tensors)
        if need[0]:
            grads[0] = torch.empty(tensors[0].shape, device=dev, dtype=torch.float32)
            a.gheat = grads[0].data_ptr()
        sparse = [i for i in range(1, n + 2) if need[i] and tensors[i] is not None]
        if sparse:     # one zero fill for every scattered gradient (each slice starts on a multiple of four floats)
            sizes = [(tensors[i].numel() + 3) // 4 * 4 for i in sparse]
            flat = torch.zeros(sum(sizes), device=dev, dtype=torch.float32)
            at = 0
            for i, sz in zip(sparse, sizes):
                grads[i] = flat[at:at + tensors[i].numel()].view(tensors[i].shape)
                at += sz
            for i in range(n):
                if grads[1 + i] is not None:
                    a.head[i].gmap = grads[1 + i].data_ptr()
                if grads[1 + n] is not None and spec["kinds"][i] == LOSS_L1_UNC:
                    a.head[i].gunc = grads[1 + n].data_ptr()
        _lib.check(_lib.load().cf_loss_backward(C.byref(a), _lib.stream_ptr()), "cf_loss_backward")
        return (None, *grads)


def generic_loss(heat, heat_gt, centers, wh, mask, cls, heads, heat_weight=1.0, out_area=None, uncertainty=None):
    """The reference's GenericLoss over one output layer on already-collected tensors (cf_loss_forward; semantics:
    include/cf_hip.h).  `heat` (B,C,h,w): the probabilities; `heat_gt` its target; `centers` (B,M,2) f32 (x, y);
    `wh` (B,M,2) f32 (its product is the layer mask); `mask` (B,M) f32; `cls` (B,M) i64.  `heads`: a list, in the order
    their terms enter the total, of (kind, map, target, aux, weight) with kind LOSS_L1 (aux None), LOSS_L1_UNC (aux None;
    `uncertainty` (B,1,h,w) is the map both depth heads share), LOSS_BINROT (target = rotres, aux = rotbin i64) or
    LOSS_BCE (aux = the (B,M,C) mask).  `out_area` defaults to h*w.

    -> (total, vec, layer_mask): `total` a 0-d tensor, `vec` = [heat-map term, one value per head, total, 0.0] (never
    carries a grad_fn), `layer_mask` (B,M) bool.  Two launches, no host sync, bitwise reproducible values; capturable in a
    HIP graph.  With grad mode on and a map requiring grad, `total` carries a grad_fn (once differentiable); backward is
    cf_loss_backward: a dense pass for `heat`, float atomic adds into zero-filled maps for the heads, only for the maps
    that require a gradient.  Device fp32 tensors only: a CPU tensor raises CfHipError, a non-fp32 map NotImplementedError."""
    kinds, weights = [int(hd[0]) for hd in heads], [float(hd[4]) for hd in heads]
    maps = [hd[1] for hd in heads]
    spec = {"kinds": kinds, "weights": weights, "heat_weight": float(heat_weight),
            "out_area": float(out_area if out_area is not None else heat.shape[-2] * heat.shape[-1])}
    tensors = [heat, *maps, uncertainty, heat_gt, centers, wh, mask, cls]
    for hd in heads:
        tensors += [hd[2], hd[3]]
    for t in [heat, *maps, uncertainty]:
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32):
            raise NotImplementedError("generic_loss: float32 maps only (no autocast, no fp16 / bf16 / float64)")
    _need_cuda(*[t for t in tensors if torch.is_tensor(t)])
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [heat, *maps, uncertainty]):
        return _GenericLossFn.apply(spec, *tensors)
    with torch.no_grad():
        return _loss_run_forward(spec, tensors)[:3]


# ---- one detection head under autograd (cf_head_train_forward / cf_head_backward / cf_head_backward_dx) ----
HEAD_HIDDEN = 256          # width of every hidden map the training kernels implement
HEAD_MAX_OUT = 16          # outputs of a head's last layer
HEAD_MAX_HIDDEN = _lib.CF_HEAD_TRAIN_MAX_HIDDEN   # 1x1 hidden layers behind the 3x3
HEAD_FINALS = (None, "heatmap", "depth")


def _head_check(x, x2, weights, biases, final):
    """Shapes / dtypes of a head_stack call (no device needed) -> (Cin of x, Cin of x2, n_hidden, n_out)."""
    if final not in HEAD_FINALS:
        raise ValueError(f"head_stack: final must be one of {HEAD_FINALS}, got {final!r}")
    weights, biases = list(weights), list(biases)
    if len(weights) != len(biases) or not 2 <= len(weights) <= HEAD_MAX_HIDDEN + 2:
        raise NotImplementedError(f"head_stack: a 3x3 layer, 0..{HEAD_MAX_HIDDEN} hidden 1x1 layers and an output layer "
                                  f"(2..{HEAD_MAX_HIDDEN + 2} weights with their biases), got {len(weights)} / {len(biases)}")
    for t in (x, x2, *weights, *biases):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32):
            raise NotImplementedError("head_stack: float32 tensors only (no autocast, no fp16 / bf16 / float64)")
    if x.dim() != 4 or (x2 is not None and (x2.dim() != 4 or x2.shape[0] != x.shape[0] or x2.shape[2:] != x.shape[2:])):
        raise ValueError("head_stack: x must be (B,Cin,h,w) and the second source (B,C2,h,w) on the same map")
    c_x, c_x2 = x.shape[1], (0 if x2 is None else x2.shape[1])
    cin = c_x + c_x2
    if cin > 512:
        raise NotImplementedError(f"head_stack: Cin={cin} above the limit of 512")
    if tuple(weights[0].shape) != (HEAD_HIDDEN, cin, 3, 3):
        raise NotImplementedError(f"head_stack: the first layer must be a 3x3 convolution ({HEAD_HIDDEN},{cin},3,3) - hidden width "
                                  f"{HEAD_HIDDEN} only - got {tuple(weights[0].shape)}")
    for w in weights[1:-1]:
        if tuple(w.shape) != (HEAD_HIDDEN, HEAD_HIDDEN, 1, 1):
            raise NotImplementedError(f"head_stack: hidden layers must be 1x1 convolutions ({HEAD_HIDDEN},{HEAD_HIDDEN},1,1), "
                                      f"got {tuple(w.shape)}")
    n_out = weights[-1].shape[0]
    if weights[-1].dim() != 4 or tuple(weights[-1].shape[1:]) != (HEAD_HIDDEN, 1, 1) or not 1 <= n_out <= HEAD_MAX_OUT:
        raise NotImplementedError(f"head_stack: the output layer must be a 1x1 convolution (Cout,{HEAD_HIDDEN},1,1) with "
                                  f"1 <= Cout <= {HEAD_MAX_OUT}, got {tuple(weights[-1].shape)}")
    for w, b in zip(weights, biases):
        if tuple(b.shape) != (w.shape[0],):
            raise ValueError(f"head_stack: bias {tuple(b.shape)} does not fit weight {tuple(w.shape)}")
    return c_x, c_x2, len(weights) - 2, n_out


def head_train_args(xn, c_x, x2n, c_x2, weights, biases, chunk_px=0) -> _lib.HeadTrainArgs:
    """The argument block of cf_head_train_forward / cf_head_backward without outputs and workspace.  xn (B,h,w,S >= c_x) and
    x2n (B,h,w,S2 >= c_x2) or None: contiguous fp32 NHWC; weights / biases: contiguous fp32 in layer order."""
    a = _lib.HeadTrainArgs()
    a.B, a.h, a.w = xn.shape[:3]
    a.x, a.x_stride, a.c_x = xn.data_ptr(), xn.shape[-1], c_x
    if x2n is not None:
        a.x2, a.x2_stride, a.c_x2 = x2n.data_ptr(), x2n.shape[-1], c_x2
    a.n_hidden, a.hidden, a.n_out, a.chunk_px = len(weights) - 2, HEAD_HIDDEN, weights[-1].shape[0], int(chunk_px)
    for l, (w, b) in enumerate(zip(weights, biases)):
        a.weight[l], a.bias[l] = w.data_ptr(), b.data_ptr()
    return a


def _workspace(a, nbytes):
    ws = torch.empty(nbytes, device=torch.device("cuda", torch.cuda.current_device()), dtype=torch.uint8)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    return ws


class _HeadStackFn(torch.autograd.Function):
    """`head_stack` under autograd: cf_head_train_forward; the NHWC sources and the raw weights saved (no hidden map is);
    backward on cf_head_backward: every layer's weight and bias gradient, none for the sources - or, with `input_grad` and a
    source that autograd asks for, on cf_head_backward_dx: also that source's gradient, in its own (B,h,w,S) shape."""

    @staticmethod
    def forward(ctx, xn, x2n, c_x, c_x2, chunk_px, n_layers, input_grad, *params):
        weights = [p.detach().contiguous() for p in params[:n_layers]]
        biases = [p.detach().contiguous() for p in params[n_layers:]]
        B, h, w = xn.shape[:3]
        with torch.cuda.device(xn.device):
            a = head_train_args(xn, c_x, x2n, c_x2, weights, biases, chunk_px)
            y = torch.empty((B, a.n_out, h, w), device=xn.device, dtype=torch.float32)
            a.y = y.data_ptr()
            ws = _workspace(a, _lib.load().cf_head_train_workspace_bytes(B, h, w, c_x + c_x2, a.n_hidden, int(chunk_px)))
            _lib.check(_lib.load().cf_head_train_forward(C.byref(a), _lib.stream_ptr()), "cf_head_train_forward")
        ctx.meta = (c_x, c_x2, int(chunk_px), n_layers, x2n is not None, bool(input_grad))
        ctx.save_for_backward(xn, *([x2n] if x2n is not None else []), *weights, *biases)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        c_x, c_x2, chunk_px, n, has2, input_grad = ctx.meta
        saved = list(ctx.saved_tensors)
        xn = saved.pop(0)
        x2n = saved.pop(0) if has2 else None
        weights, biases = saved[:n], saved[n:]
        B, h, w = xn.shape[:3]
        gy = gy.detach().to(torch.float32).contiguous()
        with torch.cuda.device(xn.device):
            a = head_train_args(xn, c_x, x2n, c_x2, weights, biases, chunk_px)
            gws = [torch.empty_like(t) for t in weights]
            gbs = [torch.empty_like(t) for t in biases]
            for l in range(n):
                a.gw[l], a.gb[l] = gws[l].data_ptr(), gbs[l].data_ptr()
            a.gy = gy.data_ptr()
            want = input_grad and ctx.needs_input_grad[0], input_grad and has2 and ctx.needs_input_grad[1]
            gx = torch.empty_like(xn) if want[0] else None
            gx2 = torch.empty_like(x2n) if want[1] else None
            if gx is None and gx2 is None:
                ws = _workspace(a, _lib.load().cf_head_bwd_workspace_bytes(B, h, w, c_x + c_x2, a.n_hidden, chunk_px))
                _lib.check(_lib.load().cf_head_backward(C.byref(a), _lib.stream_ptr()), "cf_head_backward")
            else:
                ws = _workspace(a, _lib.load().cf_head_bwd_dx_workspace_bytes(B, h, w, c_x + c_x2, a.n_hidden, chunk_px))
                _lib.check(_lib.load().cf_head_backward_dx(C.byref(a), _lib.ptr(gx), xn.shape[-1], _lib.ptr(gx2),
                                                           0 if x2n is None else x2n.shape[-1], _lib.stream_ptr()),
                           "cf_head_backward_dx")
        need = ctx.needs_input_grad[7:]
        grads = [g if nd else None for g, nd in zip(gws + gbs, need)]
        return (gx, gx2, None, None, None, None, None, *grads)


class _NchwToNhwcFn(torch.autograd.Function):
    """`head_stack`'s layout conversion under autograd: cf_nchw_to_nhwc forward, cf_nhwc_to_nchw backward."""

    @staticmethod
    def forward(ctx, x):
        with torch.cuda.device(x.device):
            return nchw_to_nhwc(x.detach().contiguous())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        with torch.cuda.device(g.device):
            return nhwc_to_nchw(g.detach().contiguous())


def head_final(y, final):
    """The reference's output activation on a head's raw map: "heatmap" = clamp(sigmoid(y), 1e-4, 1 - 1e-4) (detectHeads.py:21-23;
    zero gradient where the clamp binds), "depth" = 1 / (sigmoid(y) + 1e-6) - 1 (model/utils.py:141).  Elementwise torch ops."""
    if final == "heatmap":
        return torch.clamp(torch.sigmoid(y), min=1e-4, max=1 - 1e-4)
    if final == "depth":
        return 1.0 / (torch.sigmoid(y) + 1e-6) - 1.0
    return y


def head_stack_nhwc(xn, c_x, x2n, c_x2, weights, biases, final=None, chunk_px=0, input_grad=False):
    """`head_stack` on sources that are already NHWC: xn (B,h,w,S) whose first c_x channels are read, x2n (B,h,w,S2) / c_x2 the
    optional second source (DLASeg's training forward: the trunk's feature map and the radar map, never concatenated).
    `input_grad=True`: a source that requires grad receives its gradient in its own (B,h,w,S) shape - the channels behind
    c_x / c_x2 exactly zero; without it the sources receive none."""
    weights, biases = list(weights), list(biases)
    y = _HeadStackFn.apply(xn, x2n, int(c_x), int(c_x2), int(chunk_px), len(weights), bool(input_grad), *weights, *biases)
    return y if final is None else (head_final(y, final), y)


def head_stack(x, weights, biases, final=None, x2=None, chunk_px=0, input_grad=False):
    """One detection head of the reference (detectHeads.py:59-98) under autograd, on HIP kernels in both directions:
    conv3x3(Cin -> 256) + bias -> ReLU -> [conv1x1(256 -> 256) + bias -> ReLU] x n -> conv1x1(256 -> Cout) + bias, n = 0 .. 2,
    Cout = 1 .. 16.  `x` (B,Cin,h,w) fp32 on the device; `x2` (B,C2,h,w): an optional second source whose channels follow x's
    (the 3 radar channels of the secondary heads - nothing is concatenated); `weights` / `biases`: the head's raw parameters in
    layer order ((256,Cin+C2,3,3), (256,256,1,1) x n, (Cout,256,1,1)).  -> the raw map (B,Cout,h,w) when `final` is None;
    (activated map, raw map) for final = "heatmap" / "depth" (`head_final`: torch elementwise ops on top of the operator).

    Differentiable once in every weight and bias; in x / x2 only with `input_grad=True` (the default serves a frozen trunk, which
    never asks: a source that requires grad then raises NotImplementedError).  With it, each source that requires grad receives
    its gradient: the masked gradient of the first layer is multiplied with the 3x3 weights and scattered to the nine neighbours
    of every active pixel (cf_head_backward_dx, one more launch per list chunk); when no source asks, the backward is the
    default's.  The forward keeps no hidden map: the backward compacts the pixels with a non-zero output gradient on
    the device and recomputes the hidden maps for those alone, with the forward's own kernel - its cost follows the number of
    active pixels (plus one pass over dY and an empty launch per list chunk).  The forward is bitwise reproducible; the
    gradients are summed with float atomics and can differ in their last bits from run to run.  `chunk_px`: list positions per
    workspace chunk (a multiple of 64; 0 = 32768).  CPU tensors raise CfHipError, non-fp32 tensors and unsupported widths
    NotImplementedError."""
    weights, biases = list(weights), list(biases)
    c_x, c_x2, _, _ = _head_check(x, x2, weights, biases, final)
    _need_cuda(x, x2, *weights, *biases)
    if not input_grad and torch.is_grad_enabled() and (x.requires_grad or (x2 is not None and x2.requires_grad)):
        raise NotImplementedError("head_stack: the gradient with respect to x is off by default (frozen trunk only): detach it, "
                                  "or pass input_grad=True")
    if int(chunk_px) < 0 or int(chunk_px) % 64:
        raise ValueError("head_stack: chunk_px must be a multiple of 64 (0: the default)")

    def to_nhwc(t):
        if input_grad and torch.is_grad_enabled() and t.requires_grad:
            return _NchwToNhwcFn.apply(t)
        with torch.no_grad(), torch.cuda.device(t.device):
            return nchw_to_nhwc(t.contiguous())

    xn = to_nhwc(x)
    x2n = None if x2 is None else to_nhwc(x2)
    return head_stack_nhwc(xn, c_x, x2n, c_x2, weights, biases, final, chunk_px, input_grad)


def upsample_dw(x, weight_kkc, f, skip=None, out=None):
    _need_cuda(x, weight_kkc, skip)
    B, H, W, Cc = x.shape
    if out is None:
        out = torch.empty((B, H * f, W * f, Cc), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().cf_upsample_dw(x.data_ptr(), weight_kkc.data_ptr(), _lib.ptr(skip),
                                          out.data_ptr(), B, H, W, Cc, f, _lib.stream_ptr()),
               "cf_upsample_dw")
    return out


# ---- the neck under autograd: the DeformConv block and the IDA upsample (csrc/cf_neck_bwd.hip) ----
def _bytes(n, dev):
    return torch.empty(max(int(n), 1), device=dev, dtype=torch.uint8)


def run_bn_relu_forward(x, gamma, beta, running_mean, running_var, training, momentum, eps):
    """y = relu(batch_norm(x)) on an NHWC map (cf_bn_relu_train_forward) -> (y, mean, invstd): batch statistics and the
    running-statistics update with `training`, the running statistics' affine without."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    y = torch.empty_like(x)
    mean, invstd = torch.empty(Cc, device=x.device, dtype=torch.float32), torch.empty(Cc, device=x.device, dtype=torch.float32)
    nbytes = _lib.load().cf_bn_relu_workspace_bytes(M, Cc)
    ws = _bytes(nbytes, x.device)
    _lib.check(_lib.load().cf_bn_relu_train_forward(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _lib.ptr(running_mean),
                                                    _lib.ptr(running_var), int(bool(training)), float(momentum), float(eps), M, Cc,
                                                    y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), nbytes,
                                                    _lib.stream_ptr()), "cf_bn_relu_train_forward")
    return y, mean, invstd


def run_bn_relu_backward(gy, x, gamma, beta, mean, invstd, training, want_gz=True, want_gamma=True, want_beta=True):
    """-> (gz, ggamma, gbeta) of run_bn_relu_forward from the pre-BN map `x` and the saved statistics (cf_bn_relu_backward);
    None for what is not wanted."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    gz = torch.empty_like(x) if want_gz else None
    gg = torch.empty(Cc, device=x.device, dtype=torch.float32) if want_gamma else None
    gb = torch.empty(Cc, device=x.device, dtype=torch.float32) if want_beta else None
    nbytes = _lib.load().cf_bn_relu_workspace_bytes(M, Cc)
    ws = _bytes(nbytes, x.device)
    _lib.check(_lib.load().cf_bn_relu_backward(gy.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
                                               invstd.data_ptr(), int(bool(training)), M, Cc, _lib.ptr(gz), _lib.ptr(gg), _lib.ptr(gb),
                                               ws.data_ptr(), nbytes, _lib.stream_ptr()), "cf_bn_relu_backward")
    return gz, gg, gb


def run_offmask_activate(om):
    """The mask logits in channels 18..26 of an offset-convolution output (B,H,W,32) -> sigmoid, in place (cf_offmask_activate)."""
    _lib.check(_lib.load().cf_offmask_activate(om.data_ptr(), om.numel() // 32, _lib.stream_ptr()), "cf_offmask_activate")
    return om


def run_conv3x3_bwd_weight(gom, offmask, x, want_gw=True, want_gbias=True):
    """-> (gw (27,C,3,3), gbias (27)) of the offset convolution from the DCN backward's gom, the mask derivative folded in on load
    (cf_conv3x3_bwd_weight); None for what is not wanted."""
    B, H, W, Cc = x.shape
    gw = torch.empty((27, Cc, 3, 3), device=x.device, dtype=torch.float32) if want_gw else None
    gb = torch.empty(27, device=x.device, dtype=torch.float32) if want_gbias else None
    nbytes = _lib.load().cf_conv3x3_bwd_workspace_bytes(B, H, W, Cc)
    ws = _bytes(nbytes, x.device)
    _lib.check(_lib.load().cf_conv3x3_bwd_weight(gom.data_ptr(), offmask.data_ptr(), x.data_ptr(), B, H, W, Cc, _lib.ptr(gw),
                                                 _lib.ptr(gb), ws.data_ptr(), nbytes, _lib.stream_ptr()), "cf_conv3x3_bwd_weight")
    return gw, gb


def run_conv3x3_bwd_data(gom, offmask, weight, gx):
    """Adds the offset convolution's input gradient into gx (B,H,W,C), behind cf_dcn_v2_bwd_data on the same stream
    (cf_conv3x3_bwd_data: a new kernel on the exact fp32 MFMA, not cf_conv2d_fused with a flipped weight - the fold of the mask
    derivative rides on its operand load)."""
    B, H, W, Cc = gx.shape
    _lib.check(_lib.load().cf_conv3x3_bwd_data(gom.data_ptr(), offmask.data_ptr(), weight.data_ptr(), B, H, W, Cc, gx.data_ptr(),
                                               _lib.stream_ptr()), "cf_conv3x3_bwd_data")
    return gx


def run_upsample_dw_bwd(gout, x, weight_kkc, f, want_gx=True, want_gw=True):
    """-> (gx (B,H,W,C), gweight [k][k][C]) of `upsample_dw` (cf_upsample_dw_bwd); None for what is not wanted."""
    B, H, W, Cc = x.shape
    gx = torch.empty_like(x) if want_gx else None
    gw = torch.empty_like(weight_kkc) if want_gw else None
    nbytes = _lib.load().cf_upsample_dw_bwd_workspace_bytes(B, H, W, Cc, f)
    ws = _bytes(nbytes, x.device)
    _lib.check(_lib.load().cf_upsample_dw_bwd(gout.data_ptr(), x.data_ptr(), weight_kkc.data_ptr(), B, H, W, Cc, f, _lib.ptr(gx),
                                              _lib.ptr(gw), ws.data_ptr(), nbytes, _lib.stream_ptr()), "cf_upsample_dw_bwd")
    return gx, gw


def _pack_offset_conv(w, b):
    from . import packing
    return packing.pack_conv_f16(w, b, [packing.Source(w.shape[1], w.shape[1])])


def _f32c(t):
    t = t.detach()
    return t if t.is_contiguous() else t.contiguous()


class _DeformConvBlockFn(torch.autograd.Function):
    """`deform_conv_block` under autograd.  Saved: the block input, the offmask buffer with the ACTIVATED mask, the pre-BN map
    and the batch statistics, the raw weights.  Backward: cf_bn_relu_backward, cf_dcn_v2_bwd_data / _weight,
    cf_conv3x3_bwd_weight / _data - each only when `needs_input_grad` asks for one of its outputs."""

    @staticmethod
    def forward(ctx, xn, com_w, com_b, w, b, gamma, beta, packs, stats, training, momentum, eps, scales):
        pc, pd = packs
        B, H, W, Cin = xn.shape
        dev = xn.device
        with torch.cuda.device(dev):
            x = _f32c(xn)
            om = torch.empty((B, H, W, 32), device=dev, dtype=torch.float32)
            a = conv_args(pc, [x], [Cin], B, H, W, om, 32, ACT_NONE, None, 0, LAYOUT_NHWC, None, 0, False,
                          in_scale=None if scales is None else scales[0])
            run_conv_f16(a, pc.patch)
            run_offmask_activate(om)                   # (the backward reads the activated mask; the DCN takes it as it is)
            z = torch.empty((B, H, W, pd.n), device=dev, dtype=torch.float32)
            nbytes = _lib.load().cf_dcn_v2_workspace_bytes(B, H, W, pd.c, pd.n_pad)
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
            d = dcn_args(pd, x, om, 32, B, H, W, z, pd.n, ACT_NONE, precise=True, workspace=ws,
                         in_scale=None if scales is None else scales[1])
            d.mask_activated = 1
            run_dcn(d)
            g, be = _f32c(gamma), _f32c(beta)
            y, mean, invstd = run_bn_relu_forward(z, g, be, stats[0], stats[1], training, momentum, eps)
        ctx.training = bool(training)
        ctx.save_for_backward(x, om, z, mean, invstd, _f32c(com_w), _f32c(w), g, be)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, om, z, mean, invstd, com_w, w, gamma, beta = ctx.saved_tensors
        need_x, need_cw, need_cb, need_w, need_b, need_g, need_be = ctx.needs_input_grad[:7]
        B, H, W, Cin = x.shape
        dev = x.device
        gx = gcw = gcb = gw = gb = None
        with torch.cuda.device(dev):
            gy = _f32c(gy)
            upstream = need_x or need_cw or need_cb or need_w or need_b
            gz, gg, gbe = run_bn_relu_backward(gy, z, gamma, beta, mean, invstd, ctx.training, upstream, need_g, need_be)
            if need_x or need_cw or need_cb:
                gx = torch.zeros((B, H, W, Cin), device=dev, dtype=torch.float32) if need_x else None
                gom = torch.empty((B, H, W, 32), device=dev, dtype=torch.float32)
                run_dcn_bwd_data(dcn_bwd_args(gz, x, om, weight=w, gx=gx, gom=gom))
                if need_cw or need_cb:
                    gcw, gcb = run_conv3x3_bwd_weight(gom, om, x, need_cw, need_cb)
                if need_x:
                    run_conv3x3_bwd_data(gom, om, com_w, gx)
            if need_w or need_b:
                gw = torch.empty_like(w) if need_w else None
                gb = torch.empty(w.shape[0], device=dev, dtype=torch.float32) if need_b else None
                nbytes = _lib.load().cf_dcn_v2_bwd_workspace_bytes(B, H, W, Cin, w.shape[0])
                wsb = torch.empty(nbytes, device=dev, dtype=torch.uint8)
                run_dcn_bwd_weight(dcn_bwd_args(gz, x, om, gw=gw, gbias=gb, workspace=wsb))
        return (gx, gcw, gcb, gw, gb, gg, gbe, None, None, None, None, None, None)


def _block_check(who, x, cin, com_weight, com_bias, weight, bias, bn_weight, bn_bias, running_mean, running_var):
    for t in (x, com_weight, com_bias, weight, bias, bn_weight, bn_bias, running_mean, running_var):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise NotImplementedError(f"{who}: float32 tensors only (no autocast, no fp16 / bf16 / float64)")
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError(f"{who}: x must be a 4-D map and weight (Cout,Cin,3,3)")
    cout = weight.shape[0]
    if tuple(weight.shape) != (cout, cin, 3, 3) or tuple(com_weight.shape) != (27, cin, 3, 3):
        raise NotImplementedError(f"{who}: weight must be (Cout,{cin},3,3) and the offset convolution's (27,{cin},3,3) - 3x3, stride 1, "
                                  f"padding 1, one group, one offset group only - got {tuple(weight.shape)} / {tuple(com_weight.shape)}")
    if cin % 32 or cout % 32 or cin > 512 or cout > 1024:
        raise NotImplementedError(f"{who}: Cin={cin} (at most 512) and Cout={cout} (at most 1024) must be multiples of 32")
    for t, n, what in ((com_bias, 27, "com_bias"), (bias, cout, "bias"), (bn_weight, cout, "bn_weight"), (bn_bias, cout, "bn_bias"),
                       (running_mean, cout, "running_mean"), (running_var, cout, "running_var")):
        if tuple(t.shape) != (n,):
            raise ValueError(f"{who}: {what} must be ({n},), got {tuple(t.shape)}")
    _need_cuda(x, com_weight, com_bias, weight, bias, bn_weight, bn_bias, running_mean, running_var)


def deform_conv_block_nhwc(xn, com_weight, com_bias, weight, bias, bn_weight, bn_bias, running_mean, running_var, training=True,
                           momentum=0.1, eps=1e-5, in_scales=None, pack_verify=True):
    """`deform_conv_block` on a map that is already NHWC: xn (B,H,W,Cin) -> (B,H,W,Cout).  The neck of DLASeg's training
    forward composes these (and `upsample_dw_add_nhwc`) without a layout launch in between.  pack_verify=False: the packed-weight
    cache trusts the weights' version counters for this call (`set_dcn_pack_verify` explains the checksum it skips)."""
    _block_check("deform_conv_block", xn, xn.shape[-1] if torch.is_tensor(xn) and xn.dim() == 4 else -1, com_weight, com_bias, weight,
                 bias, bn_weight, bn_bias, running_mean, running_var)
    B, H, W, _ = xn.shape
    if training and B * H * W == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {(B, weight.shape[0], H, W)}")
    if in_scales is not None:
        scales = (float(in_scales[0]), float(in_scales[1]))
    elif _DCN_RANGE_CHECK and not torch.cuda.is_current_stream_capturing():
        with torch.cuda.device(xn.device):
            s = in_scale_for(float(absmax(_f32c(xn)).item()))          # (raises on NaN / inf)
        scales = (s, s)
    else:
        scales = None
    packs = (_packed_dcn(com_weight, com_bias, pack=_pack_offset_conv, verify=pack_verify), _packed_dcn(weight, bias, verify=pack_verify))
    return _DeformConvBlockFn.apply(xn, com_weight, com_bias, weight, bias, bn_weight, bn_bias, packs, (running_mean, running_var),
                                    bool(training), float(momentum), float(eps), scales)


class _NhwcToNchwFn(torch.autograd.Function):
    """The layout conversion behind an NCHW-outside operator: cf_nhwc_to_nchw forward, cf_nchw_to_nhwc backward."""

    @staticmethod
    def forward(ctx, x):
        with torch.cuda.device(x.device):
            return nhwc_to_nchw(x.detach().contiguous())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        with torch.cuda.device(g.device):
            return nchw_to_nhwc(g.detach().contiguous())


def _to_nhwc(t):
    if torch.is_grad_enabled() and t.requires_grad:
        return _NchwToNhwcFn.apply(t)
    with torch.no_grad(), torch.cuda.device(t.device):
        return nchw_to_nhwc(t.contiguous())


def deform_conv_block(x, com_weight, com_bias, weight, bias, bn_weight, bn_bias, running_mean, running_var, training=True,
                      momentum=0.1, eps=1e-5, in_scales=None):
    """The reference's `DeformConv(activation=True).forward` (model/networks/dla.py:456-472) as ONE operator under autograd, on HIP
    kernels in both directions: conv_offset_mask (3x3, Cin -> 27) -> chunk / cat / sigmoid -> modulated deformable 3x3 convolution
    -> BatchNorm2d -> ReLU.  `x` (B,Cin,H,W) fp32 on the device -> (B,Cout,H,W); com_weight (27,Cin,3,3), com_bias (27), weight
    (Cout,Cin,3,3), bias (Cout), bn_weight / bn_bias / running_mean / running_var (Cout); Cin and Cout multiples of 32.

    Forward: the split-fp16 offset convolution (cf_conv3x3_f16x3) and cf_dcn_v2_f16x3 on weights packed once per weight version
    (the cache of `deform_conv2d`, which also holds the offset convolution's), then cf_bn_relu_train_forward.  `training=True`:
    batch statistics (two-pass variance), running_mean / running_var updated in place with `momentum` and the unbiased variance
    as torch.nn.BatchNorm2d does (num_batches_tracked is the caller's); one value per channel raises ValueError.
    `training=False`: the affine of the running statistics, still differentiable.  The range check is `deform_conv2d`'s: with
    `set_dcn_range_check` on, every call measures max |x| (one device -> host scalar) and picks the pre-scale; `in_scales` =
    (offset convolution's, DCN's) pre-scales skips it - no check, no host sync.

    Differentiable once in x and the six parameters; only the launches `needs_input_grad` asks for run.  Parameter gradients are
    slab sums added in a fixed order (bitwise reproducible); the input gradient goes through the DCN's float atomics.  CPU tensors
    raise CfHipError, non-fp32 tensors and unsupported shapes NotImplementedError."""
    _block_check("deform_conv_block", x, x.shape[1] if torch.is_tensor(x) and x.dim() == 4 else -1, com_weight, com_bias, weight, bias,
                 bn_weight, bn_bias, running_mean, running_var)
    y = deform_conv_block_nhwc(_to_nhwc(x), com_weight, com_bias, weight, bias, bn_weight, bn_bias, running_mean, running_var,
                               training, momentum, eps, in_scales)
    return _NhwcToNchwFn.apply(y)


class _UpsampleDwAddFn(torch.autograd.Function):
    """`upsample_dw_add` under autograd: cf_upsample_dw forward; cf_upsample_dw_bwd backward (the skip's gradient is gout)."""

    @staticmethod
    def forward(ctx, xn, weight, f, skipn):
        with torch.cuda.device(xn.device):
            x, skip = _f32c(xn), _f32c(skipn)
            wk = weight.detach()[:, 0].permute(1, 2, 0).contiguous()        # (C,1,k,k) -> [k][k][C]
            out = upsample_dw(x, wk, f, skip)
        ctx.f = f
        ctx.save_for_backward(x, wk)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, wk = ctx.saved_tensors
        need_x, need_w, _, need_s = ctx.needs_input_grad
        gx = gw = None
        gout = _f32c(gout)
        if need_x or need_w:
            with torch.cuda.device(x.device):
                gx, gwk = run_upsample_dw_bwd(gout, x, wk, ctx.f, need_x, need_w)
                if need_w:
                    gw = gwk.permute(2, 0, 1).unsqueeze(1).contiguous()
        return gx, gw, None, (gout if need_s else None)


def _upsample_check(x, weight, f, skip, c, hw, skip_hw):
    for t in (x, weight, skip):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise NotImplementedError("upsample_dw_add: float32 tensors only (no autocast, no fp16 / bf16 / float64)")
    if f not in (2, 4):
        raise NotImplementedError(f"upsample_dw_add: f={f!r} (2 or 4 only: k = 2f, stride f, padding f/2)")
    if tuple(weight.shape) != (c, 1, 2 * f, 2 * f) or c % 4:
        raise NotImplementedError(f"upsample_dw_add: weight must be the depthwise ({c},1,{2 * f},{2 * f}) with C a multiple of 4, "
                                  f"got {tuple(weight.shape)}")
    if tuple(skip_hw) != (hw[0] * f, hw[1] * f):
        raise ValueError(f"upsample_dw_add: skip must be the x{f} map of x, got {tuple(skip.shape)} for {tuple(x.shape)}")
    _need_cuda(x, weight, skip)


def upsample_dw_add_nhwc(xn, weight, f, skipn):
    """`upsample_dw_add` on NHWC maps: xn (B,H,W,C), skipn (B,H*f,W*f,C) -> (B,H*f,W*f,C)."""
    if not (torch.is_tensor(xn) and torch.is_tensor(skipn) and xn.dim() == 4 and skipn.dim() == 4 and skipn.shape[0] == xn.shape[0]
            and skipn.shape[3] == xn.shape[3]):
        raise ValueError("upsample_dw_add: x and skip must be 4-D maps of one batch and channel count")
    _upsample_check(xn, weight, f, skipn, xn.shape[3], xn.shape[1:3], skipn.shape[1:3])
    return _UpsampleDwAddFn.apply(xn, weight, int(f), skipn)


def upsample_dw_add(x, weight, f, skip):
    """One IDA step of the reference (model/networks/dla.py:518-524): `up(x) + skip`, `up` the depthwise
    ConvTranspose2d(C, C, 2f, stride=f, padding=f/2, groups=C, bias=False) with `weight` (C,1,2f,2f), f = 2 or 4; x (B,C,H,W) and
    skip (B,C,H*f,W*f) fp32 on the device.  Forward cf_upsample_dw (the add fused), backward cf_upsample_dw_bwd; differentiable
    once in x, weight and skip (skip's gradient is the output gradient itself).  The weight gradient is a slab sum added in a
    fixed order: bitwise reproducible."""
    if not (torch.is_tensor(x) and torch.is_tensor(skip) and x.dim() == 4 and skip.dim() == 4 and skip.shape[:2] == x.shape[:2]):
        raise ValueError("upsample_dw_add: x and skip must be 4-D maps of one batch and channel count")
    _upsample_check(x, weight, f, skip, x.shape[1], x.shape[2:], skip.shape[2:])
    return _NhwcToNchwFn.apply(upsample_dw_add_nhwc(_to_nhwc(x), weight, f, _to_nhwc(skip)))


# ---- the base under autograd: the conv + BatchNorm block and the 2x2 max-pool (csrc/cf_base_bwd.hip) ----
def conv_out_hw(H, W, k, stride):
    """(Ho, Wo) of a k x k convolution with padding (k - 1) / 2"""
    pad = (k - 1) // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def run_conv_bwd_weight(gz, x, k, stride=1):
    """-> gw (N,C,k,k) of a k x k convolution (padding (k-1)/2, no bias) from gz (B,Ho,Wo,N) and its input x (B,H,W,C), NHWC
    (cf_conv_bwd_weight: slab partials added in slab order)."""
    B, H, W, Cc = x.shape
    N = gz.shape[-1]
    gw = torch.empty((N, Cc, k, k), device=x.device, dtype=torch.float32)
    nbytes = _lib.load().cf_conv_bwd_workspace_bytes(B, H, W, Cc, N, k, stride)
    ws = _bytes(nbytes, x.device)
    _lib.check(_lib.load().cf_conv_bwd_weight(gz.data_ptr(), x.data_ptr(), B, H, W, Cc, N, k, stride, gw.data_ptr(), ws.data_ptr(),
                                              nbytes, _lib.stream_ptr()), "cf_conv_bwd_weight")
    return gw


def run_conv_bwd_data(gz, weight, H, W, stride=1):
    """-> gx (B,H,W,C) of a k x k convolution from gz (B,Ho,Wo,N) and the raw weight (N,C,k,k) (cf_conv_bwd_data: a kernel of its
    own on the exact fp32 MFMA that reads the torch weight as it is - nothing to re-pack behind an optimizer step)."""
    B = gz.shape[0]
    N, Cc, k, _ = weight.shape
    gx = torch.empty((B, H, W, Cc), device=gz.device, dtype=torch.float32)
    _lib.check(_lib.load().cf_conv_bwd_data(gz.data_ptr(), weight.data_ptr(), B, H, W, Cc, N, k, stride, gx.data_ptr(),
                                            _lib.stream_ptr()), "cf_conv_bwd_data")
    return gx


def run_bn_act_forward(x, gamma, beta, running_mean, running_var, training, momentum, eps, residual=None, relu=True):
    """y = act(batch_norm(x) [+ residual]) on an NHWC map (cf_bn_act_train_forward) -> (y, mean, invstd); act = ReLU or nothing.
    residual=None, relu=True: the bits of `run_bn_relu_forward`."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    y = torch.empty_like(x)
    mean, invstd = torch.empty(Cc, device=x.device, dtype=torch.float32), torch.empty(Cc, device=x.device, dtype=torch.float32)
    nbytes = _lib.load().cf_bn_act_workspace_bytes(M, Cc)
    ws = _bytes(nbytes, x.device)
    _lib.check(_lib.load().cf_bn_act_train_forward(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _lib.ptr(residual), int(bool(relu)),
                                                   _lib.ptr(running_mean), _lib.ptr(running_var), int(bool(training)), float(momentum),
                                                   float(eps), M, Cc, y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(),
                                                   nbytes, _lib.stream_ptr()), "cf_bn_act_train_forward")
    return y, mean, invstd


def run_bn_act_backward(gy, x, gamma, beta, mean, invstd, training, residual=None, relu=True, want_gz=True, want_gres=True,
                        want_gamma=True, want_beta=True):
    """-> (gz, gres, ggamma, gbeta) of run_bn_act_forward from the pre-BN map `x`, the residual the forward added and the saved
    statistics (cf_bn_act_backward); None for what is not wanted."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    gz = torch.empty_like(x) if want_gz else None
    gr = torch.empty_like(x) if want_gres else None
    gg = torch.empty(Cc, device=x.device, dtype=torch.float32) if want_gamma else None
    gb = torch.empty(Cc, device=x.device, dtype=torch.float32) if want_beta else None
    nbytes = _lib.load().cf_bn_act_workspace_bytes(M, Cc)
    ws = _bytes(nbytes, x.device)
    _lib.check(_lib.load().cf_bn_act_backward(gy.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _lib.ptr(residual),
                                              int(bool(relu)), mean.data_ptr(), invstd.data_ptr(), int(bool(training)), M, Cc,
                                              _lib.ptr(gz), _lib.ptr(gr), _lib.ptr(gg), _lib.ptr(gb), ws.data_ptr(), nbytes,
                                              _lib.stream_ptr()), "cf_bn_act_backward")
    return gz, gr, gg, gb


def run_maxpool2x2_bwd(gout, x):
    """-> gx (B,H,W,C) of `maxpool2x2` from gout (B,H/2,W/2,C) and the pooled map x (cf_maxpool2x2_bwd: the first maximum of a
    window in row-major order takes the gradient, as aten's does)."""
    B, H, W, Cc = x.shape
    gx = torch.empty_like(x)
    _lib.check(_lib.load().cf_maxpool2x2_bwd(gout.data_ptr(), x.data_ptr(), B, H, W, Cc, gx.data_ptr(), _lib.stream_ptr()),
               "cf_maxpool2x2_bwd")
    return gx


def _packed_conv(weight, stride, verify=True):
    """the raw convolution weight (no bias, no BN fold) packed for the split-fp16 kernels, once per weight version: the cache of
    `deform_conv2d`.  A 3x3's slice-major packing is the same for stride 1 and 2; the entry carries the stride it was packed for."""
    import dataclasses
    from . import packing

    def pack(w, b):
        return packing.pack_conv_f16(w, b, [packing.Source(w.shape[1], w.shape[1])], stride=stride)
    pc = _packed_dcn(weight, None, pack=pack, verify=verify)
    return pc if pc.stride == stride else dataclasses.replace(pc, stride=stride)


class _ConvBnActFn(torch.autograd.Function):
    """`conv_bn_act` under autograd.  Saved: the block input, the pre-BN map, the residual only where the ReLU mask needs it, the
    batch statistics, the raw weight.  Backward: cf_bn_act_backward, then cf_conv_bwd_weight / cf_conv_bwd_data - each only when
    `needs_input_grad` asks for its output."""

    @staticmethod
    def forward(ctx, xn, w, gamma, beta, resn, pc, stats, stride, relu, training, momentum, eps, scale):
        B, H, W, _ = xn.shape
        with torch.cuda.device(xn.device):
            x = _f32c(xn)
            res = None if resn is None else _f32c(resn)
            z = conv2d_f16x3(pc, [x], B, H, W, ACT_NONE, in_scale=scale)
            g, be = _f32c(gamma), _f32c(beta)
            y, mean, invstd = run_bn_act_forward(z, g, be, stats[0], stats[1], training, momentum, eps, res, relu)
        ctx.training, ctx.relu, ctx.stride, ctx.has_res = bool(training), bool(relu), int(stride), res is not None
        ctx.save_for_backward(x, z, mean, invstd, _f32c(w), g, be, *([res] if res is not None and relu else []))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, z, mean, invstd, w, gamma, beta, *rest = ctx.saved_tensors
        res = rest[0] if rest else None
        need_x, need_w, need_g, need_be, need_r = ctx.needs_input_grad[:5]
        need_r = need_r and ctx.has_res
        _, H, W, _ = x.shape
        gx = gw = gres = None
        with torch.cuda.device(x.device):
            gy = _f32c(gy)
            gz, gres, gg, gbe = run_bn_act_backward(gy, z, gamma, beta, mean, invstd, ctx.training, res, ctx.relu, need_x or need_w,
                                                    need_r and ctx.relu, need_g, need_be)
            if need_r and not ctx.relu:
                gres = gy                              # (no mask: the residual's gradient is the output's)
            if need_w:
                gw = run_conv_bwd_weight(gz, x, w.shape[-1], ctx.stride)
            if need_x:
                gx = run_conv_bwd_data(gz, w, H, W, ctx.stride)
        return (gx, gw, gg, gbe, gres, None, None, None, None, None, None, None, None)


def _conv_bn_check(who, x, cin, hw, weight, bn_weight, bn_bias, running_mean, running_var, stride, residual, res_shape):
    for t in (x, weight, bn_weight, bn_bias, running_mean, running_var) + (() if residual is None else (residual,)):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise NotImplementedError(f"{who}: float32 tensors only (no autocast, no fp16 / bf16 / float64)")
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError(f"{who}: x must be a 4-D map and weight (Cout,Cin,k,k)")
    cout, k = weight.shape[0], weight.shape[2]
    if tuple(weight.shape) != (cout, cin, k, k) or k not in (1, 3) or stride not in (1, 2) or (stride == 2 and k != 3):
        raise NotImplementedError(f"{who}: weight must be (Cout,{cin},k,k) with k = 1 (stride 1) or k = 3 (stride 1 or 2), padding "
                                  f"(k-1)/2, one group - got {tuple(weight.shape)}, stride {stride!r}")
    if cin % 32 or cout % 32 or cin > 1280 or cout > 512:
        raise NotImplementedError(f"{who}: Cin={cin} (at most 1280) and Cout={cout} (at most 512) must be multiples of 32")
    for t, what in ((bn_weight, "bn_weight"), (bn_bias, "bn_bias"), (running_mean, "running_mean"), (running_var, "running_var")):
        if tuple(t.shape) != (cout,):
            raise ValueError(f"{who}: {what} must be ({cout},), got {tuple(t.shape)}")
    ho, wo = conv_out_hw(hw[0], hw[1], k, stride)
    if residual is not None and tuple(res_shape) != (x.shape[0], cout, ho, wo):
        raise ValueError(f"{who}: residual must have the output's shape {(x.shape[0], cout, ho, wo)}")
    _need_cuda(x, weight, bn_weight, bn_bias, running_mean, running_var, residual)
    return ho, wo


def conv_bn_act_nhwc(xn, weight, bn_weight, bn_bias, running_mean, running_var, stride=1, residual=None, relu=True, training=True,
                     momentum=0.1, eps=1e-5, in_scale=None, pack_verify=True):
    """`conv_bn_act` on maps that are already NHWC: xn (B,H,W,Cin), residual (B,Ho,Wo,Cout) or None -> (B,Ho,Wo,Cout).
    DLASeg.forward_levels composes these (and `max_pool2x2_nhwc`) without a layout launch in between.  pack_verify=False: the
    packed-weight cache trusts the weight's version counter for this call (`set_dcn_pack_verify`)."""
    ok = torch.is_tensor(xn) and xn.dim() == 4
    ho, wo = _conv_bn_check("conv_bn_act", xn, xn.shape[-1] if ok else -1, xn.shape[1:3] if ok else (0, 0), weight, bn_weight, bn_bias,
                            running_mean, running_var, stride, residual,
                            () if residual is None or residual.dim() != 4 else (residual.shape[0], residual.shape[3], *residual.shape[1:3]))
    if training and xn.shape[0] * ho * wo == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {(xn.shape[0], weight.shape[0], ho, wo)}")
    if in_scale is not None:
        scale = float(in_scale)
    elif _DCN_RANGE_CHECK and not torch.cuda.is_current_stream_capturing():
        with torch.cuda.device(xn.device):
            scale = in_scale_for(float(absmax(_f32c(xn)).item()))          # (raises on NaN / inf)
    else:
        scale = None
    pc = _packed_conv(weight, int(stride), verify=pack_verify)
    return _ConvBnActFn.apply(xn, weight, bn_weight, bn_bias, residual, pc, (running_mean, running_var), int(stride), bool(relu),
                              bool(training), float(momentum), float(eps), scale)


def conv_bn_act(x, weight, bn_weight, bn_bias, running_mean, running_var, stride=1, residual=None, relu=True, training=True,
                momentum=0.1, eps=1e-5, in_scale=None):
    """The block shape of the reference's DLA-34 base (model/networks/dla.py:44-118, 121-161) as ONE operator under autograd, on HIP
    kernels in both directions: Conv2d(k, stride, padding (k-1)/2, bias=False) -> BatchNorm2d -> [+ residual] -> [ReLU].
    BasicBlock.conv1 is (relu), BasicBlock.conv2 (residual, relu), Tree.project a 1x1 without ReLU, Root a 1x1 (relu) over a
    channel concat.  `x` (B,Cin,H,W) fp32 on the device -> (B,Cout,Ho,Wo); weight (Cout,Cin,k,k) with k = 3 (stride 1 or 2) or
    k = 1 (stride 1); bn_weight / bn_bias / running_mean / running_var (Cout); residual None or of the output's shape; Cin
    (at most 1280) and Cout (at most 512) multiples of 32.

    Forward: the split-fp16 convolution (cf_conv3x3_f16x3 / cf_conv2d_f16x3) on the raw weight - no BN fold - packed once per
    weight version (the cache of `deform_conv2d`), then cf_bn_act_train_forward.  `training=True`: batch statistics, running_mean
    / running_var updated in place as torch.nn.BatchNorm2d does (num_batches_tracked is the caller's); one value per channel
    raises ValueError.  `training=False`: the affine of the running statistics, still differentiable.  The range check is
    `deform_conv2d`'s: with `set_dcn_range_check` on, every call measures max |x| (one device -> host scalar) and picks the
    pre-scale; `in_scale` skips it - no check, no host sync.

    Differentiable once in x, weight, bn_weight, bn_bias and residual; only the launches `needs_input_grad` asks for run:
    cf_bn_act_backward, then cf_conv_bwd_weight and cf_conv_bwd_data on the exact fp32 MFMA.  Every gradient is bitwise
    reproducible (no float atomics).  CPU tensors raise CfHipError, non-fp32 tensors and unsupported shapes NotImplementedError."""
    ok = torch.is_tensor(x) and x.dim() == 4
    _conv_bn_check("conv_bn_act", x, x.shape[1] if ok else -1, x.shape[2:] if ok else (0, 0), weight, bn_weight, bn_bias, running_mean,
                   running_var, stride, residual, () if residual is None else tuple(residual.shape))
    y = conv_bn_act_nhwc(_to_nhwc(x), weight, bn_weight, bn_bias, running_mean, running_var, stride,
                         None if residual is None else _to_nhwc(residual), relu, training, momentum, eps, in_scale)
    return _NhwcToNchwFn.apply(y)


class _MaxPool2x2Fn(torch.autograd.Function):
    """`max_pool2x2` under autograd: cf_maxpool2x2 forward, cf_maxpool2x2_bwd backward."""

    @staticmethod
    def forward(ctx, xn):
        with torch.cuda.device(xn.device):
            x = _f32c(xn)
            out = maxpool2x2(x)
        ctx.save_for_backward(x)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, = ctx.saved_tensors
        with torch.cuda.device(x.device):
            return run_maxpool2x2_bwd(_f32c(gout), x)


def _pool_check(x, c, hw):
    if not torch.is_tensor(x) or x.dtype != torch.float32:
        raise NotImplementedError("max_pool2x2: float32 tensors only (no autocast, no fp16 / bf16 / float64)")
    if x.dim() != 4:
        raise ValueError("max_pool2x2: x must be a 4-D map")
    if c % 4 or hw[0] < 2 or hw[1] < 2:
        raise NotImplementedError(f"max_pool2x2: C={c} must be a multiple of 4 and the map at least 2 x 2, got {tuple(x.shape)}")
    _need_cuda(x)


def max_pool2x2_nhwc(xn):
    """`max_pool2x2` on an NHWC map: (B,H,W,C) -> (B,H/2,W/2,C)."""
    ok = torch.is_tensor(xn) and xn.dim() == 4
    _pool_check(xn, xn.shape[3] if ok else 0, xn.shape[1:3] if ok else (0, 0))
    return _MaxPool2x2Fn.apply(xn)


def max_pool2x2(x):
    """F.max_pool2d(x, 2, 2) (Tree.downsample, dla.py:96,107) under autograd: x (B,C,H,W) fp32 on the device -> (B,C,H/2,W/2).
    Forward cf_maxpool2x2, backward cf_maxpool2x2_bwd: the whole gradient of a window goes to its first maximum in row-major
    order - aten's choice on a tie, and post-ReLU maps are full of all-zero windows.  `maxpool2x2` is the plain NHWC launch."""
    ok = torch.is_tensor(x) and x.dim() == 4
    _pool_check(x, x.shape[1] if ok else 0, x.shape[2:] if ok else (0, 0))
    return _NhwcToNchwFn.apply(max_pool2x2_nhwc(_to_nhwc(x)))


# ---- the stem under autograd: the narrow convolution + BatchNorm + ReLU block (csrc/cf_stem_train.hip) ----
def run_stem_conv_forward(x, weight, stride=1, radar=None):
    """-> z (B,Ho,Wo,Cout) NHWC, the pre-BN map of a stem convolution (cf_stem_conv_forward, exact fp32 on the raw weight).
    k = 7: x is the NCHW image and `radar` None or the (B,3,H/4,W/4) map that supplies the last three input channels;
    k = 3: x is NHWC."""
    N, Cin, k, _ = weight.shape
    B, H, W = (x.shape[0], x.shape[2], x.shape[3]) if k == 7 else x.shape[:3]
    ho, wo = conv_out_hw(H, W, k, stride)
    z = torch.empty((B, ho, wo, N), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().cf_stem_conv_forward(x.data_ptr(), _lib.ptr(radar), weight.data_ptr(), B, H, W, Cin, N, k, stride,
                                                z.data_ptr(), _lib.stream_ptr()), "cf_stem_conv_forward")
    return z


def run_stem_conv_bwd_weight(gz, x, k, cin, stride=1, radar=None):
    """-> gw (Cout,cin,k,k) of a stem convolution from gz (B,Ho,Wo,Cout) and its input as `run_stem_conv_forward` takes it
    (cf_stem_conv_bwd_weight: slab partials added in slab order)."""
    B, H, W = (x.shape[0], x.shape[2], x.shape[3]) if k == 7 else x.shape[:3]
    N = gz.shape[-1]
    gw = torch.empty((N, cin, k, k), device=x.device, dtype=torch.float32)
    nbytes = _lib.load().cf_stem_conv_bwd_workspace_bytes(B, H, W, cin, N, k, stride)
    ws = _bytes(nbytes, x.device)
    _lib.check(_lib.load().cf_stem_conv_bwd_weight(gz.data_ptr(), x.data_ptr(), _lib.ptr(radar), B, H, W, cin, N, k, stride,
                                                   gw.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr()), "cf_stem_conv_bwd_weight")
    return gw


def run_stem_conv_bwd_data(gz, weight, H, W, stride=1):
    """-> gx (B,H,W,16) NHWC of a 3x3 stem convolution from gz (B,Ho,Wo,Cout) and the raw weight (cf_stem_conv_bwd_data)."""
    B = gz.shape[0]
    N, Cc, k, _ = weight.shape
    gx = torch.empty((B, H, W, Cc), device=gz.device, dtype=torch.float32)
    _lib.check(_lib.load().cf_stem_conv_bwd_data(gz.data_ptr(), weight.data_ptr(), B, H, W, Cc, N, k, stride, gx.data_ptr(),
                                                 _lib.stream_ptr()), "cf_stem_conv_bwd_data")
    return gx


class _StemConvBnReluFn(torch.autograd.Function):
    """`stem_conv_bn_relu` under autograd, in the style of `_ConvBnActFn`.  Saved: the block input (and the radar map), the pre-BN
    map, the batch statistics, the raw weight.  Backward: cf_bn_act_backward, then cf_stem_conv_bwd_weight / cf_stem_conv_bwd_data
    - each only when `needs_input_grad` asks for its output."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, radar, stats, stride, training, momentum, eps):
        with torch.cuda.device(x.device):
            x, wc, g, be = _f32c(x), _f32c(w), _f32c(gamma), _f32c(beta)
            rad = None if radar is None else _f32c(radar)
            z = run_stem_conv_forward(x, wc, stride, rad)
            y, mean, invstd = run_bn_act_forward(z, g, be, stats[0], stats[1], training, momentum, eps, None, True)
        ctx.training, ctx.stride, ctx.has_radar = bool(training), int(stride), rad is not None
        ctx.save_for_backward(x, z, mean, invstd, wc, g, be, *([rad] if rad is not None else []))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, z, mean, invstd, w, gamma, beta, *rest = ctx.saved_tensors
        rad = rest[0] if rest else None
        need_x, need_w, need_g, need_be = ctx.needs_input_grad[:4]
        k, cin = w.shape[-1], w.shape[1]
        gx = gw = None
        with torch.cuda.device(x.device):
            gy = _f32c(gy)
            gz, _, gg, gbe = run_bn_act_backward(gy, z, gamma, beta, mean, invstd, ctx.training, None, True, need_x or need_w, False,
                                                 need_g, need_be)
            if need_w:
                gw = run_stem_conv_bwd_weight(gz, x, k, cin, ctx.stride, rad)
            if need_x:
                gx = run_stem_conv_bwd_data(gz, w, x.shape[1], x.shape[2], ctx.stride)
        return (gx, gw, gg, gbe, None, None, None, None, None, None)


def _stem_check(who, x, nhwc, weight, bn_weight, bn_bias, running_mean, running_var, stride, radar):
    """-> (Ho, Wo); x is (B,H,W,C) when `nhwc`, else (B,C,H,W)"""
    for t in (x, weight, bn_weight, bn_bias, running_mean, running_var) + (() if radar is None else (radar,)):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise NotImplementedError(f"{who}: float32 tensors only (no autocast, no fp16 / bf16 / float64)")
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError(f"{who}: x must be a 4-D map and weight (Cout,Cin,k,k)")
    cout, cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
    if weight.shape[3] != k or not ((k == 7 and stride == 1 and 0 < cin <= 8) or (k == 3 and stride in (1, 2) and cin == 16)) \
            or cout not in (16, 32):
        raise NotImplementedError(f"{who}: weight must be (16 or 32, Cin, k, k) with k = 7 (stride 1, Cin <= 8) or k = 3 (stride 1 or 2, "
                                  f"Cin = 16), padding (k-1)/2, one group - got {tuple(weight.shape)}, stride {stride!r}")
    nhwc = nhwc and k == 3                                 # (the 7x7 layer reads the image as the caller holds it: NCHW planes)
    B, cx, H, W = (x.shape[0], x.shape[3], x.shape[1], x.shape[2]) if nhwc else tuple(x.shape)
    if radar is not None:
        if k != 7 or cin <= 3 or H % 4 or W % 4:
            raise NotImplementedError(f"{who}: a radar map goes with a 7x7 layer of more than 3 input channels on a map whose H, W are "
                                      "multiples of 4")
        if tuple(radar.shape) != (B, 3, H // 4, W // 4):
            raise ValueError(f"{who}: radar must be {(B, 3, H // 4, W // 4)}, got {tuple(radar.shape)}")
    if cx + (0 if radar is None else 3) != cin:
        raise NotImplementedError(f"{who}: the input has {cx}{'' if radar is None else ' + 3'} channels, the weight {cin}")
    if k == 7 and (x.requires_grad or (radar is not None and radar.requires_grad)) and torch.is_grad_enabled():
        raise NotImplementedError(f"{who}: the 7x7 layer has no input gradient (nothing differentiates the image or the radar map); "
                                  "detach the input")
    for t, what in ((bn_weight, "bn_weight"), (bn_bias, "bn_bias"), (running_mean, "running_mean"), (running_var, "running_var")):
        if tuple(t.shape) != (cout,):
            raise ValueError(f"{who}: {what} must be ({cout},), got {tuple(t.shape)}")
    _need_cuda(x, weight, bn_weight, bn_bias, running_mean, running_var, radar)
    return conv_out_hw(H, W, k, stride)


def _stem_apply(x, B, ho, wo, weight, bn_weight, bn_bias, running_mean, running_var, stride, training, momentum, eps, radar):
    if training and B * ho * wo == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {(B, weight.shape[0], ho, wo)}")
    return _StemConvBnReluFn.apply(x, weight, bn_weight, bn_bias, radar, (running_mean, running_var), int(stride), bool(training),
                                   float(momentum), float(eps))


def stem_conv_bn_relu_nhwc(xn, weight, bn_weight, bn_bias, running_mean, running_var, stride=1, training=True, momentum=0.1,
                           eps=1e-5, radar=None):
    """`stem_conv_bn_relu` with an NHWC result and, for the 3x3 layers, an NHWC input: xn (B,H,W,16) -> (B,Ho,Wo,Cout).  The 7x7
    layer still takes the NCHW image (and `radar`) as the caller holds it.  DLASeg.forward_stem_train composes the three layers
    with it, without a layout launch in between."""
    ho, wo = _stem_check("stem_conv_bn_relu", xn, True, weight, bn_weight, bn_bias, running_mean, running_var, stride, radar)
    return _stem_apply(xn, xn.shape[0], ho, wo, weight, bn_weight, bn_bias, running_mean, running_var, stride, training, momentum, eps,
                       radar)


def stem_conv_bn_relu(x, weight, bn_weight, bn_bias, running_mean, running_var, stride=1, training=True, momentum=0.1, eps=1e-5,
                      radar=None):
    """One block of the reference's DLA-34 stem (model/networks/dla.py:193-203, 250-262: base_layer, level0, level1) as ONE operator
    under autograd, on HIP kernels in both directions: Conv2d(k, stride, padding (k-1)/2, bias=False) -> BatchNorm2d -> ReLU on
    narrow channel counts.  `x` (B,Cin,H,W) fp32 on the device -> (B,Cout,Ho,Wo); weight (Cout,Cin,k,k) with Cout 16 or 32 and
    k = 7 (stride 1, Cin <= 8: base_layer) or k = 3 (stride 1 or 2, Cin = 16: level0, level1).  `radar` (k = 7 only): the
    (B,3,H/4,W/4) map of early fusion; the kernels read it as input channels Cin-3 .. Cin-1 at (y >> 2, x >> 2) - what
    F.interpolate(mode="nearest") + cat gives - and `x` then holds the other Cin - 3 channels.

    Forward: cf_stem_conv_forward, exact fp32 on the raw weight - no packing, no range check, no host sync - then
    cf_bn_act_train_forward.  `training=True`: batch statistics, running_mean / running_var updated in place as
    torch.nn.BatchNorm2d does (num_batches_tracked is the caller's); one value per channel raises ValueError.
    `training=False`: the affine of the running statistics, still differentiable.

    Differentiable once in weight, bn_weight, bn_bias and - for k = 3 - x; only the launches `needs_input_grad` asks for run:
    cf_bn_act_backward, then cf_stem_conv_bwd_weight and cf_stem_conv_bwd_data.  The 7x7 layer has no input gradient: an `x`
    or `radar` that requires grad raises NotImplementedError.  Every result is bitwise reproducible (no float atomics).  CPU
    tensors raise CfHipError, non-fp32 tensors and unsupported shapes NotImplementedError."""
    ho, wo = _stem_check("stem_conv_bn_relu", x, False, weight, bn_weight, bn_bias, running_mean, running_var, stride, radar)
    if weight.shape[2] == 7:
        y = _stem_apply(x, x.shape[0], ho, wo, weight, bn_weight, bn_bias, running_mean, running_var, stride, training, momentum, eps,
                        radar)
    else:
        y = _stem_apply(_to_nhwc(x), x.shape[0], ho, wo, weight, bn_weight, bn_bias, running_mean, running_var, stride, training,
                        momentum, eps, None)
    return _NhwcToNchwFn.apply(y)


def maxpool2x2(x, out=None):
    _need_cuda(x)
    B, H, W, Cc = x.shape
    if out is None:
        out = torch.empty((B, H // 2, W // 2, Cc), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().cf_maxpool2x2(x.data_ptr(), out.data_ptr(), B, H, W, Cc,
                                         _lib.stream_ptr()), "cf_maxpool2x2")
    return out


def nchw_to_nhwc4(x, out=None):
    _need_cuda(x)
    B, Cc, H, W = x.shape
    if out is None:
        out = torch.empty((B, H, W, 4), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().cf_nchw_to_nhwc4(x.data_ptr(), out.data_ptr(), B, Cc, H, W,
                                            _lib.stream_ptr()), "cf_nchw_to_nhwc4")
    return out


def nhwc_to_nchw(x, channels=None, out=None):
    _need_cuda(x)
    B, H, W, S = x.shape
    Cc = channels or S
    if out is None:
        out = torch.empty((B, Cc, H, W), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().cf_nhwc_to_nchw(x.data_ptr(), out.data_ptr(), B, H, W, Cc, S,
                                           _lib.stream_ptr()), "cf_nhwc_to_nchw")
    return out


CHECKSUM_PARTS = 256     # CF_CHECKSUM_PARTS of include/cf_hip.h


def checksum64(t, out=None):
    """Position-weighted 64-bit checksum of a contiguous device tensor's bits (cf_checksum64) as CHECKSUM_PARTS partial sums
    over a fixed partition of its words -> (256,) int64 device tensor: equal bits <=> equal parts.  No host sync."""
    _need_cuda(t)
    nbytes = t.numel() * t.element_size()
    if not t.is_contiguous() or nbytes % 4:
        raise _lib.CfHipError("checksum64: contiguous tensor of a multiple of 4 bytes")
    if out is None:
        out = torch.empty(CHECKSUM_PARTS, device=t.device, dtype=torch.int64)
    assert out.numel() == CHECKSUM_PARTS and out.dtype == torch.int64 and out.is_contiguous()
    _lib.check(_lib.load().cf_checksum64(t.data_ptr(), nbytes // 4, out.data_ptr(), _lib.stream_ptr()), "cf_checksum64")
    return out


def topk_peaks(heat, K=100, nms=False, out=None, only_if_changed=None):
    """(B,C,H,W) NCHW scores -> scores (B,K) f32, inds (B,K) i32, classes (B,K) i32.
    nms: False / True (3x3 equality NMS first; True = the two-pass form, 1 = suppress on the fly).
    out: (scores, inds, classes) to write into; only_if_changed: a (2 * CHECKSUM_PARTS,) int64 device tensor [expected parts |
    actual parts] - the launch does nothing when they are equal (cf_topk_peaks_if_changed: `out` then keeps what it held) and
    computes the NMS'd peaks otherwise (one workgroup per image: the rare path)."""
    _need_cuda(heat)
    if not heat.is_contiguous():
        heat = heat.contiguous()
    B, Cc, H, W = heat.shape
    dev = heat.device
    if out is not None:
        scores, inds, classes = out
    else:
        scores = torch.empty((B, K), device=dev, dtype=torch.float32)
        inds = torch.empty((B, K), device=dev, dtype=torch.int32)
        classes = torch.empty((B, K), device=dev, dtype=torch.int32)
    lib = _lib.load()
    mode = int(nms) if nms in (0, 1, 2) and not isinstance(nms, bool) else (2 if nms else 0)
    size = lib.cf_topk_workspace_bytes_nms(B, Cc, H, W, K) if mode == 2 else lib.cf_topk_workspace_bytes(B, K)
    ws = torch.empty(max(1, size), device=dev, dtype=torch.uint8)
    if only_if_changed is not None:
        _lib.check(lib.cf_topk_peaks_if_changed(heat.data_ptr(), B, Cc, H, W, K, mode, scores.data_ptr(), inds.data_ptr(),
                                                classes.data_ptr(), ws.data_ptr(), only_if_changed.data_ptr(),
                                                _lib.stream_ptr()), "cf_topk_peaks_if_changed")
        return scores, inds, classes
    _lib.check(lib.cf_topk_peaks(heat.data_ptr(), B, Cc, H, W, K, mode,
                                 scores.data_ptr(), inds.data_ptr(), classes.data_ptr(),
                                 ws.data_ptr(), _lib.stream_ptr()), "cf_topk_peaks")
    return scores, inds, classes


def topk_peaks_fused(heat, K=100, want_raw=True, want_tables=True):
    """cf_topk_peaks_fused: the NMS'd peaks (= topk_peaks(heat, K, nms=2)) [and the raw ones (= topk_peaks(heat, K))] from one
    read of the (B,C,H,W) map, and the slot tables of cf_head_fused_at built from them (= cf_head_slot_tables) - two launches.
    -> (raw | None, nms, table_ab | None, table_b | None); raw / nms = (scores (B,K) f32, inds (B,K) i32, classes (B,K) i32),
    table_ab (B, ceil(2K / 18), 18) i32, table_b (B, ceil(K / 18), 18) i32."""
    _need_cuda(heat)
    if not heat.is_contiguous():
        heat = heat.contiguous()
    B, Cc, H, W = heat.shape
    dev = heat.device
    new = lambda: (torch.empty((B, K), device=dev, dtype=torch.float32), torch.empty((B, K), device=dev, dtype=torch.int32),
                   torch.empty((B, K), device=dev, dtype=torch.int32))
    raw, nms = (new() if want_raw else (None, None, None)), new()
    t_ab = torch.empty((B, -(-2 * K // 18), 18), device=dev, dtype=torch.int32) if want_tables else None
    t_b = torch.empty((B, -(-K // 18), 18), device=dev, dtype=torch.int32) if want_tables else None
    lib = _lib.load()
    ws = torch.empty(max(1, lib.cf_topk_peaks_fused_workspace_bytes(B, Cc, H, W, K)), device=dev, dtype=torch.uint8)
    _lib.check(lib.cf_topk_peaks_fused(heat.data_ptr(), B, Cc, H, W, K, *(_lib.ptr(t) for t in raw), *(t.data_ptr() for t in nms),
                                       _lib.ptr(t_ab), _lib.ptr(t_b), ws.data_ptr(), _lib.stream_ptr()), "cf_topk_peaks_fused")
    return (raw if want_raw else None), nms, t_ab, t_b


def frustum_assoc(inds, depth, wh, dim, rot, calib, pc_dep, max_pc_dist=60.0, want_nhwc4=False,
                  pc_hm=None, pc_hm_nhwc4=None, pc_hm_split8=None):
    _need_cuda(inds, depth, wh, dim, rot, calib, pc_dep)
    B, _, H, W = pc_dep.shape
    K = inds.shape[1]
    dev = pc_dep.device
    if pc_hm is None:
        pc_hm = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32)
    if want_nhwc4 and pc_hm_nhwc4 is None:
        pc_hm_nhwc4 = torch.empty((B, H, W, 4), device=dev, dtype=torch.float32)
    ts = [t if t.is_contiguous() else t.contiguous() for t in (depth, wh, dim, rot, calib, pc_dep)]
    _lib.check(_lib.load().cf_frustum_assoc(inds.data_ptr(), K, *(t.data_ptr() for t in ts), B, H,
                                            W, float(max_pc_dist), pc_hm.data_ptr(),
                                            _lib.ptr(pc_hm_nhwc4), _lib.ptr(pc_hm_split8),
                                            _lib.stream_ptr()),
               "cf_frustum_assoc")
    return (pc_hm, pc_hm_nhwc4) if want_nhwc4 else pc_hm


def topk_frustum(heat, depth, wh, dim, rot, calib, pc_dep, K=100, max_pc_dist=60.0, want_nhwc4=False, want_split8=False,
                 want_peaks=False):
    """cf_topk_frustum: top-K of the raw heat map + frustum association in two launches (the slice lists are merged in the
    association kernel's prologue) - the same pc_hm as topk_peaks(heat, K) followed by frustum_assoc, bit for bit.
    -> pc_hm (B,3,H,W) [, nhwc4 (B,H,W,4)] [, split8 (B,H,W,2,8) bf16] [, (scores, inds, classes)]"""
    _need_cuda(heat, depth, wh, dim, rot, calib, pc_dep)
    B, Cc, H, W = heat.shape
    dev = heat.device
    ts = [t if t.is_contiguous() else t.contiguous() for t in (heat, depth, wh, dim, rot, calib, pc_dep)]
    pc_hm = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32)
    hm4 = torch.empty((B, H, W, 4), device=dev, dtype=torch.float32) if want_nhwc4 else None
    hm8 = torch.empty((B, H, W, 2, 8), device=dev, dtype=torch.bfloat16) if want_split8 else None
    peaks = (torch.empty((B, K), device=dev, dtype=torch.float32), torch.empty((B, K), device=dev, dtype=torch.int32),
             torch.empty((B, K), device=dev, dtype=torch.int32)) if want_peaks else (None, None, None)
    lib = _lib.load()
    ws = torch.empty(max(1, lib.cf_topk_workspace_bytes(B, K)), device=dev, dtype=torch.uint8)
    _lib.check(lib.cf_topk_frustum(ts[0].data_ptr(), Cc, K, *(t.data_ptr() for t in ts[1:]), B, H, W, float(max_pc_dist),
                                   pc_hm.data_ptr(), _lib.ptr(hm4), _lib.ptr(hm8), *(_lib.ptr(t) for t in peaks),
                                   ws.data_ptr(), _lib.stream_ptr()), "cf_topk_frustum")
    out = [pc_hm] + ([hm4] if want_nhwc4 else []) + ([hm8] if want_split8 else []) + ([peaks] if want_peaks else [])
    return out[0] if len(out) == 1 else tuple(out)


def _decode_args(scores, inds, classes, maps: dict, H, W, out_hw, norm2d, det):
    _need_cuda(scores, inds, classes)
    B, K = scores.shape
    a = _lib.DecodeArgs()
    a.scores, a.inds, a.classes = scores.data_ptr(), inds.data_ptr(), classes.data_ptr()
    keep = []
    for name in ("reg", "wh", "depth", "rot", "dim", "amodal", "att", "vel"):
        t = maps.get(name)
        if t is not None and not t.is_contiguous():
            t = t.contiguous()
        keep.append(t)
        setattr(a, name, _lib.ptr(t))
    a.B, a.K, a.H, a.W = B, K, H, W
    a.out_h, a.out_w, a.norm2d = int(out_hw[0]), int(out_hw[1]), int(bool(norm2d))
    a.det = _lib.ptr(det)
    return a, keep


def _uncertainty_map(uncertainty, B, H, W):
    """The `uncertainty` head's map as the contiguous fp32 (B,1,H,W) buffer cf_decode_*_unc read (None stays None)."""
    if uncertainty is None:
        return None
    _need_cuda(uncertainty)
    if uncertainty.dtype != torch.float32 or tuple(uncertainty.shape) != (B, 1, H, W):
        raise _lib.CfHipError(f"uncertainty must be a float32 ({B},1,{H},{W}) map, got {uncertainty.dtype} "
                              f"{tuple(uncertainty.shape)}")
    return uncertainty if uncertainty.is_contiguous() else uncertainty.contiguous()


def decode_gather(scores, inds, classes, maps: dict, H, W, out_hw, norm2d=False, uncertainty=None):
    """maps: optional NCHW tensors under reg/wh/depth/rot/dim/amodal/att/vel -> det (B,K,33).
    uncertainty: the (B,1,H,W) map of the `uncertainty` head: column 0 becomes score * exp(-exp(u)) at the peak
    (cf_decode_gather_unc); `scores` itself is never written."""
    B, K = scores.shape
    det = torch.empty((B, K, 33), device=scores.device, dtype=torch.float32)
    a, _keep = _decode_args(scores, inds, classes, maps, H, W, out_hw, norm2d, det)
    unc = _uncertainty_map(uncertainty, B, H, W)
    if unc is None:
        _lib.check(_lib.load().cf_decode_gather(C.byref(a), _lib.stream_ptr()), "cf_decode_gather")
    else:
        _lib.check(_lib.load().cf_decode_gather_unc(C.byref(a), unc.data_ptr(), _lib.stream_ptr()), "cf_decode_gather_unc")
    return det


def decode_post(scores, inds, classes, maps: dict, H, W, out_hw, calib, trans_inv, norm2d=False, want_det=False,
                uncertainty=None):
    """cf_decode_post: decode rows and postProcess rows in one launch -> post (B,K,54) [, det (B,K,33)].
    calib (B,3,4) f32, trans_inv (2,3) f32 device (output map -> source image affine).  uncertainty: as in
    decode_gather (cf_decode_post_unc)."""
    _need_cuda(calib, trans_inv)
    B, K = scores.shape
    dev = scores.device
    det = torch.empty((B, K, 33), device=dev, dtype=torch.float32) if want_det else None
    post = torch.empty((B, K, 54), device=dev, dtype=torch.float32)
    a, _keep = _decode_args(scores, inds, classes, maps, H, W, out_hw, norm2d, det)
    if calib.dtype != torch.float32 or not calib.is_contiguous() or calib.numel() != B * 12:
        raise _lib.CfHipError("cf_decode_post: calib must be contiguous float32 (B,3,4)")
    if trans_inv.dtype != torch.float32 or not trans_inv.is_contiguous() or trans_inv.numel() != 6:
        raise _lib.CfHipError("cf_decode_post: trans_inv must be contiguous float32 (2,3)")
    unc = _uncertainty_map(uncertainty, B, H, W)
    if unc is None:
        _lib.check(_lib.load().cf_decode_post(C.byref(a), calib.data_ptr(), trans_inv.data_ptr(), post.data_ptr(),
                                              _lib.stream_ptr()), "cf_decode_post")
    else:
        _lib.check(_lib.load().cf_decode_post_unc(C.byref(a), unc.data_ptr(), calib.data_ptr(), trans_inv.data_ptr(),
                                                  post.data_ptr(), _lib.stream_ptr()), "cf_decode_post_unc")
    return (post, det) if want_det else post


def depth_maps(maps, out=None):
    """cf_depth_maps: the normalised uint8 maps of the reference's Detector.post_process (detector.py:381-393) for a list of
    (B,1,H,W) fp32 device maps of one batch, in one launch -> (len(maps),B,H,W) uint8 device tensor.  Row 0 and column 0 of
    image 0 count as 0 (the reference's quirk); a flat image gives 0."""
    maps = list(maps)
    if not 1 <= len(maps) <= _lib.CF_DEPTH_MAPS_MAX:
        raise _lib.CfHipError(f"depth_maps: 1..{_lib.CF_DEPTH_MAPS_MAX} maps, got {len(maps)}")
    _need_cuda(*maps)
    B, one, H, W = maps[0].shape
    for t in maps:
        if t.dtype != torch.float32 or tuple(t.shape) != (B, 1, H, W):
            raise _lib.CfHipError(f"depth_maps: every map must be float32 ({B},1,{H},{W}), got {t.dtype} {tuple(t.shape)}")
    # a channel view of a wider tensor (pc_hm_in = pc_dep[:, :1]) is read in place: only its batch stride differs
    keep = [t if (B == 1 or t.stride(0) >= H * W) and t.stride(2) == W and t.stride(3) == 1 else t.contiguous() for t in maps]
    if out is None:
        out = torch.empty((len(keep), B, H, W), device=keep[0].device, dtype=torch.uint8)
    assert out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (len(keep), B, H, W)
    ptrs = (_lib._f * len(keep))(*(t.data_ptr() for t in keep))
    strides = (C.c_long * len(keep))(*(max(t.stride(0), H * W) for t in keep))
    _lib.check(_lib.load().cf_depth_maps(ptrs, strides, len(keep), B, H, W, out.data_ptr(), _lib.stream_ptr()), "cf_depth_maps")
    return out


def serialize_nuscenes(post, trans_matrix, velocity_matrix, cs_rot=None, pose_rot=None, sample_ptr=None,
                       sample_frames=None, max_per_sample=500):
    """cf_serialize_nuscenes -> rows (B*K,12) f32, rotation (B*K,4) f64, order (S,max) i32, counts (S) i32
    (order / counts are None without the sample tables)."""
    _need_cuda(post, trans_matrix, velocity_matrix)
    B, K, w = post.shape
    dev = post.device
    for t, dt, n in ((post, torch.float32, B * K * 54), (trans_matrix, torch.float32, B * 16),
                     (velocity_matrix, torch.float32, B * 16)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() != n:
            raise _lib.CfHipError("cf_serialize_nuscenes: wrong dtype / shape / non-contiguous input")
    a = _lib.SerializeArgs()
    a.post, a.B, a.K = post.data_ptr(), B, K
    a.trans_matrix, a.velocity_matrix = trans_matrix.data_ptr(), velocity_matrix.data_ptr()
    if (cs_rot is None) != (pose_rot is None):
        raise _lib.CfHipError("cf_serialize_nuscenes: cs_rot and pose_rot go together")
    for q in (cs_rot, pose_rot):
        if q is not None and (q.dtype != torch.float64 or not q.is_contiguous() or q.numel() != B * 4 or not q.is_cuda):
            raise _lib.CfHipError("cf_serialize_nuscenes: quaternions must be contiguous float64 (B,4) on the device")
    a.cs_rot, a.pose_rot = _lib.ptr(cs_rot), _lib.ptr(pose_rot)
    rows = torch.empty((B * K, 12), device=dev, dtype=torch.float32)
    rotation = torch.empty((B * K, 4), device=dev, dtype=torch.float64)
    a.rows, a.rotation = rows.data_ptr(), rotation.data_ptr()
    order = counts = None
    if sample_ptr is not None:
        _need_cuda(sample_ptr, sample_frames)
        if sample_ptr.dtype != torch.int32 or sample_frames.dtype != torch.int32:
            raise _lib.CfHipError("cf_serialize_nuscenes: sample tables must be int32")
        S = sample_ptr.numel() - 1
        order = torch.empty((S, max_per_sample), device=dev, dtype=torch.int32)
        counts = torch.empty((S,), device=dev, dtype=torch.int32)
        a.n_samples, a.sample_ptr, a.sample_frames = S, sample_ptr.data_ptr(), sample_frames.data_ptr()
        a.max_per_sample, a.order, a.counts = int(max_per_sample), order.data_ptr(), counts.data_ptr()
    _lib.check(_lib.load().cf_serialize_nuscenes(C.byref(a), _lib.stream_ptr()), "cf_serialize_nuscenes")
    return rows, rotation, order, counts


def _radar_expand(entry, extra, pc_2d, pc_3d, counts, calib, trans, out_hw, want_aux):
    """What cf_pillar_expand and cf_radar_roi_expand share: the input checks, the outputs and the call (`extra`: the
    arguments between W and pc_dep).  -> pc_dep (B,3,H,W) f32 [, keep (B,Nmax) u8, xy (B,2,Nmax) f64]."""
    _need_cuda(pc_2d, pc_3d, counts, calib, trans)
    B, _, max_n = pc_2d.shape
    H, W = out_hw
    dev = pc_2d.device
    pc_dep = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32)
    keep = torch.empty((B, max_n), device=dev, dtype=torch.uint8) if want_aux else None
    xy = torch.empty((B, 2, max_n), device=dev, dtype=torch.float64) if want_aux else None
    for t, dt in ((pc_2d, torch.float64), (pc_3d, torch.float64), (counts, torch.int32),
                  (calib, torch.float64), (trans, torch.float64)):
        if t.dtype != dt or not t.is_contiguous():
            raise _lib.CfHipError(f"{entry}: wrong dtype / non-contiguous input")
    _lib.check(getattr(_lib.load(), entry)(pc_2d.data_ptr(), pc_3d.data_ptr(), counts.data_ptr(), B, max_n, pc_3d.shape[1],
                                           calib.data_ptr(), trans.data_ptr(), H, W, *extra, pc_dep.data_ptr(),
                                           _lib.ptr(keep), _lib.ptr(xy), _lib.stream_ptr()), entry)
    return (pc_dep, keep, xy) if want_aux else pc_dep


def pillar_expand(pc_2d, pc_3d, counts, calib, trans, out_hw, pillar_dims=(1.5, 0.2, 0.2),
                  want_aux=False):
    """pc_2d (B,3,Nmax) f64, pc_3d (B,R,Nmax) f64, counts (B) i32, calib (B,3,4) f64,
    trans (B,2,3) f64  ->  pc_dep (B,3,H,W) f32 [, keep (B,Nmax) u8, xy (B,2,Nmax) f64]."""
    return _radar_expand("cf_pillar_expand", [float(v) for v in pillar_dims], pc_2d, pc_3d, counts, calib, trans, out_hw,
                         want_aux)


ROI_METHODS = {"pillars": 0, "points": 1, "heatmap": 2}     # DATASET.PC_ROI_METHOD -> `method` of cf_radar_roi_expand


def roi_method_id(roi_method):
    """generic_dataset.py:820-821: anything but the three known methods raises (before any device work)."""
    if roi_method not in ROI_METHODS:
        raise ValueError(f"Invalid PC_ROI_METHOD: {roi_method}")
    return ROI_METHODS[roi_method]


def radar_roi_expand(pc_2d, pc_3d, counts, calib, trans, out_hw, roi_method, want_aux=False):
    """cf_radar_roi_expand: the inputs / outputs of `pillar_expand` for roi_method "points" (one pixel per point) or "heatmap"
    (a depth-dependent square per point)."""
    method = roi_method_id(roi_method)
    if method == 0:
        raise ValueError("radar_roi_expand: 'pillars' is pillar_expand (it needs the pillar dimensions)")
    return _radar_expand("cf_radar_roi_expand", [method], pc_2d, pc_3d, counts, calib, trans, out_hw, want_aux)


def stem_args(ps, x, out, shape=None, out_pool=None, in_scales=None, into=None) -> _lib.StemArgs:
    """x may be None with shape=(B, C, H, W) given: the image pointer is then patched in per call.
    out_pool: optional (B, H/4, W/4, 32) buffer for the 2x2 max-pool of the level1 map.
    in_scales: activation pre-scales (powers of two) of the image, base_layer's output, level0's output (None = 16 each).
    into: fill this block (the `stem` member of a StemEarlyArgs) instead of a new one."""
    a = _lib.StemArgs() if into is None else into
    B, Cc, H, W = shape if x is None else x.shape
    a.x, a.B, a.C, a.H, a.W = (_lib.ptr(x), B, Cc, H, W)
    a.w_base, a.b_base, a.scale_base = ps.w_base.data_ptr(), ps.b_base.data_ptr(), ps.scale_base
    a.w_level0, a.b_level0, a.scale_level0 = ps.w_level0.data_ptr(), ps.b_level0.data_ptr(), ps.scale_level0
    a.w_level1, a.b_level1, a.scale_level1 = ps.w_level1.data_ptr(), ps.b_level1.data_ptr(), ps.scale_level1
    a.out = out.data_ptr()
    a.out_pool = _lib.ptr(out_pool)
    if in_scales is not None:
        for i, (s, name) in enumerate(zip(in_scales, ("scale_base", "scale_level0", "scale_level1"))):
            if s is not None and float(s) != DEFAULT_IN_SCALE:
                a.in_scale[i] = float(s)
                setattr(a, name, _scaled_out_scale(getattr(a, name), s, "stem_args"))
    return a


def stem_fused(ps, x, out=None, out_pool=None, in_scales=None):
    """images (B, C<=3, H, W) fp32 NCHW -> level1 map (B, H/2, W/2, 32) fp32 NHWC (packing.pack_stem); out_pool: also its
    MaxPool2d(2, 2), (B, H/4, W/4, 32).  in_scales: as stem_args."""
    _need_cuda(x, out_pool)
    B, Cc, H, W = x.shape
    if out is None:
        out = torch.empty((B, H // 2, W // 2, 32), device=x.device, dtype=torch.float32)
    a = stem_args(ps, x.contiguous(), out, out_pool=out_pool, in_scales=in_scales)
    _lib.check(_lib.load().cf_stem_fused(C.byref(a), _lib.stream_ptr()), "cf_stem_fused")
    return out


def stem_early_args(ps, x, pc, out, shape=None, out_pool=None, in_scales=None) -> _lib.StemEarlyArgs:
    """cf_stem_fused_early's block: stem_args (x: the 3-channel image, may be None with shape given) + the radar map pc
    (B, 3, H/4, W/4) NCHW fp32 (may be None: patched per call; its size is then taken from `shape`) + the radar fragments."""
    assert ps.w_base_radar is not None, "weights packed without the radar part (packing.pack_stem_early)"
    e = _lib.StemEarlyArgs()
    stem_args(ps, x, out, shape=shape, out_pool=out_pool, in_scales=in_scales, into=e.stem)
    e.pc = _lib.ptr(pc)
    e.pc_h, e.pc_w = (e.stem.H // 4, e.stem.W // 4) if pc is None else pc.shape[2:]
    e.w_base_radar = ps.w_base_radar.data_ptr()
    return e


def stem_fused_early(ps, x, pc, out=None, out_pool=None, in_scales=None):
    """Early radar fusion: images (B, 3, H, W) + radar map (B, 3, H/4, W/4), both fp32 NCHW -> the level1 map of the six-channel
    stem, (B, H/2, W/2, 32) fp32 NHWC (packing.pack_stem_early); out_pool as in stem_fused.  The map is read, not written.
    in_scales: as stem_args."""
    _need_cuda(x, pc, out_pool)
    B, Cc, H, W = x.shape
    if pc.dim() != 4 or pc.shape[0] != B or pc.shape[1] != 3 or pc.dtype != torch.float32:
        raise _lib.CfHipError(f"stem_fused_early: the radar map must be float32 (B, 3, H/4, W/4), got {tuple(pc.shape)}")
    if out is None:
        out = torch.empty((B, H // 2, W // 2, 32), device=x.device, dtype=torch.float32)
    a = stem_early_args(ps, x.contiguous(), pc.contiguous(), out, out_pool=out_pool, in_scales=in_scales)
    _lib.check(_lib.load().cf_stem_fused_early(C.byref(a), _lib.stream_ptr()), "cf_stem_fused_early")
    return out


def radar_ingest(pc, counts, intrinsics, img_wh, max_dist=60.0, z_offset=0.0, descending=False):
    """pc (B,R,Nmax) f64 padded raw sweeps, counts (B) i32, intrinsics (B,3,3) f64 ->
    pc_2d (B,3,Nmax) f64, pc_3d (B,R,Nmax) f64, counts_out (B) i32 - the inputs of pillar_expand."""
    _need_cuda(pc, counts, intrinsics)
    for t, dt in ((pc, torch.float64), (counts, torch.int32), (intrinsics, torch.float64)):
        if t.dtype != dt or not t.is_contiguous():
            raise _lib.CfHipError("cf_radar_ingest: wrong dtype / non-contiguous input")
    B, R, max_n = pc.shape
    pc_2d = torch.empty((B, 3, max_n), device=pc.device, dtype=torch.float64)
    pc_3d = torch.empty((B, R, max_n), device=pc.device, dtype=torch.float64)
    cnt = torch.empty((B,), device=pc.device, dtype=torch.int32)
    _lib.check(_lib.load().cf_radar_ingest(pc.data_ptr(), counts.data_ptr(), B, R, max_n, intrinsics.data_ptr(),
                                           int(img_wh[0]), int(img_wh[1]), float(max_dist), float(z_offset),
                                           int(bool(descending)), pc_2d.data_ptr(), pc_3d.data_ptr(), cnt.data_ptr(),
                                           _lib.stream_ptr()), "cf_radar_ingest")
    return pc_2d, pc_3d, cnt


OPTIM_CHUNK = _lib.CF_OPTIM_CHUNK     # elements one workgroup of the optimizer kernels owns (CF_OPTIM_CHUNK of include/cf_hip.h; optim.py)
