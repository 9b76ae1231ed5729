"""`_Plan`: the execution plan of one forward shape - every intermediate NHWC buffer laid out once, the argument block of
every launch pre-built, a forward pass = the flat list `steps` issued on the caller's stream (and, with lanes, one side
stream).  Built from a `DLASeg` (knobs, packed weights, pre-scales); the finished plan keeps no reference to the model."""
import ctypes as C
import weakref
from typing import Dict, List

import torch

from . import _lib, ops, packing
from .pending import PendingOutputs
from ._lib import (ACT_NONE, ACT_RELU, ACT_SIGMOID_CLAMP, ACT_RAW_AND_SIGDEPTH, LAYOUT_NHWC, LAYOUT_NCHW)
from .streams import _side_streams

SECONDARY_HEADS = ["velocity", "nuscenes_att", "depth2", "rotation2"]   # detectHeads.py:146-153
AT_SLOTS = 18                                  # pixels per virtual tile of cf_head_fused_at (include/cf_hip.h)
AT_TIMED = ("at.topk", "at.peaks", "at.tables", "at.primary")   # `timed` keys of the launches an at-peaks forward adds


def feat_operand(model):
    """(trailing shape, dtype) of the buffer the heads' first layers read beside the fp32 feature map (B, h4, w4, 64): the
    272-byte fp16 + FP6 rows (heads_mx), the split-bf16 copy, or None - the exact-fp32 heads read the map itself."""
    if not model._heads_bf():
        return None
    return ((packing.MX_ROW,), torch.uint8) if model._mx_active else ((2, 64), torch.bfloat16)


def act_of(h):
    return ACT_SIGMOID_CLAMP if h == "heatmap" else (ACT_RAW_AND_SIGDEPTH if h in ("depth", "depth2") else ACT_NONE)


class _Plan:
    """Buffers + pre-built launch list for one (B, H, W, device)."""

    def __init__(self, model: "DLASeg", B, H, W, device, part="all", feat=None, feat_in=None):
        """part: "all" (one plan per forward), or the two halves of the split forward (DLASeg.streams > 1):
        "base" = the backbone alone, run like a trunk (run_trunk), its level 2-5 maps kept in `levels` (DLASeg.forward_base);
        "stem" = base_layer + level0 + level1 alone, run like a trunk, the (B, H/2, W/2, 32) map of level 1 in `levels`
        (DLASeg.forward_stem; early fusion: the six-channel stem);
        "trunk" = backbone + neck of a sub-batch, its last DCN writing the feature map (and its split-bf16 copy)
        into the caller's `feat` / `feat_in` slices; "heads" = everything behind the feature map for the WHOLE
        batch, reading the full `feat` / `feat_in` buffers the trunks filled."""
        self.B, self.H, self.W, self.device = B, H, W, device
        self.h4, self.w4 = H // 4, W // 4
        self.part = part
        self.lib = _lib.load()
        self.steps = []          # (fn, args...) tuples executed in order (stream appended at run)
        self.lanes = []          # per step: 0 = the caller's stream, 1 = the plan's side stream (see _ida)
        self.lane = 0
        self.n_events = 0
        # two-lane issue of the neck for small batches (a launch cannot fill the chip there); never with the timed /
        # graph paths, which want one stream
        # (a trunk sub-batch of the two-stream forward keeps round 5's limit of 4 frames: its side lane would be a third / fourth
        #  stream beside the other trunk, and the event traffic of that costs more than the overlap gives)
        self.use_lanes = bool(model.lanes) and part != "heads" and \
            B * (H // 4) * (W // 4) <= (model.lanes_max_frames if part == "all" else min(4, model.lanes_max_frames)) * 112 * 200
        self._side = self._events = None   # the side stream and the lanes' events: taken at the first two-lane _launch
        self.keep = []           # keeps arg blocks / buffers alive
        self.bytes = 0
        self.step_index = {}     # conv name -> index in self.steps
        self.step_flops = {}     # conv name -> algorithmic FLOPs of that launch (2*MACs)
        self.timed = {}          # step index -> [(start_event, end_event)] filled while timing is on
        self.inputs = {}         # layer name -> the resident NHWC tensors that layer's GEMM reads (DLASeg.activation_ranges)
        self.hidden = set()      # layer names with operands that never reach HBM in this plan (fused intermediates)
        self.debug = {}          # NHWC stage outputs (tests only)
        # trunk: the per-call input step, the fused stem's argument block or the NHWC copy of the images, the argument block
        # of the DCN whose output is the feature map (set by _dcn_node), the max-pools already issued (data_ptr -> output)
        self.in_step = self.stem = self.x4 = self.feat_producer = None
        # early fusion: the plan's model is one; the step that normalises the caller's radar map (part "all": in front of the stem);
        # the three-hidden-layer heads on the image features (their own launch); their split-bf16 operand where the primary group reads mx rows
        self.early, self.direct_step, self.chained, self.feat_bf = bool(model.isEarly), None, [], None
        self._pooled = {}
        self._pre = {}           # projection name -> output computed ahead by a grouped launch (_ida / _dcn_group)
        # heads: per-call output tensors are patched into the arg blocks in `outs` / `tails`; the other steps patched per
        # call; the radar maps the secondary heads read; the frustum chain's top-k; the decoder's peaks lane
        self.primary, self.radar, self.frustum, self.K = [], False, False, int(model.config.MODEL.K)
        self.outs: Dict[str, List] = {}
        self.tails = {}
        self.peaks_step = self.topk_step = self.frustum_step = None
        self.pc_hm4 = self.pc_hm8 = None
        self.tk_scores = self.tk_inds = self.tk_cls = self.tk_ws = None
        self.pk_ws = self.ev_peaks = None
        # heads at the peaks (model.heads_at_peaks, _build_at): the launch blocks and slot tables, (tail block, index) of every
        # primary head in the split blocks, per group (dense FLOPs, FLOPs per pixel), the last pending outputs (weak)
        self.at, self.at_tails, self.group_flops, self.group_srcs, self._last = None, {}, {}, {}, None
        self.feat, self.feat_in = feat, feat_in
        self._m, self._pk = model, model._packed     # for the builders only: a finished plan must not hold the model
        try:                                         # (model -> _plans -> plan -> model would leave a dropped plan set to the collector)
            if part != "heads":
                self._build_trunk()
            if part not in ("trunk", "base", "stem"):
                self._build_heads()
        finally:
            self._m = self._pk = None

    # ------------------------------------------------------------------------------------------ builders: shared
    def _buf(self, *shape, dtype=torch.float32):
        t = torch.empty(shape, device=self.device, dtype=dtype)
        self.bytes += t.numel() * t.element_size()
        self.keep.append(t)
        return t

    def _add(self, name, flops, step, *keep):
        """Register one named launch: the objects it needs alive, its index and algorithmic FLOPs under `name` (a launch
        without a GEMM: flops None), the step itself (None: patched per call).  -> the step's index"""
        self.keep += keep
        self.step_index[name] = len(self.steps)
        if flops is not None:
            self.step_flops[name] = flops
        self.add_step(step)
        return len(self.steps) - 1

    def _slot(self):
        """an unnamed step that is patched per call -> its index"""
        self.add_step(None)
        return len(self.steps) - 1

    # ------------------------------------------------------------------------------------------ builders: trunk
    def _conv(self, name, srcs, h, w, act=ACT_RELU, residual=None, out=None, out_stride=None):
        # everything that feeds the DCN neck sums in two levels (cf_gemm.hip: PRECISE)
        m, B, pc = self._m, self.B, self._pk[name]
        ho = (h + 2 * pc.pad - pc.kh) // pc.stride + 1
        wo = (w + 2 * pc.pad - pc.kh) // pc.stride + 1
        if out is None:
            out = self._buf(B, ho, wo, pc.n)
        a = ops.conv_args(pc, srcs, [s.shape[-1] for s in srcs], B, h, w, out, out_stride or pc.n, act, residual,
                          residual.shape[-1] if residual is not None else 0, LAYOUT_NHWC, None, 0, m.precise,
                          in_scale=m._scale(name) if pc.out_scale > 0 else None)
        self.inputs[name] = list(srcs)
        fn = self.lib.cf_conv2d_fused
        if pc.out_scale > 0:
            fn = self.lib.cf_conv3x3_f16x3 if (pc.patch and m.conv_patch) else self.lib.cf_conv2d_f16x3
        self._add(name, 2.0 * B * ho * wo * pc.n * (pc.kh * pc.kh * sum(int(c) for c in pc.real_cin)), (fn, C.byref(a)), a)
        return out

    def _pool(self, x):
        # (a two-level Tree pools its input for its own Root AND its first sub-tree pools the same tensor again,
        #  dla.py:96,107 at both nesting levels: one launch serves both; the stem's out_pool pre-seeds the level-2 one)
        if x.data_ptr() in self._pooled:
            return self._pooled[x.data_ptr()]
        _, h, w, c = x.shape
        o = self._buf(self.B, h // 2, w // 2, c)
        self.add_step((self.lib.cf_maxpool2x2, x.data_ptr(), o.data_ptr(), self.B, h, w, c))
        self._pooled[x.data_ptr()] = o
        return o

    def _block(self, p, x, residual, pooled=None):
        m, B = self._m, self.B
        _, h, w, _ = x.shape
        t = self._conv(p + ".conv1", [x], h, w)
        _, ho, wo, _ = t.shape
        if pooled is None:
            return self._conv(p + ".conv2", [t], ho, wo, residual=residual if residual is not None else x)
        # conv2 + the Tree's project of the pooled input in one step (weights packed together: DLASeg._prepare.tree1)
        pc = self._pk[p + ".conv2"]
        o = self._buf(B, ho, wo, pc.n)
        a = ops.conv_args(pc, [t, pooled], [t.shape[-1], pooled.shape[-1]], B, ho, wo, o, pc.n, ACT_RELU, None, 0,
                          LAYOUT_NHWC, None, 0, False, in_scale=m._scale(p + ".conv2"))   # (one pre-scale for both parts)
        self.inputs[p + ".conv2"], self.inputs[p[:-len(".tree1")] + ".project"] = [t], [pooled]
        ch = (C.c_int32 * 2)(*[int(c) for c in pc.real_cin])
        step = (self.lib.cf_conv3x3_proj_f16x3, C.byref(a), ch) if m.conv_patch else (self.lib.cf_conv2d_f16x3, C.byref(a))
        self._add(p + ".conv2+project", 2.0 * B * ho * wo * pc.n * (9 * pc.real_cin[0] + pc.real_cin[1]), step, a, ch)
        return o

    def _tree(self, p, levels, x, stride, level_root, children=None):
        m, B, pk = self._m, self.B, self._pk
        children = [] if children is None else children
        bottom = self._pool(x) if stride > 1 else x
        proj_fused = levels == 1 and getattr(pk[p + ".tree1.conv2"], "proj_k", 0) > 0
        if proj_fused:
            residual = None
        elif (p + ".project") in pk:
            _, h, w, _ = bottom.shape
            residual = self._conv(p + ".project", [bottom], h, w, act=ACT_NONE)
        else:
            residual = bottom
        if level_root:
            children.append(bottom)
        if levels > 1:
            x1 = self._tree(p + ".tree1", levels - 1, x, stride, False)
            children.append(x1)
            return self._tree(p + ".tree2", levels - 1, x1, 1, False, children)
        x1 = self._block(p + ".tree1", x, residual, pooled=bottom if proj_fused else None)
        _, h, w, _ = x1.shape
        pc2, pcr = pk[p + ".tree2.conv2"], pk[p + ".root"]
        if not (m.root_fuse and m.conv_patch and pc2.out_scale > 0 and pcr.out_scale > 0
                and getattr(pc2, "patch", False) and pc2.stride == 1 and (not children or m.root_fuse_children)):
            x2 = self._block(p + ".tree2", x1, None)
            return self._conv(p + ".root", [x2, x1, *children], h, w)
        # tree2.conv2 and the Root as ONE step (cf_conv3x3_root_f16x3): x2 is never written where a workgroup
        # holds every channel of its pixels (64 / 128 / 256 channels: levels 2-4; children are read from HBM
        # inside the launch); the library runs the two launches for every other shape, bit-identical either way
        t = self._conv(p + ".tree2.conv1", [x1], h, w)
        x2, o = self._buf(B, h, w, pc2.n), self._buf(B, h, w, pcr.n)
        a2 = ops.conv_args(pc2, [t], [t.shape[-1]], B, h, w, x2, pc2.n, ACT_RELU, x1, x1.shape[-1],
                           LAYOUT_NHWC, None, 0, False, in_scale=m._scale(p + ".tree2.conv2"))
        rsrcs = [x2, x1, *children]
        ar = ops.conv_args(pcr, rsrcs, [s_.shape[-1] for s_ in rsrcs], B, h, w, o, pcr.n, ACT_RELU, None, 0,
                           LAYOUT_NHWC, None, 0, False, in_scale=m._scale(p + ".root"))
        self.inputs[p + ".tree2.conv2"], self.inputs[p + ".root"] = [t], [x1, *children]
        self.hidden.add(p + ".root")             # (x2 stays on the chip)
        rch = (C.c_int32 * len(rsrcs))(*[int(c) for c in pcr.real_cin])
        flops = 2.0 * B * h * w * (pc2.n * 9 * sum(int(c) for c in pc2.real_cin) + pcr.n * sum(int(c) for c in pcr.real_cin))
        self._add(p + ".tree2.conv2+root", flops, (self.lib.cf_conv3x3_root_f16x3, C.byref(a2), C.byref(ar), rch), a2, ar, rch)
        return o

    def _dcn_node(self, p, x, out=None, feat_producer=False):
        m, B = self._m, self.B
        _, h, w, c = x.shape
        om = self._buf(B, h, w, 32)
        self._conv(p + ".conv_offset_mask", [x], h, w, act=ACT_NONE, out=om, out_stride=32)
        pd = self._pk[p]
        o = self._buf(B, h, w, pd.n) if out is None else out
        ws = None
        if pd.out_scale > 0:
            nbytes = self.lib.cf_dcn_v2_workspace_bytes(B, h, w, pd.c, pd.n_pad)
            ws = self._buf(nbytes, dtype=torch.uint8) if nbytes else None
        a = ops.dcn_args(pd, x, om, 32, B, h, w, o, pd.n, ACT_RELU, precise=m.precise, workspace=ws,
                         in_scale=m._scale(p) if pd.out_scale > 0 else None)
        if feat_producer:
            self.feat_producer = a                       # the DCN that writes the feature map (the last node of ida_up)
        self.inputs[p] = [x]
        fn = self.lib.cf_dcn_v2_f16x3 if pd.out_scale > 0 else self.lib.cf_dcn_v2_fused
        self._add(p, 2.0 * B * h * w * pd.n * 9 * pd.c, (fn, C.byref(a)), a)
        return o

    def _dcn_group(self, members):
        """The DeformConv projections `members` = [(layer name, input)] - one shape, independent inputs - as TWO launches:
        cf_conv3x3_f16x3_grouped (the offset convolutions) and cf_dcn_v2_f16x3_grouped (+ its one reduction on K-split maps).
        `om` and the outputs are slices of one buffer each; every layer keeps its own weights, bias and pre-scale, so each
        slice carries the bits of that layer's own two launches.  -> the output slices, in order.
        The step names stay per layer (tools/layer_times.py, time_launch): the set's launch sits under its FIRST member
        with the FLOPs of all of them; the other members' names point at the same step and carry no FLOPs."""
        m, B, G = self._m, self.B, len(members)
        _, h, w, c = members[0][1].shape
        pd0 = self._pk[members[0][0]]
        om = self._buf(G, B, h, w, 32)
        out = self._buf(G, B, h, w, pd0.n)
        nbytes = self.lib.cf_dcn_v2_workspace_bytes(B, h, w, pd0.c, pd0.n_pad)
        ws = self._buf(G * nbytes, dtype=torch.uint8) if nbytes else None
        ca, da, flops_c, flops_d = [], [], 0.0, 0.0
        for g, (name, x) in enumerate(members):
            pc, pd = self._pk[name + ".conv_offset_mask"], self._pk[name]
            ca.append(ops.conv_args(pc, [x], [c], B, h, w, om[g], 32, ACT_NONE, None, 0, LAYOUT_NHWC, None, 0, m.precise,
                                    in_scale=m._scale(name + ".conv_offset_mask")))
            da.append(ops.dcn_args(pd, x, om[g], 32, B, h, w, out[g], pd.n, ACT_RELU, precise=m.precise, workspace=ws,
                                   in_scale=m._scale(name)))
            self.inputs[name + ".conv_offset_mask"], self.inputs[name] = [x], [x]
            flops_c += 2.0 * B * h * w * pc.n * 9 * sum(int(v) for v in pc.real_cin)
            flops_d += 2.0 * B * h * w * pd.n * 9 * pd.c
        cp, dp = ops.group_ptrs(ca), ops.group_ptrs(da)
        # (the other members first: whoever inverts step_index - all_launch_times - then finds the first member's name last)
        for name, _ in members[1:]:
            self.step_index[name + ".conv_offset_mask"], self.step_index[name] = len(self.steps), len(self.steps) + 1
            self.step_flops[name + ".conv_offset_mask"] = self.step_flops[name] = 0.0
        first = members[0][0]
        self._add(first + ".conv_offset_mask", flops_c, (self.lib.cf_conv3x3_f16x3_grouped, cp, G), cp, ca)
        self._add(first, flops_d, (self.lib.cf_dcn_v2_f16x3_grouped, dp, G), dp, da)
        return [out[g] for g in range(G)]

    def _groupable(self, name, x):
        """(shape key) of a projection the grouped launches can carry - split-fp16 offset convolution on the patch kernel
        (N_pad = 32) and split-fp16 DCN with whole-row epilogue - or None."""
        m, pc, pd = self._m, self._pk[name + ".conv_offset_mask"], self._pk[name]
        ok = pc.out_scale > 0 and getattr(pc, "patch", False) and m.conv_patch and pc.n_pad == 32 and \
            pd.out_scale > 0 and pd.n % 4 == 0 and pd.n_pad <= 128
        return (tuple(x.shape), pc.k_pad, pd.c, pd.n, pd.n_pad) if ok else None

    def _ida(self, p, layers, startp, endp, final_out=None, feat=False, also=()):
        """IDAUp.forward (dla.py:518-524).  The projections of one IDA level read maps that all exist when the level
        starts and do not depend on each other or on the nodes, so with `self.use_lanes` they are issued on a side
        stream (offset conv + DCN per projection) while the caller's stream runs the node chain
        upsample+skip -> offset conv -> DCN, waiting for projection j right before it consumes it.  Small
        batches only: there a single launch cannot fill the chip and the two chains overlap (bit-identical).
        Without lanes (model.neck_groups): the level's projections of ONE shape - and those of a later level in `also` =
        [(name, input)] whose inputs exist already - run as one grouped pair of launches in front of the node chain
        (_dcn_group); their outputs wait in `self._pre` for the level that consumes them."""
        projs = {}
        if self._m.neck_groups and not self.use_lanes:
            sets = {}
            for name, x in [(f"{p}.proj_{i - startp}", layers[i]) for i in range(startp + 1, endp)] + list(also):
                key = self._groupable(name, x) if name not in self._pre else None
                if key is not None:
                    sets.setdefault(key, []).append((name, x))
            for members in sets.values():
                for k in range(0, len(members), _lib.CF_MAX_GROUPS):
                    part = members[k:k + _lib.CF_MAX_GROUPS]
                    if len(part) > 1:
                        self._pre.update(zip([n for n, _ in part], self._dcn_group(part)))
        if self.use_lanes:
            self.ctl("rec", 0, ev0 := self.new_event())      # everything the projections read is complete here
            self.ctl("wait", 1, ev0)
            self.lane = 1
            for i in range(startp + 1, endp):
                projs[i] = self._dcn_node(f"{p}.proj_{i - startp}", layers[i])
                self.ctl("rec", 1, ev := self.new_event())
                projs[i] = (projs[i], ev)
            self.lane = 0
        for i in range(startp + 1, endp):
            j = i - startp
            if self.use_lanes:
                proj, ev = projs[i]
                self.ctl("wait", 0, ev)
            elif f"{p}.proj_{j}" in self._pre:
                proj = self._pre.pop(f"{p}.proj_{j}")
            else:
                proj = self._dcn_node(f"{p}.proj_{j}", layers[i])
            wk, f = self._pk[f"{p}.up_{j}"]
            _, h, w, c = proj.shape
            summed = self._buf(self.B, h * f, w * f, c)          # up(proj(x)) + skip, fused
            self.add_step((self.lib.cf_upsample_dw, proj.data_ptr(), wk.data_ptr(),
                           layers[i - 1].data_ptr(), summed.data_ptr(), self.B, h, w, c, f))
            layers[i] = self._dcn_node(f"{p}.node_{j}", summed, out=final_out if i == endp - 1 else None,
                                       feat_producer=feat and i == endp - 1)

    def _build_trunk(self):
        m, B, H, W, pk = self._m, self.B, self.H, self.W, self._pk
        if self.early and self.part == "all":
            # base_model.py:69-79: the caller's radar map is normalised in place BEFORE the stem reads it (cf_pc_hm_direct without its
            # channels-last outputs; patched per call).  The split forward does this once for the whole batch (DLASeg._forward_concurrent)
            self.direct_step = self._add("pc_hm_direct", 0.0, None)
        # ---- backbone.  The first step reads the images: patched per call (_patch_input)
        if "base.stem" in pk:
            # base_layer + level0 + level1 in one launch; the full-resolution maps stay in LDS
            y0, y1 = None, self._buf(B, H // 2, W // 2, 32)
            # ... and the level-2 Tree's 2x2 max-pool of that map (dla.py:96) comes out of the same launch
            y1p = self._buf(B, H // 4, W // 4, 32) if m.stem_pool and self.part != "stem" else None
            if y1p is not None:
                self._pooled[y1.data_ptr()] = y1p
            stem_layers = ("base.base_layer", "base.level0", "base.level1")
            kw = dict(shape=(B, 3, H, W), out_pool=y1p, in_scales=[m._scale(n) for n in stem_layers])
            self.stem = ops.stem_early_args(pk["base.stem"], None, None, y1, **kw) if self.early else \
                ops.stem_args(pk["base.stem"], None, y1, **kw)
            self.hidden.update(stem_layers)              # (the image is the caller's, the two maps stay in LDS)
            k_base = 16 * 49 * (6 if self.early else 3)
            self.in_step = self._add("base.stem", 2.0 * B * H * W * (k_base + 16 * 144 + 32 * 144 / 4), None, self.stem)
        else:
            self.in_step = self._slot()
            # (early fusion: [image 0-2 | radar 3-5 | 0 0] per pixel - the six-channel image exists only on these exact-fp32 paths)
            self.x4 = self._buf(B, H, W, 8 if self.early else 4)
            if self.early:
                self.x4.zero_()
            t = self._conv("base.base_layer", [self.x4], H, W)
            y0 = self._conv("base.level0", [t], H, W)
            y1 = self._conv("base.level1", [y0], H, W)
        layers = [y0, y1]
        if self.part == "stem":
            self.levels = [y1]                       # level 1: what DLASeg.forward_levels reads (DLASeg.forward_stem)
            return
        for lvl, levels, root in ((2, 1, False), (3, 2, True), (4, 2, True), (5, 1, True)):
            layers.append(self._tree(f"base.level{lvl}", levels, layers[-1], 2, root))
        self.debug = {f"y{i}": t for i, t in enumerate(layers) if t is not None}
        if self.part == "base":
            self.levels = layers[2:]                 # levels 2-5: what the neck reads (DLASeg.forward_base)
            return
        # ---- DLA-up + IDA-up neck
        out = [layers[-1]]
        n_ida = len(layers) - 2 - 1
        for i in range(n_ida):
            # ida_up.proj_1 reads what the level before the last leaves in layers[-1] (out[1] below): it joins the last level's set
            also = [("ida_up.proj_1", layers[-1])] if i == n_ida - 1 and i > 0 else []
            self._ida(f"dla_up.ida_{i}", layers, len(layers) - i - 2, len(layers), also=also)
            out.insert(0, layers[-1])
        for i, t in enumerate(out):
            self.debug[f"up{i}"] = t
        y = out[:3]
        self._ida("ida_up", y, 0, 3, final_out=self.feat, feat=True)
        feat = self.feat = y[-1]
        # ---- the heads' operand: written by the epilogue of the DCN that produces the map (f16x3 kernel), which is
        # patched here, behind the last _ida; a separate pass over the fp32 map only if that kernel is not in use
        spec, pr, M4 = feat_operand(m), self.feat_producer, B * self.h4 * self.w4
        if spec is None:
            self.feat_in = feat
            return
        if self.feat_in is None:
            self.feat_in = self._buf(B, self.h4, self.w4, *spec[0], dtype=spec[1])
        if m._mx_active:
            # heads' first layer on fp16 + FP6 (cf_head_fused mx = 1): the 272-byte rows it stages (no K split at this size)
            # (the feature map's DCN runs WITHOUT a K split whenever it also writes the heads' rows - the two exclude each
            #  other - so on maps small enough for the split, <= 2048 pixels per image, the summation order of that one
            #  layer depends on pack_mx_fused / heads_mx: same arithmetic, rounding differs)
            if pr.out_scale > 0 and pr.N == 64 and pr.N_pad == 64 and bool(m.pack_mx_fused):
                pr.out_mx = self.feat_in.data_ptr()
                pr.mx_scale = m._feat_scale
                pr.workspace = None
            else:
                self._add("feat.pack_mx", None, (self.lib.cf_pack_feat_mx_scaled, feat.data_ptr(), 64, self.feat_in.data_ptr(),
                                                 C.c_long(M4), C.c_float(m._feat_scale)))
        elif pr.out_scale > 0 and pr.N == 64:
            pr.out_split_bf16, pr.split_stride = self.feat_in.data_ptr(), 64
            pr.workspace = None                    # (the split output and a K-split reduction exclude each other)
        else:
            self.add_step((self.lib.cf_split_bf16, feat.data_ptr(), self.feat_in.data_ptr(), M4, 64, 64, 64))

    # ------------------------------------------------------------------------------------------ builders: heads
    def _hconv(self, name, srcs, strides, out_c=None, out=None, out_offset=0):
        """One hidden head layer of the exact-fp32 heads (model.heads_bf16 = False): fp32 NHWC, cf_conv2d_fused."""
        B, h4, w4, pc = self.B, self.h4, self.w4, self._pk[name]
        if out is None:
            out = self._buf(B, h4, w4, out_c)
        a = ops.conv_args(pc, srcs, strides, B, h4, w4, out, out.shape[-1], ACT_RELU, None, 0, LAYOUT_NHWC, None, out_offset, False, 4)
        flops = 2.0 * B * h4 * w4 * pc.n * (pc.kh * pc.kh * sum(int(c) for c in pc.real_cin))
        self._add(name, flops, (self.lib.cf_conv2d_fused, C.byref(a)), a)
        return out

    def _head_out(self, h, src, src_stride):
        B, h4, w4, act, pc = self.B, self.h4, self.w4, act_of(h), self._pk[f"heads.{h}.out"]
        a = ops.conv_args(pc, [src], [src_stride], B, h4, w4, src, 0, act, None, 0,
                          LAYOUT_NCHW, src if act == ACT_RAW_AND_SIGDEPTH else None, 0, False)
        self._add(f"heads.{h}.out", 2.0 * B * h4 * w4 * pc.n * 256, (self.lib.cf_conv2d_fused, C.byref(a)), a)
        self.outs[h] = a

    def _head_block(self, name, names, srcs, strides):
        """-> (argument block of heads `names` of the packed group `name`, their algorithmic FLOPs per pixel)"""
        B, h4, w4, heads = self.B, self.h4, self.w4, self._m.config.heads
        hd = [dict(self._pk[name][h], act=act_of(h)) for h in names]
        f = ops.head_fused_args(srcs, strides, hd[0].get("slots"), hd[0].get("k_pad", 0), B, h4, w4, hd)
        self.keep.append(f)
        return f, sum(2.0 * 256 * (9 * sum(d["real_cin"]) + 256 * len(d["w_hidden"]) + heads[h]) for h, d in zip(names, hd))

    def _fused_heads(self, name, names, srcs, strides):
        """One cf_head_fused launch: 3x3 + ReLU + tail for sibling heads, hidden never in HBM."""
        f, px_flops = self._head_block(name, names, srcs, strides)
        for n, h in enumerate(names):
            self.tails[h] = (f.tail, n)
        flops = self.B * self.h4 * self.w4 * px_flops
        self.group_flops[name] = (flops, px_flops, f)
        self.group_srcs[name] = list(srcs)
        self._add(name, flops, (self.lib.cf_head_fused, C.byref(f)), f)

    def _build_at(self, feat_in):
        """model.heads_at_peaks: what an at-peaks forward launches instead of the dense head groups (see run).  The heat-map head
        alone in a block of its own (dense: the NMS and both top-K passes read every pixel), the other primary heads in a second
        block, the slot tables of cf_head_fused_at: `tab_b` from the decoder's peaks, `tab_ab` (frustum association only) from
        the frustum chain's top-K followed by the decoder's peaks.  The chained / secondary groups reuse their dense blocks."""
        B, K, primary = self.B, self.K, self.primary
        f_hm, px_hm = self._head_block("tails.primary", primary[:1], [feat_in], [64])
        f_rest, px_rest = self._head_block("tails.primary", primary[1:], [feat_in], [64])
        self.at_tails = {primary[0]: (f_hm.tail, 0), **{h: (f_rest.tail, n) for n, h in enumerate(primary[1:])}}
        tiles_b, tiles_ab = -(-K // AT_SLOTS), -(-2 * K // AT_SLOTS)
        self.at = dict(f_hm=f_hm, flops_hm=B * self.h4 * self.w4 * px_hm, f_rest=f_rest, px_rest=px_rest,
                       tab_b=self._buf(B * tiles_b * AT_SLOTS, dtype=torch.int32), n_b=B * tiles_b,
                       tab_ab=self._buf(B * tiles_ab * AT_SLOTS, dtype=torch.int32) if self.frustum else None, n_ab=B * tiles_ab,
                       ws=self._buf(max(1, self.lib.cf_topk_peaks_fused_workspace_bytes(B, self._m.config.heads["heatmap"], self.h4,
                                                                                        self.w4, K)), dtype=torch.uint8))

    def _peaks_lane(self):
        """the side lane: starts behind whatever the caller's stream has issued so far, runs the decoder's NMS + top-k"""
        ev_a = self.new_event()
        self.ctl("rec", 0, ev_a)
        self.lane = 1
        self.ctl("wait", 1, ev_a)
        n_cls = self._m.config.heads["heatmap"]
        self.pk_ws = self._buf(max(1, self.lib.cf_topk_workspace_bytes_nms(self.B, n_cls, self.h4, self.w4, self.K)), dtype=torch.uint8)
        self.peaks_step = self._slot()
        self.ev_peaks = self.new_event()
        self.ctl("rec", 1, self.ev_peaks)
        self.lane = 0

    def _chained_heads(self, bf, feat, feat_in):
        """Early fusion: `nuscenes_att` and `velocity` (three hidden layers, detectHeads.py:59-98) on the 64 image channels alone - ONE
        further cf_head_fused launch, n_src = 1, first layers bf16x3 (the library has no mx form with hidden layers and one source).
        Where the primary group reads mx rows, the split-bf16 operand is written here from the fp32 map (one pass, whole batch)."""
        B, h4, w4, chained = self.B, self.h4, self.w4, self.chained
        if bf:
            src = feat_in
            if self._m._mx_active:
                src = self.feat_bf = self._buf(B, h4, w4, 2, 64, dtype=torch.bfloat16)
                self._add("feat.split_bf16", None, (self.lib.cf_split_bf16, feat.data_ptr(), src.data_ptr(), C.c_long(B * h4 * w4), 64, 64, 64))
            self._fused_heads("tails.chained", chained, [src], [64])
            return
        ss = 256 * len(chained)                    # (the fp32 chain, as for the secondary heads of middle fusion)
        s1 = self._hconv("heads.secondary.0", [feat_in], [64], out_c=ss)
        s2 = self._buf(B, h4, w4, ss)
        for n, h in enumerate(chained):
            self._hconv(f"heads.{h}.2", [s1], [ss], out=s2, out_offset=256 * n)
            self._hconv(f"heads.{h}.4", [s2], [ss], out=s1, out_offset=256 * n)
            self._head_out(h, s1, ss)

    def _build_heads(self):
        m, B, h4, w4, K = self._m, self.B, self.h4, self.w4, self.K
        feat, feat_in = self.feat, self.feat_in
        radar = m.isRadarEnabled and m.fusionStrategy == "middle"
        frustum = radar and m.isFrustumEnabled     # False on a radar model: the radar map itself is pc_hm (base_model.py:69-79)
        bf = m._heads_bf()                         # fused split-bf16 head launches (False: the exact-fp32 layer-by-layer heads)
        chained = [h for h in m.config.heads if len(m.config.head_conv[h]) == 3] if self.early else []
        primary = [h for h in m.config.heads if not (radar and h in SECONDARY_HEADS) and h not in chained]
        self.primary, self.radar, self.frustum, self.chained = primary, radar, frustum, chained
        if feat is not None:                                # the fp32 feature map both head groups read (as mx / split-bf16 / fp32)
            self.inputs["heads.primary.0"] = [feat]
            if radar:
                self.inputs["heads.secondary.0"] = [feat]
        # Two lanes for the decoder's index kernels (model.heads_lanes, fused heads): behind the primary launch the side stream
        # runs the decoder's NMS + top-k (handed to decode.py through the heat map tensor, see run()) beside the frustum
        # path and the secondary launch, instead of alone on the chip behind the last head launch.  (Splitting the primary
        # launch in two so that the frustum path's top-k could go there as well costs the head launches more than both
        # top-k passes take: DESIGN.md section 9.)
        split = bf and bool(m.heads_lanes) and primary[0] == "heatmap"
        if split:
            self.use_lanes = True                  # (also on a plan whose trunk was built without lanes)
        if bf:
            self._fused_heads("tails.primary", primary, [feat_in], [64])
            # radar: the lane starts behind the frustum chain (below), not behind the primary launch - its chip-wide NMS pass
            # beside the chain's slice top-k tripled that kernel's time (41 vs 14 us) on the one path everything waits for
            # (no frustum chain - MODEL.FRUSTUM = False -: behind the primary launch, as on a camera-only model)
            if split and not (frustum and m.peaks_behind_frustum):
                self._peaks_lane()
        else:
            hs = 256 * len(primary)
            hid = self._hconv("heads.primary.0", [feat_in], [64], out_c=hs)
            for h in primary:
                self._head_out(h, hid, hs)
        if chained:
            self._chained_heads(bf, feat, feat_in)
        if radar:
            self.pc_hm4 = None if bf else self._buf(B, h4, w4, 4)
            self.pc_hm8 = self._buf(B, h4, w4, 2, 8, dtype=torch.bfloat16) if bf else None
            if frustum:
                self.tk_scores = self._buf(B, K)
                self.tk_inds = self._buf(B, K, dtype=torch.int32)
                self.tk_cls = self._buf(B, K, dtype=torch.int32)
                self.tk_ws = self._buf(max(1, self.lib.cf_topk_workspace_bytes(B, K)), dtype=torch.uint8)
                # top-k of the raw heat map -> association (pointcloud.py:347-392): cf_topk_frustum (two launches: the merge of the slice
                # lists runs in the association kernel's prologue) or, model.frustum_fused = False, cf_topk_peaks + cf_frustum_assoc (three)
                if not m.frustum_fused:
                    self.topk_step = self._slot()
                self.frustum_step = self._slot()
            else:
                # MODEL.FRUSTUM = False: no top-k, no association - the slot holds cf_pc_hm_direct, which normalises the caller's map in
                # place and writes the secondary heads' channels-last copies; the secondary launch then depends on nothing the primary wrote
                self.frustum_step = self._add("pc_hm_direct", 0.0, None)
            if split and self.peaks_step is None:
                self._peaks_lane()
            if bf:
                self._fused_heads("tails.secondary", SECONDARY_HEADS, [feat_in, self.pc_hm8], [64, 8])
            else:                                  # (the fp32 secondary chain)
                ss = 256 * len(SECONDARY_HEADS)
                s1 = self._hconv("heads.secondary.0", [feat_in, self.pc_hm4], [64, 4], out_c=ss)
                s2 = self._buf(B, h4, w4, ss)
                for n, h in enumerate(SECONDARY_HEADS):
                    self._hconv(f"heads.{h}.2", [s1], [ss], out=s2, out_offset=256 * n)
                    self._hconv(f"heads.{h}.4", [s2], [ss], out=s1, out_offset=256 * n)
                    self._head_out(h, s1, ss)
        if split:
            self.ctl("wait", 0, self.ev_peaks)
        # heads at the peaks: fused heads whose plan computes the decoder's peaks in the forward (heads_lanes; without it the
        # forward runs dense: the decoder then computes its peaks itself, after the forward)
        if split and len(primary) > 1:
            self._build_at(feat_in)

    # ------------------------------------------------------------------------------------------ issue
    def add_step(self, step):
        self.steps.append(step)
        self.lanes.append(self.lane)

    def ctl(self, op, lane, ev):
        """Cross-lane ordering: ("rec" | "wait", lane, event id)."""
        self.steps.append((op, ev))
        self.lanes.append(lane)

    def new_event(self):
        self.n_events += 1
        return self.n_events - 1

    @staticmethod
    def _timed_call(ev, step, st, stream):
        """One launch bracketed by HIP events on the stream it runs on (None: the current one), appended to `ev`."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = step[0](*step[1:], st)
        e1.record(stream)
        ev.append((e0, e1))
        return rc

    def _launch(self, st, seq=None):
        """Issue the plan's steps (seq: another launch list [(key in `timed`, step, lane)], the at-peaks forward's).  With lanes (and outside a stream capture) a step runs on the caller's stream (lane 0) or
        on the plan's side stream (lane 1), ordered by the ("rec" | "wait", event) control steps; otherwise everything runs
        in list order on the caller's stream (the list order is a valid sequential order).  Timed steps (model.time_launch)
        are bracketed by HIP events recorded on the stream the step runs on."""
        lanes_on = self.use_lanes and not torch.cuda.is_current_stream_capturing()
        timed = self.timed
        if seq is None:
            seq = zip(range(len(self.steps)), self.steps, self.lanes)
        if not lanes_on:
            for i, step, _ in seq:
                if isinstance(step[0], str):
                    continue                                   # one stream: program order is the dependency order
                ev = timed.get(i) if timed else None
                rc = step[0](*step[1:], st) if ev is None else self._timed_call(ev, step, st, None)
                if rc != 0:
                    _lib.check(rc, step[0].__name__)
            return
        cur = torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = _side_streams(self.device, cur.cuda_stream, 1)[0]
            self._events = [torch.cuda.Event() for _ in range(self.n_events)]
        streams = (cur, self._side)
        ptrs = (st, self._side.cuda_stream)
        for i, step, lane in seq:
            op = step[0]
            if op == "rec":
                self._events[step[1]].record(streams[lane])
            elif op == "wait":
                streams[lane].wait_event(self._events[step[1]])
            else:
                ev = timed.get(i) if timed else None
                rc = op(*step[1:], ptrs[lane]) if ev is None else self._timed_call(ev, step, ptrs[lane], streams[lane])
                if rc != 0:
                    _lib.check(rc, op.__name__)
        # (every side-lane launch is waited for by a main-lane step that consumes it: the caller's stream is again
        #  the only one with work in flight when this returns)

    def _patch_input(self, x, pc=None):
        """the trunk's first step reads this call's images (early fusion: and this call's normalised radar map `pc`)"""
        if self.early and self.stem is not None:
            self.stem.stem.x, self.stem.pc = x.data_ptr(), pc.data_ptr()
            self.steps[self.in_step] = (self.lib.cf_stem_fused_early, C.byref(self.stem))
        elif self.early:
            self.steps[self.in_step] = (_early_input, x, pc, self.x4)
        elif self.stem is not None:
            self.stem.x = x.data_ptr()
            self.steps[self.in_step] = (self.lib.cf_stem_fused, C.byref(self.stem))
        else:
            self.steps[self.in_step] = (self.lib.cf_nchw_to_nhwc4, x.data_ptr(), self.x4.data_ptr(), self.B, 3, self.H, self.W)

    def run_trunk(self, x, pc=None):
        """part == "trunk": images of this sub-batch -> its slice of the shared feature buffers (current stream).
        pc (early fusion): the sub-batch's slice of the ALREADY normalised radar map."""
        self._patch_input(x, pc)
        self._launch(_lib.stream_ptr())

    def _radar_outputs(self, y, out, heads, pc_dep, pc_hm):
        """The radar maps and the secondary heads' outputs of one call.  pc_hm: the (B, >= 1, h4, w4) tensor whose channel 0
        the secondary heads saw - the association's map, or the caller's normalised pc_dep (MODEL.FRUSTUM = False)."""
        y["pc_hm_in"] = pc_dep[:, :1]
        y["pc_hm"] = pc_hm[:, 0, :, :].unsqueeze(1)
        for h in SECONDARY_HEADS:
            y[h] = out(h, heads[h])
        y["pc_hm_out"] = pc_hm[:, :1]
        y["depthMap"] = y["depth2"]                    # raw depth2 logits (detectHeads.py:188-190)
        y["depth2"] = out("depth2", 1, second=True)

    def run(self, model, x, pc_dep, calib, alloc=None):
        """alloc(c): where a (B, c, h4, w4) output goes (default: a fresh tensor).  part == "heads": `x` is unused
        (the feature buffers were filled by the trunk plans)."""
        B, dev, lib, K = self.B, self.device, self.lib, self.K
        st = _lib.stream_ptr()
        h4, w4 = self.h4, self.w4
        heads = model.config.heads
        self.flush_pending()                               # (before anything the last forward's maps depend on is patched or overwritten)
        # at the peaks: eval forwards outside a stream capture (the training forward never comes here; a capture, and with it
        # model.use_graph, records the dense launches)
        at = self.at if (self.at is not None and getattr(model, "heads_at_peaks", True)
                         and not torch.cuda.is_current_stream_capturing()) else None
        y, written = {}, []                                # written: every tensor a head launch of this forward writes
        new = alloc or (lambda c: torch.empty((B, c, h4, w4), device=dev, dtype=torch.float32))

        def out(h, c, second=False):
            """a (B, c, h4, w4) output tensor, patched into head h's argument block (second: its `out2`)"""
            t = new(c)
            written.append(t)
            if h in self.tails:
                a, n = self.tails[h]
                (a.out2 if second else a.out)[n] = t.data_ptr()
                if h in self.at_tails:                     # (the split primary blocks of the at-peaks forward)
                    a, n = self.at_tails[h]
                    (a.out2 if second else a.out)[n] = t.data_ptr()
            elif second:
                self.outs[h].out2 = t.data_ptr()
            else:
                self.outs[h].out = t.data_ptr()
            return t

        for h in self.primary + self.chained:              # (early fusion: nuscenes_att, velocity behind the seven - the reference's order)
            y[h] = out(h, heads[h])
        depth_raw = y["depth"]                             # raw logits; "depth" gets the sigmoid form.  (Held until the launches are
        y["depthMap"] = depth_raw                          #  issued: a radar model hands out depth2's logits as depthMap instead)
        y["depth"] = out("depth", 1, second=True)
        y["calib"] = calib
        hm = y["heatmap"]
        if self.peaks_step is not None:
            # the decoder's peaks (3x3 NMS + top-K of the heat map, decode.py) are computed on the side lane beside the second
            # primary launch and travel with the heat map tensor: decode._peaks_and_maps picks them up when K and the
            # tensor's version still match, and computes them itself otherwise
            peaks_on = not torch.cuda.is_current_stream_capturing()   # (a captured forward hands out copies of its maps: nothing to carry)
            if peaks_on:
                pk_s = torch.empty((B, K), device=dev, dtype=torch.float32)
                pk_i = torch.empty((B, K), device=dev, dtype=torch.int32)
                pk_c = torch.empty((B, K), device=dev, dtype=torch.int32)
                pk_sum = torch.empty(2 * ops.CHECKSUM_PARTS, device=dev, dtype=torch.int64)   # checksum parts of the map the peaks belong to | decode's re-check
                n_words = B * heads["heatmap"] * h4 * w4
                peaks = (_peaks_and_checksum, lib, (hm.data_ptr(), B, heads["heatmap"], h4, w4, K, 2,
                         pk_s.data_ptr(), pk_i.data_ptr(), pk_c.data_ptr(), self.pk_ws.data_ptr()),
                         (hm.data_ptr(), C.c_long(n_words), pk_sum.data_ptr()))
                self.steps[self.peaks_step] = peaks if at is None else (_no_launch,)   # (at the peaks: in line, see _at_seq)
            else:
                self.steps[self.peaks_step] = (_no_launch,)
        if self.direct_step is not None:
            self.steps[self.direct_step] = (lib.cf_pc_hm_direct, pc_dep.data_ptr(), B, h4, w4,
                                            C.c_float(float(model.config.DATASET.MAX_PC_DIST)), None, None)
        if self.in_step is not None:
            self._patch_input(x, pc_dep)
        if self.radar:
            max_dist = C.c_float(float(model.config.DATASET.MAX_PC_DIST))
            maps = (_lib.ptr(self.pc_hm4), _lib.ptr(self.pc_hm8))
            if not self.frustum:
                # base_model.py:69-79 + detectHeads.py:172-190: ONE in-place normalisation of the caller's tensor per forward;
                # pc_hm_in, pc_hm and pc_hm_out are all channel 0 of that tensor
                pc_hm = pc_dep
                self.steps[self.frustum_step] = (lib.cf_pc_hm_direct, pc_dep.data_ptr(), B, h4, w4, max_dist, *maps)
            else:
                pc_hm = new(3)
                geom = (y["depth"].data_ptr(), y["widthHeight"].data_ptr(), y["dimension"].data_ptr(), y["rotation"].data_ptr(),
                        calib.data_ptr(), pc_dep.data_ptr(), B, h4, w4, max_dist, pc_hm.data_ptr(), *maps)
                tk = (self.tk_scores.data_ptr(), self.tk_inds.data_ptr(), self.tk_cls.data_ptr(), self.tk_ws.data_ptr())
                if at is not None:                         # the top-K runs in front of the at-peaks launch that feeds the association
                    if self.topk_step is not None:
                        self.steps[self.topk_step] = (_no_launch,)
                    self.steps[self.frustum_step] = (lib.cf_frustum_assoc, self.tk_inds.data_ptr(), K, *geom)
                elif self.topk_step is None:
                    self.steps[self.frustum_step] = (lib.cf_topk_frustum, hm.data_ptr(), heads["heatmap"], K, *geom, *tk)
                else:
                    self.steps[self.topk_step] = (lib.cf_topk_peaks, hm.data_ptr(), B, heads["heatmap"], h4, w4, K, 0, *tk)
                    self.steps[self.frustum_step] = (lib.cf_frustum_assoc, self.tk_inds.data_ptr(), K, *geom)
            self._radar_outputs(y, out, heads, pc_dep, pc_hm)
        for name, (flops, px_flops, _) in self.group_flops.items():    # FLOPs of the launch each named step issues THIS forward
            self.step_flops[name] = flops
        if at is None:
            self._launch(st)
        else:
            raw = tk[:3] if self.frustum else (None, None, None)   # (the frustum chain's top-K: from the same read of the map)
            fused = (hm.data_ptr(), B, heads["heatmap"], h4, w4, K, *raw, pk_s.data_ptr(), pk_i.data_ptr(), pk_c.data_ptr(),
                     at["tab_ab"].data_ptr() if self.frustum else None, at["tab_b"].data_ptr(), at["ws"].data_ptr())
            self._launch(st, self._at_seq(at, (_peaks_fused_and_checksum, lib, fused, peaks[3])))
            y = self._pending(y, model, written)
        if self.peaks_step is not None and peaks_on:
            # (decode.py re-checks the map's contents against pk_sum[0] on the device before it trusts the peaks)
            hm._cf_peaks = (K, hm.data_ptr(), pk_s, pk_i, pk_c, pk_sum)
            if self._side is not None:                         # (allocator: these tensors were also used on the side stream)
                for t in (hm, pk_s, pk_i, pk_c, pk_sum):
                    t.record_stream(self._side)
        return [y]

    # ------------------------------------------------------------------------------------------ heads at the peaks
    def _at_seq(self, at, peaks):
        """The launch list of an at-peaks forward: the plan's steps with the head groups replaced.  `tails.primary` = the dense
        heat-map head (cf_head_fused on that head alone), followed IN LINE by the index pass (`peaks`: cf_topk_peaks_fused - the
        frustum chain's top-K on frustum models, the decoder's NMS + top-K and the slot tables, two launches - and the checksum;
        the decoder's lane stays empty) and the other primary heads at the listed pixels; `tails.chained` / `tails.secondary` =
        those groups at the decoder's peaks (cf_head_fused_at).  `at.topk` and `at.tables`, launches of their own before the
        fused pass, issue nothing.  The step FLOPs under the three names are set to what these launches compute.  (The
        decoder's pass on the side lane beside the chain's top-K, joined in front of the tables, measured no faster:
        docs/experiments/heads_at_peaks.md.)"""
        lib, idx = self.lib, self.step_index
        tab_b, n_b = at["tab_b"].data_ptr(), at["n_b"]
        tab_p, n_p = (at["tab_ab"].data_ptr(), at["n_ab"]) if self.frustum else (tab_b, n_b)
        HP_PX = 48                                         # pixel columns a virtual tile computes: its three centre rows (18 of them are written)
        extra = ([("at.topk", (_no_launch,), 0)] if self.frustum else []) + [
                  ("at.peaks", peaks, 0), ("at.tables", (_no_launch,), 0),
                  ("at.primary", (lib.cf_head_fused_at, C.byref(at["f_rest"]), tab_p, n_p), 0)]
        repl = {idx["tails.primary"]: (lib.cf_head_fused, C.byref(at["f_hm"]))}
        self.step_flops["tails.primary"] = at["flops_hm"]
        self.step_flops["at.primary"] = n_p * HP_PX * at["px_rest"]
        for name in ("tails.chained", "tails.secondary"):
            if name in idx:
                _, px_flops, f = self.group_flops[name]
                repl[idx[name]] = (lib.cf_head_fused_at, C.byref(f), tab_b, n_b)
                self.step_flops[name] = n_b * HP_PX * px_flops
        seq = []
        for i, (step, lane) in enumerate(zip(self.steps, self.lanes)):
            seq.append((i, repl.get(i, step), lane))
            if i == idx["tails.primary"]:
                seq += extra
        return seq

    def _pending(self, y, model, written):
        """The outputs of an at-peaks forward as a PendingOutputs.  Its materialiser runs the dense head launches from PRIVATE
        copies of the groups' argument blocks (the pointers of this forward's output tensors are in them) on the forward's
        stream, and orders the reading stream behind them.  Until the next forward of this plan the blocks read the plan's own
        operand buffers (the heads' feature rows, the radar planes); that forward calls `release` first (flush_pending), which
        copies those buffers - one pass over ~110 MB at bs 16, tens of microseconds - and points the blocks at the copies: a
        dict held across later forwards stays pending, and complete."""
        fwd = torch.cuda.current_stream(self.device)
        lib, dev = self.lib, self.device
        names = [n for n in ("tails.primary", "tails.chained", "tails.secondary") if n in self.step_index]
        blocks = []
        for n in names:
            f = self.group_flops[n][2]
            c = _lib.HeadFusedArgs()
            C.memmove(C.byref(c), C.byref(f), C.sizeof(f))
            blocks.append(c)
        bufs = {t.data_ptr(): t for n in names for t in self.group_srcs[n]}
        # (alive as long as the outputs are pending: every tensor the dense launches write - also one the dict does not hand out,
        #  a radar model's raw `depth` logits -, the operand buffers or their copies, the plan that owns the former - the model
        #  may drop it, or be dropped itself - and the packed weights the blocks point to)
        keep = [written, list(y.values()), self, model._packed, bufs]

        def materialise():
            with torch.cuda.device(dev):                   # (under the model's lock: PendingOutputs takes it)
                for c in blocks:
                    rc = lib.cf_head_fused(C.byref(c), fwd.cuda_stream)
                    if rc != 0:
                        _lib.check(rc, "cf_head_fused")
                rd = torch.cuda.current_stream(dev)
                if rd != fwd:
                    rd.wait_stream(fwd)
            keep.clear()

        def release():
            with torch.cuda.device(dev), torch.cuda.stream(fwd):
                for ptr, t in list(bufs.items()):
                    snap = t.clone()
                    for c in blocks:
                        for i in range(c.n_src):
                            if c.src[i] == ptr:
                                c.src[i] = snap.data_ptr()
                    bufs[ptr] = snap
            keep[2] = None                                 # (the plan's buffers are no longer read)

        p = PendingOutputs(y, materialise, model._lock, release)
        self._last = weakref.ref(p)
        return p

    def flush_pending(self):
        """The last at-peaks forward's outputs, if someone still holds them unread, stop depending on this plan's buffers: the
        next forward is about to overwrite them (PendingOutputs.release: a copy of the operand buffers; never a wrong map)."""
        last, self._last = (self._last() if self._last is not None else None), None
        if last is not None:
            last.release()


def _early_input(x, pc, x8, stream):
    """Early fusion on the exact-fp32 paths (conv_f16 / stem_fused off, the range guards' shadow model): the six-channel image of
    fusionModules.py:18-35 as 8-channel pixels, [image | radar map nearest-upsampled x4 | 0 0] (channels 6, 7 stay zero).  torch
    ops on the current stream - the stream every trunk is issued on; off the hot path."""
    x8[..., :3].copy_(x.permute(0, 2, 3, 1))
    x8[..., 3:6].copy_(pc.permute(0, 2, 3, 1).repeat_interleave(4, dim=1).repeat_interleave(4, dim=2))
    return 0


def _no_launch(stream):
    """a plan step that issues nothing (status 0)"""
    return 0


def _peaks_fused_and_checksum(lib, fused_args, sum_args, stream):
    """the index pass of an at-peaks forward (both top-K lists and the slot tables) and the checksum of the map (one plan step)"""
    rc = lib.cf_topk_peaks_fused(*fused_args, stream)
    return rc if rc != 0 else lib.cf_checksum64(*sum_args, stream)


def _peaks_and_checksum(lib, topk_args, sum_args, stream):
    """the decoder's NMS + top-k of the heat map and the checksum of the bits they were computed from (one plan step)"""
    rc = lib.cf_topk_peaks(*topk_args, stream)
    return rc if rc != 0 else lib.cf_checksum64(*sum_args, stream)
