"""`DLASeg`: the CenterFusion / CenterNet inference model on the MI355X HIP path.

Drop-in boundary: same factory (`getModel(config)`, model/model.py:18-44), same
`state_dict` key names and shapes as the reference's DLASeg (model/networks/dla.py:571-635 +
base_model.py:30-53 + detectHeads.py:32-163), same call
`model(images, pc_hm=None, pc_dep=None, calib=None) -> [dict]` (base_model.py:67-106) with the
same keys, order, shapes and the `pc_hm_in` view of the caller's `pc_dep`
(detectHeads.py:172).  Eval mode, and one training mode: the heads on a frozen trunk (MODEL.FREEZE_BACKBONE, `_forward_train`); `forward_trunk` /
`forward_heads` are its two halves, the second differentiable in a caller's feature map.  `unfreeze_neck()` lets dla_up / ida_up
learn too (`forward_base` / `forward_neck`, `_forward_train_neck`); `unfreeze_base()` adds the base's levels 2-5 (`forward_stem` /
`forward_levels`, `_forward_train_base`); the stem stays frozen unless `unfreeze_stem()` (`forward_stem_train`), after which every
parameter learns.

Nothing else is shared with the reference's design.  The module is a parameter tree plus an
*execution plan*: at first call for a given (B,H,W) it lays out every intermediate NHWC buffer in
HBM once, folds BN into the conv weights, packs them into the implicit-GEMM layout, pre-builds the
argument block of every kernel launch, and from then on a forward pass is a flat list of
asynchronous launches on the current stream (no allocation except the returned head maps, no host
sync, hipGraph-capturable).  There is no CPU fallback: without libcfhip.so / a GPU it raises.
"""
import math
import threading
from typing import List

import torch
from torch import nn

from . import _lib, ops, packing
from .packing import Source
from .plan import AT_TIMED, SECONDARY_HEADS, _Plan, feat_operand
from .streams import (_CAPTURE_LOCK, _PROBE_LOG, _PROBE_US, _SIDE_STREAMS,     # (tests and tools reach these through this module)
                      _concurrent, _pick_streams, _side_streams)

CHANNELS = [16, 32, 64, 128, 256, 512]                                    # dla.py:303-307


class _Scope(nn.Module):
    """Empty container: only exists so parameters get the reference's dotted names."""


def _register(root: nn.Module, dotted: str, tensor: torch.Tensor, buffer=False):
    mod = root
    parts = dotted.split(".")
    for p in parts[:-1]:
        if not hasattr(mod, p):
            mod.add_module(p, _Scope())
        mod = getattr(mod, p)
    if buffer:
        mod.register_buffer(parts[-1], tensor)
    else:
        mod.register_parameter(parts[-1], nn.Parameter(tensor, requires_grad=False))


# ----------------------------------------------------------------------------- parameter spec
def _conv_init(co, ci, k):
    w = torch.empty(co, ci, k, k)
    nn.init.kaiming_uniform_(w, a=math.sqrt(5))
    return w


def is_early(config):
    """Early radar fusion (model/model.py:35-40): the radar map rides in the image as channels 3-5, the heads see no radar."""
    return bool(config.DATASET.RADAR_PC) and config.MODEL.FUSION_STRATEGY == "early"


def _param_spec(config) -> List[tuple]:
    """[(name, tensor, is_buffer)] in the reference's registration order."""
    spec = []

    def conv(name, co, ci, k, bias=False):
        spec.append((name + ".weight", _conv_init(co, ci, k), False))
        if bias:
            bound = 1 / math.sqrt(ci * k * k)
            spec.append((name + ".bias", torch.empty(co).uniform_(-bound, bound), False))

    def bn(name, c):
        spec.append((name + ".weight", torch.ones(c), False))
        spec.append((name + ".bias", torch.zeros(c), False))
        spec.append((name + ".running_mean", torch.zeros(c), True))
        spec.append((name + ".running_var", torch.ones(c), True))
        spec.append((name + ".num_batches_tracked", torch.tensor(0, dtype=torch.long), True))

    conv("base.base_layer.0", 16, 6 if is_early(config) else 3, 7); bn("base.base_layer.1", 16)
    conv("base.level0.0", 16, 16, 3); bn("base.level0.1", 16)
    conv("base.level1.0", 32, 16, 3); bn("base.level1.1", 32)

    def block(p, ci, co):
        conv(p + ".conv1", co, ci, 3); bn(p + ".bn1", co)
        conv(p + ".conv2", co, co, 3); bn(p + ".bn2", co)

    def tree1(p, ci, co, root_dim):
        block(p + ".tree1", ci, co)
        block(p + ".tree2", co, co)
        conv(p + ".root.conv", co, root_dim, 1); bn(p + ".root.bn", co)
        if ci != co:
            conv(p + ".project.0", co, ci, 1); bn(p + ".project.1", co)

    tree1("base.level2", 32, 64, 128)
    for lvl, ci, co in ((3, 64, 128), (4, 128, 256)):
        tree1(f"base.level{lvl}.tree1", ci, co, 2 * co)
        tree1(f"base.level{lvl}.tree2", co, co, 3 * co + ci)
    tree1("base.level5", 256, 512, 2 * 512 + 256)

    def dcn(p, ci, co):
        stdv = 1.0 / math.sqrt(ci * 9)
        spec.append((p + ".weight", torch.empty(co, ci, 3, 3).uniform_(-stdv, stdv), False))
        spec.append((p + ".bias", torch.zeros(co), False))
        bn(p + ".activation.0", co)
        spec.append((p + ".conv_offset_mask.weight", torch.zeros(27, ci, 3, 3), False))
        spec.append((p + ".conv_offset_mask.bias", torch.zeros(27), False))

    def up(p, c, f):
        k = 2 * f
        fl = math.ceil(k / 2)
        cc = (2 * fl - 1 - fl % 2) / (2.0 * fl)
        w = torch.zeros(c, 1, k, k)
        for i in range(k):
            for j in range(k):
                w[:, 0, i, j] = (1 - abs(i / fl - cc)) * (1 - abs(j / fl - cc))
        spec.append((p + ".weight", w, False))

    def ida(p, o, srcs, fs):
        for n in range(1, len(srcs)):
            dcn(f"{p}.proj_{n}", srcs[n], o)
            up(f"{p}.up_{n}", o, fs[n])
            dcn(f"{p}.node_{n}", o, o)

    chans = CHANNELS[2:]
    in_ch = list(chans)
    for i in range(3):
        j = -i - 2
        ida(f"dla_up.ida_{i}", chans[j], in_ch[j:], [1] + [2] * (len(in_ch[j:]) - 1))
        in_ch[j + 1:] = [chans[j]] * len(in_ch[j + 1:])
    ida("ida_up", 64, [64, 128, 256], [1, 2, 4])

    radar_middle = bool(config.DATASET.RADAR_PC) and config.MODEL.FUSION_STRATEGY == "middle"

    def head_conv_layer(name, co, ci, k, zero_bias, bias_fill=None):
        spec.append((name + ".weight", _conv_init(co, ci, k), False))
        bound = 1 / math.sqrt(ci * k * k)
        b = torch.zeros(co) if zero_bias else torch.empty(co).uniform_(-bound, bound)
        if bias_fill is not None:
            b.fill_(bias_fill)
        spec.append((name + ".bias", b, False))

    for h, n_out in config.heads.items():
        hc = list(config.head_conv[h])
        cin = 67 if (radar_middle and h in SECONDARY_HEADS) else 64
        p = f"detectHead_0.{h}"
        zero = h != "heatmap"                     # initConv2dWeights: bias 0 on non-heatmap heads
        head_conv_layer(p + ".0", hc[0], cin, 3, zero)
        idx = 2
        for i in range(1, len(hc)):
            head_conv_layer(f"{p}.{idx}", hc[i], hc[i - 1], 1, zero)
            idx += 2
        head_conv_layer(f"{p}.{idx}", n_out, hc[-1], 1, zero,
                        -4.6 if h == "heatmap" else None)      # detectHeads.py:93
    return spec


# ----------------------------------------------------------------------------------- the module
class DLASeg(nn.Module):
    def __init__(self, num_layers, in_channels, config):
        super().__init__()
        if str(num_layers) != "34":
            raise NotImplementedError("only DLA-34 is implemented (the reference ships nothing else)")
        if getattr(config.DATASET, "ONE_HOT_PC", False):
            raise NotImplementedError("ONE_HOT_PC is outside the hot path")
        early = is_early(config)
        if early and any(h in config.heads for h in ("depth2", "rotation2")):
            # (the reference derives the heads from the strategy, config/utils.py:69-166; a config whose strategy was switched
            #  afterwards still lists middle fusion's radar heads, which an early model has no input for)
            raise NotImplementedError("early fusion with depth2 / rotation2 in config.heads: the heads were derived for middle "
                                      "fusion - run update_heads(config) after setting MODEL.FUSION_STRATEGY")
        if in_channels != (6 if early else 3):
            raise NotImplementedError(f"in_channels={in_channels}: 6 with DATASET.RADAR_PC and MODEL.FUSION_STRATEGY = 'early' "
                                      "(image + 3 radar channels), 3 otherwise")
        if config.MODEL.DLA.NODE != "DeformConv":
            raise NotImplementedError("MODEL.DLA.NODE must be DeformConv (the only node type that works upstream)")
        self.config = config
        self.heads = config.heads
        self.isRadarEnabled = bool(config.DATASET.RADAR_PC)
        self.fusionStrategy = config.MODEL.FUSION_STRATEGY if self.isRadarEnabled else None
        if self.fusionStrategy not in (None, "middle", "early"):
            raise NotImplementedError(f"fusion strategy {self.fusionStrategy!r} is outside the hot path")
        # early fusion (base_model.py:89-92): the normalised radar map is channels 3-5 of the stem's input; nine image-only heads
        self.isEarly = early
        # middle fusion with MODEL.FRUSTUM = False: the normalised radar map goes straight to the secondary heads (base_model.py:69-79)
        self.isFrustumEnabled = self.isRadarEnabled and bool(config.MODEL.FRUSTUM) and not early
        try:                                               # dla.py:578-580
            config.defrost()
            config.MODEL.PYRAMID_OUT_SIZE = [config.MODEL.OUTPUT_SIZE]
            config.freeze()
        except Exception:
            pass
        for name, tensor, is_buf in _param_spec(config):
            _register(self, name, tensor, is_buf)
        self._packed = None
        self._plans = {}         # (B, H, W, device, stream id [, role...]) -> _Plan; key[:5] names a plan SET (one forward shape)
        self._plan_sets = {}     # plan-set keys in least-recently-used order (dict order)
        self._graphs = {}        # (B, H, W, device, stream id, "graph", streams) -> captured forward, LRU as well
        self.max_plan_sets = 4   # plan sets / graphs kept per model: a set holds every intermediate of a forward (~6 GB at
                                 # bs=16, 448x800), so a service with varying batch sizes must not keep them all
        self._lock = threading.RLock()     # plans (buffers + argument blocks) are built / patched / launched under it
        self.precise = True      # two-level fp32 summation in backbone + neck (see cf_gemm.hip)
        self.conv_f16 = True     # backbone / offset convs: fp32 storage, split-fp16 products (cf_gemm_f16.hip)
        self.lanes = True        # small batches: the IDA projections on a side stream beside the node chain (plan.py: _Plan._ida)
        self.lanes_max_frames = 10 # ... up to this many 448x800-frame equivalents per single-stream forward (round 6, ms per step with /
                                   # without: bs 5 3.35 / 3.39, 6 4.00 / 4.08, 7 4.23 / 4.31, 8 4.60 / 4.67, 10 5.26 / 5.35, 11 5.69 / 5.67)
        self.streams = 2         # > 1 (and batch >= min_sub_batch * streams): backbone + neck as that many sub-batches on
                                 # concurrent HIP streams with their own plans; heads on the caller's stream
        self.trunk_on_caller = True   # ... the last of those sub-batches on the caller's stream itself (one event wait less in front of the heads)
        self.min_sub_batch = 6   # ... and only when a sub-batch keeps at least this many 448x800-frame equivalents: measured (tools/
                                 # bench_small_batch.py, ms per forward + decode, one stream vs two): B=8 5.28 vs 5.91,
                                 # B=12 7.72 vs 6.86, B=16 9.16 vs 8.61 - four-frame trunks lose to one eight-frame forward
        self.use_graph = False   # replay the forward as ONE captured HIP graph (inputs / outputs staged through
                                 # static buffers) instead of ~100 launches from Python (_forward_graph)
        self.stem_fused = True   # with conv_f16: base_layer + level0 + level1 in one launch (cf_stem.hip)
        self.stem_pool = True    # ... which also writes the level-2 Tree's max-pool of its output (one launch less per trunk)
        self.conv_patch = True   # 3x3 stride-1 f16x3 convs: LDS patch reuse (cf_conv3x3_f16.hip)
        self.neck_groups = True  # neck without lanes: the same-shape DeformConv projections of an IDA level (dla_up.ida_1.proj_1-2; dla_up.ida_2.
                                 # proj_1-3 + ida_up.proj_1) as ONE offset-convolution launch and ONE DCN launch per set (plan.py:
                                 # _Plan._dcn_group); same bits; set before the first forward
        self.root_fuse = True    # one-level Trees: tree2.conv2 + Root as one step (cf_conv3x3_root_f16x3) ...
        self.root_fuse_children = False   # ... also where the Root has further sources (level3.tree2, level4.tree2): same bits, and
                                          # in the two-stream step the two launches are 0.024 ms faster (round 5, 6 of 6 A/B pairs)
        self.heads_lanes = True  # fused heads: the decoder's NMS + top-k on a side stream beside the frustum path and the secondary
                                 # launch (plan.py: _Plan._build_heads), handed to decode.py with the heat map
        self.heads_at_peaks = True  # eval forwards (fused heads, heads_lanes, no stream capture): only the heat-map head runs over the
                                    # whole map; the other heads are evaluated at the pixels the frustum association and the decoder
                                    # read (cf_head_fused_at) and the returned dict computes the full maps on first read
                                    # (pending.PendingOutputs; same bits either way).  False: every head over every pixel
        self.peaks_behind_frustum = True  # heads_lanes on a radar model: the decoder's lane starts behind the frustum chain instead of
                                          # behind the primary head launch (False: round 5's order; same results)
        self.frustum_fused = True  # radar: top-k of the raw heat map + frustum association as cf_topk_frustum (2 launches, the merge in the
                                   # association kernel's prologue) instead of cf_topk_peaks + cf_frustum_assoc (3); same bits
        self.proj_fuse = True    # the sub-tree that opens a level: `project` of the pooled input as k-steps of tree1.conv2
                                 # (cf_conv3x3_proj_f16x3) instead of a launch + a residual tensor; set before the first forward
        self.heads_bf16 = True   # head GEMMs on the bf16 / f16 MFMA pipe with split operands: ONE cf_head_fused launch per head group
                                 # on v_mfma_f32_16x16x32_* (hidden maps stay in LDS).  False - or a head with more than 16 outputs,
                                 # which the 16-row output tile of that kernel does not hold - : exact-fp32 layer-by-layer heads
        self.heads_mx = True     # ... and the FIRST layer of every fused head as fp16 main term + block-scaled FP6 cross terms
                                 # (v_mfma_scale_f32_16x16x128_f8f6f4): 1.5 MFMA passes per product instead of 3; hidden and
                                 # output layers stay bf16x3 (the float64-anchored gate rejects FP6 cross terms there)
        self._mx_active = False  # set by _prepare: heads_mx and everything it needs (bf16 fused heads on 16x16x32 fragments)
        self.pack_mx_fused = True  # with heads_mx: the feature map's DCN writes the heads' operand rows from its epilogue
                                   # (cf_dcn_args.out_mx); False: a separate cf_pack_feat_mx pass (A/B, byte-identical)
        self.record_spans = False  # dev / tests: keep HIP events around each trunk of _forward_concurrent (trunk_overlap)
        self.trunk_spans = []
        # Dynamic range of the split-fp16 operands: every activation is multiplied by a per-layer power of
        # two before it is split into fp16 hi + lo - 16 unless `calibrate` has measured that a layer's inputs need less.
        self._ranges = None        # {layer name: max |input| measured by calibrate()}; None = the default pre-scale everywhere
        self._feat_scale = ops.DEFAULT_IN_SCALE   # pre-scale of the heads' mx feature rows (set by _prepare from _ranges)
        self.range_headroom = 8.0  # a calibrated layer keeps max |input| * scale <= 65504 / this
        self._range_checked = False  # a check_ranges / calibrate has run on these weights (Detector's first-batch guard)
        self.register_load_state_dict_post_hook(lambda m, _k: m._weights_changed())
        # MODEL.FREEZE_BACKBONE (dla.py:617-621): base, dla_up and ida_up stay frozen, the detection heads learn - the one training
        # mode of this model (_forward_train).  Without it every parameter stays an inference constant, as before.
        self.freezeBackbone = bool(getattr(config.MODEL, "FREEZE_BACKBONE", False))
        if self.freezeBackbone:
            for name, p in self.named_parameters():
                p.requires_grad_(name.startswith("detectHead_0."))
        self._stale = False      # a training forward has run: the packed head weights may lag an optimiser step (eval re-packs)
        self._neck_train = False  # unfreeze_neck(): dla_up / ida_up learn too (the training forward goes through forward_neck)
        self._base_train = False  # unfreeze_base(): base levels 2-5 learn too (the training forward goes through forward_levels)
        self._stem_train = False  # unfreeze_stem(): the stem learns too (the base-training forward runs forward_stem_train's blocks)
        self.eval()

    def train(self, mode=True):
        super().train(mode)
        if not mode:
            self._repack_if_stale()
        return self

    def _repack_if_stale(self):
        """Behind a training forward the eval path's packed head weights may be an optimiser step old: drop them (and the plans
        built on them).  The trunk did not change, so the calibrated ranges stay."""
        if getattr(self, "_stale", False):
            with self._lock:
                self._stale = False
                self.invalidate()

    def _weights_changed(self):
        """load_state_dict: new weights - re-pack lazily, and whatever was known about the activation ranges is void."""
        self._ranges = None
        self._range_checked = False
        self.invalidate()

    # weights changed or moved (load_state_dict / .to()) -> re-pack lazily
    def invalidate(self):
        self._packed = None
        self._plans = {}
        self._plan_sets = {}
        with _CAPTURE_LOCK:                  # (graphs are never destroyed while another thread's stream is capturing)
            self._graphs = {}

    def _plan(self, key, build, store=None):
        """The plan under `key`, built on first use.  Plans of the eager path live in `self._plans` under an LRU of
        `max_plan_sets` plan sets (key[:5] = batch, height, width, device, stream): the least recently used set is
        dropped whole, its buffers go back to torch's allocator (every launch that used them was issued on - or joined
        into - the stream they were allocated on, so the allocator's stream-ordered reuse is safe).  Plans captured
        into a HIP graph live in the graph's own `store` instead: the graph addresses their buffers by raw pointer, so
        they must live exactly as long as the graph."""
        if store is not None:
            plan = store.get(key)
            if plan is None:
                plan = store[key] = build()
            return plan
        sk = key[:5]
        self._plan_sets.pop(sk, None)
        self._plan_sets[sk] = True                           # most recently used last
        while len(self._plan_sets) > max(1, int(self.max_plan_sets)):
            old = next(iter(self._plan_sets))
            del self._plan_sets[old]
            for k in [k for k in self._plans if k[:5] == old]:
                del self._plans[k]
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = build()
        return plan

    def _all_plans(self):
        """Every live plan: the eager ones and those owned by captured graphs."""
        out = list(self._plans.values())
        for g in self._graphs.values():
            out += list(g[-1].values())
        return out

    def _apply(self, fn, *a, **k):
        self.invalidate()
        return super()._apply(fn, *a, **k)

    # ------------------------------------------------------------------------------ weight prep
    def _prepare(self, device):
        sd = {k: v.detach() for k, v in self.state_dict().items()}
        pk = {}
        self._mx_active = False

        def bn(p):
            return (sd[p + ".weight"], sd[p + ".bias"], sd[p + ".running_mean"], sd[p + ".running_var"])

        f16 = bool(self.conv_f16)

        def pack_any(w, b, sources, stride=1):
            """split-fp16 products (fp32 storage) wherever the sources allow 8-channel slots."""
            # (<= 32 output channels stay on the fp32 kernels: a 32-row MFMA tile per wave leaves the
            #  f16 path bound by the on-the-fly operand split)
            ok8 = all(s.stride % 8 == 0 and s.channels % 8 == 0 for s in sources)
            patchable = (w.shape[2] == 3 and stride == 1 and len(sources) == 1 and sources[0].channels % 16 == 0)
            if f16 and ok8 and (w.shape[0] > 32 or patchable):
                return packing.pack_conv_f16(w, b, sources, stride=stride).to(device)
            return packing.pack_conv(w, b, sources, stride=stride).to(device)

        def conv_bn(name, wkey, bnkey, sources, stride=1, bias=None):
            w, b = packing.fold_bn(sd[wkey], bias, bn(bnkey) if bnkey else None)
            pk[name] = pack_any(w, b, sources, stride=stride)

        if f16 and self.stem_fused:
            folded = [packing.fold_bn(sd[f"base.{n}.0.weight"], None, bn(f"base.{n}.1"))
                      for n in ("base_layer", "level0", "level1")]
            pack = packing.pack_stem_early if self.isEarly else packing.pack_stem
            pk["base.stem"] = pack(*[t for wb in folded for t in wb]).to(device)
        else:
            # (early fusion: the six-channel image is materialised as 8-channel pixels on these paths - plan.py: _early_input)
            conv_bn("base.base_layer", "base.base_layer.0.weight", "base.base_layer.1", [Source(6, 8) if self.isEarly else Source(3, 4)])
            conv_bn("base.level0", "base.level0.0.weight", "base.level0.1", [Source(16, 16)])
            conv_bn("base.level1", "base.level1.0.weight", "base.level1.1", [Source(16, 16)], stride=2)

        def tree1(p, ci, co, root_srcs):
            conv_bn(p + ".tree1.conv1", p + ".tree1.conv1.weight", p + ".tree1.bn1", [Source(ci, ci)],
                    stride=2 if ci != co else 1)
            if f16 and self.proj_fuse and (p + ".project.0.weight") in sd and co >= 64 and ci % 32 == 0:
                # the Tree's project (dla.py:98-103) rides in tree1.conv2's accumulators: no ".project" entry, no launch
                w2, b2 = packing.fold_bn(sd[p + ".tree1.conv2.weight"], None, bn(p + ".tree1.bn2"))
                wp, bp = packing.fold_bn(sd[p + ".project.0.weight"], None, bn(p + ".project.1"))
                pk[p + ".tree1.conv2"] = packing.pack_conv_f16(w2, b2, [Source(co, co)],
                                                               proj=(wp, bp, Source(ci, ci))).to(device)
            else:
                conv_bn(p + ".tree1.conv2", p + ".tree1.conv2.weight", p + ".tree1.bn2", [Source(co, co)])
            conv_bn(p + ".tree2.conv1", p + ".tree2.conv1.weight", p + ".tree2.bn1", [Source(co, co)])
            conv_bn(p + ".tree2.conv2", p + ".tree2.conv2.weight", p + ".tree2.bn2", [Source(co, co)])
            conv_bn(p + ".root", p + ".root.conv.weight", p + ".root.bn", [Source(c, c) for c in root_srcs])
            if (p + ".project.0.weight") in sd and not pk[p + ".tree1.conv2"].proj_k:
                conv_bn(p + ".project", p + ".project.0.weight", p + ".project.1", [Source(ci, ci)])

        tree1("base.level2", 32, 64, [64, 64])
        for lvl, ci, co in ((3, 64, 128), (4, 128, 256)):
            tree1(f"base.level{lvl}.tree1", ci, co, [co, co])
            tree1(f"base.level{lvl}.tree2", co, co, [co, co, ci, co])
        tree1("base.level5", 256, 512, [512, 512, 256])

        def dcn(p, ci, co):
            w, b = packing.fold_bn(sd[p + ".weight"], sd[p + ".bias"], bn(p + ".activation.0"))
            pk[p] = (packing.pack_dcn_f16 if f16 else packing.pack_dcn)(w, b).to(device)
            pk[p + ".conv_offset_mask"] = pack_any(
                sd[p + ".conv_offset_mask.weight"].float().cpu(),
                sd[p + ".conv_offset_mask.bias"].float().cpu(), [Source(ci, ci)])

        def ida(p, o, srcs, fs):
            for n in range(1, len(srcs)):
                dcn(f"{p}.proj_{n}", srcs[n], o)
                dcn(f"{p}.node_{n}", o, o)
                pk[f"{p}.up_{n}"] = (packing.pack_upsample(sd[f"{p}.up_{n}.weight"]).to(device), fs[n])

        chans = CHANNELS[2:]
        in_ch = list(chans)
        for i in range(3):
            j = -i - 2
            ida(f"dla_up.ida_{i}", chans[j], in_ch[j:], [1] + [2] * (len(in_ch[j:]) - 1))
            in_ch[j + 1:] = [chans[j]] * len(in_ch[j + 1:])
        ida("ida_up", 64, [64, 128, 256], [1, 2, 4])

        # heads: sibling first layers share their input -> one GEMM with concatenated outputs
        heads = dict(self.config.heads)
        head_conv = {k: list(v) for k, v in self.config.head_conv.items()}
        radar = self.isRadarEnabled and self.fusionStrategy == "middle"
        hp = "detectHead_0"
        chained = [h for h in heads if len(head_conv[h]) == 3] if self.isEarly else []   # early: velocity / nuscenes_att, image only
        primary = [h for h in heads if not (radar and h in SECONDARY_HEADS) and h not in chained]
        for h in heads:
            if any(c != 256 for c in head_conv[h]):
                raise NotImplementedError("head_conv widths other than 256 are not on the path")
        bf = self._heads_bf()
        feat_src = Source(64, 64)
        pc_src = Source(3, 8 if bf else 4)
        hw = lambda h, i: sd[f"{hp}.{h}.{i}.weight"].float().cpu()
        hb = lambda h, i: sd[f"{hp}.{h}.{i}.bias"].float().cpu()
        for h in primary:
            assert len(head_conv[h]) == 1
        for h in (SECONDARY_HEADS if radar else ()):
            assert len(head_conv[h]) == 3
        if not bf:
            # the exact-fp32 layer-by-layer heads (cf_conv2d_fused); the fused launches below read none of these
            pack = packing.pack_conv
            pk["heads.primary.0"] = pack(torch.cat([hw(h, 0) for h in primary], 0),
                                         torch.cat([hb(h, 0) for h in primary], 0), [feat_src]).to(device)
            for n, h in enumerate(primary):
                pk[f"heads.{h}.out"] = pack(hw(h, 2), hb(h, 2), [Source(256, 256 * len(primary), 256 * n)]).to(device)
            if radar or chained:
                sec = SECONDARY_HEADS if radar else chained
                pk["heads.secondary.0"] = pack(torch.cat([hw(h, 0) for h in sec], 0),
                                               torch.cat([hb(h, 0) for h in sec], 0),
                                               [feat_src, pc_src] if radar else [feat_src]).to(device)
                ns = 256 * len(sec)
                for n, h in enumerate(sec):
                    for idx in (2, 4):
                        pk[f"heads.{h}.{idx}"] = pack(hw(h, idx), hb(h, idx), [Source(256, ns, 256 * n)]).to(device)
                    pk[f"heads.{h}.out"] = pack(hw(h, 6), hb(h, 6), [Source(256, ns, 256 * n)]).to(device)
        else:
            # 16x16x32 fragments: what head_patch16_kernel reads (_heads_bf: every head has <= 16 outputs)
            pf = packing.pack_fragments16
            def tail(h, hidden_idx, out_idx):
                n_out = heads[h]
                b32 = torch.zeros(32)
                b32[:n_out] = hb(h, out_idx)
                w2 = hw(h, out_idx).view(n_out, 256)
                return dict(w_hidden=[pf(hw(h, i).view(256, 256)).to(device) for i in hidden_idx],
                            b_hidden=[hb(h, i).to(device) for i in hidden_idx],
                            w_out=pf(w2).to(device), w_out_perm=pf(w2, acc_order=True).to(device),
                            b_out=b32.to(device), n_out=n_out, mfma16=True)
            mx = bool(self.heads_mx)
            self._mx_active = mx
            # the mx rows' pre-scale: one for both head groups (they read the same rows)
            fr = [self._ranges[n] for n in ("heads.primary.0", "heads.secondary.0") if self._ranges and n in self._ranges]
            self._feat_scale = ops.in_scale_for_large(max(fr), self.range_headroom) if (mx and fr) else ops.DEFAULT_IN_SCALE
            def first(h, srcs, mx=mx):
                if mx:
                    d = packing.pack_head_first_mx(hw(h, 0), hb(h, 0), pc=len(srcs) == 2, feat_scale=self._feat_scale)
                    return dict(w_first=d["w_first"].to(device), b_first=d["b_first"].to(device), first_scale=d["first_scale"],
                                real_cin=d["real_cin"])
                pc = packing.pack_conv_bf16(hw(h, 0), hb(h, 0), srcs).to(device)
                return dict(w_first=pc.weight, b_first=pc.bias[:256].contiguous(), slots=pc.slots, k_pad=pc.k_pad,
                            real_cin=pc.real_cin)
            pk["tails.primary"] = {h: dict(tail(h, [], 2), **first(h, [feat_src])) for h in primary}
            if radar:
                pk["tails.secondary"] = {h: dict(tail(h, [2, 4], 6), **first(h, [feat_src, pc_src]))
                                         for h in SECONDARY_HEADS}
            if chained:
                # three-layer heads on the image features alone: bf16x3 first layers (cf_head_fused has no mx form with hidden layers
                # and one source), reading the split-bf16 copy of the feature map the plan keeps beside the primary group's mx rows
                pk["tails.chained"] = {h: dict(tail(h, [2, 4], 6), **first(h, [feat_src], mx=False)) for h in chained}
        self._packed = pk

    def _heads_bf(self):
        """The heads run as fused split-operand launches (cf_head_fused on 16x16x32 fragments): model.heads_bf16 and every head's
        output count fits that kernel's one 16-row output tile; otherwise the exact-fp32 layer-by-layer heads."""
        return bool(self.heads_bf16) and all(int(n) <= 16 for n in self.config.heads.values())

    # ----------------------------------------------------------------------------- dynamic range
    def _range_groups(self):
        """{layer name: the layer names that share ONE activation pre-scale with it} for every layer of the packed model whose
        operands are split to fp16 (f16x3 convolutions / DCNs, the fused stem, the heads' mx first layers).  Names are the
        unfused plan's: `X.tree1.conv2` with its Tree's `X.project` when the projection rides in conv2's accumulators."""
        pk = self._packed
        groups = {}
        for name, pc in pk.items():
            if isinstance(pc, (dict, tuple)) or getattr(pc, "out_scale", 0.0) <= 0 or name == "base.stem":
                continue
            g = self._group_of(name)
            for n in g:
                groups[n] = g
        if "base.stem" in pk:
            for n in ("base.base_layer", "base.level0", "base.level1"):
                groups[n] = (n,)
        if self._mx_active:
            g = ("heads.primary.0",) + (("heads.secondary.0",) if "tails.secondary" in pk else ())
            for n in g:
                groups[n] = g
        return groups

    def _group_of(self, name):
        """(name,) or, where a Tree's `project` rides in its tree1.conv2's accumulators, that pair: one pre-scale for both."""
        pk = self._packed or {}
        if name.endswith(".project"):
            c2 = name[:-len(".project")] + ".tree1.conv2"
            if getattr(pk.get(c2), "proj_k", 0) > 0:
                return (c2, name)
        if getattr(pk.get(name), "proj_k", 0) > 0:
            return (name, name[:-len(".tree1.conv2")] + ".project")
        return (name,)

    def _scale(self, name):
        """The activation pre-scale of layer `name` under the current calibration (None = the kernels' default, 16)."""
        if self._ranges is None:
            return None
        vals = [self._ranges[n] for n in self._group_of(name) if n in self._ranges]
        return ops.in_scale_for(max(vals), self.range_headroom) if vals else None

    def activation_ranges(self):
        """{layer name: max |x| over the layer's input tensors} read from the RESIDENT buffers of the live plans, i.e. for
        the most recent forward of each plan: one reduction launch per buffer on the current stream, one device -> host
        copy - off the hot path, no re-run.  Covers every operand that exists in HBM; the operands fused launches keep on
        the chip (the stem's two full-resolution maps, x2 of a conv2 + Root launch) are not seen - `hidden_layers()` names
        them, `measure_ranges` sees them too.  NaN / inf inputs come out as nan / inf."""
        items = [(name, t) for plan in self._all_plans() for name, ts in plan.inputs.items() for t in ts]
        if not items:
            return {}
        lib, st = _lib.load(), _lib.stream_ptr()
        dev = items[0][1].device
        with torch.cuda.device(dev):
            out = torch.zeros(len(items), device=dev, dtype=torch.float32)
            for i, (_, t) in enumerate(items):
                c = t.shape[-1]
                _lib.check(lib.cf_absmax_f32(t.data_ptr(), t.numel() // c, c, c, out.data_ptr() + 4 * i, st), "cf_absmax_f32")
            vals = out.cpu().tolist()
        r = {}
        for (name, _), v in zip(items, vals):
            old = r.get(name, 0.0)
            r[name] = old if old != old else (v if v != v else max(old, v))      # (a NaN sticks)
        return r

    def hidden_layers(self):
        """Layer names with operands `activation_ranges` cannot see in the live plans (kept in LDS / registers by a fused launch)."""
        return sorted(set().union(*[p.hidden for p in self._all_plans()])) if self._all_plans() else []

    def measure_ranges(self, images, pc_dep=None, calib=None):
        """{layer name: max |x| over that layer's inputs} for THIS batch, every layer, measured on a shadow of the model
        that runs the exact-fp32 kernels with nothing fused (every intermediate in HBM, no fp16 split anywhere, so no value
        measured here can itself be a clamped one).  One slow forward (~30 ms at bs=16) + one reduction per buffer; the
        shadow's plans are freed on return.  Reference semantics this protects: the fp32 convolutions of
        model/networks/dla.py:124-159 accept any magnitude."""
        if not images.is_cuda:
            raise _lib.CfHipError("measure_ranges needs device tensors: the HIP path has no CPU fallback")
        with self._lock, torch.cuda.device(images.device), torch.no_grad():
            with torch.random.fork_rng(devices=[]):            # (the shadow's throw-away initialisation draws random numbers)
                shadow = DLASeg(34, 6 if self.isEarly else 3, self.config)
            shadow.load_state_dict(self.state_dict())
            shadow.to(images.device)
            shadow.conv_f16, shadow.heads_bf16, shadow.streams, shadow.lanes, shadow.use_graph = False, False, 1, False, False
            if pc_dep is not None and self.isRadarEnabled and not self.isFrustumEnabled:
                pc_dep = pc_dep.clone()        # (without frustum / with early fusion the forward normalises pc_dep in place: that one mutation is the real forward's)
            shadow(images, pc_dep=pc_dep, calib=calib)
            r = shadow.activation_ranges()
            del shadow
        return r

    def range_violations(self, ranges, fraction=0.5):
        """[(layer, max |input|, pre-scale)] for every fp16-split layer whose inputs, under the CURRENT pre-scales, reach
        `fraction` of the fp16 limit (65504) or are not finite.  ranges: from measure_ranges / activation_ranges."""
        if self._packed is None:
            raise _lib.CfHipError("range_violations: run a forward (or check_ranges) first - the weights are not packed yet")
        out = []
        for name, g in sorted(self._range_groups().items()):
            vals = [ranges[n] for n in g if n in ranges]
            if not vals:
                continue
            m = float("nan") if any(v != v for v in vals) else max(vals)
            s = (self._feat_scale if name.startswith("heads.") else self._scale(name)) or ops.DEFAULT_IN_SCALE
            if not (m * s < fraction * ops.F16_MAX):
                out.append((name, m, s))
        return out

    def _raise_on(self, viol, how):
        if viol:
            worst = ", ".join(f"{n}: max |input| {m:.4g} x pre-scale {s:g}" for n, m, s in viol[:6])
            raise _lib.CfHipError(
                f"activation range guard ({how}): {len(viol)} layer(s) would be clamped at +-65504 / pre-scale by the split-fp16 "
                f"kernels ({worst}{', ...' if len(viol) > 6 else ''}).  Call model.calibrate(images, pc_dep=..., calib=...) "
                "on representative batches (per-layer power-of-two pre-scales), or Detector(..., range_policy='calibrate').")

    def check_ranges(self, images, pc_dep=None, calib=None):
        """Range guard: measure this batch's activation ranges (`measure_ranges`) and raise `CfHipError` naming every layer
        whose inputs reach HALF the fp16 limit under the current pre-scales - 65504 / 16 / 2 = 2047 on an uncalibrated
        model - instead of ever returning a silently clamped map.  -> the ranges."""
        r = self.measure_ranges(images, pc_dep, calib)
        with self._lock, torch.cuda.device(images.device):
            if self._packed is None:
                self._prepare(images.device)
            self._raise_on(self.range_violations(r), "check_ranges")
        self._range_checked = True
        return r

    def check_resident_ranges(self):
        """The cheap form of the guard for a running service: the same test on `activation_ranges()` - the buffers the last
        forwards left in HBM - without a second forward.  Blind to `hidden_layers()`."""
        r = self.activation_ranges()
        self._raise_on(self.range_violations(r), "check_resident_ranges")
        return r

    def calibrate(self, images, pc_dep=None, calib=None, reset=True):
        """Choose the per-layer activation pre-scales from this batch (accumulating over calls with reset=False): layers whose
        inputs stay below 1023 keep the default 16 (bit-identical results), the others get the largest power of two with
        max |input| * scale <= 65504 / range_headroom.  Plans and packed weights are rebuilt lazily.  -> the ranges."""
        r = self.measure_ranges(images, pc_dep, calib)
        bad = [n for n, v in r.items() if v != v or v == float("inf")]
        if bad:
            raise _lib.CfHipError(f"calibrate: non-finite activations in the inputs of {bad[:6]}")
        if not reset and self._ranges:
            r = {k: max(r.get(k, 0.0), self._ranges.get(k, 0.0)) for k in set(r) | set(self._ranges)}
        with self._lock:
            self._ranges = r
            self.invalidate()
        self._range_checked = True
        return r

    def calibration(self):
        """The ranges `calibrate` holds (None if uncalibrated) - save them beside a checkpoint, restore with `set_calibration`."""
        return None if self._ranges is None else dict(self._ranges)

    def set_calibration(self, ranges):
        with self._lock:
            self._ranges = None if ranges is None else {str(k): float(v) for k, v in ranges.items()}
            self.invalidate()
        self._range_checked = ranges is not None

    def activation_scales(self):
        """{layer: pre-scale} of every fp16-split layer under the current calibration (after the weights were packed)."""
        if self._packed is None:
            return {}
        return {n: ((self._feat_scale if n.startswith("heads.") else self._scale(n)) or ops.DEFAULT_IN_SCALE)
                for n in self._range_groups()}

    # ----------------------------------------------------------------------------------- forward
    def forward(self, x, pc_hm=None, pc_dep=None, calib=None):
        if self.training:
            if not self.freezeBackbone:
                raise NotImplementedError("training: only the frozen-backbone mode is implemented (build the model with "
                                          "MODEL.FREEZE_BACKBONE = True: the heads learn on the frozen trunk, unfreeze_neck() / "
                                          "unfreeze_base() / unfreeze_stem() add the rest - unfreeze_stem() trains every "
                                          "parameter); call model.eval()")
            if self._base_train:
                return self._forward_train_base(x, pc_hm, pc_dep, calib)
            if self._neck_train:
                return self._forward_train_neck(x, pc_hm, pc_dep, calib)
            return self._forward_train(x, pc_hm, pc_dep, calib)
        self._repack_if_stale()
        if not x.is_cuda:
            raise _lib.CfHipError("DLASeg.forward needs device tensors: the HIP path has no CPU fallback")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 32 or x.shape[3] % 32:
            raise ValueError(f"images must be (B,3,H,W) with H,W multiples of 32, got {tuple(x.shape)}")
        B, _, H, W = x.shape
        dev = x.device
        x = x.float().contiguous()
        if self.isRadarEnabled:
            if pc_dep is None or (calib is None and not self.isEarly):    # (early fusion only hands calib through)
                raise ValueError("radar model: pc_dep and calib are required")
            if tuple(pc_dep.shape) != (B, 3, H // 4, W // 4):
                raise ValueError(f"pc_dep must be {(B, 3, H // 4, W // 4)}, got {tuple(pc_dep.shape)}")
            if pc_dep.dtype != torch.float32 or not pc_dep.is_contiguous():
                raise ValueError("pc_dep must be contiguous float32")
            if calib is not None:
                calib = calib.reshape(B, 3, 4).float().contiguous()
        # One model may be driven from several HIP streams and host threads.  A plan owns its intermediate buffers, so
        # plans are keyed by the stream the call is issued on (two forwards in flight on two streams never share a
        # buffer); building, patching the per-call pointers into the argument blocks and issuing the launches happen
        # under the model's lock (kernel arguments are copied at launch, so the blocks are free again on return).
        with self._lock, torch.cuda.device(dev):
            if self._packed is None:
                self._prepare(dev)
            sid = torch.cuda.current_stream(dev).cuda_stream
            if self.use_graph:
                return self._forward_graph(x, pc_dep, calib, B, H, W, dev, sid)
            return self._forward_eager(x, pc_dep, calib, B, H, W, dev, sid)

    # ---------------------------------------------------------------------------------- training
    def _head_params(self, h):
        """(weights, biases) of head h: the module's own nn.Parameters in layer order (indices 0, 2, 4, ... of the Sequential)"""
        n = len(self.config.head_conv[h]) + 1
        return ([self.get_parameter(f"detectHead_0.{h}.{2 * i}.weight") for i in range(n)],
                [self.get_parameter(f"detectHead_0.{h}.{2 * i}.bias") for i in range(n)])

    def _train_trunk(self, x, pc, B, H, W, dev, sid):
        """The frozen trunk of a training forward: the eval plan's launches (split-fp16, BN folded with the running statistics)
        under no_grad -> the (B, H/4, W/4, 64) NHWC feature map, a buffer of the plan (valid until the next training forward of
        this shape on this stream).  model.streams > 1: sub-batches on concurrent streams, under the eval forward's rule.
        pc (early fusion): the normalised radar map the stem reads."""
        h4, w4, n = H // 4, W // 4, int(self.streams)
        if not (n > 1 and B % n == 0 and (B // n) * H * W >= self.min_sub_batch * 448 * 800):
            n = 1
        k = B // n

        def first():
            feat = torch.empty((B, h4, w4, 64), device=dev, dtype=torch.float32)
            p = _Plan(self, k, H, W, dev, part="trunk", feat=feat[:k])
            p.train_feat = feat
            return p

        with torch.no_grad():
            p0 = self._plan((B, H, W, dev, sid, "train-trunk", 0, n), first)
            feat = p0.train_feat
            if n == 1:
                p0.run_trunk(x, pc)
                return feat
            cur = torch.cuda.current_stream(dev)
            pool = _side_streams(dev, sid, n)
            for i in range(n):
                sl = slice(i * k, (i + 1) * k)
                tp = p0 if i == 0 else self._plan((B, H, W, dev, sid, "train-trunk", i, n),
                                                  lambda: _Plan(self, k, H, W, dev, part="trunk", feat=feat[sl]))
                s = cur if i == n - 1 else pool[i]
                if s is not cur:
                    s.wait_stream(cur)
                with torch.cuda.stream(s):
                    tp.run_trunk(x[sl], pc[sl] if pc is not None else None)
            for s in pool[:n - 1]:
                cur.wait_stream(s)
            return feat

    def _check_train_images(self, x):
        if self.use_graph:
            raise NotImplementedError("training mode: model.use_graph is not supported (autograd does not record through a captured "
                                      "graph); set model.use_graph = False")
        if not x.is_cuda:
            raise _lib.CfHipError("DLASeg.forward needs device tensors: the HIP path has no CPU fallback")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 32 or x.shape[3] % 32:
            raise ValueError(f"images must be (B,3,H,W) with H,W multiples of 32, got {tuple(x.shape)}")

    def _check_train_radar(self, B, h4, w4, pc_hm, pc_dep):
        """the radar arguments of a training forward on a (B, h4, w4) feature map -> pc_hm detached and contiguous (or None)"""
        if not self.isRadarEnabled:
            return pc_hm
        if pc_hm is None:
            raise ValueError("radar model in training mode: pc_hm (the dataset's radar map) is required - no frustum "
                             "association runs in training (detectHeads.py:176-181)")
        if tuple(pc_hm.shape) != (B, 3, h4, w4) or pc_hm.dtype != torch.float32:
            raise ValueError(f"pc_hm must be float32 {(B, 3, h4, w4)}, got {pc_hm.dtype} {tuple(pc_hm.shape)}")
        if not self.isEarly and (pc_dep is None or tuple(pc_dep.shape) != (B, 3, h4, w4)):
            raise ValueError(f"radar model: pc_dep must be {(B, 3, h4, w4)}")
        return pc_hm.detach().contiguous()

    def _forward_train(self, x, pc_hm, pc_dep, calib):
        """model.train() with MODEL.FREEZE_BACKBONE: the reference's training forward (base_model.py:83-106, detectHeads.py:117-191)
        with the trunk frozen.  The trunk runs through the eval plan under no_grad; every head runs through `ops.head_stack` on the
        module's own parameters, so `loss.backward()` leaves a gradient on each `detectHead_0.*` parameter and on nothing else.
        Middle fusion: the caller's `pc_hm` (B,3,H/4,W/4) - the dataset's association map - feeds the secondary heads; no frustum
        association runs and nothing is normalised in place.  Early fusion: `pc_hm` is the map the six-channel stem reads.
        Deviation from the reference: the frozen trunk always uses the folded running statistics of its BatchNorm layers (the
        reference leaves dla_up / ida_up - and, without MODEL.NORM_EVAL, base - in batch-statistics mode).
        It is `forward_heads` on `_train_trunk`'s map.
        After `unfreeze_neck()` the training forward is `_forward_train_neck` instead: the base (levels 0-5) stays frozen on the
        eval plan, dla_up / ida_up run through `forward_neck` (ops.deform_conv_block / ops.upsample_dw_add, NHWC, batch statistics
        as in the reference) and the heads with their input gradient on, so `loss.backward()` also leaves a gradient on every
        `dla_up.*` / `ida_up.*` parameter."""
        self._check_train_images(x)
        B, _, H, W = x.shape
        dev = x.device
        x = x.detach().float().contiguous()
        pc_hm = self._check_train_radar(B, H // 4, W // 4, pc_hm, pc_dep)
        with self._lock, torch.cuda.device(dev):
            if self._packed is None:
                self._prepare(dev)
            sid = torch.cuda.current_stream(dev).cuda_stream
            # (a copy: autograd keeps the map until backward, the plan's buffer is overwritten by the next forward)
            feat = self._train_trunk(x, pc_hm if self.isEarly else None, B, H, W, dev, sid).clone()
            return self._heads_train(feat, False, pc_hm, pc_dep, calib)

    # ------------------------------------------------------------------------- training: the neck
    NECK_LEVEL_CHANNELS = (64, 128, 256, 512)

    def unfreeze_neck(self, flag=True):
        """Let `dla_up.*` / `ida_up.*` learn beside the heads (flag=False: freeze them again): sets their `requires_grad` and
        selects the neck-training forward for `model.train()` - forward_heads(forward_neck(forward_base(x)), ...) with the heads'
        input gradient on.  The base (DLA-34 levels 0-5) stays frozen, so this needs MODEL.FREEZE_BACKBONE; without this call
        every path is what it was.  -> self"""
        if not self.freezeBackbone:
            raise NotImplementedError("unfreeze_neck: only with MODEL.FREEZE_BACKBONE = True (the base stays frozen; training the "
                                      "whole trunk is not implemented)")
        for name, p in self.named_parameters():
            if name.startswith(("dla_up.", "ida_up.")):
                p.requires_grad_(bool(flag))
        self._neck_train = bool(flag)
        return self

    def _base_levels(self, x, pc, B, H, W, dev, sid):
        """the frozen base of a training forward: the eval plan's backbone launches under no_grad -> the NHWC maps of levels 2-5,
        buffers of the plan (valid until the next call of this shape on this stream)"""
        with torch.no_grad():
            p = self._plan((B, H, W, dev, sid, "train-base"), lambda: _Plan(self, B, H, W, dev, part="base"))
            p.run_trunk(x, pc)
            return p.levels

    def forward_base(self, images, pc_hm=None):
        """The frozen base alone: images (B,3,H,W) -> the four level maps the neck reads (levels 2-5: 64, 128, 256, 512 channels at
        H/4 .. H/32), NCHW, fresh tensors, under no_grad through the eval plan (split-fp16, BatchNorm folded with the running
        statistics).  Early fusion: `pc_hm` (B,3,H/4,W/4) is the radar map the six-channel stem reads, as in `forward_trunk`."""
        self._check_train_images(images)
        B, _, H, W = images.shape
        dev = images.device
        x = images.detach().float().contiguous()
        pc = self._check_train_radar(B, H // 4, W // 4, pc_hm, None) if self.isEarly else None
        with self._lock, torch.cuda.device(dev):
            if self._packed is None:
                self._prepare(dev)
            sid = torch.cuda.current_stream(dev).cuda_stream
            with torch.no_grad():
                return [ops.nhwc_to_nchw(t) for t in self._base_levels(x, pc, B, H, W, dev, sid)]

    def _neck_block(self, p, xn):
        """one DeformConv of the neck (dla.py:456-472) on the module's own parameters; BatchNorm follows model.training"""
        g, b = self.get_parameter, self.get_buffer
        s = (self._scale(p + ".conv_offset_mask"), self._scale(p))
        y = ops.deform_conv_block_nhwc(xn, g(p + ".conv_offset_mask.weight"), g(p + ".conv_offset_mask.bias"), g(p + ".weight"),
                                       g(p + ".bias"), g(p + ".activation.0.weight"), g(p + ".activation.0.bias"),
                                       b(p + ".activation.0.running_mean"), b(p + ".activation.0.running_var"),
                                       training=self.training, in_scales=None if None in s else s, pack_verify=False)
        if self.training:
            b(p + ".activation.0.num_batches_tracked").add_(1)
        return y

    def _neck_ida(self, p, layers, startp, endp):
        """IDAUp.forward (dla.py:518-524) through the two operators"""
        for i in range(startp + 1, endp):
            j = i - startp
            up_w = self.get_parameter(f"{p}.up_{j}.weight")
            proj = self._neck_block(f"{p}.proj_{j}", layers[i])
            layers[i] = self._neck_block(f"{p}.node_{j}", ops.upsample_dw_add_nhwc(proj, up_w, up_w.shape[-1] // 2, layers[i - 1]))

    def _neck_nhwc(self, levels):
        """DLAUp.forward + IDAUp.forward (dla.py:553-559, 627-635) on the NHWC maps of levels 2-5 -> the (B,h,w,64) feature map.
        A plain composition on the caller's stream: no lanes, groups or sub-batch streams."""
        layers = list(levels)
        out = [layers[-1]]
        for i in range(len(layers) - 1):
            self._neck_ida(f"dla_up.ida_{i}", layers, len(layers) - i - 2, len(layers))
            out.insert(0, layers[-1])
        y = out[:3]
        self._neck_ida("ida_up", y, 0, 3)
        return y[-1]

    def forward_neck(self, levels):
        """The reference's neck, `DLAUp.forward` + `IDAUp.forward` (dla.py:518-559, 627-635), on the model's own parameters through
        `ops.deform_conv_block` and `ops.upsample_dw_add`: `levels` = the four (B,C,h,w) fp32 maps of levels 2-5 (`forward_base`'s,
        or a caller's own) -> the (B,64,H/4,W/4) feature map, differentiable in every `dla_up.*` / `ida_up.*` parameter that
        requires grad and in the levels that do.  NHWC inside, on the caller's stream.  BatchNorm follows `model.training`: batch
        statistics (and the running statistics' update) under `model.train()`, as the reference runs dla_up / ida_up; the running
        statistics otherwise.  A calibrated model passes its per-layer pre-scales, so no range check and no host sync runs per
        layer; an uncalibrated one checks each block's input as `ops.deform_conv2d` does.  In training mode the packed weights
        are marked stale: the next eval forward re-packs with the new weights and running statistics."""
        levels = list(levels)
        if len(levels) != 4 or not all(torch.is_tensor(t) and t.is_cuda for t in levels):
            raise _lib.CfHipError("DLASeg.forward_neck needs the four level maps as device tensors: the HIP path has no CPU fallback")
        for t, c in zip(levels, self.NECK_LEVEL_CHANNELS):
            if t.dim() != 4 or t.shape[1] != c or t.dtype != torch.float32:
                raise ValueError(f"levels must be float32 (B,{c},h,w) maps of levels 2-5, got {t.dtype} {tuple(t.shape)}")
        if self.use_graph and self.training:
            raise NotImplementedError("training mode: model.use_graph is not supported (autograd does not record through a captured "
                                      "graph); set model.use_graph = False")
        dev = levels[0].device
        with self._lock, torch.cuda.device(dev):
            if self._packed is None:
                self._prepare(dev)
            if self.training:
                self._stale = True
            feat = self._neck_nhwc([ops._to_nhwc(t) for t in levels])
            return ops._NhwcToNchwFn.apply(feat)

    def _forward_train_neck(self, x, pc_hm, pc_dep, calib):
        """model.train() after unfreeze_neck(): forward_heads(forward_neck(forward_base(x)), ...) without the layout launches in
        between - the base on the eval plan under no_grad, the neck and the heads under autograd (NHWC throughout)."""
        self._check_train_images(x)
        B, _, H, W = x.shape
        dev = x.device
        x = x.detach().float().contiguous()
        pc_hm = self._check_train_radar(B, H // 4, W // 4, pc_hm, pc_dep)
        with self._lock, torch.cuda.device(dev):
            if self._packed is None:
                self._prepare(dev)
            sid = torch.cuda.current_stream(dev).cuda_stream
            # (copies: autograd keeps the maps until backward, the plan's buffers are overwritten by the next forward)
            levels = [t.clone() for t in self._base_levels(x, pc_hm if self.isEarly else None, B, H, W, dev, sid)]
            self._stale = True
            feat = self._neck_nhwc(levels)
            return self._heads_train(feat, True, pc_hm, pc_dep, calib)

    # ------------------------------------------------------------------------- training: the base, levels 2-5
    def unfreeze_base(self, flag=True):
        """Let the DLA-34 base from level 2 upward (`base.level2.*` .. `base.level5.*`, nearly all of the base's parameters) learn
        beside the neck and the heads (flag=False: freeze base and neck again): implies `unfreeze_neck(flag)`, sets their
        `requires_grad` and selects the base-training forward for `model.train()` -
        forward_heads(forward_neck(forward_levels(forward_stem(x))), ...).  Needs MODEL.FREEZE_BACKBONE, like `unfreeze_neck`;
        without this call every path is what it was.
        Deviation from the reference, unless `unfreeze_stem()`: the stem stays frozen.  `base.base_layer`, `level0` and `level1`
        (the 7x7 convolution and the 16 / 32-channel layers: a fraction of a percent of the base's parameters) keep running on
        the eval stem kernel with their folded running statistics and receive no gradient; `unfreeze_stem()` trains them too.
        -> self"""
        if not self.freezeBackbone:
            raise NotImplementedError("unfreeze_base: only with MODEL.FREEZE_BACKBONE = True (the stem stays frozen; training the "
                                      "whole trunk is not implemented)")
        self.unfreeze_neck(flag)
        for name, p in self.named_parameters():
            if name.startswith(("base.level2.", "base.level3.", "base.level4.", "base.level5.")):
                p.requires_grad_(bool(flag))
        self._base_train = bool(flag)
        if not flag and self._stem_train:                # (a stem that learns under a frozen base is no mode of this model)
            for name, p in self.named_parameters():
                if name.startswith(("base.base_layer.", "base.level0.", "base.level1.")):
                    p.requires_grad_(False)
            self._stem_train = False
        return self

    def _stem_map(self, x, pc, B, H, W, dev, sid):
        """the frozen stem of a training forward: the eval plan's stem launch under no_grad -> the (B, H/2, W/2, 32) NHWC map of
        level 1, a buffer of the plan (valid until the next call of this shape on this stream)"""
        with torch.no_grad():
            p = self._plan((B, H, W, dev, sid, "train-stem"), lambda: _Plan(self, B, H, W, dev, part="stem"))
            p.run_trunk(x, pc)
            return p.levels[0]

    def forward_stem(self, images, pc_hm=None):
        """The frozen stem alone (`base.base_layer`, `level0`, `level1`): images (B,3,H,W) -> the (B,32,H/2,W/2) map of level 1,
        NCHW, a fresh tensor, under no_grad through the eval plan (split-fp16, BatchNorm folded with the running statistics).
        Early fusion: `pc_hm` (B,3,H/4,W/4) is the radar map the six-channel stem reads, as in `forward_base`."""
        self._check_train_images(images)
        B, _, H, W = images.shape
        dev = images.device
        x = images.detach().float().contiguous()
        pc = self._check_train_radar(B, H // 4, W // 4, pc_hm, None) if self.isEarly else None
        with self._lock, torch.cuda.device(dev):
            if self._packed is None:
                self._prepare(dev)
            sid = torch.cuda.current_stream(dev).cuda_stream
            with torch.no_grad():
                return ops.nhwc_to_nchw(self._stem_map(x, pc, B, H, W, dev, sid))

    # ------------------------------------------------------------------------- training: the stem
    STEM_LAYERS = (("base.base_layer", 1), ("base.level0", 1), ("base.level1", 2))

    def unfreeze_stem(self, flag=True):
        """Let the stem (`base.base_layer.*`, `base.level0.*`, `base.level1.*`) learn too, so that every parameter of the model
        trains as in the reference's normal run (flag=False: freeze stem, base and neck again): implies `unfreeze_base(flag)`,
        sets the stem parameters' `requires_grad` and makes the base-training forward run the stem through
        `ops.stem_conv_bn_relu` under autograd (`forward_stem_train`) - batch statistics, running statistics updated - instead
        of the eval stem kernel.  An early-fusion model then learns its radar input through `base.base_layer.0.weight[:, 3:6]`.
        Needs MODEL.FREEZE_BACKBONE, like its siblings; without this call every path is what it was.  -> self"""
        if not self.freezeBackbone:
            raise NotImplementedError("unfreeze_stem: only with MODEL.FREEZE_BACKBONE = True (build the model frozen, then call "
                                      "unfreeze_stem(): that is the full-training mode)")
        self.unfreeze_base(flag)
        for name, p in self.named_parameters():
            if name.startswith(("base.base_layer.", "base.level0.", "base.level1.")):
                p.requires_grad_(bool(flag))
        self._stem_train = bool(flag)
        return self

    def _stem_train_nhwc(self, x, pc):
        """DLA.forward's base_layer, level0, level1 (dla.py:225-228) on the module's own parameters: the NCHW image (and, early
        fusion, the radar map) -> the (B, H/2, W/2, 32) NHWC map of level 1; BatchNorm follows model.training"""
        g, b = self.get_parameter, self.get_buffer
        t = x
        for i, (p, stride) in enumerate(self.STEM_LAYERS):
            t = ops.stem_conv_bn_relu_nhwc(t, g(p + ".0.weight"), g(p + ".1.weight"), g(p + ".1.bias"), b(p + ".1.running_mean"),
                                           b(p + ".1.running_var"), stride=stride, training=self.training,
                                           radar=pc if i == 0 else None)
            if self.training:
                b(p + ".1.num_batches_tracked").add_(1)
        return t

    def forward_stem_train(self, images, pc_hm=None):
        """The differentiable twin of `forward_stem`: images (B,3,H,W) -> the (B,32,H/2,W/2) map of level 1, NCHW, through three
        `ops.stem_conv_bn_relu` blocks on the model's own parameters (exact fp32 on the raw weights, NHWC inside, on the caller's
        stream), differentiable in every `base.base_layer.*` / `level0.*` / `level1.*` parameter that requires grad.  Early
        fusion: `pc_hm` (B,3,H/4,W/4) is the radar map the six-channel first layer samples; neither it nor the images receive a
        gradient.  BatchNorm follows `model.training`: batch statistics with the running statistics updated in the kernel and
        `num_batches_tracked` incremented here, the running statistics otherwise.  In training mode the packed weights are
        marked stale: the next eval forward re-packs and equals a fresh model loaded from the `state_dict`."""
        self._check_train_images(images)
        B, _, H, W = images.shape
        dev = images.device
        x = images.detach().float().contiguous()
        pc = self._check_train_radar(B, H // 4, W // 4, pc_hm, None) if self.isEarly else None
        with self._lock, torch.cuda.device(dev):
            if self._packed is None:
                self._prepare(dev)
            if self.training:
                self._stale = True
            return ops._NhwcToNchwFn.apply(self._stem_train_nhwc(x, pc))

    def _cba(self, name, conv, bn, x, stride=1, residual=None, relu=True):
        """one conv + BatchNorm block of the base on the module's own parameters; BatchNorm follows model.training"""
        g, b = self.get_parameter, self.get_buffer
        y = ops.conv_bn_act_nhwc(x, g(conv + ".weight"), g(bn + ".weight"), g(bn + ".bias"), b(bn + ".running_mean"),
                                 b(bn + ".running_var"), stride=stride, residual=residual, relu=relu, training=self.training,
                                 in_scale=self._scale(name), pack_verify=False)
        if self.training:
            b(bn + ".num_batches_tracked").add_(1)
        return y

    def _lv_block(self, p, x, stride, residual):
        """BasicBlock.forward (dla.py:144-161)"""
        t = self._cba(p + ".conv1", p + ".conv1", p + ".bn1", x, stride=stride)
        return self._cba(p + ".conv2", p + ".conv2", p + ".bn2", t, residual=x if residual is None else residual)

    def _lv_tree(self, p, levels, x, stride, level_root, children=None, pooled=None):
        """Tree.forward (dla.py:104-118); a nested Tree computes its own residual (the outer Trees of levels 3 and 4 have no project).
        pooled: the 2x2 max-pool of x where the enclosing Tree has taken it already (both pool the same tensor: one launch)."""
        children = [] if children is None else children
        bottom = pooled if pooled is not None else (ops.max_pool2x2_nhwc(x) if stride > 1 else x)
        if (p + ".project.0.weight") in self._base_names:
            residual = self._cba(p + ".project", p + ".project.0", p + ".project.1", bottom, relu=False)
        else:
            residual = bottom
        if level_root:
            children.append(bottom)
        if levels > 1:
            x1 = self._lv_tree(p + ".tree1", levels - 1, x, stride, False, pooled=bottom if stride > 1 else None)
            children.append(x1)
            return self._lv_tree(p + ".tree2", levels - 1, x1, 1, False, children)
        x1 = self._lv_block(p + ".tree1", x, stride, residual)
        x2 = self._lv_block(p + ".tree2", x1, 1, None)
        # Root.forward (dla.py:36-42; residual_root is False for DLA-34): one 1x1 block over the channel concat, autograd splits
        return self._cba(p + ".root", p + ".root.conv", p + ".root.bn", torch.cat([x2, x1, *children], dim=3))

    def _levels_nhwc(self, y1):
        """DLA.forward's levels 2-5 (dla.py:225-232) on the NHWC map of level 1 -> the four NHWC level maps"""
        self._base_names = {n for n, _ in self.named_parameters() if n.startswith("base.")}
        out, x = [], y1
        for lvl, levels, root in ((2, 1, False), (3, 2, True), (4, 2, True), (5, 1, True)):
            x = self._lv_tree(f"base.level{lvl}", levels, x, 2, root)
            out.append(x)
        return out

    def forward_levels(self, level1):
        """The reference's `DLA.forward` from level 2 upward (dla.py:44-118, 121-161, 193-232) on the model's own parameters through
        `ops.conv_bn_act` and `ops.max_pool2x2`: `level1` = the (B,32,h,w) fp32 map of level 1 (`forward_stem`'s, or a caller's
        own; h, w multiples of 16) -> the four level maps (64, 128, 256, 512 channels at h/2 .. h/16), NCHW, differentiable in
        every `base.level[2-5].*` parameter that requires grad and in `level1` if that does.  NHWC inside, on the caller's stream.
        BatchNorm follows `model.training`: batch statistics with the running statistics updated in the kernel and
        `num_batches_tracked` incremented here, the running statistics otherwise.  A calibrated model passes its per-layer
        pre-scales (no range check, no host sync); an uncalibrated one checks each block's input as `ops.deform_conv2d` does.  In
        training mode the packed weights are marked stale: the next eval forward re-packs and equals a fresh model loaded from
        the `state_dict`."""
        if not torch.is_tensor(level1) or not level1.is_cuda:
            raise _lib.CfHipError("DLASeg.forward_levels needs a device tensor: the HIP path has no CPU fallback")
        if level1.dim() != 4 or level1.shape[1] != 32 or level1.dtype != torch.float32 or level1.shape[2] % 16 or level1.shape[3] % 16:
            raise ValueError(f"level1 must be a float32 (B,32,h,w) map with h, w multiples of 16, got {level1.dtype} {tuple(level1.shape)}")
        if self.use_graph and self.training:
            raise NotImplementedError("training mode: model.use_graph is not supported (autograd does not record through a captured "
                                      "graph); set model.use_graph = False")
        with self._lock, torch.cuda.device(level1.device):
            if self._packed is None:
                self._prepare(level1.device)
            if self.training:
                self._stale = True
            return [ops._NhwcToNchwFn.apply(t) for t in self._levels_nhwc(ops._to_nhwc(level1))]

    def _forward_train_base(self, x, pc_hm, pc_dep, calib):
        """model.train() after unfreeze_base(): forward_heads(forward_neck(forward_levels(forward_stem(x))), ...) without the layout
        launches in between - the stem on the eval plan under no_grad, levels 2-5, the neck and the heads under autograd (NHWC
        throughout).  After unfreeze_stem() the stem runs under autograd too (`_stem_train_nhwc`, forward_stem_train's body)."""
        self._check_train_images(x)
        B, _, H, W = x.shape
        dev = x.device
        x = x.detach().float().contiguous()
        pc_hm = self._check_train_radar(B, H // 4, W // 4, pc_hm, pc_dep)
        with self._lock, torch.cuda.device(dev):
            if self._packed is None:
                self._prepare(dev)
            sid = torch.cuda.current_stream(dev).cuda_stream
            if self._stem_train:
                y1 = self._stem_train_nhwc(x, pc_hm if self.isEarly else None)
            else:
                # (a copy: autograd keeps the map until backward, the plan's buffer is overwritten by the next forward)
                y1 = self._stem_map(x, pc_hm if self.isEarly else None, B, H, W, dev, sid).clone()
            self._stale = True
            feat = self._neck_nhwc(self._levels_nhwc(y1))
            return self._heads_train(feat, True, pc_hm, pc_dep, calib)

    def forward_trunk(self, images, pc_hm=None):
        """The frozen trunk alone: images (B,3,H,W) -> the (B,64,H/4,W/4) NCHW feature map the heads read, under no_grad, a fresh
        tensor (`forward_heads(forward_trunk(images), ...)` is the training forward).  Early fusion: `pc_hm` (B,3,H/4,W/4) is the
        radar map the six-channel stem reads.  Works in either mode and whatever MODEL.FREEZE_BACKBONE says: the trunk always
        runs through the eval plan (split-fp16, BatchNorm folded with the running statistics) and is not differentiable."""
        self._check_train_images(images)
        B, _, H, W = images.shape
        dev = images.device
        x = images.detach().float().contiguous()
        pc = None
        if self.isEarly:
            pc = self._check_train_radar(B, H // 4, W // 4, pc_hm, None)
        with self._lock, torch.cuda.device(dev):
            if self._packed is None:
                self._prepare(dev)
            sid = torch.cuda.current_stream(dev).cuda_stream
            with torch.no_grad():
                return ops.nhwc_to_nchw(self._train_trunk(x, pc, B, H, W, dev, sid))

    def forward_heads(self, feat, pc_hm=None, pc_dep=None, calib=None):
        """The reference's `detectHead_0(imgFeatures, pc_hm, pc_dep, calib)` in training mode on a caller's feature map: `feat`
        (B,64,h,w) fp32 on the device - `forward_trunk`'s, or the output of a trunk / neck of the caller's own.  Same dict, keys,
        order and argument checks as the training forward.  Differentiable in every `detectHead_0.*` parameter and, when `feat`
        requires grad, in `feat` (`ops.head_stack(..., input_grad=True)`: the eleven heads' gradients are summed by autograd);
        the radar map is never differentiated.  Training mode only, whatever MODEL.FREEZE_BACKBONE says; marks the packed head
        weights stale as a training forward does."""
        if not self.training:
            raise NotImplementedError("forward_heads is the training forward of the heads: call model.train() first (the eval "
                                      "forward runs the packed heads at the peaks, model(images, ...))")
        if self.use_graph:
            raise NotImplementedError("training mode: model.use_graph is not supported (autograd does not record through a captured "
                                      "graph); set model.use_graph = False")
        if not torch.is_tensor(feat) or not feat.is_cuda:
            raise _lib.CfHipError("DLASeg.forward_heads needs device tensors: the HIP path has no CPU fallback")
        if feat.dim() != 4 or feat.shape[1] != 64 or feat.dtype != torch.float32:
            raise ValueError(f"feat must be float32 (B,64,h,w), got {feat.dtype} {tuple(feat.shape)}")
        B, _, h4, w4 = feat.shape
        pc_hm = self._check_train_radar(B, h4, w4, pc_hm, pc_dep)
        with self._lock, torch.cuda.device(feat.device):
            grad = torch.is_grad_enabled() and feat.requires_grad
            if grad:
                featn = ops._NchwToNhwcFn.apply(feat)
            else:
                with torch.no_grad():
                    featn = ops.nchw_to_nhwc(feat.contiguous())
            return self._heads_train(featn, grad, pc_hm, pc_dep, calib)

    def _heads_train(self, feat, input_grad, pc_hm, pc_dep, calib):
        """every head through `ops.head_stack_nhwc` on the NHWC map `feat` (B,h,w,64) and the module's own parameters; the
        arguments are checked (`_check_train_radar`), the lock is held"""
        middle = self.isRadarEnabled and not self.isEarly
        heads, secondary = self.config.heads, (SECONDARY_HEADS if middle else [])
        self._stale = True
        y = {}

        def run(h, x2n):
            ws, bs = self._head_params(h)
            final = "heatmap" if h == "heatmap" else ("depth" if h in ("depth", "depth2") else None)
            return ops.head_stack_nhwc(feat, 64, x2n, 0 if x2n is None else 3, ws, bs, final=final, input_grad=input_grad)

        for h in heads:
            if h in secondary:
                continue
            r = run(h, None)
            y[h] = r[0] if isinstance(r, tuple) else r
            if h == "depth":
                depth_raw = r[1]
        if "depth" in heads:
            y["depthMap"] = depth_raw
        y["calib"] = calib
        if middle:
            y["pc_hm_in"] = pc_dep[:, :1]
            y["pc_hm"] = pc_hm[:, 0, :, :].unsqueeze(1)
            with torch.no_grad():
                pcn = ops.nchw_to_nhwc(pc_hm)
            for h in secondary:
                if h not in heads:
                    continue
                r = run(h, pcn)
                y[h] = r[1] if h == "depth2" else r          # (depth2: the raw map until depthMap has taken it)
                if h == "depth2":
                    act = r[0]
            y["pc_hm_out"] = pc_hm[:, :1]
            if "depth2" in heads:
                y["depthMap"] = y["depth2"]
                y["depth2"] = act
        return [y]

    def _forward_eager(self, x, pc_dep, calib, B, H, W, dev, sid, store=None):
        # (min_sub_batch counts 448 x 800 frames: a sub-batch of a larger input carries proportionally more work)
        if self.streams > 1 and B % self.streams == 0 and (B // self.streams) * H * W >= self.min_sub_batch * 448 * 800:
            return self._forward_concurrent(x, pc_dep, calib, B, H, W, dev, sid, store)
        plan = self._plan((B, H, W, dev, sid), lambda: _Plan(self, B, H, W, dev), store)
        return plan.run(self, x, pc_dep, calib)

    def _forward_graph(self, x, pc_dep, calib, B, H, W, dev, sid):
        """model.use_graph: the whole forward - including the fork into the trunk streams and the join in front of
        the heads - captured ONCE as a HIP graph over static input / output buffers and replayed per call (one
        hipGraphLaunch instead of ~100-350 launches from Python: with 4 trunk streams the eager path is bound by the
        host's launch rate).  Semantics are those of the eager forward: fresh output tensors every call (copies out
        of the static ones), `pc_hm_in` a view of the CALLER's pc_dep, `calib` the caller's tensor.  MODEL.FRUSTUM = False:
        the graph normalises its static copy of pc_dep; channel 0 is copied back, so the caller's tensor ends up normalised
        exactly once per call and `pc_hm_in` / `pc_hm` / `pc_hm_out` are views of it, as in the eager forward.  Early fusion: the same copy-back of channel 0; there are no pc_hm outputs."""
        in_place = pc_dep is not None and self.isRadarEnabled and not self.isFrustumEnabled
        key = (B, H, W, dev, sid, "graph", self.streams)
        g = self._graphs.pop(key, None)
        if g is None:
            # warm-up (one-time attribute calls, the stream probe) with a throw-away plan set: its buffers are freed
            # again before the capture allocates the set the graph keeps
            # (in_place: the warm-up must not be the caller's tensor's first normalisation)
            self._forward_eager(x, pc_dep.clone() if in_place else pc_dep, calib, B, H, W, dev, sid, store={})
            torch.cuda.synchronize(dev)
            gx = x.clone()
            gpc = pc_dep.clone() if pc_dep is not None else None
            gcal = calib.clone() if calib is not None else None
            graph = torch.cuda.CUDAGraph()
            plans = {}                                                 # owned by the graph (see _plan)
            # No garbage collection may run inside the capture: a collected object with device-side teardown (an older
            # captured graph of a model that is itself garbage, say) aborts the process when its destructor runs while a
            # stream is capturing - and torch.cuda.graph() no longer collects on entry by default.  Collect now, then hold
            # the collector off until the capture has ended.
            import gc
            with _CAPTURE_LOCK:
                gc.collect()
                gc_was_on = gc.isenabled()
                gc.disable()
                try:
                    with torch.cuda.graph(graph):
                        cap_sid = torch.cuda.current_stream(dev).cuda_stream   # plans of the capture stream (own buffers)
                        gout = self._forward_eager(gx, gpc, gcal, B, H, W, dev, cap_sid, store=plans)[0]
                finally:
                    if gc_was_on:
                        gc.enable()
            g = (graph, gx, gpc, gcal, gout, plans)
        self._graphs[key] = g                                          # most recently used last
        while len(self._graphs) > max(1, int(self.max_plan_sets)):
            with _CAPTURE_LOCK:
                self._graphs.pop(next(iter(self._graphs)))
        graph, gx, gpc, gcal, gout, _plans = g
        gx.copy_(x)
        if gpc is not None:
            gpc.copy_(pc_dep)
        if gcal is not None:
            gcal.copy_(calib)
        graph.replay()
        if in_place:
            pc_dep[:, :1].copy_(gpc[:, :1])
        y, fresh = {}, {}
        for k, v in gout.items():
            if k == "calib":
                y[k] = calib
            elif k == "pc_hm_in" or (in_place and k == "pc_hm_out"):
                y[k] = pc_dep[:, :1]
            elif in_place and k == "pc_hm":
                y[k] = pc_dep[:, 0, :, :].unsqueeze(1)
            else:                                                   # aliases in gout stay aliases (depthMap / pc_hm views)
                base = v._base if v._base is not None else v
                if id(base) not in fresh:
                    fresh[id(base)] = base.clone()
                nb = fresh[id(base)]
                y[k] = nb if v._base is None else nb.as_strided(v.size(), v.stride(), v.storage_offset() - base.storage_offset())
        return [y]

    def _forward_concurrent(self, x, pc_dep, calib, B, H, W, dev, sid, store=None):
        """Backbone + neck as `self.streams` sub-batches, each with its OWN trunk plan (own intermediate buffers)
        on its OWN HIP stream: several of those layers cannot fill the chip on their own (level4: 175 workgroups
        for 256 CUs, the 14x25 / 28x50 maps of the neck, the tail round of most grids) and the other sub-batch's
        launches fill the holes.  The trunks write their slices of ONE full-batch feature map; the heads, top-k,
        frustum association and secondary heads then run for the whole batch on the caller's stream (their grids
        fill the chip, and a launch there overlaps nothing - HIP-event and rocprofv3 durations of the head kernels
        mean the same thing as in the single-stream forward).  Frames are independent, so the result is the
        single-stream one bit for bit."""
        n = self.streams
        k = B // n
        h4, w4 = H // 4, W // 4
        cur = torch.cuda.current_stream(dev)
        pool = _side_streams(dev, sid, n)
        spec = feat_operand(self)
        bf = spec is not None

        def heads_plan():
            feat = torch.empty((B, h4, w4, 64), device=dev, dtype=torch.float32)
            feat_in = torch.empty((B, h4, w4, *spec[0]), device=dev, dtype=spec[1]) if bf else feat
            return _Plan(self, B, H, W, dev, part="heads", feat=feat, feat_in=feat_in)

        hplan = self._plan((B, H, W, dev, sid, "heads", n), heads_plan, store)
        hplan.flush_pending()                              # (unread at-peaks outputs need the feature buffers the trunks are about to overwrite)
        if self.isEarly:
            # early fusion: the in-place normalisation (base_model.py:69-79) once, for the whole batch, on the caller's stream in
            # front of the forks; each trunk's stem reads its sub-batch's slice of the normalised map
            _lib.check(_lib.load().cf_pc_hm_direct(pc_dep.data_ptr(), B, h4, w4, float(self.config.DATASET.MAX_PC_DIST), None, None,
                                                   _lib.stream_ptr()), "cf_pc_hm_direct")
        spans = []
        # model.trunk_on_caller: the LAST trunk is issued on the caller's stream itself (behind the forks of the others), so the
        # heads follow its last launch in stream order and wait for n - 1 events instead of n
        on_cur = bool(self.trunk_on_caller)
        for i in range(n):
            sl = slice(i * k, (i + 1) * k)
            tplan = self._plan((B, H, W, dev, sid, "trunk", i, n),
                               lambda: _Plan(self, k, H, W, dev, part="trunk", feat=hplan.feat[sl],
                                             feat_in=hplan.feat_in[sl] if bf else None), store)
            s = cur if (on_cur and i == n - 1) else pool[i]
            if s is not cur:
                s.wait_stream(cur)
            with torch.cuda.stream(s):
                if self.record_spans:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                tplan.run_trunk(x[i * k:(i + 1) * k], pc_dep[i * k:(i + 1) * k] if self.isEarly else None)
                if self.record_spans:
                    e1.record(s)
                    spans.append((e0, e1))
        for s in (pool[:n - 1] if on_cur else pool):
            cur.wait_stream(s)
        if self.record_spans:
            self.trunk_spans = spans
        return hplan.run(self, None, pc_dep, calib)

    def trunk_overlap(self):
        """With `record_spans` set: the last concurrent forward's trunk spans -> (ms each trunk took, ms during which
        the first two ran at the same time).  Streams on one hardware queue give ~0 overlap.  Syncs."""
        torch.cuda.synchronize()
        (a0, a1), (b0, b1) = self.trunk_spans[:2]
        la, lb = a0.elapsed_time(a1), b0.elapsed_time(b1)
        start_b = a0.elapsed_time(b0)                       # b's start relative to a's
        return [la, lb], max(0.0, min(la, start_b + lb) - max(0.0, start_b))


    # ------------------------------------------------------------------------- instrumentation
    def time_launch(self, name, on=True):
        """Bracket the named launch with HIP events (recorded on the launch stream) in every existing plan that
        holds it; read back with launch_times().  Names: 'tails.primary', 'base.level2.root', ..."""
        for plan in self._all_plans():
            idx = plan.step_index.get(name)
            if idx is None:
                continue
            if on:
                plan.timed.setdefault(idx, [])
            else:
                plan.timed.pop(idx, None)

    def launch_times(self, name):
        """-> (list of ms per recorded launch, algorithmic FLOPs of one launch); syncs."""
        torch.cuda.synchronize()
        out, flops = [], 0.0
        for plan in self._all_plans():
            idx = plan.step_index.get(name)
            if idx is None:
                continue
            flops = plan.step_flops[name]
            for e0, e1 in plan.timed.get(idx, []):
                out.append(e0.elapsed_time(e1))
            if idx in plan.timed:
                plan.timed[idx] = []
        return out, flops

    def time_all(self, on=True):
        """Bracket EVERY launch of every plan with HIP events (dev tool: tools/layer_times.py)."""
        for plan in self._all_plans():
            plan.timed = {i: [] for i in range(len(plan.steps))} if on else {}
            if on and plan.at is not None:
                plan.timed.update({k: [] for k in AT_TIMED})      # (the launches an at-peaks forward adds behind tails.primary)

    def all_launch_times(self):
        """-> [(step name or kernel entry point, mean ms, algorithmic FLOPs)] in launch order (single-plan forward)."""
        torch.cuda.synchronize()
        plan = list(self._plans.values())[-1]
        names = {v: k for k, v in plan.step_index.items()}
        out = []
        for i, step in enumerate(plan.steps):
            ev = plan.timed.get(i, [])
            if not ev:
                continue
            ms = sum(a.elapsed_time(b) for a, b in ev) / len(ev)
            nm = names.get(i, step[0].__name__)
            out.append((nm, ms, plan.step_flops.get(names.get(i, ""), 0.0)))
            if nm == "tails.primary":
                for k in AT_TIMED:
                    ev = plan.timed.get(k, [])
                    if ev:
                        out.append((k, sum(a.elapsed_time(b) for a, b in ev) / len(ev), plan.step_flops.get(k, 0.0)))
        return out

    def conv_flops_per_forward(self):
        """Algorithmic FLOPs (2*MACs) of all conv / DCN / head launches of one forward (the plans in use), as the LAST forward
        of each plan issued them: after an at-peaks forward (heads_at_peaks) the head groups count the pixels they were
        evaluated at (`tails.*`, `at.primary`), after a dense one every pixel."""
        return sum(sum(p.step_flops.values()) for p in self._all_plans())


_network_factory = {"dla": DLASeg}


def getModel(config):
    """model/model.py:18-44 (early fusion: the three radar channels join the image, model.py:35-40)."""
    arch = config.MODEL.ARCH
    num_layers = arch[arch.find("_") + 1:] if "_" in arch else 0
    arch = arch[:arch.find("_")] if "_" in arch else arch
    return _network_factory[arch](num_layers, in_channels=6 if is_early(config) else 3, config=config)
