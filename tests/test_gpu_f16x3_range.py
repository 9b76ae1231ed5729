"""GPU: the split-fp16 ("f16x3") kernels off the default activation pre-scale, every entry point and launch form
(tests/f16x3_ref.py holds the tables, the seeded inputs and the float64 references; tests/test_f16x3_cpu.py their CPU side).

A. Scale invariance, bit for bit.  Inputs, residual, children, pooled input and every bias times 2^k with in_scale times 2^-k
   must give the very bits of the first call times 2^k: every scaling is exact, ReLU commutes with it, DCN offsets and masks
   do not move.  A form that reads the constant 16, another group's scale or another operand's scale cannot pass.
B. Small inputs against float64: inputs relu(randn) * 3 * amp, amp = 2^-24 .. 2^10, in_scale = ops.in_scale_for(max |x|).
   max|err| / max|ref| < 1e-6 (convolutions) / 2e-6 (DCN), and the worst per-channel max|err_c| / max|ref_c| within twice the
   larger of two yardsticks on the same inputs (torch's fp32 operation, the split arithmetic restated in float64).  At
   amp = 2^-12 the same call at the default pre-scale must MISS the first gate - the hazard the host rule removes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import f16x3_ref as R
from tests.f16x3_ref import nhwc, nchw

NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X box"
    from centerfusiondetect3d_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _seed(name):
    return R.SMALL_SEEDS.get(name, 0)


# ------------------------------------------------------------------------------------------------ launchers
# each -> list of NHWC device tensors (one per output / group); amp scales every activation and bias of the case
def _launch_conv(dev, name, amp, scale):
    from centerfusiondetect3d_amd import ops, packing
    c = R.CONV_CASES[name]
    x, w, b, r = R.conv_inputs(c, amp, _seed(name))
    pc = packing.pack_conv_f16(w, b, [packing.Source(c["Ci"], c["Ci"])], stride=c["stride"]).to(dev)
    assert pc.patch and pc.stride == c["stride"]
    Ho, Wo = R.out_hw(c["H"], c["W"], c["stride"])
    out = torch.full((c["B"], Ho, Wo, 32 if c["Co"] == 27 else c["Co"]), NAN, device=dev)
    ops.conv2d_f16x3(pc, [nhwc(x).to(dev)], c["B"], c["H"], c["W"], act=c["act"], residual=None if r is None else nhwc(r).to(dev),
                     out=out, patch=c["entry"] == "patch", in_scale=scale)
    assert bool(torch.isnan(out[..., c["Co"]:]).all())               # the padding channels are never written
    return [out[..., :c["Co"]]]


def _launch_root_concat(dev, amp, scale):
    from centerfusiondetect3d_amd import ops, packing
    c = R.ROOT_CONCAT_CASE
    xs, w, b = R.root_concat_inputs(amp)
    pc = packing.pack_conv_f16(w, b, [packing.Source(n, n) for n in c["chans"]]).to(dev)
    assert not pc.patch
    return [ops.conv2d_f16x3(pc, [nhwc(x).to(dev) for x in xs], c["B"], c["H"], c["W"], act=1, in_scale=scale)]


def _root_operands(dev, name, amp_t, amp_x):
    """packed conv2 / Root and the device operands; amp_t scales t and conv2's bias, amp_x the Root's own inputs and bias"""
    from centerfusiondetect3d_amd import packing
    case = R.ROOT_CASES[name]
    C_, kids = case[0], case[4]
    t, _, _, (w2, b2), _ = R.root_inputs(case, amp_t, _seed(name))
    _, x1, ch, _, (wr, br) = R.root_inputs(case, amp_x, _seed(name))
    pc2 = packing.pack_conv_f16(w2, b2, [packing.Source(C_, C_)]).to(dev)
    pcr = packing.pack_conv_f16(wr, br, [packing.Source(C_, C_), packing.Source(C_, C_)] + [packing.Source(c, c) for c in kids]).to(dev)
    assert pc2.patch and pcr.k_pad == 2 * C_ + sum(kids)
    return pc2, pcr, nhwc(t).to(dev), nhwc(x1).to(dev), [nhwc(c).to(dev) for c in ch]


def _launch_root(dev, name, amp, scales):
    """-> [out, the x2 buffer (NaN where the launch was fused)]"""
    from centerfusiondetect3d_amd import ops
    pc2, pcr, td, x1d, chd = _root_operands(dev, name, amp, amp)
    x2 = torch.full(tuple(td.shape), NAN, device=dev)
    out, _ = ops.conv3x3_root_f16x3(pc2, pcr, td, x1d, chd, x2_out=x2, in_scale=scales[0], root_in_scale=scales[1])
    return [out, x2]


def _launch_proj(dev, name, amp, scale):
    from centerfusiondetect3d_amd import ops, packing
    B, Cp, C_, H, W, _ = R.PROJ_CASES[name]
    t, pooled, (w2, b2), (wp, bp) = R.proj_inputs(R.PROJ_CASES[name], amp, _seed(name))
    pc = packing.pack_conv_f16(w2, b2, [packing.Source(C_, C_)], proj=(wp, bp, packing.Source(Cp, Cp))).to(dev)
    assert pc.patch and pc.proj_k == Cp
    return [ops.conv3x3_proj_f16x3(pc, nhwc(t).to(dev), nhwc(pooled).to(dev), in_scale=scale)]


def _launch_grouped_conv(dev, name, amps, scales):
    from centerfusiondetect3d_amd import ops, packing
    G, B, H, W, Ci, form, _ = R.GROUPED_CONV_CASES[name]
    gs = R.grouped_conv_inputs(R.GROUPED_CONV_CASES[name], amps, _seed(name))
    pcs = [packing.pack_conv_f16(w, b, [packing.Source(Ci, Ci)]).to(dev) for _, w, b in gs]
    xs = [nhwc(x).to(dev) for x, _, _ in gs]
    out = torch.full((G, B, H, W, 32), NAN, device=dev)
    blocks = [ops.conv_args(pc, [x], [Ci], B, H, W, out[g], 32, 0, None, 0, 0, None, 0, False, in_scale=scales[g])
              for g, (pc, x) in enumerate(zip(pcs, xs))]
    got = ops.conv3x3_grouped_form(blocks)
    assert {k: got[k] for k in form} == form, got                     # the form the table claims, scales and all
    ops.conv3x3_f16x3_grouped(pcs, xs, out=out, in_scales=scales)
    assert bool(torch.isnan(out[..., 27:]).all())
    return [out[g, ..., :27] for g in range(G)]


def _dcn_operands(dev, inputs):
    from centerfusiondetect3d_amd import packing
    x, off, ml, w, b = inputs
    return packing.pack_dcn_f16(w, b).to(dev), nhwc(x).to(dev), R.offmask32(off, ml).to(dev)


def _launch_grouped_dcn(dev, name, amps, scales, act=R.ACT_RELU):
    from centerfusiondetect3d_amd import _lib, ops
    case = R.GROUPED_DCN_CASES[name]
    G, B, H, W, Ci, Co, mag, shared, k_split, _ = case
    gs = R.grouped_dcn_inputs(case, amps, _seed(name))
    trip = [_dcn_operands(dev, g) for g in gs]
    xs = [t[1] for t in trip]
    for a, b in shared:
        xs[b] = xs[a]                                                # two groups on ONE input pointer
        assert scales[a] == scales[b]
    if k_split:
        assert _lib.load().cf_dcn_v2_workspace_bytes(B, H, W, Ci, trip[0][0].n_pad) > 0        # the K split + reduction really run
    om = torch.stack([t[2] for t in trip], 0)
    out = ops.dcn_v2_f16x3_grouped([t[0] for t in trip], xs, om, act=act, k_split=k_split, in_scales=scales)
    return [out[g] for g in range(G)]


def _launch_dcn(dev, name, amp, scale, act=R.ACT_RELU, want_split=False):
    """-> [out] or, want_split: [out, the launch without a workspace, its split-bf16 second output (as float)]"""
    from centerfusiondetect3d_amd import _lib, ops
    B, Ci, Co, H, W, mag, form = R.DCN_CASES[name]
    pd, xd, om = _dcn_operands(dev, R.dcn_inputs(B, Ci, Co, H, W, mag, amp, _seed(name)))
    if form == "dcn:k_split_reduce":
        assert _lib.load().cf_dcn_v2_workspace_bytes(B, H, W, Ci, pd.n_pad) > 0
    outs = [ops.dcn_v2_fused(pd, xd, om, act=act, in_scale=scale)]
    if want_split:
        split = torch.full((B, H, W, 2, Co), NAN, device=dev, dtype=torch.bfloat16)
        out2 = torch.full((B, H, W, Co), NAN, device=dev)
        ops.run_dcn(ops.dcn_args(pd, xd, om, 32, B, H, W, out2, Co, act=act, out_split=split, in_scale=scale))
        assert torch.equal(split, ops.split_bf16(out2))
        outs += [out2, split.float()]
    return outs


def _launch_stem(dev, kind, name, amp, scales):
    """-> [level1 map, its 2x2 max-pool]"""
    from centerfusiondetect3d_amd import ops, packing
    if kind == "stem":
        B, Cc, H, W, _ = R.STEM_CASES[name]
        x, pc, w = R.stem_inputs(B, Cc, H, W, amp, seed=_seed(name))
        ps = packing.pack_stem(*w).to(dev)
    else:
        B, H, W, _ = R.EARLY_CASES[name]
        x, pc, w = R.stem_inputs(B, 3, H, W, amp, early=True, seed=_seed(name))
        ps = packing.pack_stem_early(*w).to(dev)
    pool = torch.full((B, H // 4, W // 4, 32), NAN, device=dev)
    if kind == "stem":
        out = ops.stem_fused(ps, x.to(dev), out_pool=pool, in_scales=scales)
    else:
        out = ops.stem_fused_early(ps, x.to(dev), pc.to(dev), out_pool=pool, in_scales=scales)
    return [out, pool]


def _assert_scaled(base, got, f, what):
    assert len(base) == len(got)
    for i, (a, b) in enumerate(zip(base, got)):
        nan_a, nan_b = torch.isnan(a), torch.isnan(b)
        if bool(nan_a.any()) or bool(nan_b.any()):                   # an output the launch does not write (x2 of a fused Root)
            assert bool(nan_a.all()) and bool(nan_b.all()), (what, i)
            continue
        assert bool((a != 0).any()), (what, i)
        assert torch.equal(b, a * f), (what, i, float((b - a * f).abs().max() / (a * f).abs().max()))


def _invariance(launch, what, form):
    """launch(amp, scale) at k = 0 and at every k of R.KS"""
    base = launch(1.0, 16.0)
    for k in R.KS:
        _assert_scaled(base, launch(2.0 ** k, 16.0 * 2.0 ** -k), 2.0 ** k, (what, k))
    print(f"[f16x3 range] form {form} reached: scale-invariant at k = {R.KS}")


# ------------------------------------------------------------------------------------------------ A. scale invariance
@pytest.mark.parametrize("name", list(R.CONV_CASES))
def test_scale_invariance_conv(dev, name):
    """cf_conv2d_f16x3 (slot kernel) and cf_conv3x3_f16x3 (LDS patch, stride 1 and 2) at the smallest rows that reach each form."""
    _invariance(lambda amp, s: _launch_conv(dev, name, amp, s), name, R.CONV_CASES[name]["form"])


def test_scale_invariance_root_concat(dev):
    _invariance(lambda amp, s: _launch_root_concat(dev, amp, s), "root_concat", R.ROOT_CONCAT_CASE["form"])


@pytest.mark.parametrize("name", list(R.ROOT_CASES))
def test_scale_invariance_root(dev, name):
    """cf_conv3x3_root_f16x3, conv2's and the Root's pre-scale moving together; x2 stays on the chip in the fused forms (its
    buffer keeps the NaN fill), the fallback writes it - scaled like everything else."""
    fused = R.ROOT_CASES[name][-1] != "root:two_launches"
    base = _launch_root(dev, name, 1.0, (16.0, 16.0))
    assert bool(torch.isnan(base[1]).all()) == fused
    for k in R.KS:
        _assert_scaled(base, _launch_root(dev, name, 2.0 ** k, (16.0 * 2.0 ** -k,) * 2), 2.0 ** k, (name, k))
    print(f"[f16x3 range] form {R.ROOT_CASES[name][-1]} reached: scale-invariant at k = {R.KS}")


@pytest.mark.parametrize("k", R.ROOT_ONLY_KS)
def test_root_scale_alone(dev, k):
    """Only the Root's pre-scale moves: x1 and the children times 2^k, t / conv2's bias / conv2's pre-scale as they were, so x2
    keeps its magnitude and the two pre-scales of the launch differ.  The fused launch must give the bits of the two
    launches called with the same two scales (a kernel that split x2 or x1 by conv2's scale would not)."""
    from centerfusiondetect3d_amd import ops
    name = R.ROOT_SCALE_ONLY_CASE
    _, B, H, W, _, _ = R.ROOT_CASES[name]
    pc2, pcr, td, x1d, chd = _root_operands(dev, name, 1.0, 2.0 ** k)
    sr = 16.0 * 2.0 ** -k
    x2 = torch.full(tuple(td.shape), NAN, device=dev)
    out, _ = ops.conv3x3_root_f16x3(pc2, pcr, td, x1d, chd, x2_out=x2, in_scale=16.0, root_in_scale=sr)
    assert bool(torch.isnan(x2).all())                               # the fused form ran
    x2_two = ops.conv2d_f16x3(pc2, [td], B, H, W, act=1, residual=x1d, in_scale=16.0)
    out_two = ops.conv2d_f16x3(pcr, [x2_two, x1d, *chd], B, H, W, act=1, in_scale=sr)
    assert torch.equal(out, out_two) and bool((out != 0).any())
    wrong = ops.conv2d_f16x3(pcr, [x2_two, x1d, *chd], B, H, W, act=1, in_scale=16.0)
    assert not torch.equal(out, wrong)                               # (the comparison can tell the two scales apart)
    print(f"[f16x3 range] form {R.ROOT_SCALE_ONLY_FORM} reached at k = {k}")


@pytest.mark.parametrize("name", list(R.PROJ_CASES))
def test_scale_invariance_proj(dev, name):
    """cf_conv3x3_proj_f16x3: ONE pre-scale for the 3x3 operand and the pooled one; both biases are scaled."""
    _invariance(lambda amp, s: _launch_proj(dev, name, amp, s), name, R.PROJ_CASES[name][-1])


@pytest.mark.parametrize("name", list(R.GROUPED_CONV_CASES))
def test_scale_invariance_grouped_conv(dev, name):
    """cf_conv3x3_f16x3_grouped with a different k per group: each group must read ITS block's pre-scale."""
    G = R.GROUPED_CONV_CASES[name][0]
    ks = R.GROUP_KS[G]
    base = _launch_grouped_conv(dev, name, [1.0] * G, [16.0] * G)
    got = _launch_grouped_conv(dev, name, [2.0 ** k for k in ks], [16.0 * 2.0 ** -k for k in ks])
    for g, k in enumerate(ks):
        _assert_scaled([base[g]], [got[g]], 2.0 ** k, (name, g, k))
    print(f"[f16x3 range] form {R.GROUPED_CONV_CASES[name][-1]} reached: scale-invariant at per-group k = {ks}")


@pytest.mark.parametrize("name", list(R.GROUPED_DCN_CASES))
def test_scale_invariance_grouped_dcn(dev, name):
    """cf_dcn_v2_f16x3_grouped, a different k per group, through the K split and its one reduction over all groups' rows (each
    with its own bias and out_scale) and without a workspace."""
    G = R.GROUPED_DCN_CASES[name][0]
    ks = R.GROUP_KS[G]
    base = _launch_grouped_dcn(dev, name, [1.0] * G, [16.0] * G)
    got = _launch_grouped_dcn(dev, name, [2.0 ** k for k in ks], [16.0 * 2.0 ** -k for k in ks])
    for g, k in enumerate(ks):
        _assert_scaled([base[g]], [got[g]], 2.0 ** k, (name, g, k))
    print(f"[f16x3 range] form {R.GROUPED_DCN_CASES[name][-1]} reached: scale-invariant at per-group k = {ks}")


@pytest.mark.parametrize("name", list(R.DCN_CASES))
def test_scale_invariance_dcn(dev, name):
    """cf_dcn_v2_f16x3 with the K split + reduction where the map has one, without a workspace, and the split-bf16 second output."""
    _invariance(lambda amp, s: _launch_dcn(dev, name, amp, s, want_split=True), name, R.DCN_CASES[name][-1])


@pytest.mark.parametrize("kind,name", [("stem", n) for n in R.STEM_CASES] + [("early", n) for n in R.EARLY_CASES])
def test_scale_invariance_stem(dev, kind, name):
    """cf_stem_fused / cf_stem_fused_early: image (and radar planes), the three biases and the three pre-scales move together;
    both outputs (the level1 map and its 2x2 max-pool) are checked."""
    form = (R.STEM_CASES if kind == "stem" else R.EARLY_CASES)[name][-1]
    _invariance(lambda amp, s: _launch_stem(dev, kind, name, amp, [s] * 3), name, form)


# ------------------------------------------------------------------------------------------------ B. small inputs against float64
def _launch_small(dev, kind, name, amp, scales):
    """-> list of NCHW float64 CPU maps, in the order of R.small_case(...)['ref']"""
    if kind == "conv":
        outs = _launch_conv(dev, name, amp, scales[0])
    elif kind == "root":
        outs = _launch_root(dev, name, amp, scales)[:1]
    elif kind == "proj":
        outs = _launch_proj(dev, name, amp, scales[0])
    elif kind == "gconv":
        outs = _launch_grouped_conv(dev, name, [amp] * len(scales), scales)
    elif kind == "gdcn":
        outs = _launch_grouped_dcn(dev, name, [amp] * len(scales), scales, act=R.ACT_NONE)
    elif kind == "dcn":
        outs = _launch_dcn(dev, name, amp, scales[0], act=R.ACT_NONE)
    else:
        outs = _launch_stem(dev, kind, name, amp, scales)[:1]
    return [nchw(o).cpu().double() for o in outs]


@pytest.mark.parametrize("amp", R.AMPS, ids=lambda a: f"amp{a:g}")
@pytest.mark.parametrize("kind,name", R.SMALL_CASES)
def test_small_inputs_against_float64(dev, kind, name, amp):
    from centerfusiondetect3d_amd import ops
    e = R.small_case(kind, name, amp)
    scales = [ops.in_scale_for(a) for a in e["absmax"]]
    assert scales == e["in_scales"] and all((s == 16.0) == (amp == 1.0) for s in scales), scales
    got = _launch_small(dev, kind, name, amp, scales)
    rel = max(R.relerr(g, r) for g, r in zip(got, e["ref"]))
    per_ch = max(R.relerr_per_channel(g, r) for g, r in zip(got, e["ref"]))
    print(f"[f16x3 small] {name} amp {amp:g} in_scale {scales}: relerr {rel:.2e} (gate {e['tol']:g}; torch fp32 {e['torch_rel']:.2e}, "
          f"split model {e['model_rel']:.2e}); per channel {per_ch:.2e} (gate {e['gate_ch']:.2e} = 2 x max(torch fp32 {e['torch_ch']:.2e}, "
          f"split model {e['model_ch']:.2e}))")
    assert e["gate_ch"] <= e["ceiling"]
    hazard = None
    if amp == R.HAZARD_AMP:
        bad = _launch_small(dev, kind, name, amp, [16.0] * len(scales))
        hazard = max(R.relerr(g, r) for g, r in zip(bad, e["ref"]))
        print(f"[f16x3 small] {name} amp {amp:g} at the default pre-scale 16: relerr {hazard:.2e} (split model {e['default_rel']:.2e})")
    assert rel < e["tol"], rel
    assert per_ch <= e["gate_ch"], (per_ch, e["gate_ch"])
    if hazard is not None:
        assert hazard > e["tol"], hazard                             # the hazard is real: the default scale misses the gate
