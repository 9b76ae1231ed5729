"""Cases and CPU yardsticks of the exact-fp32 operator tests (tests/test_gpu_exact_fp32.py, the two tightened tests of
tests/test_gpu_ops.py) and of tests/test_exact_fp32_cpu.py, which proves from the library that the tables reach every tile
form `cf_conv2d_fused` / `cf_dcn_v2_fused` can launch: the case tables, the seeded inputs, the float64 references and two fp32
yardsticks for convolution - torch's own fp32 `F.conv2d` and the kernels' summation scheme restated.  No GPU."""
import ctypes as C

import torch
import torch.nn.functional as F

from oracle import dcn_ref

ACT_NONE, ACT_RELU, ACT_SIGMOID_CLAMP, ACT_RAW_AND_SIGDEPTH = 0, 1, 2, 3
NHWC, NCHW = 0, 1
KIND_TILE, KIND_N16 = 0, 1
S1 = (1, 1)

GATE_CEILING = 4e-6            # no convolution gate may come out above this,
GATE_CEILING_PRECISE = 1.5e-6  # and a precise one not above the split-fp16 convolution's own gate
DCN_GATE, DCN_ORACLE_LIMIT = 5e-6, 2.5e-6


# ------------------------------------------------------------------------------------------------ the tile rule
def tile_rule(M, N, N_pad, layout, act, precise, dcn):
    """The dispatch rule of cf_gemm.hip restated: -> (kind, bm, bn)"""
    if not dcn and N <= 16 and layout == NHWC and act != ACT_SIGMOID_CLAMP:
        return (KIND_N16, 128, 16)
    bn = 128 if N_pad % 128 == 0 else 64 if N_pad % 64 == 0 else 32
    bm = 128 if -(-M // 128) * (N_pad // bn) >= 512 else 64
    if bm == 64 and bn == 128 and -(-M // 64) * (N_pad // 128) < 512:
        bn = 64
    if (precise or dcn) and bn >= 64:
        bm = 64
    if (bm, bn) not in ((128, 128), (128, 64), (128, 32), (64, 128), (64, 64)):
        bm, bn = 128, 32
    return (KIND_TILE, bm, bn)


def tile_form(lib, M, N, N_pad, layout, act, precise, dcn):
    """What the library says it launches (cf_gemm_tile_form) -> (kind, bm, bn)"""
    k, bm, bn = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    st = lib.cf_gemm_tile_form(M, N, N_pad, layout, act, int(precise), int(dcn), C.byref(k), C.byref(bm), C.byref(bn))
    assert st == 0, lib.cf_last_error()
    return (k.value, bm.value, bn.value)


def n_pad_of(n):
    return (n + 31) // 32 * 32


# ------------------------------------------------------------------------------------------------ the case tables
# convolution: id -> B, Ci, Co, H, W, k, stride, act, residual, layout, precise, the form it is there for
def _c(B, Ci, Co, H, W, k, stride, act, res, layout, precise, form, src4=False, hconv=False):
    return dict(B=B, Ci=Ci, Co=Co, H=H, W=W, k=k, stride=stride, act=act, res=res, layout=layout, precise=precise,
                form=form, src4=src4, hconv=hconv)


T = KIND_TILE
CONV_CASES = {
    "c64x128_precise_res": _c(4, 32, 256, 63, 65, 3, 1, ACT_RELU, True, NHWC, True, (T, 64, 128)),
    "c128x128_plain": _c(8, 32, 256, 63, 65, 3, 1, ACT_RELU, False, NHWC, False, (T, 128, 128)),
    "c64x128_plain": _c(8, 32, 128, 63, 65, 3, 1, ACT_RELU, False, NHWC, False, (T, 64, 128)),
    "c128x64_plain_res_noact": _c(6, 32, 192, 61, 60, 3, 1, ACT_NONE, True, NHWC, False, (T, 128, 64)),
    "c64x64_plain_k4608": _c(1, 512, 64, 7, 13, 3, 1, ACT_RELU, False, NHWC, False, (T, 64, 64)),
    "c64x64_precise_k4608": _c(1, 512, 64, 7, 13, 3, 1, ACT_RELU, False, NHWC, True, (T, 64, 64)),
    "c128x32_plain_stride2": _c(2, 64, 96, 23, 31, 3, 2, ACT_RELU, False, NHWC, False, (T, 128, 32)),
    "head_out_9x7_raw": _c(2, 256, 10, 9, 7, 1, 1, ACT_NONE, False, NCHW, False, (T, 128, 32)),
    "head_out_9x7_sigmoid": _c(2, 256, 10, 9, 7, 1, 1, ACT_SIGMOID_CLAMP, False, NCHW, False, (T, 128, 32)),
    "head_out_9x7_sigdepth": _c(2, 256, 10, 9, 7, 1, 1, ACT_RAW_AND_SIGDEPTH, False, NCHW, False, (T, 128, 32)),
    "head_out_63x65_raw": _c(2, 256, 10, 63, 65, 1, 1, ACT_NONE, False, NCHW, False, (T, 128, 32)),
    "head_out_63x65_sigmoid": _c(2, 256, 10, 63, 65, 1, 1, ACT_SIGMOID_CLAMP, False, NCHW, False, (T, 128, 32)),
    "head_out_63x65_sigdepth": _c(2, 256, 10, 63, 65, 1, 1, ACT_RAW_AND_SIGDEPTH, False, NCHW, False, (T, 128, 32)),
    "n16_3x3": _c(3, 16, 16, 23, 31, 3, 1, ACT_RELU, False, NHWC, False, (KIND_N16, 128, 16)),
    "n16_stem7x7": _c(2, 3, 16, 32, 48, 7, 1, ACT_RELU, False, NHWC, False, (KIND_N16, 128, 16), src4=True),
    # plan.py:_hconv: feat 64 || pc_hm 3 (stored with stride 4), written at column 64 of a 384-wide buffer
    "hconv_two_sources_offset": _c(2, 67, 256, 13, 19, 3, 1, ACT_RELU, False, NHWC, False, (T, 64, 64), hconv=True),
}

# DCN: id -> B, Ci, Co, H, W, offset magnitude, form; each runs with precise on and off
DCN_CASES = {
    "d64x128": (4, 32, 256, 63, 65, 2.0, (T, 64, 128)),
    "d128x32": (2, 32, 96, 13, 19, 3.0, (T, 128, 32)),
    "d64x64_a": (2, 64, 64, 28, 50, 2.0, (T, 64, 64)),
    "d64x64_far": (2, 256, 128, 9, 11, 30.0, (T, 64, 64)),
}
DCN_MASK_ACTIVATED_CASE = "d128x32"

# the shapes of tests/test_gpu_ops.py::test_conv2d_fused / test_dcn_v2_fused (precise, NHWC): their forms count as run
OPS_CONV_SHAPES = [(2, 16, 16, 40, 56, 3, 1, 1, False),     # level0-like, N_pad 32
                   (2, 16, 32, 40, 56, 3, 2, 1, False),     # level1 stride 2
                   (1, 64, 64, 28, 50, 3, 1, 1, True),      # BasicBlock conv2 + residual
                   (2, 128, 256, 14, 25, 3, 2, 1, False),   # 128-wide N tile, stride 2
                   (1, 512, 512, 7, 13, 3, 1, 1, True),     # small M, long K
                   (3, 64, 27, 23, 31, 3, 1, 0, False),     # conv_offset_mask (N=27), ragged M
                   (1, 256, 10, 16, 24, 1, 1, 0, False)]    # head output 1x1
OPS_DCN_SHAPES = [(2, 64, 64, 28, 50, 2.0), (1, 128, 64, 14, 25, 8.0), (1, 512, 256, 7, 13, 1.0), (2, 256, 128, 9, 11, 30.0)]

# the three launches whose frames, run alone (a 64x64 launch), must give the full launch's bits
SHARD_CONV_CASES = ("c128x128_plain", "c64x128_precise_res")
SHARD_DCN_CASE = "d64x128"


def out_hw(H, W, k, stride):
    p = k // 2
    return (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1


def conv_case_key(c):
    """(M, N, N_pad, layout, act, precise, dcn) of a convolution case: the arguments of the tile rule"""
    Ho, Wo = out_hw(c["H"], c["W"], c["k"], c["stride"])
    return (c["B"] * Ho * Wo, c["Co"], n_pad_of(c["Co"]), c["layout"], c["act"], c["precise"], False)


def dcn_case_key(case, precise):
    B, Ci, Co, H, W, mag, form = case
    return (B * H * W, Co, n_pad_of(Co), NHWC, ACT_RELU, precise, True)


def table_forms(form_of):
    """{(dcn, kind, bm, bn, precise)} the tables above reach, `form_of(*key)` being the rule or the library's export"""
    got = set()
    for c in CONV_CASES.values():
        got.add((False,) + form_of(*conv_case_key(c)) + (bool(c["precise"]),))
    for case in DCN_CASES.values():
        for precise in (False, True):
            got.add((True,) + form_of(*dcn_case_key(case, precise)) + (precise,))
    for (B, Ci, Co, H, W, k, stride, act, res) in OPS_CONV_SHAPES:
        Ho, Wo = out_hw(H, W, k, stride)
        got.add((False,) + form_of(B * Ho * Wo, Co, n_pad_of(Co), NHWC, act, True, False) + (True,))
    for (B, Ci, Co, H, W, mag) in OPS_DCN_SHAPES:
        got.add((True,) + form_of(B * H * W, Co, n_pad_of(Co), NHWC, ACT_RELU, True, True) + (True,))
    return got


# ------------------------------------------------------------------------------------------------ inputs
def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def conv_inputs(c):
    """x, w, b, residual (or None): the seeds of test_conv2d_fused"""
    Ho, Wo = out_hw(c["H"], c["W"], c["k"], c["stride"])
    x = rnd(c["B"], c["Ci"], c["H"], c["W"], seed=1)
    w = rnd(c["Co"], c["Ci"], c["k"], c["k"], seed=2, scale=(c["Ci"] * c["k"] * c["k"]) ** -0.5)
    b = rnd(c["Co"], seed=3)
    r = rnd(c["B"], c["Co"], Ho, Wo, seed=6) if c["res"] else None
    return x, w, b, r


def conv_sources(c, x):
    """(packing sources as (channels, stride) pairs, the NHWC source tensors) of a case"""
    if c["hconv"]:
        pch4 = torch.zeros(c["B"], c["H"], c["W"], 4)
        pch4[..., :3] = nhwc(x[:, 64:67])
        return [(64, 64), (3, 4)], [nhwc(x[:, :64]), pch4]
    if c["src4"]:
        x4 = torch.zeros(c["B"], c["H"], c["W"], 4)
        x4[..., :3] = nhwc(x)
        return [(3, 4)], [x4]
    return [(c["Ci"], c["Ci"])], [nhwc(x)]


def dcn_inputs(case):
    """x, offsets (B,18,H,W) = randn * mag, mask logits (B,9,H,W), w, b: the seeds of test_dcn_v2_fused"""
    B, Ci, Co, H, W, mag, _ = case
    om = rnd(B, 27, H, W, seed=2)
    return (rnd(B, Ci, H, W, seed=1), om[:, :18] * mag, om[:, 18:].contiguous(),
            rnd(Co, Ci, 3, 3, seed=3, scale=(Ci * 9) ** -0.5), rnd(Co, seed=4))


def offmask32(off, mask):
    """NHWC (B,H,W,32): offsets in 0..17, mask (logits or factors) in 18..26, the rest zero"""
    B, _, H, W = off.shape
    om = torch.zeros(B, H, W, 32)
    om[..., :18] = nhwc(off)
    om[..., 18:27] = nhwc(mask)
    return om


# ------------------------------------------------------------------------------------------------ references
def apply_act(v, act):
    return F.relu(v) if act == ACT_RELU else v      # (acts 2 and 3 are formed from the raw map by the tests)


def conv_ref(x, w, b, r, stride, act, dtype=torch.float64):
    """F.conv2d + residual + act in `dtype`, NCHW: float64 is the reference, float32 the torch yardstick"""
    t = lambda v: None if v is None else v.to(dtype)
    y = F.conv2d(t(x), t(w), t(b), stride, w.shape[-1] // 2)
    if r is not None:
        y = y + t(r)
    return apply_act(y, act)


def dcn_ref_out(x, off, mask_logits, w, b, dtype=torch.float64):
    t = lambda v: v.to(dtype)
    return dcn_ref.deform_conv2d(t(x), t(off), t(w), t(b), S1, S1, S1, torch.sigmoid(t(mask_logits)))


def relerr(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


def dcn_gate(oracle_errors):
    """The backward tests' rule: 5e-6 while the fp32 oracle's own error stays below 2.5e-6 on every case, else twice its worst"""
    worst = max(oracle_errors)
    return DCN_GATE if worst < DCN_ORACLE_LIMIT else 2.0 * worst


# ------------------------------------------------------------------------------------------------ the summation model
def gather_a(pc, srcs, B, H, W):
    """The A matrix the kernel stages, from the packed slot table: (M, K_pad) fp32, k in slot order (source, tap, channel
    group of 4), zero outside the image and in pad slots.  srcs: NHWC fp32 CPU tensors."""
    Ho, Wo = (H + 2 * pc.pad - pc.kh) // pc.stride + 1, (W + 2 * pc.pad - pc.kh) // pc.stride + 1
    P = pc.kh                                         # a margin that covers every (dy, dx)
    padded = []
    for s in srcs:
        cp = (s.shape[-1] + 3) // 4 * 4
        t = torch.zeros(B, H + 2 * P, W + 2 * P, cp)
        t[:, P:P + H, P:P + W, :s.shape[-1]] = s
        padded.append(t)
    A = torch.zeros(B * Ho * Wo, pc.k_pad)
    st = pc.stride
    for j, (si, dy, dx, c) in enumerate(pc.slots.tolist()):
        if c < 0:
            continue
        v = padded[si][:, P + dy:P + dy + (Ho - 1) * st + 1:st, P + dx:P + dx + (Wo - 1) * st + 1:st, c:c + 4]
        A[:, 4 * j:4 * j + 4] = v.reshape(B * Ho * Wo, 4)
    return A, Ho, Wo


def summation_model(pc, srcs, B, H, W, precise, residual=None, act=ACT_NONE):
    """The kernels' summation scheme in fp32 on the CPU -> NHWC (B,Ho,Wo,N).  Every product is rounded to fp32; plain: the
    products go into ONE running sum in k order (the chain model); precise: each 32-wide chunk is summed on its own from zero
    and then added to the running sum (the blocked model).  Bias, residual and activation follow in the epilogue's order."""
    A, Ho, Wo = gather_a(pc, srcs, B, H, W)
    Wt = pc.weight[:pc.n].t().contiguous()            # (K_pad, N)
    M = A.shape[0]
    acc, part, prod = torch.zeros(M, pc.n), torch.zeros(M, pc.n), torch.empty(M, pc.n)
    live = (Wt != 0).any(dim=1).tolist()              # (a pad column adds +-0: skipped)
    for c0 in range(0, pc.k_pad, 32):
        tgt = part.zero_() if precise else acc
        for k in range(c0, c0 + 32):
            if live[k]:
                torch.mul(A[:, k:k + 1], Wt[k:k + 1], out=prod)
                tgt.add_(prod)
        if precise:
            acc.add_(part)
    v = acc + pc.bias[:pc.n]
    if residual is not None:
        v = v + residual.reshape(M, pc.n)
    return apply_act(v, act).view(B, Ho, Wo, pc.n)


def conv_gate(ref64, torch32, model32):
    """-> (gate, torch fp32 error, summation-model error): twice the larger yardstick error (the kernel's order - two products
    per MFMA step, K in slot order - is a third fp32 order beside them)"""
    e_t, e_m = relerr(torch32, ref64), relerr(model32, ref64)
    return 2.0 * max(e_t, e_m), e_t, e_m
