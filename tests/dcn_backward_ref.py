"""Cases and CPU yardsticks of the deform_conv2d backward tests (tests/test_gpu_deform_conv2d_backward.py), shared with
tools/dcn_backward_oracle_error.py, which measures the fp32 oracle's own error on them: the constructed inputs, autograd through
oracle/dcn_ref.deform_conv2d in a chosen dtype, and the reference's DeformConv call sequence as a graph over any operator.
No GPU, no library."""
import torch
import torch.nn.functional as F

from oracle import dcn_ref

S, P, D = (1, 1), (1, 1), (1, 1)
NAMES = ("gx", "goffset", "gw", "gbias", "gmask")

# (B, Cin, Cout, H, W, offset scale, with mask)
CASES = [(1, 32, 27, 5, 7, 1.0, True),       # one chunk, N not a multiple of anything
         (2, 64, 64, 9, 13, 2.0, True),      # two chunks, odd map
         (2, 32, 64, 17, 21, 8.0, True),     # samples far outside every border, partial tiles in both directions
         (1, 128, 32, 8, 40, 3.0, True),     # wide row, four chunks
         (2, 64, 64, 9, 13, 2.0, False),     # mask=None: its gradient is None, the others as for a mask of ones
         (1, 160, 192, 6, 9, 2.0, True),     # five chunks (a wave of the data kernel takes two), two groups of output tiles (the second partial)
         # ---- the launch-size branches of csrc/cf_dcn_bwd.hip (NEW_CASES below; the geometry each one is there for is asserted, not
         # claimed: SLAB_GEOMETRY, tests/test_dcn_backward_cpu.py) ----
         (1, 512, 256, 7, 9, 2.0, True),     # 16 chunks, four per wave; N = 256: dynamic LDS at its 32768-byte floor, two full output groups; partial 32-pixel tile
         (1, 512, 256, 35, 53, 2.0, True),   # smallest map on which the slab cap binds for 512 -> 256; odd slab length rounded up, short last slab
         (1, 512, 256, 61, 89, 2.0, True),   # that layer's training slab length: about 800 pixels summed in one accumulator chain
         (1, 64, 64, 116, 250, 2.0, True),   # the 64 -> 64 cap: 113 slabs through the reduce kernel, M just above 113 * 256
         (1, 256, 128, 6, 11, 3.0, True),    # channel pair of the network
         (2, 128, 128, 5, 9, 2.0, False),    # channel pair of the network, mask=None
         (1, 256, 64, 9, 7, 30.0, True),     # channel pair of the network, offsets far outside
         (1, 64, 320, 5, 6, 2.0, True),      # N > 256: the data kernel's LDS limit raised above 64 KB; three output groups, the last half full
         (1, 32, 1024, 3, 5, 2.0, True)]     # the largest N the entry points accept: 156,672 B of LDS
NEW_CASES = range(6, len(CASES))             # their gates come from the fp32 oracle at test time (case_gates of the GPU test)
EPS = 1e-3

# (slabs, cap, pixels per slab, pixels of the last slab) of the weight gradient, per case index: what slab_geometry() must give
SLAB_GEOMETRY = {6: (1, 7, 64, 63), 7: (7, 7, 266, 259), 8: (7, 7, 776, 773), 9: (113, 113, 258, 104), 10: (1, 28, 66, 66),
                 11: (1, 56, 90, 90), 12: (1, 28, 64, 63), 13: (1, 37, 30, 30), 14: (1, 28, 16, 15)}


# ---- the launch geometry of csrc/cf_dcn_bwd.hip, restated (bwd_tiles_per_wave, bwd_slabs, the slab length of
# cf_dcn_v2_bwd_weight, the LDS of cf_dcn_v2_bwd_data); tests/test_dcn_backward_cpu.py holds the slab count against the library's ----
def tiles_per_wave(N):
    return 1 if N <= 32 else 2 if N <= 64 else 4


def slab_geometry(M, C, N):
    """-> (slabs, cap, slab_px, pixels of the last slab) for M = B*H*W pixels, C input and N output channels"""
    nt = tiles_per_wave(N)
    per_slab = 9 * (C // 32) * ((N + 32 * nt - 1) // (32 * nt))
    cap = max(2048 // per_slab, 1)
    slabs = max(min((M + 255) // 256, cap), 1)
    slab_px = (M + slabs - 1) // slabs
    slab_px += slab_px & 1
    return slabs, cap, slab_px, M - (slabs - 1) * slab_px


def data_kernel_geometry(C, N):
    """-> (chunks per wave, dynamic LDS bytes, static + dynamic LDS bytes) of the data kernel"""
    chunks, waves = C // 32, min(C // 32, 4)
    dyn = (N + 1) // 2 * 256
    return (chunks + waves - 1) // waves, dyn, 9 * 32 * 2 * 16 + 4 * 32 * 32 * 4 + dyn


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def tap_grid(H, W, dtype):
    """(18, H, W): the undisplaced sampling coordinate of every offset channel (2k: row y - 1 + i, 2k + 1: column x - 1 + j)."""
    ys = torch.arange(H, dtype=dtype).view(H, 1).expand(H, W)
    xs = torch.arange(W, dtype=dtype).view(1, W).expand(H, W)
    return torch.stack([(ys - 1 + k // 3) if c == 0 else (xs - 1 + k % 3) for k in range(9) for c in (0, 1)])


def integer_distance(off, H, W, dtype):
    pos = tap_grid(H, W, dtype) + off.to(dtype)
    return (pos - torch.round(pos)).abs().min()


def constructed_offsets(B, H, W, scale, seed):
    """randn * scale, every sampling coordinate at least 1e-3 from an integer (moved in float64, then rounded to fp32)."""
    base = tap_grid(H, W, torch.float64)
    pos = base + rnd(B, 18, H, W, seed=seed, scale=scale).double()
    fl = torch.floor(pos)
    fr = pos - fl
    fr = torch.where(fr < EPS, torch.full_like(fr, EPS), fr)
    fr = torch.where(fr > 1 - EPS, torch.full_like(fr, 1 - EPS), fr)
    off = (fl + fr - base).float()
    for dt in (torch.float32, torch.float64):       # none is left near an integer, as fp32 and as float64 arithmetic see them
        assert float(integer_distance(off, H, W, dt)) >= EPS - 1e-5
    return off


def make_case(i):
    B, Ci, Co, H, W, scale, with_mask = CASES[i]
    x = rnd(B, Ci, H, W, seed=11 + i)
    off = constructed_offsets(B, H, W, scale, seed=23 + i)
    mask = torch.sigmoid(rnd(B, 9, H, W, seed=37 + i)) if with_mask else None
    w, b = rnd(Co, Ci, 3, 3, seed=41 + i, scale=(Ci * 9) ** -0.5), rnd(Co, seed=53 + i)
    R = rnd(B, Co, H, W, seed=67 + i)
    return x, off, w, b, mask, R


def oracle_grads(x, off, w, b, mask, R, dtype=torch.float64):
    """gradients of (oracle(x, off, w, b, mask) * R).sum() on the CPU in `dtype`, keyed as NAMES (gmask None without a mask)"""
    leaves = [None if t is None else t.detach().to(dtype).requires_grad_(True) for t in (x, off, w, b, mask)]
    out = dcn_ref.deform_conv2d(leaves[0], leaves[1], leaves[2], leaves[3], S, P, D, leaves[4])
    (out * R.to(dtype)).sum().backward()
    return {n: (None if t is None else t.grad) for n, t in zip(NAMES, leaves)}


def relerr(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


BASE_GATE, CEILING = 5e-6, 1.25e-5


def case_gate(e32):
    """the gate of one gradient of one of NEW_CASES from the fp32 oracle's own error on it: the project's 5e-6 while that error is
    below half of it, otherwise twice the error (the kernel's summation order is one more fp32 order, nothing else); above the
    ceiling the case measures nothing and is refused"""
    assert e32 <= CEILING, f"fp32 oracle error {e32:.2e} above {CEILING:.2e}: the case is unusable"
    return BASE_GATE if e32 < BASE_GATE / 2 else 2 * e32


# ---- the reference's DeformConv call sequence (dla.py:456-472) with a loss behind it ----
SEQ_SHAPE = (1, 32, 32, 12, 16)              # B, Cin, Cout, H, W
SEQ_NAMES = ("com_w", "com_b", "w", "b", "x")


def sequence_inputs():
    B, Ci, Co, H, W = SEQ_SHAPE
    x = rnd(B, Ci, H, W, seed=1)
    com_w, com_b = rnd(27, Ci, 3, 3, seed=2, scale=0.02), rnd(27, seed=3)
    w, b = rnd(Co, Ci, 3, 3, seed=4, scale=1 / 17), rnd(Co, seed=5)
    g = torch.Generator().manual_seed(8)
    bn = (torch.rand(Co, generator=g) + 0.5, rnd(Co, seed=6, scale=0.1), rnd(Co, seed=7, scale=0.1),
          torch.rand(Co, generator=g) + 0.5)
    R = rnd(B, Co, H, W, seed=9)
    return (com_w, com_b, w, b, x), bn, R


def sequence_grads(op, dv, dt):
    """conv_offset_mask -> chunk -> cat -> sigmoid -> op -> BN -> ReLU -> (. * R).sum(), backward to SEQ_NAMES; also the offsets
    and the ReLU's input, for the caller to see how far the graph stays from its kinks"""
    params, bn, R = sequence_inputs()
    t = lambda v: v.to(device=dv, dtype=dt)
    leaves = [t(v).detach().clone().requires_grad_(True) for v in params]
    cw, cb, ww, bb, xx = leaves
    offset_mask = F.conv2d(xx, cw, cb, stride=(1, 1), padding=(1, 1))
    offset1, offset2, mask = torch.chunk(offset_mask, 3, dim=1)
    offset = torch.cat((offset1, offset2), dim=1)
    mask = torch.sigmoid(mask)
    y = op(input=xx, offset=offset, weight=ww, bias=bb, stride=(1, 1), padding=(1, 1), dilation=(1, 1), mask=mask)
    z = F.batch_norm(y, t(bn[2]), t(bn[3]), t(bn[0]), t(bn[1]), False, 0.1, 1e-5)
    (F.relu(z) * t(R)).sum().backward()
    return [v.grad for v in leaves], offset.detach(), z.detach()
