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
         (1, 160, 192, 6, 9, 2.0, True)]     # five chunks (a wave of the data kernel takes two), two groups of output tiles (the second partial)
EPS = 1e-3


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
