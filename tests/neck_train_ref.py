"""Cases and CPU yardsticks of the neck-training tests (tests/test_neck_train_cpu.py, tests/test_gpu_neck_ops.py): the graphs of
ops.deform_conv_block / ops.upsample_dw_add and of their parts as torch autograd over F.conv2d, oracle.dcn_ref.deform_conv2d,
F.batch_norm, F.relu and F.conv_transpose2d in a chosen dtype, and the launch geometry of csrc/cf_neck_bwd.hip, restated.
Loss = (output * R).sum() with a fixed random R everywhere.  No GPU, no library."""
import functools

import torch
import torch.nn.functional as F

from oracle import dcn_ref
from tests.dcn_backward_ref import integer_distance, relerr, rnd  # noqa: F401  (re-exported)

KINK = 1e-5                      # distance every sampling coordinate and every ReLU input keeps from its kink, in float64
MOMENTUM, EPS = 0.1, 1e-5

# ---- offset convolution backward alone: (B, C, H, W) ----
CONV_CASES = [(1, 32, 1, 1), (1, 32, 3, 5), (2, 64, 9, 13), (1, 512, 7, 9), (1, 256, 14, 25), (1, 64, 116, 250),
              # ---- one per branch of the launch geometry (CONV_GEOMETRY below; asserted in tests/test_neck_train_cpu.py) ----
              (1, 512, 35, 53),      # eight slabs of 512 channels, odd slab length rounded up, short last slab
              (1, 160, 5, 7),        # five chunks: a wave of the data kernel takes two; partial 32-pixel tile
              (1, 512, 121, 119)]    # the slab cap binds (56 slabs for 512 channels, one fewer than 256-pixel ones), short last slab
# (slabs, cap, pixels per slab, pixels of the last slab, waves of the data kernel, chunks per wave)
CONV_GEOMETRY = {0: (1, 910, 2, 1, 1, 1), 1: (1, 910, 16, 15, 1, 1), 2: (1, 455, 234, 234, 2, 1), 3: (1, 56, 64, 63, 4, 4),
                 4: (2, 113, 176, 174, 4, 2), 5: (114, 455, 256, 72, 2, 1), 6: (8, 56, 232, 231, 4, 4), 7: (1, 182, 36, 35, 4, 2),
                 8: (56, 56, 258, 209, 4, 4)}

# ---- batch norm + ReLU: (B, C, H, W) ----
BN_CASES = [(2, 64, 3, 5), (2, 64, 9, 13), (1, 128, 17, 21), (2, 256, 7, 9), (1, 64, 61, 89)]
BN_COND_CASE = (2, 64, 9, 13)    # input mean 100, std 0.1: catches a single-pass variance
# (slabs, rows per slab, rows per trip of a workgroup)
BN_GEOMETRY = {0: (1, 30, 16), 1: (2, 117, 16), 2: (3, 119, 8), 3: (1, 126, 4), 4: (43, 127, 16)}

# ---- upsample backward: (B, C, H, W, f) ----
UP_CASES = [(1, 64, 1, 1, 2), (2, 64, 3, 5, 2), (1, 128, 7, 9, 4), (1, 256, 14, 25, 2), (2, 64, 28, 50, 4)]
UP_GEOMETRY = {0: (1, 1, 16), 1: (1, 30, 16), 2: (1, 63, 8), 3: (3, 117, 4), 4: (22, 128, 16)}

# ---- the block: (B, Cin, Cout, H, W) ----
BLOCK_CASES = [(1, 32, 32, 12, 16), (2, 64, 64, 9, 13), (1, 128, 64, 7, 9), (1, 512, 256, 3, 5), (2, 256, 128, 5, 7)]
BLOCK_NAMES = ("x", "com_w", "com_b", "w", "b", "bn_w", "bn_b")
BLOCK_GATE = 1e-5                # SEQ_GATE of tests/test_gpu_deform_conv2d_backward.py: this very graph


# ---- the launch geometry of csrc/cf_neck_bwd.hip, restated ----
def conv_slabs(M, C):
    """cw_slabs and the slab length of cf_conv3x3_bwd_weight -> (slabs, cap, slab_px, pixels of the last slab)"""
    cap = max(8192 // (9 * (C // 32)), 1)
    slabs = max(min((M + 255) // 256, cap), 1)
    slab_px = (M + slabs - 1) // slabs
    slab_px += slab_px & 1
    return slabs, cap, slab_px, M - (slabs - 1) * slab_px


def conv_geometry(M, C):
    waves = min(C // 32, 4)
    return conv_slabs(M, C) + (waves, (C // 32 + waves - 1) // waves)


def conv_workspace_bytes(M, C):
    return conv_slabs(M, C)[0] * (9 * 27 * C + 27) * 4


def red_slabs(M, C):
    """red_slabs / row_split -> (slabs, rows per slab, rows a workgroup of 256 threads takes per trip)"""
    s0 = max(min((M + 127) // 128, 256), 1)
    rows = (M + s0 - 1) // s0
    return (M + rows - 1) // rows, rows, 256 // (C // 4)


def bn_workspace_bytes(M, C):
    return (red_slabs(M, C)[0] * 3 + 2) * C * 4


def up_workspace_bytes(B, H, W, C, f):
    return red_slabs(B * H * W, C)[0] * 4 * f * f * C * 4


# ---- graphs ----
def _leaves(ts, dt):
    return [t.detach().to(dt).clone().requires_grad_(True) for t in ts]


def conv_inputs(i):
    B, C, H, W = CONV_CASES[i]
    x = rnd(B, C, H, W, seed=101 + i)
    cw, cb = rnd(27, C, 3, 3, seed=103 + i, scale=1.0 / (9 * C) ** 0.5), rnd(27, seed=107 + i)
    G = rnd(B, 27, H, W, seed=109 + i)
    return x, cw, cb, G


def conv_graph(inputs, dt):
    """conv_offset_mask -> (offsets, sigmoid(mask logits)); loss = sum of both times G.  -> (grads {gx, gw, gbias}, offmask (B,27,H,W)
    with the mask activated): the fold m (1 - m) is sigmoid's autograd here."""
    x, cw, cb, G = inputs
    lx, lw, lb = _leaves((x, cw, cb), dt)
    om = F.conv2d(lx, lw, lb, stride=1, padding=1)
    act = torch.cat((om[:, :18], torch.sigmoid(om[:, 18:])), dim=1)
    (act * G.to(dt)).sum().backward()
    return {"gx": lx.grad, "gw": lw.grad, "gbias": lb.grad}, act.detach()


def _margin_seed(make, margin_of, tries=400):
    """the first seed whose float64 graph keeps `KINK` from every kink"""
    for seed in range(tries):
        if margin_of(make(seed)) >= KINK:
            return seed
    raise AssertionError("no seed keeps the graph away from its kinks")


def _bn_make(shape, seed, mean=0.0, std=1.0):
    B, C, H, W = shape
    x = rnd(B, C, H, W, seed=seed) * std + mean
    g = torch.Generator().manual_seed(1000 + seed)
    gamma, var = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5
    beta, rm = rnd(C, seed=2000 + seed, scale=0.3), rnd(C, seed=3000 + seed, scale=0.1) + mean
    R = rnd(B, C, H, W, seed=4000 + seed)
    return x, gamma, beta, rm, var, R


def bn_graph(inputs, dt, training=True):
    """-> (dict y, gx, ggamma, gbeta, running_mean, running_var; min |ReLU input|)"""
    x, gamma, beta, rm, rv, R = inputs
    lx, lg, lb = _leaves((x, gamma, beta), dt)
    rm, rv = rm.to(dt).clone(), rv.to(dt).clone()
    z = F.batch_norm(lx, rm, rv, lg, lb, training, MOMENTUM, EPS)
    y = F.relu(z)
    (y * R.to(dt)).sum().backward()
    return {"y": y.detach(), "gx": lx.grad, "ggamma": lg.grad, "gbeta": lb.grad, "running_mean": rm, "running_var": rv}, \
        float(z.detach().abs().min())


@functools.lru_cache(maxsize=None)
def bn_inputs(i, cond=False, training=True):
    shape = BN_COND_CASE if cond else BN_CASES[i]
    kw = dict(mean=100.0, std=0.1) if cond else {}
    make = lambda seed: _bn_make(shape, 7 * seed + (50 if cond else i), **kw)
    return make(_margin_seed(make, lambda inp: bn_graph(inp, torch.float64, training)[1]))


def up_inputs(i):
    B, C, H, W, f = UP_CASES[i]
    return (rnd(B, C, H, W, seed=201 + i), rnd(C, 1, 2 * f, 2 * f, seed=203 + i, scale=0.5), rnd(B, C, H * f, W * f, seed=207 + i),
            rnd(B, C, H * f, W * f, seed=209 + i))


def up_graph(inputs, f, dt):
    x, w, skip, R = inputs
    lx, lw, ls = _leaves((x, w, skip), dt)
    out = F.conv_transpose2d(lx, lw, stride=f, padding=f // 2, groups=x.shape[1]) + ls
    (out * R.to(dt)).sum().backward()
    return {"out": out.detach(), "gx": lx.grad, "gw": lw.grad, "gskip": ls.grad}


def block_params(Ci, Co, seed):
    """(com_w, com_b, w, b, bn_w, bn_b, running_mean, running_var) of one DeformConv; the offsets the convolution produces spread
    by about 0.35 around its bias"""
    g = torch.Generator().manual_seed(500 + seed)
    return (rnd(27, Ci, 3, 3, seed=seed + 1, scale=0.35 / (9 * Ci) ** 0.5), rnd(27, seed=seed + 2),
            rnd(Co, Ci, 3, 3, seed=seed + 3, scale=1.0 / (9 * Ci) ** 0.5), rnd(Co, seed=seed + 4),
            torch.rand(Co, generator=g) + 0.5, rnd(Co, seed=seed + 5, scale=0.3), rnd(Co, seed=seed + 6, scale=0.1),
            torch.rand(Co, generator=g) + 0.5)


def block_forward(x, params, dt, training=True, stats=None):
    """the reference's DeformConv.forward (dla.py:456-472) on leaves -> (y, offset, pre-ReLU map); `stats`: the running statistics
    to update (default: copies)"""
    cw, cb, w, b, gamma, beta = params[:6]
    rm, rv = stats if stats is not None else (params[6].to(dt).clone(), params[7].to(dt).clone())
    offset_mask = F.conv2d(x, cw, cb, stride=(1, 1), padding=(1, 1))
    offset1, offset2, mask = torch.chunk(offset_mask, 3, dim=1)
    offset = torch.cat((offset1, offset2), dim=1)
    mask = torch.sigmoid(mask)
    t = dcn_ref.deform_conv2d(x, offset, w, b, (1, 1), (1, 1), (1, 1), mask)
    z = F.batch_norm(t, rm, rv, gamma, beta, training, MOMENTUM, EPS)
    return F.relu(z), offset, z


def _block_make(shape, seed):
    B, Ci, Co, H, W = shape
    return (rnd(B, Ci, H, W, seed=seed + 11), block_params(Ci, Co, seed), rnd(B, Co, H, W, seed=seed + 12))


def block_graph(inputs, dt, training=True):
    """-> (dict y + the seven gradients keyed as BLOCK_NAMES + running statistics, margin to the nearest kink)"""
    x, params, R = inputs
    lx, *lp = _leaves((x, *params[:6]), dt)
    stats = (params[6].to(dt).clone(), params[7].to(dt).clone())
    y, offset, z = block_forward(lx, lp, dt, training, stats)
    (y * R.to(dt)).sum().backward()
    res = {"y": y.detach(), "running_mean": stats[0], "running_var": stats[1]}
    res.update({n: t.grad for n, t in zip(BLOCK_NAMES, [lx, *lp])})
    H, W = x.shape[2:]
    margin = min(float(integer_distance(offset.detach(), H, W, dt)), float(z.detach().abs().min()))
    return res, margin


@functools.lru_cache(maxsize=None)
def block_inputs(i):
    make = lambda seed: _block_make(BLOCK_CASES[i], 100 * seed + i)
    return make(_margin_seed(make, lambda inp: block_graph(inp, torch.float64)[1]))


# ---- one IDA stage: proj 128 -> 64 at 4 x 6, up f = 2, skip 64 at 8 x 12, node 64 -> 64 ----
IDA_NAMES = ("x", "skip", "up_w") + tuple(f"proj.{n}" for n in BLOCK_NAMES[1:]) + tuple(f"node.{n}" for n in BLOCK_NAMES[1:])


def _ida_make(seed):
    return (rnd(2, 128, 4, 6, seed=seed + 21), rnd(2, 64, 8, 12, seed=seed + 22), rnd(64, 1, 4, 4, seed=seed + 23, scale=0.5),
            block_params(128, 64, seed + 30), block_params(64, 64, seed + 40), rnd(2, 64, 8, 12, seed=seed + 24))


def ida_graph(inputs, dt):
    x, skip, up_w, pp, pn, R = inputs
    lx, ls, lu = _leaves((x, skip, up_w), dt)
    lpp, lpn = _leaves(pp[:6], dt), _leaves(pn[:6], dt)
    p, off1, z1 = block_forward(lx, list(lpp) + [pp[6].to(dt), pp[7].to(dt)], dt)
    s = F.conv_transpose2d(p, lu, stride=2, padding=1, groups=64) + ls
    y, off2, z2 = block_forward(s, list(lpn) + [pn[6].to(dt), pn[7].to(dt)], dt)
    (y * R.to(dt)).sum().backward()
    res = {"y": y.detach()}
    res.update({n: t.grad for n, t in zip(IDA_NAMES, [lx, ls, lu, *lpp, *lpn])})
    margin = min(float(integer_distance(off1.detach(), 4, 6, dt)), float(integer_distance(off2.detach(), 8, 12, dt)),
                 float(z1.detach().abs().min()), float(z2.detach().abs().min()))
    return res, margin


@functools.lru_cache(maxsize=None)
def ida_inputs():
    make = lambda seed: _ida_make(1000 * seed)
    return make(_margin_seed(make, lambda inp: ida_graph(inp, torch.float64)[1]))
