"""Cases and CPU yardsticks of the base-training tests (tests/test_base_train_cpu.py, tests/test_gpu_base_ops.py,
tests/test_gpu_base_train.py): the graphs of ops.conv_bn_act / ops.max_pool2x2, of their parts and of DLA-34's levels 2-5
(model/networks/dla.py:36-42, 104-118, 144-161, 225-232) as torch autograd over F.conv2d, F.batch_norm, F.relu and F.max_pool2d in
a chosen dtype, and the launch geometry of csrc/cf_base_bwd.hip, restated.  Loss = (output * R).sum() with a fixed random R
everywhere.  Inputs come from seeds chosen as tests/neck_train_ref.py chooses them: every ReLU input stays KINK away from zero in
float64.  No GPU, no library."""
import functools

import torch
import torch.nn.functional as F

from tests.dcn_backward_ref import relerr, rnd  # noqa: F401  (re-exported)
from tests.neck_train_ref import EPS, KINK, MOMENTUM, _leaves, _margin_seed, red_slabs

# ---- convolution backward alone: (B, Cin, Cout, H, W, k, stride) ----
CONV_CASES = [(1, 32, 32, 1, 1, 3, 1), (1, 32, 64, 1, 1, 1, 1),   # one pixel
              (1, 32, 64, 7, 9, 3, 2),                            # odd H and W under stride 2
              (2, 64, 64, 9, 13, 3, 1),                           # M no multiple of the pixel tile, the batch boundary inside a tile
              (1, 64, 128, 8, 12, 3, 2), (1, 256, 512, 4, 6, 3, 2), (1, 512, 512, 3, 5, 3, 1), (1, 128, 64, 5, 7, 1, 1),
              (1, 896, 256, 4, 6, 1, 1),
              (1, 1280, 512, 2, 3, 1, 1),                         # the widest K
              (1, 64, 64, 116, 250, 3, 1),                        # more than one slab (114; the cap, 227, does not bind)
              (1, 512, 512, 25, 31, 3, 1)]                        # the slab cap binds: 3 slabs for 512 -> 512, 256-pixel ones would be 4
# (slabs, cap, pixels per slab, pixels of the last slab) per case
CONV_GEOMETRY = {0: (1, 227, 2, 1), 1: (1, 2048, 2, 1), 2: (1, 227, 20, 20), 3: (1, 227, 234, 234), 4: (1, 113, 24, 24),
                 5: (1, 7, 6, 6), 6: (1, 3, 16, 15), 7: (1, 1024, 36, 35), 8: (1, 36, 24, 24), 9: (1, 12, 6, 6),
                 10: (114, 227, 256, 72), 11: (3, 3, 260, 255)}

# ---- batch norm + [residual] + [ReLU]: (B, C, H, W), every combination of (residual, relu) ----
BN_CASES = [(2, 64, 3, 5), (1, 128, 17, 21), (2, 512, 2, 3)]
BN_MODES = [(False, False), (False, True), (True, False), (True, True)]

# ---- max-pool: (B, C, H, W) ----
POOL_CASES = [(1, 32, 2, 2), (2, 64, 6, 10), (1, 512, 2, 6)]

# ---- the block, one per layer kind: (B, input channels (a tuple: Root's concat), Cout, H, W, k, stride, residual, relu) ----
BLOCK_CASES = {"conv1": (2, (64,), 64, 9, 13, 3, 1, False, True),
               "conv1_stride2": (2, (32,), 64, 9, 13, 3, 2, False, True),
               "conv2_residual": (2, (64,), 64, 9, 13, 3, 1, True, True),
               "project": (2, (64,), 128, 9, 13, 1, 1, False, False),
               "root": (2, (32, 32, 64), 64, 9, 13, 1, 1, False, True)}
BLOCK_GATE = 1e-5                # the neck block's gate (tests/neck_train_ref.py)


# ---- the launch geometry of csrc/cf_base_bwd.hip, restated ----
def out_hw(H, W, k, stride):
    pad = (k - 1) // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def conv_slabs(M, C, N, k):
    """bw_slabs and the slab length of cf_conv_bwd_weight for M output pixels -> (slabs, cap, slab_px, pixels of the last slab)"""
    cap = max(2048 // (k * k * ((C // 32 + 1) // 2) * ((N // 32 + 1) // 2)), 1)
    slabs = max(min((M + 255) // 256, cap), 1)
    slab_px = (M + slabs - 1) // slabs
    slab_px += slab_px & 1
    return slabs, cap, slab_px, M - (slabs - 1) * slab_px


def conv_workspace_bytes(B, H, W, C, N, k, stride):
    ho, wo = out_hw(H, W, k, stride)
    return conv_slabs(B * ho * wo, C, N, k)[0] * k * k * N * C * 4


def bn_workspace_bytes(M, C):
    return (red_slabs(M, C)[0] * 3 + 2) * C * 4


# ---- graphs ----
def conv_inputs(i):
    B, Ci, Co, H, W, k, s = CONV_CASES[i]
    ho, wo = out_hw(H, W, k, s)
    return (rnd(B, Ci, H, W, seed=301 + i), rnd(Co, Ci, k, k, seed=303 + i, scale=1.0 / (k * k * Ci) ** 0.5),
            rnd(B, Co, ho, wo, seed=307 + i))


def conv_graph(inputs, k, stride, dt, mask_odd=False):
    """gradients of (conv(x, w) * G).sum(); mask_odd: G zero on every odd output pixel (row or column)"""
    x, w, G = inputs
    G = G.clone()
    if mask_odd:
        G[:, :, 1::2, :] = 0
        G[:, :, :, 1::2] = 0
    lx, lw = _leaves((x, w), dt)
    z = F.conv2d(lx, lw, None, stride=stride, padding=(k - 1) // 2)
    (z * G.to(dt)).sum().backward()
    return {"gx": lx.grad, "gw": lw.grad}, G


def _bn_make(shape, seed):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(1000 + seed)
    gamma, var = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5
    return (rnd(B, C, H, W, seed=seed), gamma, rnd(C, seed=2000 + seed, scale=0.3), rnd(C, seed=3000 + seed, scale=0.1), var,
            rnd(B, C, H, W, seed=5000 + seed), rnd(B, C, H, W, seed=4000 + seed))


def bn_graph(inputs, dt, residual, relu, training=True):
    """-> (dict y, gx, gres, ggamma, gbeta, running_mean, running_var; min |ReLU input|)"""
    x, gamma, beta, rm, rv, res, R = inputs
    lx, lg, lb, lr = _leaves((x, gamma, beta, res), dt)
    rm, rv = rm.to(dt).clone(), rv.to(dt).clone()
    z = F.batch_norm(lx, rm, rv, lg, lb, training, MOMENTUM, EPS)
    if residual:
        z = z + lr
    y = F.relu(z) if relu else z
    (y * R.to(dt)).sum().backward()
    out = {"y": y.detach(), "gx": lx.grad, "ggamma": lg.grad, "gbeta": lb.grad, "running_mean": rm, "running_var": rv}
    if residual:
        out["gres"] = lr.grad
    return out, (float(z.detach().abs().min()) if relu else 1.0)


@functools.lru_cache(maxsize=None)
def bn_inputs(i, residual, relu, training=True):
    make = lambda seed: _bn_make(BN_CASES[i], 11 * seed + i)
    return make(_margin_seed(make, lambda inp: bn_graph(inp, torch.float64, residual, relu, training)[1]))


def pool_input(i):
    """relu(randn) with about half of the windows all zero and, in about a quarter of the others, the window's maximum written a
    second time into another cell (two equal positive maxima) -> (x, R)"""
    B, C, H, W = POOL_CASES[i]
    g = torch.Generator().manual_seed(700 + i)
    x = torch.relu(torch.randn(B, C, H, W, generator=g))
    zero = torch.rand(B, C, H // 2, W // 2, generator=g) < 0.5
    x = x * (~zero).repeat_interleave(2, 2).repeat_interleave(2, 3)
    win = x.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4).clone()
    dup = (torch.rand(B, C, H // 2, W // 2, generator=g) < 0.25) & ~zero
    cell = torch.randint(0, 4, (B, C, H // 2, W // 2), generator=g)
    mx = win.max(dim=-1).values
    win.scatter_(-1, cell.unsqueeze(-1), torch.where(dup, mx, win.gather(-1, cell.unsqueeze(-1)).squeeze(-1)).unsqueeze(-1))
    x = win.view(B, C, H // 2, W // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H, W).contiguous()
    return x, rnd(B, C, H // 2, W // 2, seed=710 + i)


def pool_graph(x, R, channels_last=False):
    """torch's CPU max-pool autograd on the fp32 values -> (out, gx)"""
    lx = x.detach().clone()
    if channels_last:
        lx = lx.contiguous(memory_format=torch.channels_last)
    lx.requires_grad_(True)
    out = F.max_pool2d(lx, 2, 2)
    (out * R).sum().backward()
    return out.detach(), lx.grad.contiguous()


def block_params(Ci, Co, k, seed):
    """(w, bn_w, bn_b, running_mean, running_var)"""
    g = torch.Generator().manual_seed(500 + seed)
    return (rnd(Co, Ci, k, k, seed=seed + 3, scale=1.0 / (k * k * Ci) ** 0.5), torch.rand(Co, generator=g) + 0.5,
            rnd(Co, seed=seed + 5, scale=0.3), rnd(Co, seed=seed + 6, scale=0.1), torch.rand(Co, generator=g) + 0.5)


def _block_make(kind, seed):
    B, cins, Co, H, W, k, s, has_res, relu = BLOCK_CASES[kind]
    ho, wo = out_hw(H, W, k, s)
    xs = tuple(rnd(B, c, H, W, seed=seed + 11 + j) for j, c in enumerate(cins))
    return (xs, block_params(sum(cins), Co, k, seed), rnd(B, Co, ho, wo, seed=seed + 7) if has_res else None,
            rnd(B, Co, ho, wo, seed=seed + 8))


def block_graph(kind, inputs, dt, training=True):
    """-> (dict y, x0.. (one per input map), w, bn_w, bn_b, [res], running statistics; margin to the ReLU's kink)"""
    _, cins, _, _, _, k, s, has_res, relu = BLOCK_CASES[kind]
    xs, params, res, R = inputs
    lxs = _leaves(xs, dt)
    lw, lg, lb = _leaves(params[:3], dt)
    rm, rv = params[3].to(dt).clone(), params[4].to(dt).clone()
    x = torch.cat(lxs, dim=1) if len(lxs) > 1 else lxs[0]
    z = F.batch_norm(F.conv2d(x, lw, None, stride=s, padding=(k - 1) // 2), rm, rv, lg, lb, training, MOMENTUM, EPS)
    lr = None
    if has_res:
        lr, = _leaves((res,), dt)
        z = z + lr
    y = F.relu(z) if relu else z
    (y * R.to(dt)).sum().backward()
    out = {"y": y.detach(), "w": lw.grad, "bn_w": lg.grad, "bn_b": lb.grad, "running_mean": rm, "running_var": rv}
    out.update({f"x{j}": t.grad for j, t in enumerate(lxs)})
    if has_res:
        out["res"] = lr.grad
    return out, (float(z.detach().abs().min()) if relu else 1.0)


@functools.lru_cache(maxsize=None)
def block_inputs(kind):
    make = lambda seed: _block_make(kind, 100 * seed + 17 * sorted(BLOCK_CASES).index(kind))
    return make(_margin_seed(make, lambda inp: block_graph(kind, inp, torch.float64)[1]))


# ---- DLA-34 levels 2-5 on a state dict ----
LEVELS = ((2, 1, False), (3, 2, True), (4, 2, True), (5, 1, True))      # (level, Tree levels, level_root); every one has stride 2


def level_param_names(sd):
    return [n for n in sd if n.startswith(("base.level2.", "base.level3.", "base.level4.", "base.level5."))
            and n.endswith((".weight", ".bias"))]


def levels_forward(P, stats, x, training=True):
    """DLA.forward's levels 2-5 (dla.py:225-232) on tensors `P` (name -> weight / bias) and running statistics `stats` (name ->
    tensor, updated in place) -> (the four level maps, min |ReLU input|)"""
    kinks = []

    def cba(conv, bn, t, stride=1, residual=None, relu=True):
        w = P[conv + ".weight"]
        z = F.conv2d(t, w, None, stride=stride, padding=(w.shape[-1] - 1) // 2)
        z = F.batch_norm(z, stats[bn + ".running_mean"], stats[bn + ".running_var"], P[bn + ".weight"], P[bn + ".bias"], training,
                         MOMENTUM, EPS)
        if residual is not None:
            z = z + residual
        if relu:
            kinks.append(float(z.detach().abs().min()))
            z = F.relu(z)
        return z

    def block(p, t, stride, residual):
        o = cba(p + ".conv1", p + ".bn1", t, stride=stride)
        return cba(p + ".conv2", p + ".bn2", o, residual=t if residual is None else residual)

    def tree(p, levels, t, stride, level_root, children=None):
        children = [] if children is None else children
        bottom = F.max_pool2d(t, stride, stride) if stride > 1 else t
        residual = cba(p + ".project.0", p + ".project.1", bottom, relu=False) if (p + ".project.0.weight") in P else bottom
        if level_root:
            children.append(bottom)
        if levels > 1:
            x1 = tree(p + ".tree1", levels - 1, t, stride, False)
            children.append(x1)
            return tree(p + ".tree2", levels - 1, x1, 1, False, children)
        x1 = block(p + ".tree1", t, stride, residual)
        x2 = block(p + ".tree2", x1, 1, None)
        return cba(p + ".root.conv", p + ".root.bn", torch.cat([x2, x1, *children], 1))

    out = []
    for lvl, levels, root in LEVELS:
        x = tree(f"base.level{lvl}", levels, x, 2, root)
        out.append(x)
    return out, min(kinks)


def levels_graph(sd, level1, Rs, dt, training=True):
    """-> ({"level2".."level5": maps, "level1": the input's gradient, parameter name: gradient}, margin) of
    sum over the levels of (map * R).sum() on the state dict's level 2-5 tensors"""
    names = level_param_names(sd)
    P = dict(zip(names, _leaves([sd[n] for n in names], dt)))
    stats = {n: t.detach().to(dt).clone() for n, t in sd.items() if n.endswith(("running_mean", "running_var"))}
    lx, = _leaves((level1,), dt)
    maps, margin = levels_forward(P, stats, lx, training)
    sum((m * R.to(dt)).sum() for m, R in zip(maps, Rs)).backward()
    out = {f"level{2 + j}": m.detach() for j, m in enumerate(maps)}
    out["level1"] = lx.grad
    out.update({n: t.grad for n, t in P.items()})
    return out, margin


def levels_input(sd, shape, hint=None, tries=1000):
    """a post-ReLU-like level-1 map (B,32,h,w) whose float64 graph on `sd` keeps KINK from every ReLU kink, and one R per level.
    Levels 2-5 hold some 2e5 ReLU inputs on a 32 x 48 map, so fewer than one draw in a hundred qualifies: `hint` is the seed a
    caller found earlier for these weights, tried first (and checked like any other)."""
    names = level_param_names(sd)
    P = {n: sd[n].detach().double() for n in names}
    B, _, h, w = shape

    def margin(seed):
        stats = {n: t.detach().double().clone() for n, t in sd.items() if n.endswith(("running_mean", "running_var"))}
        with torch.no_grad():
            return levels_forward(P, stats, torch.relu(rnd(*shape, seed=900 + seed)).double())[1]
    seed = hint if hint is not None and margin(hint) >= KINK else _margin_seed(lambda s: s, margin, tries)
    Rs = [rnd(B, c, h >> (j + 1), w >> (j + 1), seed=950 + j) for j, c in enumerate((64, 128, 256, 512))]
    return torch.relu(rnd(*shape, seed=900 + seed)), Rs
