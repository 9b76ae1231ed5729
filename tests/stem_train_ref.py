"""Cases and CPU yardsticks of the stem-training tests (tests/test_stem_train_cpu.py, tests/test_gpu_stem_ops.py,
tests/test_gpu_stem_train.py): the graphs of ops.stem_conv_bn_relu, of its convolution alone and of DLA-34's stem
(model/networks/dla.py:193-203, 225-228, 250-262: base_layer, level0, level1) as torch autograd over F.conv2d, F.batch_norm and
F.relu in a chosen dtype, and the launch geometry of csrc/cf_stem_train.hip, restated.  Loss = (output * R).sum() with a fixed
random R everywhere.  Inputs come from seeds chosen as tests/base_train_ref.py chooses them: every ReLU input stays KINK away from
zero in float64.  No GPU, no library."""
import functools

import torch
import torch.nn.functional as F

from tests import early_ref
from tests.base_train_ref import BLOCK_GATE, EPS, KINK, MOMENTUM, _margin_seed, block_params, conv_graph, out_hw, relerr, rnd  # noqa: F401
from tests.neck_train_ref import _leaves

CONV_GATE = 5e-6                 # the project's gate of cf_conv_bwd_* (tests/dcn_backward_ref.BASE_GATE), or twice the fp32 CPU error

# ---- the convolution alone, forward and backward: (B, Cin, Cout, H, W, k, stride); Cin = 6: three image planes + the radar map ----
CONV_CASES = [(1, 3, 16, 1, 1, 7, 1),                             # one pixel
              (1, 3, 16, 5, 4, 7, 1),                             # map smaller than the filter
              (2, 3, 16, 9, 13, 7, 1),                            # batch boundary inside a tile, M not a multiple of the tile
              (1, 6, 16, 8, 12, 7, 1),                            # radar map 2 x 3 sampled in the kernel
              (2, 16, 16, 9, 13, 3, 1),                           # 3x3 stride 1
              (1, 16, 32, 7, 9, 3, 2),                            # odd H and W under stride 2
              (2, 16, 32, 8, 12, 3, 2),                           # 3x3 stride 2, even map
              # ---- one per branch of the launch geometry (CONV_GEOMETRY below; asserted in tests/test_stem_train_cpu.py) ----
              (1, 16, 16, 120, 250, 3, 1),                        # 118 slabs with a short last one; four column tiles of the grids
              (1, 16, 32, 6, 140, 3, 2),                          # two column tiles of a parity class under stride 2
              (1, 6, 16, 276, 272, 7, 1)]                         # the slab cap binds (292 for 19 column tiles); 7x7 column tiles
# (slabs, cap, pixels per slab, pixels of the last slab, column tiles of the forward grid, column tiles of the data grid)
CONV_GEOMETRY = {0: (1, 512, 4, 1, 1, 0), 1: (1, 512, 20, 20, 1, 0), 2: (1, 512, 236, 234, 1, 0), 3: (1, 292, 96, 96, 1, 0),
                 4: (1, 682, 236, 234, 1, 1), 5: (1, 682, 20, 20, 1, 1), 6: (1, 682, 48, 48, 1, 1), 7: (118, 682, 256, 48, 4, 4),
                 8: (1, 682, 212, 210, 2, 2), 9: (289, 292, 260, 192, 5, 0)}

# ---- the block, one per layer kind: (B, Cin, Cout, H, W, k, stride) ----
BLOCK_CASES = {"base_layer": (2, 3, 16, 9, 13, 7, 1), "base_layer_early": (2, 6, 16, 8, 12, 7, 1), "level0": (2, 16, 16, 9, 13, 3, 1),
               "level1": (2, 16, 32, 9, 13, 3, 2)}

STEM = (("base.base_layer", 1), ("base.level0", 1), ("base.level1", 2))
STEM_SHAPE = (2, 3, 32, 32)      # some 8e4 ReLU inputs: about every second draw keeps KINK


# ---- the launch geometry of csrc/cf_stem_train.hip, restated ----
TILE_COLS, TILE_ROWS = 64, 4     # ST_COLS, ST_ROWS: pixels of a workgroup of the forward / data kernels
COL_TILES_PER_WAVE = 3           # SW_CT


def weight_slabs(M, Cin, k):
    """sw_slabs of cf_stem_conv_bwd_weight for M output pixels -> (slabs, cap, slab_px, pixels of the last slab)"""
    ntiles = (k * k * Cin + 15) // 16
    groups = (ntiles + COL_TILES_PER_WAVE - 1) // COL_TILES_PER_WAVE
    cap = max(2048 // groups, 1)
    s = max(min((M + 255) // 256, cap), 1)
    slab_px = ((M + s - 1) // s + 3) // 4 * 4
    slabs = (M + slab_px - 1) // slab_px
    return slabs, cap, slab_px, M - (slabs - 1) * slab_px


def conv_geometry(B, Cin, Cout, H, W, k, stride):
    ho, wo = out_hw(H, W, k, stride)
    data_tiles = ((W + stride - 1) // stride + TILE_COLS - 1) // TILE_COLS if k == 3 else 0
    return weight_slabs(B * ho * wo, Cin, k) + ((wo + TILE_COLS - 1) // TILE_COLS, data_tiles)


def conv_workspace_bytes(B, Cin, Cout, H, W, k, stride):
    ho, wo = out_hw(H, W, k, stride)
    return weight_slabs(B * ho * wo, Cin, k)[0] * Cout * k * k * Cin * 4


# ---- graphs ----
def conv_inputs(i):
    """-> (x as the kernels take it (the image planes alone when Cin = 6), radar map or None, w, G)"""
    B, Ci, Co, H, W, k, s = CONV_CASES[i]
    ho, wo = out_hw(H, W, k, s)
    radar = rnd(B, 3, H // 4, W // 4, seed=411 + i) if Ci == 6 else None
    return (rnd(B, 3 if Ci == 6 else Ci, H, W, seed=401 + i), radar, rnd(Co, Ci, k, k, seed=403 + i, scale=1.0 / (k * k * Ci) ** 0.5),
            rnd(B, Co, ho, wo, seed=407 + i))


def full_input(x, radar):
    """the convolution's input as the reference holds it: early_ref.combine's six channels, or x itself"""
    return x if radar is None else early_ref.combine(x, radar)


def conv_all(inputs, k, stride, dt, mask_odd=False):
    """-> ({"z", "gx", "gw"}, G) of the convolution on the materialised input (tests/base_train_ref.conv_graph, plus the forward)"""
    x, radar, w, G = inputs
    xf = full_input(x, radar)
    out, G = conv_graph((xf, w, G), k, stride, dt, mask_odd)
    out["z"] = F.conv2d(xf.to(dt), w.to(dt), None, stride=stride, padding=(k - 1) // 2)
    return out, G


def _block_make(kind, seed):
    B, Ci, Co, H, W, k, s = BLOCK_CASES[kind]
    ho, wo = out_hw(H, W, k, s)
    radar = rnd(B, 3, H // 4, W // 4, seed=seed + 12) if Ci == 6 else None
    return rnd(B, 3 if Ci == 6 else Ci, H, W, seed=seed + 11), radar, block_params(Ci, Co, k, seed), rnd(B, Co, ho, wo, seed=seed + 8)


def block_graph(kind, inputs, dt, training=True):
    """-> (dict y, x (3x3 only), w, bn_w, bn_b, running statistics; margin to the ReLU's kink)"""
    _, _, _, _, _, k, s = BLOCK_CASES[kind]
    x, radar, params, R = inputs
    lx, = _leaves((full_input(x, radar),), dt)
    lw, lg, lb = _leaves(params[:3], dt)
    rm, rv = params[3].to(dt).clone(), params[4].to(dt).clone()
    z = F.batch_norm(F.conv2d(lx, lw, None, stride=s, padding=(k - 1) // 2), rm, rv, lg, lb, training, MOMENTUM, EPS)
    y = F.relu(z)
    (y * R.to(dt)).sum().backward()
    out = {"y": y.detach(), "w": lw.grad, "bn_w": lg.grad, "bn_b": lb.grad, "running_mean": rm, "running_var": rv}
    if k == 3:
        out["x"] = lx.grad
    return out, float(z.detach().abs().min())


@functools.lru_cache(maxsize=None)
def block_inputs(kind, training=True):
    make = lambda seed: _block_make(kind, 100 * seed + 17 * sorted(BLOCK_CASES).index(kind))
    return make(_margin_seed(make, lambda inp: block_graph(kind, inp, torch.float64, training)[1]))


# ---- DLA-34's stem on a state dict ----
def stem_param_names(sd):
    return [n for n in sd if n.startswith(("base.base_layer.", "base.level0.", "base.level1.")) and n.endswith((".weight", ".bias"))]


def stem_forward(P, stats, x, training=True):
    """DLA.forward's base_layer, level0, level1 on tensors `P` (name -> weight / bias) and running statistics `stats` (name ->
    tensor, updated in place); x: the three- or six-channel image -> (the level-1 map, min |ReLU input|)"""
    kinks, t = [], x
    for p, stride in STEM:
        w = P[p + ".0.weight"]
        z = F.conv2d(t, w, None, stride=stride, padding=(w.shape[-1] - 1) // 2)
        z = F.batch_norm(z, stats[p + ".1.running_mean"], stats[p + ".1.running_var"], P[p + ".1.weight"], P[p + ".1.bias"], training,
                         MOMENTUM, EPS)
        kinks.append(float(z.detach().abs().min()))
        t = F.relu(z)
    return t, min(kinks)


def _stats(sd, dt):
    return {n: t.detach().to(dt).clone() for n, t in sd.items() if n.endswith(("running_mean", "running_var"))}


def stem_eval(sd, x):
    """the eval-mode fp32 graph on a state dict: what tests/early_ref.stem computes"""
    names = stem_param_names(sd)
    with torch.no_grad():
        return stem_forward({n: sd[n].float() for n in names}, _stats(sd, torch.float32), x.float(), training=False)[0]


def stem_graph(sd, images, pc, R, dt, training=True):
    """-> ({"level1": map, parameter name: gradient, running statistic name: value}, margin) of (level1 * R).sum() on the state
    dict's stem tensors; pc: the radar map of early fusion or None"""
    names = stem_param_names(sd)
    P = dict(zip(names, _leaves([sd[n] for n in names], dt)))
    stats = _stats(sd, dt)
    y, margin = stem_forward(P, stats, full_input(images, pc).to(dt), training)
    (y * R.to(dt)).sum().backward()
    out = {"level1": y.detach()}
    out.update({n: t.grad for n, t in P.items()})
    return out, margin


def stem_input(sd, early, hint=None, tries=400):
    """images (and, early fusion, a radar map) whose float64 graph on `sd` keeps KINK from every ReLU kink, and R.  `hint` is the
    seed a caller found earlier for these weights, tried first (and checked like any other).  -> (images, pc or None, R, seed)"""
    names = stem_param_names(sd)
    P = {n: sd[n].detach().double() for n in names}
    B, _, H, W = STEM_SHAPE

    def make(seed):
        x = rnd(*STEM_SHAPE, seed=800 + seed)
        pc = torch.relu(rnd(B, 3, H // 4, W // 4, seed=850 + seed)) if early else None
        return x, pc

    def margin(seed):
        with torch.no_grad():
            return stem_forward(P, _stats(sd, torch.float64), full_input(*make(seed)).double())[1]
    seed = hint if hint is not None and margin(hint) >= KINK else _margin_seed(lambda s: s, margin, tries)
    x, pc = make(seed)
    return x, pc, rnd(B, 32, H // 2, W // 2, seed=870), seed
