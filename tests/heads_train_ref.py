"""Shared reference of the head training tests (tests/test_heads_train_cpu.py, tests/test_gpu_heads_train.py,
tools/heads_train_oracle_error.py): the reference-structured head (detectHeads.py:59-98) as a torch nn.Sequential on the CPU in
float64 and fp32, the case table and the two constructions that keep the ReLU masks of fp32 and float64 identical.

(a) "dyadic": x, the hidden layers' weights and all hidden biases are small dyadic rationals - every fp32 summation order gives the
    exact pre-activation (asserted: max sum |terms| / resolution < 2^24 per layer), exact zeros occur (ReLU'(0) = 0 is tested);
    the output layer's weights and dY are ordinary randn.
(b) "linear": randn everything, hidden biases raised until every hidden pre-activation exceeds 1 in float64 - no mask can flip.

Geometry the cases reach (the kernels' constants, restated here and asserted by the CPU test against the library): 32-position
tiles of the layer kernel, 256-position slabs of the weight-gradient kernels, 128-position slabs of the output layer's, chunks
that are multiples of 64 positions; the three launch caps behind which a kernel loops (GEMM_GRID_CAP, OUT_BWD_GRID_CAP,
OUT_FWD_THREAD_CAP).

REPLICATED holds the sizes a direct reference cannot reach (the fp32 oracle's own error on a large dense gradient exceeds the
rule's limit): a head is per-image, so R copies of a base batch give R copies of its float64 map, and the gradients are those of
the few images that carry a dY - a small batch the float64 reference runs directly (`rep_reference`)."""
import functools

import torch
from torch import nn

HID = 256
TILE, SLAB, OUT_SLAB = 32, 256, 128
DEFAULT_CHUNK = 32768            # cf_heads_bwd.hip:22
# the launch caps of cf_heads_bwd.hip, kernel-internal (no entry point reports them): above them a kernel loops
GEMM_GRID_CAP = 4096             # head_gemm_kernel: grid.x = min(tiles of a chunk, 4096); cf_heads_bwd.hip:447 and :551, loop at :61
OUT_BWD_GRID_CAP = 4096          # head_out_bwd_data_kernel: grid = min(chunk, 4096) blocks, one position each; :539, loop at :325
OUT_FWD_THREAD_CAP = 4096 * 256  # head_out_fwd_kernel: blocks_for(chunk * n_out, 4096) blocks of 256 threads; :503, loop at :303
COMPACT_BLOCK = 256              # head_compact_kernel: pixels per block; :527

# name: (B, c_x, c_x2, n_hidden, Cout, h, w, family, dY pattern, chunk_px, final)
CASES = {
    "dy_5x7_c1":          (1, 64, 0, 0, 1, 5, 7, "dyadic", "dense", 0, None),          # 35 positions: one tile and 3; below every slab
    "dy_3x5_c1":          (1, 64, 0, 0, 1, 3, 5, "dyadic", "dense", 0, None),          # smaller than a tile, every pixel but 3 on a border
    "dy_one_tile_c2":     (1, 64, 0, 0, 2, 4, 8, "dyadic", "dense", 0, None),          # exactly one 32-position tile
    "dy_17x33_sec_c3":    (2, 64, 3, 2, 3, 17, 33, "dyadic", "dense", 0, None),        # ragged tiles and slabs, second source, ragged K
    "dy_17x33_sparse_c8": (2, 64, 3, 2, 8, 17, 33, "dyadic", "sparse", 0, None),       # 3 pixels in image 0 (two corners), none in image 1
    "dy_zero_c10":        (2, 64, 0, 0, 10, 5, 7, "dyadic", "zero", 0, None),          # every gradient exactly 0
    "lin_tile32_c16":     (2, 64, 0, 0, 16, 17, 33, "linear", ("count", 32), 0, None),  # the list is exactly one tile
    "lin_tile33_c10":     (2, 64, 3, 2, 10, 17, 33, "linear", ("count", 33), 0, None),  # ... and one more
    "lin_slab257_c2":     (2, 64, 0, 0, 2, 17, 33, "linear", ("count", 257), 0, None),  # one weight-gradient slab and one position
    "lin_two_chunks_c2":  (2, 64, 3, 2, 2, 17, 33, "linear", "dense", 576, None),       # 1122 positions: chunks of 576 and 546
    "lin_heatmap_c3":     (1, 64, 0, 0, 3, 5, 7, "linear", "dense", 0, "heatmap"),
    "lin_depth_c1":       (1, 64, 0, 0, 1, 5, 7, "linear", "dense", 0, "depth"),
    # maps one pixel high / wide / both: two thirds (eight ninths) of the taps outside
    "dy_1x40_c2":         (1, 64, 0, 0, 2, 1, 40, "dyadic", "dense", 0, None),
    "dy_40x1_sec_c2":     (1, 64, 3, 2, 2, 40, 1, "dyadic", "dense", 0, None),
    "dy_1x1_c3":          (2, 64, 0, 0, 3, 1, 1, "dyadic", "dense", 0, None),          # M = 2: only the centre tap inside
    "dy_nh1_c4":          (2, 64, 3, 1, 4, 17, 33, "dyadic", "dense", 0, None),        # one hidden layer: odd parity of the g / g2 swap
    "dy_cx72_sec_c3":     (1, 72, 3, 2, 3, 9, 11, "dyadic", "dense", 0, None),         # kvec = 64 < c_x = 72 < K = 75: the k-tail reads both rows
    "dy_cx8_c2":          (1, 8, 0, 0, 2, 9, 11, "dyadic", "dense", 0, None),          # c_x < 16: kvec = 0
    "lin_cin512_c2":      (1, 448, 64, 0, 2, 5, 7, "linear", "dense", 0, None),        # Cin at the limit: 16 channel chunks
    "lin_8img_dense_c3":  (8, 64, 3, 2, 3, 17, 33, "linear", "dense", 0, None),        # 4488 positions in one chunk: above OUT_BWD_GRID_CAP
    "lin_8img_5chunks_c2": (8, 64, 3, 2, 2, 17, 33, "linear", "dense", 1088, None),    # chunks 4 x 1088 + 136
    "lin_8img_1500_c2":   (8, 64, 0, 0, 2, 17, 33, "linear", ("count", 1500), 1088, None),  # the list ends inside chunk 1; 2 .. 4 empty
    "lin_8img_heat_c10":  (8, 64, 0, 0, 10, 17, 33, "linear", "dense", 0, "heatmap"),  # the workload's dense heat-map gradient
    "lin_1img_nh1_c16":   (1, 64, 3, 1, 16, 17, 33, "linear", "dense", 0, None),       # the base of rep234_gridcaps
}

# name: (base case, R copies of the base's batch, chunk_px, {image of the replicated batch: its dY})
# a dY is "base" (the base's dY of that image), "sparse" (the three pixels of the sparse pattern) or ("count", n) (n random pixels)
REPLICATED = {
    # M = 131274; one chunk of 131136 = 4098 tiles (> GEMM_GRID_CAP) x 16 outputs = 2.1 M elements (> OUT_FWD_THREAD_CAP), then 138
    # positions; 33 + 3 + 561 = 597 list positions out of the first, a middle and the last of 513 compaction blocks
    "rep234_gridcaps":     ("lin_1img_nh1_c16", 234, 131136, {0: ("count", 33), 117: "sparse", 233: "base"}),
    # M = 35904 at the default chunk: 32768 + 3136, the boundary inside image 58
    "rep64_default_chunk": ("lin_two_chunks_c2", 32, 0, {0: ("count", 33), 58: "base", 63: "base"}),
}


def _chunk(M, chunk_px):
    return min(chunk_px or DEFAULT_CHUNK, (M + 63) // 64 * 64)


def geometry(name):
    """what the case reaches: positions, chunks, tiles of the last chunk, weight-gradient slabs (of a dense list); the chunk the
    backward's list ends in, how far into it, and the chunks behind it that hold none of the list; the widths the first layer's
    k loop sees on the packed sources `ops.head_stack` makes (K, and kvec: the leading channels read as vectors)"""
    B, c_x, c_x2, n_hidden, cout, h, w, _, pattern, chunk_px, _ = CASES[name]
    M = B * h * w
    chunk = _chunk(M, chunk_px)
    n_act = M if pattern == "dense" else 0 if pattern == "zero" else 3 if pattern == "sparse" else pattern[1]
    chunks = (M + chunk - 1) // chunk
    list_chunks = (n_act + chunk - 1) // chunk
    return dict(M=M, chunk=chunk, chunks=chunks, active=n_act,
                tiles=(min(n_act, chunk) + TILE - 1) // TILE, slabs=(min(n_act, chunk) + SLAB - 1) // SLAB,
                list_end_chunk=list_chunks - 1, list_end_at=n_act - (list_chunks - 1) * chunk if n_act else 0,
                empty_chunks=chunks - list_chunks, bwd_data_grid=min(chunk, OUT_BWD_GRID_CAP),
                K=c_x + c_x2, kvec=c_x // 16 * 16 if c_x % 4 == 0 else 0, n_hidden=n_hidden,
                taps_inside=min(h, 3) * min(w, 3))


def rep_geometry(name):
    """what a replicated case reaches: positions, the chunk, its tiles and output elements (the forward's two grid caps), the
    backward's list and the compaction blocks it comes from, the images a forward chunk boundary falls strictly inside of"""
    base, R, chunk_px, _ = REPLICATED[name]
    B, _, _, _, cout, h, w = CASES[base][:7]
    hw, M = h * w, R * B * h * w
    chunk = _chunk(M, chunk_px)
    dy = rep_build(name)["dy_full"]
    at = (dy != 0).any(dim=1).flatten().nonzero().flatten()
    return dict(M=M, images=R * B, chunk=chunk, chunks=(M + chunk - 1) // chunk, tiles=(chunk + TILE - 1) // TILE,
                out_elems=chunk * cout, active=int(at.numel()), compact_blocks=(M + COMPACT_BLOCK - 1) // COMPACT_BLOCK,
                active_blocks=sorted({int(v) // COMPACT_BLOCK for v in at}),
                split_images=[c // hw for c in range(chunk, M, chunk) if c % hw])


def _dyadic(gen, shape, step, lo, hi):
    return (torch.randint(lo, hi + 1, shape, generator=gen).double() * step)


def _sparse_pm1(gen, rows, cols, nnz):
    w = torch.zeros(rows, cols, dtype=torch.float64)
    for r in range(rows):
        at = torch.randperm(cols, generator=gen)[:nnz]
        w[r, at] = (torch.randint(0, 2, (nnz,), generator=gen).double() * 2 - 1)
    return w


def _conv(x, w, b):
    return torch.nn.functional.conv2d(x, w, b, padding=w.shape[-1] // 2)


@functools.lru_cache(maxsize=None)
def build(name):
    """-> dict(x, x2 | None, weights, biases, dy, final, chunk_px, checks) in float64 (every value fp32-representable).
    checks: per hidden layer, "dyadic": max sum |terms| / resolution; "linear": min pre-activation."""
    B, c_x, c_x2, n_hidden, cout, h, w, family, pattern, chunk_px, final = CASES[name]
    gen = torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(name)))
    cin = c_x + c_x2
    checks = []
    if family == "dyadic":
        x = _dyadic(gen, (B, cin, h, w), 0.5, -2, 2)
        weights = [_dyadic(gen, (HID, cin, 3, 3), 0.5, -2, 2)]
        weights += [_sparse_pm1(gen, HID, HID, nnz).view(HID, HID, 1, 1) for nnz in (16, 8)[:n_hidden]]
        biases = [_dyadic(gen, (HID,), 0.25, -4, 4) for _ in range(n_hidden + 1)]
        cur = x
        for wl, bl in zip(weights, biases):
            mag = _conv(cur.abs(), wl.abs(), bl.abs())
            checks.append(float(mag.max()) / 0.25)          # (every term is a multiple of 0.25)
            cur = torch.relu(_conv(cur, wl, bl))
    else:
        x = torch.randn((B, cin, h, w), generator=gen).float().double()
        weights, biases, cur = [], [], x
        for l in range(n_hidden + 1):
            k, ci = (3, cin) if l == 0 else (1, HID)
            wl = (torch.randn((HID, ci, k, k), generator=gen) / (ci * k * k) ** 0.5).float().double()
            pre = _conv(cur, wl, None)
            bl = (1.5 - pre.amin(dim=(0, 2, 3))).float().double()       # raised until the smallest pre-activation is ~1.5
            cur = _conv(cur, wl, bl)
            checks.append(float(cur.min()))
            cur = torch.relu(cur)
            weights.append(wl)
            biases.append(bl)
    # the output layer: ordinary randn, scaled so that the raw map has a spread of a few units (the heat-map case needs both
    # clamped and unclamped elements: |y| beyond and within log(1e4) = 9.21)
    wo = torch.randn((cout, HID, 1, 1), generator=gen).double()
    pre = _conv(cur, wo, None)
    wo = (wo * (6.0 / float(pre.std()) if final == "heatmap" else 1.0 / max(1.0, float(pre.abs().max()) / 4.0))).float().double()
    bo = torch.randn((cout,), generator=gen).float().double() * 0.5
    weights.append(wo)
    biases.append(bo)
    dy = torch.randn((B, cout, h, w), generator=gen).float().double()
    if pattern == "zero":
        dy.zero_()
    elif pattern == "sparse":
        keep = torch.zeros((B, 1, h, w), dtype=torch.float64)
        keep[0, 0, 0, 0] = keep[0, 0, h - 1, w - 1] = keep[0, 0, h // 2, w // 3] = 1.0       # image 1 (and any further) has none
        dy = dy * keep
    elif isinstance(pattern, tuple):
        at = torch.randperm(B * h * w, generator=gen)[:pattern[1]]
        keep = torch.zeros(B * h * w, dtype=torch.float64)
        keep[at] = 1.0
        keep = keep.view(B, 1, h, w).clone()
        if cout > 1:                                     # (an active pixel need not be non-zero in every channel)
            dy[:, 0] = 0.0
            b0, r0 = int(at[0]) // (h * w), int(at[0]) % (h * w)
            dy[b0, 0, r0 // w, r0 % w] = 1.0
        dy = dy * keep
    return dict(x=x[:, :c_x].contiguous(), x2=x[:, c_x:].contiguous() if c_x2 else None, weights=weights, biases=biases, dy=dy,
                final=final, chunk_px=chunk_px, checks=checks, family=family)


@functools.lru_cache(maxsize=None)
def rep_build(name):
    """-> dict(base = the base case, images = the images that carry a dY, small = the case of just those images (float64, what
    `run_reference` takes), dy_full = the replicated batch's dY (fp32, zero elsewhere), R, chunk_px).  The replicated sources
    themselves are `rep_sources`' (not cached: 35 MB)."""
    base_name, R, chunk_px, dys = REPLICATED[name]
    base = build(base_name)
    B, _, _, _, cout, h, w = CASES[base_name][:7]
    gen = torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(name)))
    images, parts = sorted(dys), []
    for img in images:
        pattern = dys[img]
        if pattern == "base":
            d = base["dy"][img % B].clone()
        else:
            d = torch.randn((cout, h, w), generator=gen).float().double()
            keep = torch.zeros(h * w, dtype=torch.float64)
            if pattern == "sparse":
                keep[0] = keep[h * w - 1] = keep[(h // 2) * w + w // 3] = 1.0
            else:
                keep[torch.randperm(h * w, generator=gen)[:pattern[1]]] = 1.0
            d = d * keep.view(1, h, w)
        parts.append(d)
    dy_full = torch.zeros((R * B, cout, h, w), dtype=torch.float32)
    dy_full[images] = torch.stack(parts).float()
    pick = [i % B for i in images]
    small = dict(x=base["x"][pick].contiguous(), x2=None if base["x2"] is None else base["x2"][pick].contiguous(),
                 weights=base["weights"], biases=base["biases"], dy=torch.stack(parts), final=base["final"], chunk_px=0,
                 family=base["family"])
    return dict(base=base, images=images, small=small, dy_full=dy_full, R=R, chunk_px=chunk_px)


def rep_sources(name):
    """(x, x2 | None) of the replicated batch in fp32: R copies of the base's"""
    rep = rep_build(name)
    x, x2 = rep["base"]["x"].float(), rep["base"]["x2"]
    return x.repeat(rep["R"], 1, 1, 1), None if x2 is None else x2.float().repeat(rep["R"], 1, 1, 1)


@functools.lru_cache(maxsize=None)
def rep_reference(name):
    """(float64 result, fp32 result) of the batch of just the images that carry a dY: its gradients are the replicated batch's"""
    small = rep_build(name)["small"]
    return run_reference(small, torch.float64), run_reference(small, torch.float32)


def rep_oracle_errors(name):
    """{label: error of the fp32 CPU oracle against float64}: "y" on the base case (every replica's map is the base's), the
    gradients on the batch of the images that carry a dY"""
    r64, r32 = rep_reference(name)
    e = {k: rel_err(v32, v64) for (k, v64), (_, v32) in zip(quantities(r64), quantities(r32)) if k[0] == "g"}
    e["y"] = oracle_errors(REPLICATED[name][0])["y"]
    return e


def final_act(y, final):
    if final == "heatmap":
        return torch.clamp(torch.sigmoid(y), min=1e-4, max=1 - 1e-4)         # detectHeads.py:21-23
    if final == "depth":
        return 1.0 / (torch.sigmoid(y) + 1e-6) - 1.0                         # model/utils.py:141
    return y


def sequential(weights, biases, dtype):
    """the reference's head: Conv2d(3x3) ReLU [Conv2d(1x1) ReLU]* Conv2d(1x1) with these parameters"""
    layers = []
    for l, (w, b) in enumerate(zip(weights, biases)):
        conv = nn.Conv2d(w.shape[1], w.shape[0], w.shape[-1], padding=w.shape[-1] // 2, bias=True).to(dtype)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        layers.append(conv)
        if l + 1 < len(weights):
            layers.append(nn.ReLU())
    return nn.Sequential(*layers)


def run_reference(case, dtype):
    """-> dict(y = the raw map, out = the activated map, gw = [...], gb = [...]) of the CPU nn.Sequential in `dtype`; the
    gradient arriving at the activated map is the case's dy."""
    x = case["x"] if case["x2"] is None else torch.cat([case["x"], case["x2"]], 1)
    seq = sequential(case["weights"], case["biases"], dtype)
    y = seq(x.to(dtype))
    out = final_act(y, case["final"])
    out.backward(case["dy"].to(dtype))
    convs = [m for m in seq if isinstance(m, nn.Conv2d)]
    return dict(y=y.detach(), out=out.detach(), gw=[c.weight.grad for c in convs], gb=[c.bias.grad for c in convs])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 result, fp32 result) of case `name`, computed once"""
    case = build(name)
    return run_reference(case, torch.float64), run_reference(case, torch.float32)


def rel_err(got, ref64):
    """max |got - ref64| / max |ref64| (0 / 0 = 0)"""
    d = float((got.double() - ref64).abs().max())
    m = float(ref64.abs().max())
    return d / m if m > 0 else d


def quantities(res):
    """[(label, tensor)] of a result: the maps and every layer's gradients"""
    out = [("y", res["y"]), ("out", res["out"])]
    for l, (gw, gb) in enumerate(zip(res["gw"], res["gb"])):
        out += [(f"gw{l}", gw), (f"gb{l}", gb)]
    return out


def oracle_errors(name):
    """{label: error of the fp32 CPU oracle against float64} of case `name`"""
    r64, r32 = reference(name)
    return {k: rel_err(v32, v64) for (k, v64), (_, v32) in zip(quantities(r64), quantities(r32))}


def case_gate(oracle_err):
    """the project's rule (tests/test_gpu_deform_conv2d_backward.py): 5e-6 where the fp32 CPU oracle's own error is below 2.5e-6,
    otherwise twice that error; above 1.25e-5 the case is unusable"""
    assert oracle_err <= 1.25e-5, f"oracle error {oracle_err:.3g}: the case is unusable and must be replaced"
    return 5e-6 if oracle_err < 2.5e-6 else 2.0 * oracle_err
