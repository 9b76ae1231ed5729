"""cf_topk_peaks_fused: the index pass of an at-peaks forward - the 3x3 equality NMS inside the register-cached slice kernel, both
top-K lists from one read of the map, one merge launch that also writes cf_head_fused_at's slot tables.

Everything is compared bit for bit (`torch.equal`) with the entry points it replaces in that forward: cf_topk_peaks(nms = 0),
cf_topk_peaks(nms = 2) and cf_head_slot_tables on their lists - with the raw list (both lists from one launch) and without it
(the NMS'd list alone)."""
import pytest
import torch

gpu = pytest.mark.gpu

# (B, C, H, W, K): slices of 42 elements just above K, borders inside rows and planes | several images, odd slice length | one
# image of the workload's map (14,000-element slices: 13.7 elements per thread) | K = 1 | K > 128: four threads per group |
# slices of 10 elements, fewer than K: the tiny-slice path | slices of 16,640 elements, more than the register-cached kernel
# holds: cf_topk_peaks' own slice passes in front of the one merge
SHAPES = [(2, 3, 13, 17, 40), (3, 2, 40, 56, 100), (1, 10, 112, 200, 100), (2, 1, 9, 11, 1), (1, 4, 64, 64, 256),
          (2, 2, 8, 10, 100), (1, 1, 520, 512, 100)]
DATA = ["normal", "plateau", "constant", "band_random", "band_plateau", "ramp"]
SLICES, RT = 16, 1024


def make_map(kind, B, C, H, W, K):
    g = torch.Generator().manual_seed(B * 1000 + C * 100 + H + W + K)
    n = C * H * W
    if kind == "normal":                       # negatives: suppression raises them to -0, which ties with +0
        return torch.randn(B, C, H, W, generator=g)
    if kind == "plateau":                      # a heat map's clamp plateau: ties at the bound overflow the candidates, go by index
        return (torch.randn(B, C, H, W, generator=g) - 2.0).relu().clamp(min=1e-4)
    if kind == "constant":
        return torch.full((B, C, H, W), 0.25)
    if kind in ("band_random", "band_plateau"):
        # high values at the elements of the first 99 eight-thread groups of a slice's workgroup, low ones elsewhere: the K-th
        # largest group maximum is a low value with up to 99 * 8 * 14 = 11,088 elements above it (> the 4,096 candidates: the
        # radix select) - random ones for the raw list, a plateau (which the equality NMS keeps whole) for both lists
        length = -(-n // SLICES)
        idx = torch.arange(n)
        band = ((idx % length) % RT) < 8 * 99
        low = torch.rand(B, n, generator=g) * 0.5
        high = 1.0 + torch.rand(B, n, generator=g) if kind == "band_random" else torch.full((B, n), 1.5)
        return torch.where(band[None], high, low).view(B, C, H, W)
    if kind == "ramp":                         # one local maximum per plane: fewer than K in a slice, the zero plateau ranked by index
        y, x = torch.arange(H).view(1, 1, H, 1), torch.arange(W).view(1, 1, 1, W)
        c, b = torch.arange(C).view(1, C, 1, 1), torch.arange(B).view(B, 1, 1, 1)
        return (1.0 + x + 0.01 * y + 0.001 * c + 0.0001 * b).float().expand(B, C, H, W).contiguous()
    raise ValueError(kind)


def slot_tables(la, lb, B, K, HW):
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    dev = lb.device
    t_ab = torch.full((B, -(-2 * K // 18), 18), 12345, device=dev, dtype=torch.int32)
    t_b = torch.full((B, -(-K // 18), 18), 12345, device=dev, dtype=torch.int32)
    _lib.check(lib.cf_head_slot_tables(_lib.ptr(la), _lib.ptr(lb), B, K, HW, _lib.ptr(t_ab), _lib.ptr(t_b), _lib.stream_ptr()),
               "cf_head_slot_tables")
    return t_ab, t_b


@gpu
@pytest.mark.parametrize("kind", DATA)
@pytest.mark.parametrize("B,C,H,W,K", SHAPES)
def test_fused_index_pass_equals_the_separate_entry_points(B, C, H, W, K, kind):
    from centerfusiondetect3d_amd import ops
    assert torch.cuda.is_available()
    heat = make_map(kind, B, C, H, W, K).to("cuda:0")
    want_raw = ops.topk_peaks(heat, K, nms=0)
    want_nms = ops.topk_peaks(heat, K, nms=2)
    # B1: the NMS'd list alone (the NMS inside the slice kernel); the tables hold -1 where the raw list would stand
    raw, nms, t_ab, t_b = ops.topk_peaks_fused(heat, K, want_raw=False)
    assert raw is None
    for got, want, name in zip(nms, want_nms, ("scores", "inds", "classes")):
        assert torch.equal(got, want), ("nms alone", name)
    r_ab, r_b = slot_tables(None, want_nms[1], B, K, H * W)
    assert torch.equal(t_ab, r_ab) and torch.equal(t_b, r_b)
    # B2: both lists from one read, one merge, the tables from the merge
    raw, nms, t_ab, t_b = ops.topk_peaks_fused(heat, K)
    for got, want, name in zip(raw, want_raw, ("scores", "inds", "classes")):
        assert torch.equal(got, want), ("raw", name)
    for got, want, name in zip(nms, want_nms, ("scores", "inds", "classes")):
        assert torch.equal(got, want), ("nms", name)
    # (scores compare as floats: +0 == -0; the bits as well)
    assert torch.equal(nms[0].view(torch.int32), want_nms[0].view(torch.int32))
    assert torch.equal(raw[0].view(torch.int32), want_raw[0].view(torch.int32))
    r_ab, r_b = slot_tables(want_raw[1], want_nms[1], B, K, H * W)
    assert torch.equal(t_ab, r_ab) and torch.equal(t_b, r_b)
    # without tables: the lists alone
    raw, nms, none_ab, none_b = ops.topk_peaks_fused(heat, K, want_tables=False)
    assert none_ab is None and none_b is None
    assert all(torch.equal(a, b) for a, b in zip(raw + nms, want_raw + want_nms))


def test_fused_entry_point_refuses_bad_arguments():
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    nulls = (None,) * 10
    assert lib.cf_topk_peaks_fused(None, 1, 1, 1, 1, 1, *nulls) == -22 and b"null buffer" in lib.cf_last_error()
    # register-cached slices: two sets of slice lists; longer slices: + the suppressed map of the two-pass form
    assert lib.cf_topk_peaks_fused_workspace_bytes(16, 10, 112, 200, 100) == 2 * lib.cf_topk_workspace_bytes(16, 100)
    assert lib.cf_topk_peaks_fused_workspace_bytes(2, 10, 224, 400, 100) == (
        lib.cf_topk_workspace_bytes(2, 100) + lib.cf_topk_workspace_bytes_nms(2, 10, 224, 400, 100))
