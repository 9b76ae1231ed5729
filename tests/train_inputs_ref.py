"""TEST INFRASTRUCTURE ONLY - CPU statement of the image side of a TRAINING item of the reference dataset
(dataset/generic_dataset.py:166-168, 414-439 with the colorAugmentor of :92-105): numpy flip -> cv2.warpAffine -> / 255 ->
RandomOrder(ColorJitter brightness / contrast / saturation) -> lightingAug -> Normalize, in torch-CPU fp32.

PARITY UNPINNED.  `cv2` and torchvision are third-party dependencies that this repository does not install.  The warp is
oracle/preprocess_ref.warp_affine_u8 (its header says what it restates); the colour chain below restates torchvision's tensor
functions (torchvision/transforms/_functional_tensor.py: `_blend`, `rgb_to_grayscale`, `adjust_brightness`, `adjust_contrast`,
`adjust_saturation`) and `Normalize`, written as they are written there, in fp32 on torch's CPU kernels.  Two things are not
torchvision's and are chosen so that a device can reproduce the result exactly:
  * the random draws (the order and the three factors) are arguments;
  * adjust_contrast's mean is float32(float64 sum / n) instead of torch's own fp32 `mean` (pairwise, vectorised: no
    statement of its order exists).  Over the six orders on the 44x80 warps of case `b`
    (tests/train_inputs_cases.py) the two differ by at most 3.6e-7 in the output.
`ToTensor` keeps the channel order it is given, and cv2.imread gives BGR: the grey weights fall on B, G, R in that order.
"""
import numpy as np
import torch

from oracle import preprocess_ref

BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2          # positions in the reference's ColorJitter list (generic_dataset.py:95-101)


def _blend(img1, img2, ratio):
    ratio = float(ratio)
    return (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 1.0)


def rgb_to_grayscale(img):
    r, g, b = img.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).to(img.dtype).unsqueeze(dim=-3)


def grey_mean(img):
    """-> (float64 mean of the grey level, its fp32 rounding): what adjust_contrast blends with"""
    m = rgb_to_grayscale(img).to(torch.float64).sum().item() / (img.shape[-1] * img.shape[-2])
    return m, np.float32(m)


def adjust_brightness(img, factor):
    return _blend(img, torch.zeros_like(img), factor)


def adjust_contrast(img, factor, means=None):
    m64, m32 = grey_mean(img)
    if means is not None:
        means.append(m64)
    return _blend(img, torch.full((1, 1, 1), float(m32), dtype=img.dtype), factor)


def adjust_saturation(img, factor):
    return _blend(img, rgb_to_grayscale(img), factor)


def colour_chain(img, order, factor, lighting, means=None):
    """img (3,H,W) fp32 in [0,1]; order: a permutation of 0..2; factor[k]: operation k's; lighting (3) -> (3,H,W) fp32.
    `means`: a list that collects the float64 contrast mean."""
    ops = {BRIGHTNESS: adjust_brightness, SATURATION: adjust_saturation,
           CONTRAST: lambda i, f: adjust_contrast(i, f, means)}
    for k in order:
        img = ops[int(k)](img, float(np.float32(factor[int(k)])))
    return img + torch.as_tensor(np.asarray(lighting, np.float32)).reshape(3, 1, 1)


def warp_u8(frame, trans_in, input_size, flip):
    """-> (inH, inW, 3) uint8: the reference's img[:, ::-1, :] and cv2.warpAffine"""
    inH, inW = input_size
    img = np.ascontiguousarray(frame[:, ::-1, :]) if flip else frame
    return preprocess_ref.warp_affine_u8(img, trans_in, (inW, inH))


def augment_frame(frame, trans_in, input_size, flip, order, factor, lighting, mean, std, colour=True, means=None):
    """frame (Hs,Ws,3) uint8, trans_in forward 2x3 -> (3,inH,inW) float32 ndarray"""
    w = warp_u8(frame, trans_in, input_size, flip)
    t = torch.from_numpy(w.transpose(2, 0, 1).copy()).to(torch.float32).div(255)                       # ToTensor
    if colour:
        t = colour_chain(t, order, factor, lighting, means)
    mean_t = torch.as_tensor(np.asarray(mean, np.float32)).reshape(3, 1, 1)
    std_t = torch.as_tensor(np.asarray(std, np.float32)).reshape(3, 1, 1)
    return t.sub(mean_t).div(std_t).numpy()                                                              # Normalize


def augment_images(frames, params, input_size, mean, std, colour=True, means=None):
    """frames (B,Hs,Ws,3) uint8 ndarray, params: an AugmentParams on the host -> (B,3,inH,inW) float32"""
    out = []
    for b in range(len(frames)):
        out.append(augment_frame(np.asarray(frames[b]), params.trans_in[b].numpy(), input_size, bool(params.flip[b]),
                                 params.order[b].tolist(), params.factor[b].numpy(), params.lighting[b].numpy(), mean, std,
                                 colour, means))
    return np.stack(out, 0)


def mean_margin(m64):
    """Relative distance of a float64 mean from the nearest fp32 rounding boundary (the midpoint of two neighbouring
    fp32 values): a device sum that differs from this one in the last bits of float64 rounds to the same fp32 as long as
    this stays far above 2^-52."""
    if m64 == 0.0:
        return np.inf
    m32 = np.float32(m64)
    lo = np.nextafter(m32, np.float32(-np.inf)).astype(np.float64)
    hi = np.nextafter(m32, np.float32(np.inf)).astype(np.float64)
    mid_lo, mid_hi = 0.5 * (lo + np.float64(m32)), 0.5 * (np.float64(m32) + hi)
    return min(abs(m64 - mid_lo), abs(m64 - mid_hi)) / abs(m64)
