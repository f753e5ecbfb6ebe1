"""Correction-click samplers -- sam2_video/model/modeling/sam2_utils.py:202-323 of the reference under its names
and signatures: sample_random_points_from_errors, sample_one_point_from_error_center (the RITM clicker) and
get_next_point.

The reference's centre sampler copies, per object, two full-resolution masks to the host, pads them, runs
cv2.distanceTransform twice and takes an argmax; its uniform sampler draws B * num_pt * H * W * 2 random floats
to pick one pixel.  Here both run on csrc/clicks.hip (`on_device=True`): the exact squared Euclidean distance
transform with the argmax fused in, and a rank selection among the error pixels; only the clicks exist as output.
`on_device=False` is the host twin on numpy / scipy, which computes the same integer definitions, so both paths
return equal tensors.

Definitions ("Correction clicks"): D2 is the squared distance to the nearest pixel that is clear
or outside the image, i.e. the square of cv2.distanceTransform(pad(mask, 1), DIST_L2, 0)[1:-1, 1:-1]; the argmax
of D2 is the argmax of the reference's float32 distances because sqrt is strictly increasing on the integers
below 2^22, which H, W <= 4092 guarantees.  That OpenCV's precise mode is the exact transform rests on its
documentation, not on a comparison (cv2 is not a dependency of this package).

Departures: padding=False raises (the unpadded transform of a mask without background is an artefact of
cv2, and get_next_point never asks for it); the uniform sampler has the reference's distribution -- one uniformly
random pixel of the error regions per click -- but not its random stream: it draws one 32-bit integer r per click
and takes the (r * n) >> 32 -th of the n candidates in row-major order.  sample_box_points (training-time box
jitter) is not restated."""
import numpy as np
import torch

MAX_SIDE = 4092  # csrc/clicks.h CK_MAX_SIDE


def _check(gt_masks, pred_masks):
    assert gt_masks.dtype == torch.bool and gt_masks.dim() == 4 and gt_masks.size(1) == 1
    if pred_masks is not None:
        assert pred_masks.dtype == torch.bool and pred_masks.shape == gt_masks.shape
    B, _, H, W = gt_masks.shape
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE and H * W <= 1 << 24):
        raise ValueError(f"masks of {H} x {W}: both sides must be in [1, {MAX_SIDE}] and H * W <= 2^24")
    return B, H, W


def _bytes(masks, B, H, W):
    """bool [B, 1, H, W] -> uint8 [B, H, W] sharing the storage when it is contiguous"""
    return None if masks is None else masks.reshape(B, H, W).contiguous().view(torch.uint8)


def _edt_sq_host(mask):
    """D2 of one bool [H, W] numpy mask: rint(e^2) of scipy's exact transform of the padded mask (e^2 is an
    integer below 2^22 up to float64 rounding)"""
    from scipy import ndimage
    e = ndimage.distance_transform_edt(np.pad(mask, 1))[1:-1, 1:-1]
    return np.rint(e * e).astype(np.int64)


def sample_one_point_from_error_center(gt_masks, pred_masks, padding=True, on_device=True):
    """The point with the largest distance to the boundary of the larger error region, per mask.

    gt_masks: [B, 1, H, W] bool; pred_masks: the same or None (empty prediction).
    -> points [B, 1, 2] float32 (x, y), labels [B, 1] int32 (1: in the missed region FN = gt & ~pred, 0: in the
    wrongly predicted region FP = ~gt & pred), both on gt_masks.device.  The first pixel in row-major order wins
    a tie inside a region, FP wins a tie between the regions, no error at all gives (0, 0) with label 0."""
    if not padding:
        raise NotImplementedError("sample_one_point_from_error_center(padding=False) is not restated: "
                                  "get_next_point always pads")
    B, H, W = _check(gt_masks, pred_masks)
    device = gt_masks.device
    if on_device:
        from ...kernels import ops
        points, labels, _ = ops.error_center_click(_bytes(gt_masks, B, H, W), _bytes(pred_masks, B, H, W))
        return points.view(B, 1, 2), labels.view(B, 1)
    gt = gt_masks.reshape(B, H, W).cpu().numpy()
    pred = np.zeros_like(gt) if pred_masks is None else pred_masks.reshape(B, H, W).cpu().numpy()
    points = np.zeros((B, 1, 2), np.float32)
    labels = np.zeros((B, 1), np.int32)
    for b in range(B):
        fn_d2 = _edt_sq_host(gt[b] & ~pred[b]).reshape(-1)
        fp_d2 = _edt_sq_host(~gt[b] & pred[b]).reshape(-1)
        fn_argmax, fp_argmax = np.argmax(fn_d2), np.argmax(fp_d2)
        is_positive = fn_d2[fn_argmax] > fp_d2[fp_argmax]
        idx = fn_argmax if is_positive else fp_argmax
        points[b, 0] = (idx % W, idx // W)
        labels[b, 0] = int(is_positive)
    return torch.from_numpy(points).to(device), torch.from_numpy(labels).to(device)


def sample_random_points_from_errors(gt_masks, pred_masks, num_pt=1, generator=None, on_device=True):
    """`num_pt` points drawn independently and uniformly from the error regions, per mask.

    gt_masks: [B, 1, H, W] bool; pred_masks: the same or None (empty prediction); generator: a torch.Generator
    of gt_masks.device or None (the device's default generator).
    -> points [B, num_pt, 2] float32 (x, y), labels [B, num_pt] int32: 0 for a pixel of FP -- or of the
    background when the prediction is entirely correct --, 1 for a pixel of FN.  Nothing to draw from (gt covers
    the image and the prediction equals it) gives (0, 0) with label 0."""
    assert num_pt >= 0
    B, H, W = _check(gt_masks, pred_masks)
    device = gt_masks.device
    r = torch.randint(0, 2 ** 32, (B, num_pt), dtype=torch.int64, device=device, generator=generator)
    if on_device:
        from ...kernels import ops
        points, labels, _ = ops.error_uniform_click(_bytes(gt_masks, B, H, W), _bytes(pred_masks, B, H, W), r)
        return points, labels
    gt = gt_masks.reshape(B, H * W).cpu().numpy()
    pred = np.zeros_like(gt) if pred_masks is None else pred_masks.reshape(B, H * W).cpu().numpy()
    draws = r.cpu().numpy()
    points = np.zeros((B, num_pt, 2), np.float32)
    labels = np.zeros((B, num_pt), np.int32)
    for b in range(B):
        fn = gt[b] & ~pred[b]
        all_correct = bool((gt[b] == pred[b]).all())
        union = np.flatnonzero(fn | (~gt[b] & pred[b]) | (all_correct & ~gt[b]))
        n = len(union)
        for k in range(num_pt if n else 0):
            idx = int(union[(int(draws[b, k]) * n) >> 32])
            points[b, k] = (idx % W, idx // W)
            labels[b, k] = int(fn[idx])
    return torch.from_numpy(points).to(device), torch.from_numpy(labels).to(device)


def get_next_point(gt_masks, pred_masks, method, generator=None, on_device=True):
    """the next corrective click per mask: "uniform" (anywhere in the error) or "center" (the RITM clicker)"""
    if method == "uniform":
        return sample_random_points_from_errors(gt_masks, pred_masks, generator=generator, on_device=on_device)
    elif method == "center":
        return sample_one_point_from_error_center(gt_masks, pred_masks, on_device=on_device)
    else:
        raise ValueError(f"unknown sampling method {method}")
