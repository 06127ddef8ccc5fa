"""numpy restatement of the array part of the two training datasets' ``__getitem__`` (datasets/dtu_yao.py:70-125,186-206,
datasets/blend.py:97-101,186-243), written from the rules and not from the reference's text; it imports neither cv2 nor the
reference tree.  ``resize_nearest`` follows OpenCV's published INTER_NEAREST rule:
    sx = min(floor(x * (1 / (dst / src))), src - 1)      in double, per axis.
PARITY WITH cv2 ITSELF IS UNPINNED: cv2 is not installed where these tests run.
"""
import numpy as np

STAGES = ("stage1", "stage2", "stage3", "stage4")
DTU_SCALES = {"stage0": 0.25, "stage1": 0.5, "stage2": 1.0, "stage3": 2.0, "stage4": 4.0}
BLEND_DIVISORS = {"stage0": 16.0, "stage1": 8.0, "stage2": 4.0, "stage3": 2.0, "stage4": 1.0}


def nearest_index(dst, src):
    inv = 1.0 / (float(dst) / float(src))
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * inv).astype(np.int64), src - 1)


def resize_nearest(a, dst_w, dst_h):
    """cv2.resize(a, (dst_w, dst_h), interpolation=cv2.INTER_NEAREST) for a 2-D array."""
    return np.ascontiguousarray(a[nearest_index(dst_h, a.shape[0])][:, nearest_index(dst_w, a.shape[1])])


def pyramid(a):
    """{"stage1": /8, "stage2": /4, "stage3": /2, "stage4": a} by nearest resize."""
    h, w = a.shape
    return {"stage1": resize_nearest(a, w // 8, h // 8), "stage2": resize_nearest(a, w // 4, h // 4),
            "stage3": resize_nearest(a, w // 2, h // 2), "stage4": a}


def images(raws):
    """list of uint8 [h,w,3] -> [N,3,h,w] float32 = x / 255."""
    return np.stack([r.astype(np.float32) / np.float32(255.0) for r in raws]).transpose(0, 3, 1, 2)


def dtu_prepare(a, crop_hw):
    """Half-size nearest resize, then the centred crop."""
    h, w = a.shape
    half = resize_nearest(a, w // 2, h // 2)
    hh, hw_ = half.shape
    ch, cw = crop_hw
    sy, sx = (hh - ch) // 2, (hw_ - cw) // 2
    return np.ascontiguousarray(half[sy:sy + ch, sx:sx + cw])


def dtu_ground_truth(depth_full, mask_png_full, crop_hw):
    """-> (depth_ms, mask_ms): the mask is thresholded BEFORE it is resized, as a float image."""
    mask = (mask_png_full.astype(np.float32) > 10).astype(np.float32)
    return pyramid(dtu_prepare(depth_full.astype(np.float32), crop_hw)), pyramid(dtu_prepare(mask, crop_hw))


def blend_masks(depth_ms, depth_min, depth_max):
    """Per level, on that level's own depth; numpy compares a float32 array with the Python float rounded to float32."""
    lo, hi = np.float32(depth_min), np.float32(depth_max)
    with np.errstate(invalid="ignore"):
        return {k: ((d >= lo) & (d <= hi)).astype(np.float32) for k, d in depth_ms.items()}


def blend_ground_truth(depth, depth_min, depth_max):
    depth_ms = pyramid(depth.astype(np.float32))
    return depth_ms, blend_masks(depth_ms, depth_min, depth_max)


def read_cam(path):
    """cam.txt -> (intrinsic [3,3], extrinsic [4,4], floats of the depth line)."""
    lines = [ln.rstrip() for ln in open(path).readlines()]
    ext = np.array([float(v) for ln in lines[1:5] for v in ln.split()], dtype=np.float32).reshape(4, 4)
    k = np.array([float(v) for ln in lines[7:10] for v in ln.split()], dtype=np.float32).reshape(3, 3)
    return k, ext, [float(v) for v in lines[11].split()]


def projections(cam_paths, scales=None, divisors=None):
    mats = np.zeros((len(cam_paths), 2, 4, 4), dtype=np.float32)
    for i, p in enumerate(cam_paths):
        k, ext, _ = read_cam(p)
        mats[i, 0] = ext
        mats[i, 1, :3, :3] = k
    out = {}
    for name in (scales or divisors):
        m = mats.copy()
        m[:, 1, :2, :] = mats[:, 1, :2, :] * scales[name] if scales else mats[:, 1, :2, :] / divisors[name]
        out[name] = m
    return out


def dtu_depth_values(depth_min, ndepths, dispmaxfirst):
    interval = 2.5 * (1.06 / (float(ndepths) / 192.0))
    depth_max = interval * ndepths + depth_min
    if dispmaxfirst == "first":
        return np.linspace(1 / depth_min, 1 / depth_max, ndepths, dtype=np.float32)
    return np.linspace(1 / depth_max, 1 / depth_min, ndepths, dtype=np.float32)


def blend_depth_values(depth_min, depth_max, ndepths):
    return np.linspace(1 / depth_max, 1 / depth_min, ndepths, endpoint=False).astype(np.float32)
