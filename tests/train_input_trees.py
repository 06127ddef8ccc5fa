"""Synthetic DTU (Yao Yao's layout) and BlendedMVS trees for the training-dataset tests: PNG / JPG by PIL, PFM by
``data_io.save_pfm``, cam files and pair.txt.  Every writer returns what it stored, decoded again where the format is lossy."""
import os

import numpy as np

from effi_mvs_plus_amd.datasets import data_io


def cam_text(ext, k, last_line):
    rows = lambda m: "\n".join(" ".join(repr(float(v)) for v in r) for r in m)  # noqa: E731
    return f"extrinsic\n{rows(ext)}\n\nintrinsic\n{rows(k)}\n\n{last_line}\n"


def random_cam(rng):
    e = np.eye(4)
    e[:3, :3] = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    e[:3, 3] = rng.standard_normal(3) * 300
    k = np.array([[361.54, 0, 82.3], [0, 360.4, 61.9], [0, 0, 1]]) + rng.standard_normal((3, 3)) * 1e-3
    return e, k


def smooth_image(h, w, v):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([127 + 120 * np.sin(xx / (7.0 + v) + c) * np.cos(yy / (11.0 + c)) for c in range(3)], -1).astype(np.uint8)


def write_pairs(path, sources):
    """sources: {ref: [src ids]}"""
    with open(path, "w") as f:
        f.write(f"{len(sources)}\n")
        for ref, srcs in sources.items():
            f.write(f"{ref}\n{len(srcs)} " + " ".join(f"{u} {100.0 - u}" for u in srcs) + "\n")


def plant_mask_bytes(mask):
    """10 and 11 (the two sides of ``> 10``) in a quarter of the even raw positions (the half-size resize reads those) and at odd
    ones (nothing reads those)."""
    mask[0::4, 0::4] = 10
    mask[2::4, 0::4] = 11
    mask[1::2, 1::2][::3, ::3] = 11
    mask[1::2, 1::2][1::3, ::3] = 10
    return mask


def write_dtu_tree(root, scans, n_views, raw_hw, img_hw, lights=range(7), cams=None, depth_min=425.0, seed=0):
    """-> (listfile, {"imgs": {(scan, vid, light): uint8 [h,w,3]}, "depth": {(scan, vid): fp32 raw}, "mask": {(scan, vid): uint8 raw},
    "sources": {ref: [...]}}).  cams: optional list of (extrinsic, intrinsic) per view."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "Cameras", "train"), exist_ok=True)
    sources = {v: [(v + 1 + j) % n_views for j in range(n_views - 1)] for v in range(n_views)}
    write_pairs(os.path.join(root, "Cameras", "pair.txt"), sources)
    for v in range(n_views):
        e, k = cams[v] if cams is not None else random_cam(rng)
        with open(os.path.join(root, "Cameras", "train", f"{v:08d}_cam.txt"), "w") as f:
            f.write(cam_text(e, k, f"{depth_min} 2.5"))
    stored = {"imgs": {}, "depth": {}, "mask": {}, "sources": sources}
    for scan in scans:
        os.makedirs(os.path.join(root, "Rectified", f"{scan}_train"), exist_ok=True)
        os.makedirs(os.path.join(root, "Depths_raw", scan), exist_ok=True)
        for v in range(n_views):
            for light in lights:
                img = rng.integers(0, 256, size=(img_hw[0], img_hw[1], 3), dtype=np.uint8)
                Image.fromarray(img).save(os.path.join(root, "Rectified", f"{scan}_train", f"rect_{v + 1:03d}_{light}_r5000.png"))
                stored["imgs"][scan, v, light] = img
            depth = (depth_min + 500.0 * rng.random(raw_hw)).astype(np.float32)
            data_io.save_pfm(os.path.join(root, "Depths_raw", scan, f"depth_map_{v:04d}.pfm"), depth)
            mask = plant_mask_bytes(rng.integers(0, 256, size=raw_hw, dtype=np.uint8))
            Image.fromarray(mask).save(os.path.join(root, "Depths_raw", scan, f"depth_visual_{v:04d}.png"))
            stored["depth"][scan, v], stored["mask"][scan, v] = depth, mask
    listfile = os.path.join(root, "list.txt")
    with open(listfile, "w") as f:
        f.write("".join(s + "\n" for s in scans))
    return listfile, stored


def write_blend_tree(root, scans, n_views, hw, ranges=None, seed=0):
    """n_views >= 9: view 0 gets 6 sources (dropped by the < 7 rule), the others 7 or more.  ranges: {vid: (dmin, dmax)}, default
    one range for all.  -> (listfile, {"imgs": {(scan, vid): decoded uint8}, "depth": {(scan, vid): fp32}, "range": {vid: (lo, hi)},
    "sources": {...}})."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    sources = {v: [(v + 1 + j) % n_views for j in range(6 if v == 0 else 7 + v % 2)] for v in range(n_views)}
    stored = {"imgs": {}, "depth": {}, "range": {}, "sources": sources}
    for scan in scans:
        for sub in ("cams", "blended_images", "rendered_depth_maps"):
            os.makedirs(os.path.join(root, scan, sub), exist_ok=True)
        write_pairs(os.path.join(root, scan, "cams", "pair.txt"), sources)
        for v in range(n_views):
            lo, hi = (ranges or {}).get(v, (2.5, 11.75))
            stored["range"][v] = (lo, hi)
            e, k = random_cam(rng)
            with open(os.path.join(root, scan, "cams", f"{v:08d}_cam.txt"), "w") as f:
                f.write(cam_text(e, k, f"{lo!r} 0.05 128 {hi!r}"))
            p = os.path.join(root, scan, "blended_images", f"{v:08d}.jpg")
            Image.fromarray(smooth_image(hw[0], hw[1], v)).save(p, quality=95)
            stored["imgs"][scan, v] = np.array(Image.open(p))
            depth = (lo - 1.0 + (hi - lo + 2.0) * rng.random(hw)).astype(np.float32)          # some of it out of range
            depth[0, 0], depth[0, 8 % hw[1]], depth[1, 1] = lo, hi, np.nan
            data_io.save_pfm(os.path.join(root, scan, "rendered_depth_maps", f"{v:08d}.pfm"), depth)
            stored["depth"][scan, v] = depth
    listfile = os.path.join(root, "blend_list.txt")
    with open(listfile, "w") as f:
        f.write("".join(s + "\n" for s in scans))
    return listfile, stored
