"""Gipuma / fusibile depth-map fusion on the HIP path: ``--filter_method gipuma`` of the reference's drivers (``misc/gipuma.py``)
without the external ``fusibile`` executable, a CUDA program that cannot run here.

PARITY WITH THE EXTERNAL BINARY UNPINNED: neither ``fusibile``'s source nor a binary is available to this project and the reference
holds no fixtures of its output, so the fusion is the one DESIGN.md section 7.10 SPECIFIES -- the consistency fusion of Galliani et
al. 2015 as the MVSNet-family drivers configure it (fake normals and ``normal_thresh = 360``: the normal test is vacuous and is not
built).  What IS pinned to the reference, byte for byte, is every file-format function below (``tests/golden/g18_gipuma_io.npz``).

Device level: ``fuse_scan`` -- a scan's device-resident maps in, point cloud out, ready for ``dtu_eval.point_compare``.  The method is
ORDER DEPENDENT: reference views are fused one launch after the other (csrc/gipuma.hip, ``effi_fusion_gipuma_view_f32``) and a fused
point consumes the source pixels that supported it (``used``), so later reference views do not emit the same surface again.

File level: the reference's names with the reference's signatures -- ``read_gipuma_dmb``, ``write_gipuma_dmb``,
``mvsnet_to_gipuma_dmb``, ``mvsnet_to_gipuma_cam``, ``fake_gipuma_normal``, ``mvsnet_to_gipuma``, ``probability_filter``,
``read_camera_parameters`` -- plus ``depth_map_fusion`` and ``gipuma_filter``, which fuse on the device where the reference shells
out; ``fusibile_exe_path`` is accepted for the signature and never executed.
"""
from __future__ import annotations

import os
import shutil
from struct import pack, unpack

import numpy as np
import torch

from . import ops
from .datasets.data_io import read_pfm, save_pfm
from .dtu_fusion import read_camera_parameters, read_img, write_ply  # noqa: F401  (read_camera_parameters: misc/gipuma.py:12-22, the same function)
from .fusion import fuse_chunks

DEPTH_MIN, DEPTH_MAX = 0.001, 100000.0          # misc/gipuma.py:195-196
GIPUMA_PREFIX = "2333__"                        # misc/gipuma.py:147
PLY_SUBDIR = "consistencyCheck-hip"


# ---------------------------------------------------------------------------------------------------------------------------
# device level
# ---------------------------------------------------------------------------------------------------------------------------
def scan_rows(n_views, pair_data=None):
    """Host only: the ordered (reference view, ordered sources) list of a scan, checked.  ``pair_data=None``: every view is a
    reference view, in ascending id, with every other view as its sources in ascending id (fusibile's behaviour); otherwise the
    ``read_pair_file`` list in its own order.  ValueError for a view listed as its own source, an id outside [0, n_views), a
    reference view without a source or with more than 64."""
    if pair_data is None:
        pair_data = [(r, [s for s in range(n_views) if s != r]) for r in range(n_views)]
    rows = [(int(ref), ops.gipuma_check_sources(n_views, ref, srcs)) for ref, srcs in pair_data]
    if not rows:
        raise ValueError("gipuma: no reference view")
    return rows


@ops.on_tensor_device
def fuse_scan(depths, confidences, cams, images, pair_data=None, prob_threshold=0.5, disp_threshold=0.25, num_consistent=4, chunk=None,
              depth_min=DEPTH_MIN, depth_max=DEPTH_MAX):
    """The fusion of ``depth_map_fusion`` (misc/gipuma.py:192-213) for a WHOLE scan on the device (PARITY UNPINNED,
    module docstring).  depths [n_views,h,w]; confidences [n_views,h,w] or None (``probability_filter``: depth kept where confidence >
    prob_threshold); cams [n_views,2,4,4] (extrinsic; intrinsic in the top-left 3x3); images [n_views,h,w,3] fp32 in [0,1] or None
    (black vertices); ``pair_data``: see ``scan_rows`` -> dict(xyz [M,3] float32, rgb [M,3] uint8 -- reference views in list order,
    row-major survivors --, offsets [n_ref+1] int32, ref_ids, mask [n_ref,h,w] bool, count [n_ref,h,w] uint8 = consistent sources per
    pixel, used [n_views,h,w] bool = the consumed pixels).  The dense points of ``chunk`` reference views exist at a time (None: below
    400 MB); the flags live outside the chunk loop and the result does not depend on ``chunk``."""
    if depths.dim() != 3:
        raise ValueError(f"gipuma.fuse_scan: depths [n_views,h,w] expected, got {tuple(depths.shape)}")
    n_views, h, w = depths.shape
    rows = scan_rows(n_views, pair_data)
    dev = depths.device
    depths, cams = depths.contiguous(), cams.contiguous()
    if confidences is not None:
        depths = ops.fusion_gipuma_prob(depths, confidences.contiguous(), prob_threshold)
    images = torch.zeros(n_views, h, w, 3, device=dev, dtype=torch.float32) if images is None else images.contiguous()
    used = torch.zeros(n_views, h, w, device=dev, dtype=torch.uint8)
    n_ref = len(rows)
    chunk = max(1, (1 << 25) // (h * w)) if chunk is None else int(chunk)
    chunk = max(1, min(chunk, n_ref))
    # the averaged colours of a chunk are the compaction's "images": row r of a chunk takes colour map r - r0 (an identity row table)
    colours = torch.empty(chunk, h, w, 3, device=dev, dtype=torch.float32)
    table = (torch.arange(n_ref, dtype=torch.int32) % chunk).reshape(n_ref, 1)

    def filter_chunk(t_, r0, r1):
        res = []
        for i in range(r0, r1):
            r = ops.fusion_gipuma_view(depths, cams, images, rows[i][0], rows[i][1], used, disp_threshold, num_consistent, depth_min, depth_max)
            colours[i - r0].copy_(r["colour"])
            res.append(r)
        return {k: torch.stack([r[k] for r in res]) for k in ("mask", "points", "count")}

    out = fuse_chunks(table, filter_chunk, colours, "hwc", chunk, ("mask", "count"))
    return {"xyz": out["xyz"], "rgb": out["rgb"], "offsets": out["offsets"], "ref_ids": [ref for ref, _ in rows],
            "mask": out["mask"].bool(), "count": out["count"], "used": used.bool()}


# ---------------------------------------------------------------------------------------------------------------------------
# file level: the reference's formats
# ---------------------------------------------------------------------------------------------------------------------------
def read_gipuma_dmb(path):
    """misc/gipuma.py:25-36: Gipuma .dmb image -> [h,w] or [h,w,c] float32."""
    with open(path, "rb") as fid:
        unpack("<i", fid.read(4))[0]                     # image type
        height = unpack("<i", fid.read(4))[0]
        width = unpack("<i", fid.read(4))[0]
        channel = unpack("<i", fid.read(4))[0]
        array = np.fromfile(fid, np.float32)
    array = array.reshape((width, height, channel), order="F")
    return np.transpose(array, (1, 0, 2)).squeeze()


def write_gipuma_dmb(path, image):
    """misc/gipuma.py:39-60.  A 3-channel image is written PLANAR ([c][h][w], the reference's transpose), which ``read_gipuma_dmb``
    does not undo: the reference only writes such files (the fake normals), it never reads them back."""
    image_shape = np.shape(image)
    width, height = image_shape[1], image_shape[0]
    channels = image_shape[2] if len(image_shape) == 3 else 1
    if len(image_shape) == 3:
        image = np.transpose(image, (2, 0, 1)).squeeze()
    with open(path, "wb") as fid:
        fid.write(pack("<i", 1))
        fid.write(pack("<i", height))
        fid.write(pack("<i", width))
        fid.write(pack("<i", channels))
        image.tofile(fid)


def mvsnet_to_gipuma_dmb(in_path, out_path):
    """misc/gipuma.py:63-69: .pfm -> .dmb."""
    image, _ = read_pfm(in_path)
    write_gipuma_dmb(out_path, image)


def mvsnet_to_gipuma_cam(in_path, out_path):
    """misc/gipuma.py:72-92: ``_cam.txt`` -> the 3x4 projection matrix K [R|t] as text, ``str(float64)`` per entry (the product of the
    float64-padded intrinsic with the float32 extrinsic is formed in float64)."""
    intrinsic, extrinsic = read_camera_parameters(in_path)
    intrinsic_new = np.zeros((4, 4))
    intrinsic_new[:3, :3] = intrinsic
    projection_matrix = np.matmul(intrinsic_new, extrinsic)[0:3][:]
    with open(out_path, "w") as f:
        for i in range(0, 3):
            for j in range(0, 4):
                f.write(str(projection_matrix[i][j]) + " ")
            f.write("\n")
        f.write("\n")


def fake_gipuma_normal(in_depth_path, out_normal_path):
    """misc/gipuma.py:95-113: the constant normal (1, 1, 1) / 1.732050808 where the depth is positive, 0 elsewhere."""
    depth_image = read_gipuma_dmb(in_depth_path)
    image_shape = np.shape(depth_image)
    normal_image = np.ones_like(depth_image)
    normal_image = np.reshape(normal_image, (image_shape[0], image_shape[1], 1))
    normal_image = np.tile(normal_image, [1, 1, 3])
    normal_image = normal_image / 1.732050808
    mask_image = np.squeeze(np.where(depth_image > 0, 1, 0))
    mask_image = np.reshape(mask_image, (image_shape[0], image_shape[1], 1))
    mask_image = np.tile(mask_image, [1, 1, 3])
    mask_image = np.float32(mask_image)
    normal_image = np.float32(np.multiply(normal_image, mask_image))
    write_gipuma_dmb(out_normal_path, normal_image)


def _image_names(image_folder):
    return [i for i in os.listdir(image_folder) if not i.startswith(".")]


def mvsnet_to_gipuma(dense_folder, gipuma_point_folder):
    """misc/gipuma.py:116-157: cameras as .P files, the images copied, per view ``2333__<prefix>/disp.dmb`` from the probability-filtered
    depth and ``normals.dmb`` with the fake normals."""
    image_folder = os.path.join(dense_folder, "images")
    cam_folder = os.path.join(dense_folder, "cams")
    gipuma_cam_folder = os.path.join(gipuma_point_folder, "cams")
    gipuma_image_folder = os.path.join(gipuma_point_folder, "images")
    for d in (gipuma_point_folder, gipuma_cam_folder, gipuma_image_folder):
        if not os.path.isdir(d):
            os.mkdir(d)
    image_names = _image_names(image_folder)
    for image_name in image_names:
        image_prefix = os.path.splitext(image_name)[0]
        mvsnet_to_gipuma_cam(os.path.join(cam_folder, image_prefix + "_cam.txt"), os.path.join(gipuma_cam_folder, image_name + ".P"))
    for image_name in image_names:
        shutil.copy(os.path.join(image_folder, image_name), os.path.join(gipuma_image_folder, image_name))
    for image_name in image_names:
        image_prefix = os.path.splitext(image_name)[0]
        sub_depth_folder = os.path.join(gipuma_point_folder, GIPUMA_PREFIX + image_prefix)
        if not os.path.isdir(sub_depth_folder):
            os.mkdir(sub_depth_folder)
        out_depth_dmb = os.path.join(sub_depth_folder, "disp.dmb")
        mvsnet_to_gipuma_dmb(os.path.join(dense_folder, "depth_est", image_prefix + "_prob_filtered.pfm"), out_depth_dmb)
        fake_gipuma_normal(out_depth_dmb, os.path.join(sub_depth_folder, "normals.dmb"))


def probability_filter(dense_folder, prob_threshold):
    """misc/gipuma.py:160-189: ``depth_est/<prefix>.pfm`` with the pixels of ``confidence/<prefix>.pfm`` not above the threshold zeroed
    -> ``depth_est/<prefix>_prob_filtered.pfm``."""
    for image_name in _image_names(os.path.join(dense_folder, "images")):
        image_prefix = os.path.splitext(image_name)[0]
        depth_map, _ = read_pfm(os.path.join(dense_folder, "depth_est", image_prefix + ".pfm"))
        prob_map, _ = read_pfm(os.path.join(dense_folder, "confidence", image_prefix + ".pfm"))
        depth_map = np.array(depth_map)
        depth_map[~(prob_map > prob_threshold)] = 0
        save_pfm(os.path.join(dense_folder, "depth_est", image_prefix + "_prob_filtered.pfm"), depth_map)


def decompose_projection(P):
    """Host only: P = K [R|t] (3x4, as ``mvsnet_to_gipuma_cam`` writes it) -> (K [3,3], R [3,3], t [3]) by an RQ decomposition of
    P[:, :3] in float64.  Sign convention: the diagonal of K is positive, K[2,2] is normalised to 1 (P is defined up to scale) and
    det R = +1 (a P whose scale is negative is negated as a whole)."""
    P = np.asarray(P, np.float64).reshape(3, 4)
    M = P[:, :3]
    q, r = np.linalg.qr(np.flipud(M).T)
    K, R = np.fliplr(np.flipud(r.T)), np.flipud(q.T)                  # M = K R, K upper triangular
    D = np.diag(np.where(np.diag(K) < 0, -1.0, 1.0))
    K, R = K @ D, D @ R
    t = np.linalg.solve(K, P[:, 3])
    if np.linalg.det(R) < 0:
        R, t = -R, -t
    return K / K[2, 2], R, t


def _cam_array(K, E):
    cam = np.zeros((2, 4, 4), np.float32)
    cam[0], cam[1, :3, :3] = E, K
    return cam


def _fuse_and_write(depths, cams, images, ply_path, disp_threshold, num_consistent, device):
    h, w = depths[0].shape
    for im in images:
        if im.shape[:2] != (h, w):
            raise ValueError(f"gipuma: image of size {im.shape[:2]} for depth maps of size {(h, w)}; resize the images first")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.stack(a), dtype=np.float32)).to(device)
    r = fuse_scan(t(depths), None, t(cams), t(images), None, 0.0, float(disp_threshold), int(num_consistent))
    os.makedirs(os.path.dirname(ply_path), exist_ok=True)
    write_ply(ply_path, r["xyz"].cpu().numpy(), r["rgb"].cpu().numpy())
    return ply_path


def depth_map_fusion(point_folder, fusibile_exe_path=None, disp_thresh=0.25, num_consistent=4, color=True, device="cuda"):
    """misc/gipuma.py:192-213 without the external program: fuses a folder ``mvsnet_to_gipuma`` wrote -- ``cams/<image>.P``,
    ``images/<image>``, ``2333__<prefix>/disp.dmb`` -- on the device, views in ascending name order, every other view a source, and
    writes ``<point_folder>/consistencyCheck-hip/final3d_model.ply`` -> its path.  ``fusibile_exe_path`` is never executed."""
    names = sorted(_image_names(os.path.join(point_folder, "images")))
    depths, cams, images = [], [], []
    for name in names:
        K, R, t = decompose_projection(np.loadtxt(os.path.join(point_folder, "cams", name + ".P")))
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = R, t
        cams.append(_cam_array(K, E))
        depths.append(read_gipuma_dmb(os.path.join(point_folder, GIPUMA_PREFIX + os.path.splitext(name)[0], "disp.dmb")))
        images.append(read_img(os.path.join(point_folder, "images", name)) if color else np.zeros(depths[-1].shape + (3,), np.float32))
    return _fuse_and_write(depths, cams, images, os.path.join(point_folder, PLY_SUBDIR, "final3d_model.ply"), disp_thresh, num_consistent,
                           device)


def gipuma_filter(testlist, outdir, prob_threshold, disp_threshold, num_consistent, fusibile_exe_path=None, device="cuda"):
    """misc/gipuma.py:216-236 for every scan of ``testlist``: ``probability_filter`` as the reference runs it (writes
    ``*_prob_filtered.pfm``), then the fusion on the device from ``<outdir>/<scan>/{images,cams,depth_est}``, views in ascending name
    order, every other view a source -> ``<outdir>/<scan>/points_mvsnet/consistencyCheck-hip/final3d_model.ply``.  Images whose size
    differs from the depth maps are refused.  ``fusibile_exe_path`` is never executed."""
    plys = []
    for scan in testlist:
        dense_folder = os.path.join(outdir, scan)
        point_folder = os.path.join(dense_folder, "points_mvsnet")
        if not os.path.isdir(point_folder):
            os.mkdir(point_folder)
        probability_filter(dense_folder, prob_threshold)
        depths, cams, images = [], [], []
        for name in sorted(_image_names(os.path.join(dense_folder, "images"))):
            prefix = os.path.splitext(name)[0]
            K, E = read_camera_parameters(os.path.join(dense_folder, "cams", prefix + "_cam.txt"))
            cams.append(_cam_array(K, E))
            depths.append(read_pfm(os.path.join(dense_folder, "depth_est", prefix + "_prob_filtered.pfm"))[0])
            images.append(read_img(os.path.join(dense_folder, "images", name)))
        plys.append(_fuse_and_write(depths, cams, images, os.path.join(point_folder, PLY_SUBDIR, "final3d_model.ply"), disp_threshold,
                                    num_consistent, device))
    return plys
