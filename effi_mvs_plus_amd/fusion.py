"""Depth-map filtering + fusion on the HIP path: the functions of the reference's
``misc/fusion.py`` that the Tanks-and-Temples driver calls (``test_tank.py:455-571``) under their own names and signatures --
``get_pixel_grids``, ``bin_op_reduce``, ``idx_img2cam``, ``idx_cam2world``, ``idx_world2cam``, ``idx_cam2img``,
``get_reproj_dynamic``, ``vis_filter_dynamic`` -- so that ``import effi_mvs_plus_amd.fusion as fusion`` lets the driver's lines
486-509 run unchanged; each is one kernel of csrc/fusion.hip behind the C ABI.  ``dynamic_filter`` is the same block of the driver
as ONE fused kernel per reference view (no ``[n,v,3,h,w]`` intermediates), what bench.py times.  ``dynamic_filter_scan`` is the
driver's whole loop over a scan's reference views -- depth maps of a scan in, point cloud out -- in scan-batched launches with the
survivors compacted on the device.  CUDA (ROCm) fp32 tensors only; no CPU fallback.

The module's other filter, the FIXED-threshold visibility fusion of Vis-MVSNet (``misc/fusion.py:50-115``), is here under the
reference's names and signatures too: ``project_img``, ``prob_filter``, ``get_reproj``, ``vis_filter``, ``ave_fusion``.
``static_filter`` is their composition as ONE fused kernel per reference view and ``static_filter_scan`` the scan-level form
(depth maps of a scan in, point cloud out), the twins of ``dynamic_filter`` / ``dynamic_filter_scan``.

Not mirrored: ``vis_filter_dynamic_open3d``, ``filter_depth``, ``generate_points_from_depth`` and ``homo_warping``
(``misc/fusion.py:185-311``).  ``filter_depth`` ends without a ``return``, so that family cannot run in the reference either.
"""
from __future__ import annotations

from typing import List

import torch

from . import ops


def get_pixel_grids(height, width):
    """misc/fusion.py:8-13 -> [h,w,3,1] homogeneous pixel centres (x + 0.5, y + 0.5, 1) on the current CUDA device (the reference
    calls ``.cuda()``).  Index arithmetic only: plain tensor construction."""
    dev = torch.device("cuda", torch.cuda.current_device())
    grid = torch.ones(height, width, 3, 1, dtype=torch.float32, device=dev)
    grid[:, :, 0, 0] = torch.arange(width, dtype=torch.float32, device=dev).add_(0.5).view(1, width)
    grid[:, :, 1, 0] = torch.arange(height, dtype=torch.float32, device=dev).add_(0.5).view(height, 1)
    return grid


def bin_op_reduce(lst: List, func):
    """misc/fusion.py:16-20."""
    result = lst[0]
    for i in range(1, len(lst)):
        result = func(result, lst[i])
    return result


@ops.on_tensor_device
def idx_img2cam(idx_img_homo, depth, cam):  # nhw31, n1hw -> nhw41
    """misc/fusion.py:23-28: K^-1 . pixel, normalised by its z (+1e-9), times depth; homogeneous 1 appended."""
    return ops.fusion_points(ops.FUSION_IMG2CAM, idx_img_homo.contiguous(), cam.contiguous(), depth.contiguous())


@ops.on_tensor_device
def idx_cam2world(idx_cam_homo, cam):  # nhw41 -> nhw41
    """misc/fusion.py:31-34: E^-1 . point, normalised by its w (+1e-9)."""
    return ops.fusion_points(ops.FUSION_CAM2WORLD, idx_cam_homo.contiguous(), cam.contiguous())


@ops.on_tensor_device
def idx_world2cam(idx_world_homo, cam):  # nhw41 -> nhw41
    """misc/fusion.py:37-40."""
    return ops.fusion_points(ops.FUSION_WORLD2CAM, idx_world_homo.contiguous(), cam.contiguous())


@ops.on_tensor_device
def idx_cam2img(idx_cam_homo, cam):  # nhw41 -> nhw31
    """misc/fusion.py:43-47."""
    return ops.fusion_points(ops.FUSION_CAM2IMG, idx_cam_homo.contiguous(), cam.contiguous())


@ops.on_tensor_device
def get_reproj_dynamic(ref_depth, srcs_depth, ref_cam, srcs_cam):
    """misc/fusion.py:117-156.  ref_depth [n,1,h,w]; srcs_depth [n,v,1,h,w]; ref_cam [n,2,4,4]; srcs_cam [n,v,2,4,4]
    -> (reproj_xyd [n,v,3,h,w], ref_idx_cam [n*v,h,w,4,1], src2ref_idx_cam [n*v,h,w,4,1]) like the reference.

    ``reproj_xyd`` (x, y in reference pixels, depth in the reference camera) comes from the fused kernel.  The two point tensors
    are by-products the reference's caller only forwards to ``vis_filter_dynamic``, which ignores them; ``ref_idx_cam`` is
    ``idx_img2cam`` of the pixel grid, ``src2ref_idx_cam`` is rebuilt from the reprojected pixel and depth (K_ref^-1 . [x, y, 1] . d),
    which equals the reference's chain to fp32 rounding (~1e-6 relative), not bitwise."""
    n, v, _, h, w = srcs_depth.shape
    outs = []
    for b in range(n):
        r = ops.fusion_dynamic_filter(ref_depth[b, 0].contiguous(), srcs_depth[b, :, 0].contiguous(), ref_cam[b].contiguous(),
                                      srcs_cam[b].contiguous(), dh_view_num=1, want_points=False, want_reproj=True)
        outs.append(r["reproj_xyd"])
    reproj = torch.stack(outs)
    ref_cam_r = ref_cam[:, None].expand(n, v, 2, 4, 4).reshape(n * v, 2, 4, 4)          # every (sample, source view) pair sees its reference camera
    ref_depth_f = ref_depth[:, None].expand(n, v, 1, h, w).reshape(n * v, 1, h, w)
    ref_idx_cam = idx_img2cam(get_pixel_grids(h, w)[None], ref_depth_f, ref_cam_r)
    rp = reproj.view(n * v, 3, h, w)
    back_pix = torch.stack([rp[:, 0], rp[:, 1], torch.ones_like(rp[:, 0])], dim=-1).unsqueeze(-1)
    src2ref_idx_cam = idx_img2cam(back_pix, rp[:, 2:3].contiguous(), ref_cam_r)
    return reproj, ref_idx_cam, src2ref_idx_cam


@ops.on_tensor_device
def vis_filter_dynamic(ref_depth, reproj_xyd, ref_idx_world, src2ref_idx_cam, dist_base=4, rel_diff_base=1300, thres_view=2,
                       relative=False):
    """misc/fusion.py:157-181 -> (masks [n,v,v+1-thres_view,h,w] bool, mask = the loosest threshold's plane [n,v,1,h,w]).
    ``ref_idx_world`` and ``src2ref_idx_cam`` are accepted and, as in the reference (:161-165: only reshaped), do not enter the result."""
    masks = ops.fusion_vis_filter(ref_depth.contiguous(), reproj_xyd.contiguous(), dist_base, rel_diff_base, thres_view, relative).bool()
    return masks, masks[:, :, -1:, :, :]


def _filter_samples(op, ref_depth, src_depths, ref_cam, src_cams, ref_conf, *params):
    """What ``dynamic_filter`` and ``static_filter`` share: one launch of the single-view ``op`` per sample, results stacked."""
    n = ref_depth.shape[0]
    res = [op(ref_depth[b, 0].contiguous(), src_depths[b, :, 0].contiguous(), ref_cam[b].contiguous(), src_cams[b].contiguous(),
              None if ref_conf is None else ref_conf[b].contiguous(), *params) for b in range(n)]
    out = {"depth": torch.stack([r["depth"] for r in res]).unsqueeze(1), "points": torch.stack([r["points"] for r in res])}
    for k in ("geo_mask", "prob_mask", "mask"):
        out[k] = torch.stack([r[k] for r in res]).unsqueeze(1).bool()
    return out


@ops.on_tensor_device
def dynamic_filter(ref_depth, src_depths, ref_cam, src_cams, ref_conf, prob_threshold, dh_view_num, dist_filter, depth_filter,
                   relative=False):
    """The tensor part of ``dynamic_filter_depth`` (test_tank.py:466-512) for a batch of reference views as ONE kernel each:
    -> dict(depth [n,1,h,w] averaged depth, geo_mask / prob_mask / mask [n,1,h,w] bool, points [n,3,h,w])."""
    return _filter_samples(ops.fusion_dynamic_filter, ref_depth, src_depths, ref_cam, src_cams, ref_conf, prob_threshold, dh_view_num,
                           dist_filter, depth_filter, relative)


@ops.on_tensor_device
def project_img(src_img, dst_depth, src_cam, dst_cam, height=None, width=None):  # nchw, n1hw -> nchw, n1hw
    """misc/fusion.py:50-65 -> (warped_img [n,c,height,width], in_range [n,1,height,width] as 0/1 in the image's dtype): the source
    image sampled (bilinear, zeros, align_corners=True) where the destination pixels of depth ``dst_depth`` fall in the source view.
    The projection is normalised by ``width`` / ``height`` (not minus one) and clamped to +-1.1, as the reference does."""
    return ops.fusion_project_img(src_img.contiguous(), dst_depth.contiguous(), src_cam.contiguous(), dst_cam.contiguous(), height, width)


@ops.on_tensor_device
def prob_filter(ref_prob, prob_thresh, greater=True):  # n31hw -> n1hw
    """misc/fusion.py:68-76: the AND over the channels of ``ref_prob[:, [i]] > prob_thresh[i]`` -> bool [n,1,1,h,w] for ref_prob
    [n,c,1,h,w].  ``greater`` is accepted and ignored, as in the reference."""
    mask = ops.fusion_prob_filter(ref_prob.contiguous(), prob_thresh)
    return None if mask is None else mask.bool()


@ops.on_tensor_device
def get_reproj(ref_depth, srcs_depth, ref_cam, srcs_cam):  # n1hw, nv1hw -> n1hw
    """misc/fusion.py:79-96 -> (reproj_xyd [n,v,3,h,w], in_range [n,v,1,h,w]): per reference pixel and source view, the source
    view's pixels mapped into the reference view (x, y, depth), sampled at the reference pixel's projection.  The by-products of the
    fused kernel (``ops.fusion_static_filter``), one launch per sample."""
    n, v, _, h, w = srcs_depth.shape
    xyd, rng = [], []
    for b in range(n):
        r = ops.fusion_static_filter(ref_depth[b, 0].contiguous(), srcs_depth[b, :, 0].contiguous(), ref_cam[b].contiguous(),
                                     srcs_cam[b].contiguous(), want_points=False, want_reproj=True)
        xyd.append(r["reproj_xyd"]), rng.append(r["in_range"])
    return torch.stack(xyd), torch.stack(rng).unsqueeze(2)


@ops.on_tensor_device
def vis_filter(ref_depth, reproj_xyd, in_range, img_dist_thresh, depth_thresh, vthresh):
    """misc/fusion.py:99-110 -> (masks [n,v,1,h,w] 0/1 in ref_depth's dtype, mask [n,1,h,w] bool = sum_v masks >= vthresh - 1.1).
    ``in_range`` is accepted and, as in the reference (:106 overwrites it with ones), does not enter the result."""
    masks, mask = ops.fusion_static_vis_filter(ref_depth.contiguous(), reproj_xyd.contiguous(), img_dist_thresh, depth_thresh, vthresh)
    return masks, mask.bool()


@ops.on_tensor_device
def ave_fusion(ref_depth, reproj_xyd, masks):
    """misc/fusion.py:113-115 -> [n,1,h,w]: (sum_v d * masks + ref_depth) / (sum_v masks + 1)."""
    return ops.fusion_static_ave(ref_depth.contiguous(), reproj_xyd.contiguous(), masks.to(ref_depth.dtype).contiguous())


@ops.on_tensor_device
def static_filter(ref_depth, src_depths, ref_cam, src_cams, ref_conf, prob_threshold, img_dist_thresh, depth_thresh, vthresh):
    """``get_reproj`` + ``vis_filter`` + ``ave_fusion`` with the driver's photometric mask and points (test_tank.py:471-475,512-515)
    for a batch of reference views as ONE kernel each; shapes as ``dynamic_filter``, ref_conf [n,H,W] or None
    -> dict(depth [n,1,h,w] = ave_fusion, geo_mask = vis_filter's mask, prob_mask, mask = their AND [n,1,h,w] bool, points [n,3,h,w])."""
    return _filter_samples(ops.fusion_static_filter, ref_depth, src_depths, ref_cam, src_cams, ref_conf, prob_threshold, img_dist_thresh,
                           depth_thresh, vthresh)


def pair_table(pair_data):
    """Host only: the ``read_pair_file`` list [(ref_view, [src_views...]), ...] -> int32 CPU tensor [n_ref, 1 + v_max] (reference id,
    source ids, -1 padding), the table the scan launches index a scan's depth maps and cameras with."""
    return ops.fusion_pair_table(pair_data)


def fuse_chunks(table, filter_chunk, images, layout, chunk, mask_keys):
    """The chunk loop both scan drivers share.  ``filter_chunk(rows, r0, r1)`` runs the scan-batched filter on table rows r0:r1 and
    returns its dict (``mask`` = the final mask, ``points``); every chunk's survivors are compacted in order, so the dense points of
    only one chunk exist at a time and the result does not depend on ``chunk``."""
    n_ref = table.shape[0]
    h, w = images.shape[1:3] if layout == "hwc" else images.shape[2:4]
    if chunk is None:
        chunk = max(1, (1 << 25) // (h * w))                    # <= 400 MB of dense points per chunk
    chunk = max(1, min(int(chunk), n_ref))
    xyz, rgb, offs, kept, total = [], [], [], {k: [] for k in mask_keys}, 0
    for r0 in range(0, n_ref, chunk):
        rows = table[r0:r0 + chunk].contiguous()
        r = filter_chunk(rows, r0, r0 + rows.shape[0])
        x, c, o = ops.fusion_compact(r["mask"], r["points"], images, layout, rows)
        xyz.append(x), rgb.append(c), offs.append(o[:-1] + total)
        total += x.shape[0]
        for k in mask_keys:
            kept[k].append(r[k])
    offs.append(torch.tensor([total], dtype=torch.int32, device=images.device))
    out = {"xyz": torch.cat(xyz), "rgb": torch.cat(rgb), "offsets": torch.cat(offs)}
    for k in mask_keys:
        out[k] = torch.cat(kept[k])
    return out


def _filter_scan(op, rows, depths, confidences, cams, images, chunk, *params):
    """What ``dynamic_filter_scan`` and ``static_filter_scan`` share: the scan-batched ``op`` over the kept ``rows`` of the pair list,
    chunk by chunk, survivors compacted."""
    dev = depths.device
    if not rows:
        h, w = depths.shape[-2:]
        z = lambda *sh, dt=torch.float32: torch.empty(*sh, device=dev, dtype=dt)
        return {"xyz": z(0, 3), "rgb": z(0, 3, dt=torch.uint8), "offsets": torch.zeros(1, dtype=torch.int32, device=dev), "ref_ids": [],
                "depth": z(0, h, w), "prob_mask": z(0, h, w, dt=torch.bool), "geo_mask": z(0, h, w, dt=torch.bool),
                "mask": z(0, h, w, dt=torch.bool)}
    table = pair_table(rows)
    depths, cams, images = depths.contiguous(), cams.contiguous(), images.contiguous()

    def filter_chunk(t_, r0, r1):
        conf = None if confidences is None else confidences[t_[:, 0].long().to(dev)].contiguous()
        return op(depths, cams, t_, conf, *params)

    out = fuse_chunks(table, filter_chunk, images, "chw", chunk, ("depth", "prob_mask", "geo_mask", "mask"))
    for k in ("prob_mask", "geo_mask", "mask"):
        out[k] = out[k].bool()
    out["ref_ids"] = [ref for ref, _ in rows]
    return out


@ops.on_tensor_device
def dynamic_filter_scan(depths, confidences, cams, images, pair_data, prob_threshold=0.3, dh_view_num=2, dist_filter=4.0,
                        depth_filter=1300.0, relative=False, chunk=None):
    """``dynamic_filter_depth`` (test_tank.py:455-570) from the maps a scan's forward pass left on the device to the fused point
    cloud, ``filter_dixt``'s fields as keywords.  depths [n_views,h,w]; confidences [n_views,ch,cw] or None; cams [n_views,2,4,4];
    images [n_views,3,h,w] fp32 in [0,1]; ``pair_data`` the ``read_pair_file`` list.  A reference view with fewer than
    ``dh_view_num + 1`` sources contributes nothing (:478) -> dict(xyz [M,3] float32, rgb [M,3] uint8 -- vertices in the reference's
    order: retained reference views in list order, row-major survivors --, offsets [n_kept+1] int32, ref_ids: the retained reference
    ids, depth [n_kept,h,w], prob_mask / geo_mask / mask [n_kept,h,w] bool).  Works through the reference views ``chunk`` at a time
    (None: sized so that a chunk's dense points stay below 400 MB); the result is the same for every ``chunk``."""
    rows = [(ref, srcs) for ref, srcs in pair_data if len(srcs) >= dh_view_num + 1]
    return _filter_scan(ops.fusion_dynamic_filter_scan, rows, depths, confidences, cams, images, chunk, prob_threshold, dh_view_num,
                        dist_filter, depth_filter, relative)


def static_scan_rows(pair_data):
    """Host only: the rows of a ``read_pair_file`` list the fixed-threshold filter keeps -- a reference view without a source has
    nothing to be checked against and contributes nothing."""
    return [(ref, list(srcs)) for ref, srcs in pair_data if len(srcs) >= 1]


@ops.on_tensor_device
def static_filter_scan(depths, confidences, cams, images, pair_data, prob_threshold=0.3, img_dist_thresh=1.0, depth_thresh=0.01,
                       vthresh=4, chunk=None):
    """``static_filter`` over a scan's reference views, from the maps on the device to the fused point cloud; arguments, chunking and
    result as ``dynamic_filter_scan``.  Reference views without a source are dropped; ``ref_ids`` lists the ones that remain."""
    return _filter_scan(ops.fusion_static_filter_scan, static_scan_rows(pair_data), depths, confidences, cams, images, chunk,
                        prob_threshold, img_dist_thresh, depth_thresh, vthresh)
