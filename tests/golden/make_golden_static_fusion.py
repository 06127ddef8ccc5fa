#!/usr/bin/env python3
"""Golden vectors for the fixed-threshold visibility filter, produced by RUNNING the reference's own
misc/fusion.py functions -- get_reproj, vis_filter, ave_fusion, prob_filter, project_img -- on ``synth.synth_depth_maps`` rigs
(tests/static_fusion_ref.py::CASES); the driver lines that combine their outputs (photometric mask, final mask, world points) are
data-generation arithmetic typed here with their test_tank.py line numbers.

Per case and per output kind the script prints the distance of the reference's fp32 result from the float64 restatement of
tests/static_fusion_ref.py; 4 x the largest distance per kind is the value bound E the tests use, stored in the file.  It also prints
the share of mask elements E leaves undecided and how full the masks are.  Only rig "a" keeps its arrays (the other rigs are checked
against the float64 restatement alone), which keeps the file below g12_fusion.npz.

The reference hard-codes ``.cuda()`` in get_pixel_grids (misc/fusion.py:9-10); this script runs it on the CPU with ``Tensor.cuda`` as
the identity.  Run from the repo root:  python tests/golden/make_golden_static_fusion.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
torch.Tensor.cuda = lambda self, *a, **k: self
import misc.fusion as fusion  # noqa: E402  (the reference)

import static_fusion_ref as SR  # noqa: E402

PROB3 = dict(seed=41, thresholds=(0.2, 0.5, 0.35))                   # prob_filter: 3 channels, three thresholds
PROJ = dict(seed=42, C=5, height=48, width=64)                       # project_img: C = 5, destination 48x64, source 96x128


def reference_run(c):
    """The reference on one case (batch of one) -> dict of numpy arrays."""
    t = torch.from_numpy
    ref_depth, src = t(c["ref_depth"])[None, None], t(c["src_depths"])[None, :, None]
    ref_cam, src_cams = t(c["ref_cam"])[None], t(c["src_cams"])[None]
    reproj_xyd, in_range = fusion.get_reproj(ref_depth, src, ref_cam, src_cams)
    masks, mask = fusion.vis_filter(ref_depth, reproj_xyd, in_range, c["img_dist_thresh"], c["depth_thresh"], c["vthresh"])
    depth = fusion.ave_fusion(ref_depth, reproj_xyd, masks)
    h, w = ref_depth.shape[-2:]
    conf = F.interpolate(t(c["conf"])[None].unsqueeze(1), size=[h, w], mode="nearest")                 # test_tank.py:473
    prob_mask = conf > c["prob_thr"]                                                                    # :474
    final = fusion.bin_op_reduce([prob_mask, mask], torch.min)                                          # :512
    idx_img = fusion.get_pixel_grids(*depth.size()[-2:]).unsqueeze(0)                                   # :513
    idx_cam = fusion.idx_img2cam(idx_img, depth, ref_cam)                                               # :514
    points = fusion.idx_cam2world(idx_cam, ref_cam)[..., :3, 0].permute(0, 3, 1, 2)                     # :515
    # project_img's warp coordinate (misc/fusion.py:53-61) per source, for the in_range bound
    g = []
    for s in range(src.shape[1]):
        sc = src_cams[:, s]
        img = fusion.idx_cam2img(fusion.idx_world2cam(fusion.idx_cam2world(fusion.idx_img2cam(idx_img, ref_depth, ref_cam), ref_cam), sc), sc)
        wc = img[..., :2, 0]
        wc[..., 0] /= w
        wc[..., 1] /= h
        g.append((wc * 2 - 1).clamp(-1.1, 1.1)[0])
    g = torch.stack(g).numpy()
    return dict(reproj_xyd=reproj_xyd[0].numpy(), in_range=in_range[0, :, 0].numpy(), masks=masks[0, :, 0].numpy(), mask=mask[0, 0].numpy(),
                depth=depth[0, 0].numpy(), prob_mask=prob_mask[0, 0].numpy(), final=final[0, 0].numpy(), points=points[0].numpy(),
                gx=g[..., 0], gy=g[..., 1])


@torch.no_grad()
def main():
    runs, refs, dist = {}, {}, {k: {} for k in SR.KINDS + ("g", "img")}
    for name in SR.CASES:
        c = SR.case(name)
        got, want = reference_run(c), SR.case_ref(name)
        assert all(np.isfinite(got[k]).all() for k in ("reproj_xyd", "depth", "points")), name
        runs[name], refs[name] = got, want
        dist["xy"][name] = np.abs(got["reproj_xyd"][:, :2] - want["xyd"][:, :2]).max()
        dist["d"][name] = np.abs(got["reproj_xyd"][:, 2] - want["xyd"][:, 2]).max()
        dist["g"][name] = max(np.abs(got["gx"] - want["gx"]).max(), np.abs(got["gy"] - want["gy"]).max())
        # averaged depth and points: against float64 on the reference's OWN masks (a flipped mask is a decision, not a value error)
        ave = SR.ave(c["ref_depth"], want["xyd"], got["masks"])
        dist["ave"][name] = np.abs(got["depth"] - ave).max()
        dist["pts"][name] = np.abs(got["points"] - SR.points(ave, c["ref_cam"])).max()
    # project_img on rig "a": C = 5, the destination smaller than the source
    a = SR.case("a")
    src_img = torch.rand(1, PROJ["C"], 96, 128, generator=torch.Generator().manual_seed(PROJ["seed"]))
    dst_depth = torch.from_numpy(np.ascontiguousarray(a["ref_depth"][:PROJ["height"], :PROJ["width"]]))[None, None]
    warped, proj_in = fusion.project_img(src_img, dst_depth, torch.from_numpy(a["src_cams"][:1]), torch.from_numpy(a["ref_cam"])[None],
                                         PROJ["height"], PROJ["width"])
    w64, pgx, pgy = SR.project_img(src_img[0].numpy(), dst_depth[0, 0].numpy(), a["src_cams"][0], a["ref_cam"], PROJ["height"], PROJ["width"])
    dist["img"]["a"] = np.abs(warped[0].numpy() - w64).max()
    # prob_filter: 3 channels, three thresholds
    prob = torch.rand(1, 3, 1, 96, 128, generator=torch.Generator().manual_seed(PROB3["seed"]))
    prob_mask3 = fusion.prob_filter(prob, PROB3["thresholds"])

    E = {k: 4.0 * max(v.values()) for k, v in dist.items()}
    for k, v in dist.items():
        print(f"|reference fp32 - float64| {k:4s}: " + "  ".join(f"{n} {x:.3e}" for n, x in v.items()) + f"   -> E = {E[k]:.3e}")
    for name in SR.CASES:
        c, got = SR.case(name), runs[name]
        r = SR.case_ref(name, tuple(sorted(E.items())))
        und = 1.0 - r["masks_decided"].mean()
        flips = (got["masks"].astype(bool) != r["masks"])
        assert not (flips & r["masks_decided"]).any() and not ((got["mask"] != r["mask"]) & r["mask_decided"]).any(), name
        print(f"{name}: undecided per-view {und:.4f}  final {1.0 - r['mask_decided'].mean():.4f}  per-view masks {got['masks'].mean():.3f} full  "
              f"geo {got['mask'].mean():.3f}  final {got['final'].mean():.3f}  in_range {got['in_range'].mean():.3f}  "
              f"reference flips {int(flips.sum())}")
        assert und <= SR.UNDECIDED_CAP and 0.2 <= got["masks"].mean() <= 0.9, name

    out = {f"E_{k}": np.float64(v) for k, v in E.items()}
    g = runs["a"]
    out.update(a_reproj_xyd=g["reproj_xyd"], a_in_range=g["in_range"].astype(np.uint8), a_masks=g["masks"].astype(np.uint8),
               a_mask=g["mask"].astype(np.uint8), a_depth=g["depth"], a_prob_mask=g["prob_mask"].astype(np.uint8),
               a_final=g["final"].astype(np.uint8), a_points=g["points"],
               proj_seed=np.int64(PROJ["seed"]), proj_warped=warped[0].numpy(), proj_in_range=proj_in[0, 0].numpy().astype(np.uint8),
               prob3_seed=np.int64(PROB3["seed"]), prob3_thresholds=np.asarray(PROB3["thresholds"], np.float64),
               prob3_mask=prob_mask3[0, 0, 0].numpy().astype(np.uint8))
    import inspect
    for fn in SR.NAMES:                                              # the parameter lists (names and defaults), for the signature test
        out[f"sig_{fn}"] = np.asarray([str(inspect.signature(getattr(fusion, fn)))])
    for name in SR.CASES:                                            # the inputs' seeds: the rigs are rebuilt from them
        out[f"{name}_seed"] = np.int64(SR.CASES[name][3])
    path = os.path.join(HERE, "g17_static_fusion.npz")
    np.savez_compressed(path, **out)
    print(f"g17_static_fusion.npz: {os.path.getsize(path) / 1024:.1f} KiB (g12_fusion.npz: "
          f"{os.path.getsize(os.path.join(HERE, 'g12_fusion.npz')) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
