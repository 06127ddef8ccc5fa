#!/usr/bin/env python3
"""A/B of the fixed-threshold visibility filter: one reference view with 10 sources at 1056x1920,

  fused    : ``ops.fusion_static_filter`` -- one kernel, no [v,3,h,w] intermediate;
  unfused  : the same result composed from the pieces the package had before: the four ``idx_*`` kernels, torch's ``grid_sample`` and
             the tensor lines of get_reproj / project_img / vis_filter / ave_fusion / the driver's points.

Both are timed alternated in one process with HIP events after a warm-up; medians and the p10-p90 range are reported, and the two
sides' final masks and averaged depths are compared.  Then ``fusion.static_filter_scan`` on a DTU-sized scan (49 reference views x 10
sources at 1152x1600, device maps -> compacted cloud on the device).  Results go to --out (default out/fusion_static_ab.txt).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, N_SRC = 1056, 1920, 10
SCAN_H, SCAN_W, SCAN_VIEWS = 1152, 1600, 49
THR = dict(prob=0.3, img_dist=0.5, depth=0.5, vthresh=3)


def unfused(fusion, torch, F, ref_depth, src_depths, ref_cam, src_cams, conf):
    """ref_depth [1,1,h,w], src_depths [1,v,1,h,w], cameras [1,2,4,4] / [1,v,2,4,4] -> (mask, averaged depth, points)."""
    v, h, w = src_depths.shape[1], ref_depth.shape[-2], ref_depth.shape[-1]
    grid = fusion.get_pixel_grids(h, w)[None]
    rc, sc = ref_cam.expand(v, 2, 4, 4).contiguous(), src_cams[0]
    # every source pixel into the reference view: (x, y, depth) maps
    cam = fusion.idx_world2cam(fusion.idx_cam2world(fusion.idx_img2cam(grid, src_depths[0], sc), sc), rc)
    img = fusion.idx_cam2img(cam, rc)
    smap = torch.cat([img[..., :2, 0], cam[..., 2:3, 0]], -1).permute(0, 3, 1, 2)
    # every reference pixel into the source views, normalised by the size, clamped, sampled
    uv = fusion.idx_cam2img(fusion.idx_world2cam(fusion.idx_cam2world(fusion.idx_img2cam(grid, ref_depth.expand(v, 1, h, w).contiguous(), rc), rc), sc), sc)
    g = torch.stack([uv[..., 0, 0] / w, uv[..., 1, 0] / h], -1).mul(2).sub(1).clamp(-1.1, 1.1)
    xyd = F.grid_sample(smap, g, mode="bilinear", padding_mode="zeros", align_corners=True)[None]
    masks = ((xyd[:, :, :2] - grid[0, :, :, :2, 0].permute(2, 0, 1)).norm(dim=2, keepdim=True) < 1. / THR["img_dist"]) \
        & ((ref_depth[:, None] - xyd[:, :, 2:]).abs() < 1. / THR["depth"])
    masks = masks.to(ref_depth.dtype)
    geo = masks.sum(1) >= THR["vthresh"] - 1.1
    depth = ((xyd[:, :, 2:] * masks).sum(1) + ref_depth) / (masks.sum(1) + 1)
    prob = F.interpolate(conf[:, None], size=[h, w], mode="nearest") > THR["prob"]
    pts = fusion.idx_cam2world(fusion.idx_img2cam(grid, depth, ref_cam), ref_cam)[..., :3, 0].permute(0, 3, 1, 2)
    return geo & prob, depth, pts


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]        # noqa: E731
    return f"median {q(0.5):.3f} ms (p10 {q(0.1):.3f}, p90 {q(0.9):.3f}, n {len(s)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "fusion_static_ab.txt"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--scan-reps", type=int, default=5)
    ap.add_argument("--no-scan", action="store_true")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from effi_mvs_plus_amd import fusion, ops, synth
    dev = "cuda:0"
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    d, cams = synth.synth_depth_maps(H, W, N_SRC + 1, seed=3, noise_mm=0.05, outlier_frac=0.3)
    d, cams = d.to(dev), cams.to(dev)
    conf = torch.rand(1, H // 2, W // 2, generator=torch.Generator().manual_seed(5)).to(dev)
    rd, sd, rc, sc = d[0].contiguous(), d[1:].contiguous(), cams[0].contiguous(), cams[1:].contiguous()
    fused = lambda: ops.fusion_static_filter(rd, sd, rc, sc, conf[0], THR["prob"], THR["img_dist"], THR["depth"], THR["vthresh"])   # noqa: E731
    comp = lambda: unfused(fusion, torch, F, rd[None, None], sd[None, :, None], rc[None], sc[None], conf)                       # noqa: E731
    with torch.no_grad():
        for _ in range(3):
            rf, ru = fused(), comp()
        torch.cuda.synchronize()
        dd = (rf["depth"] - ru[1][0, 0]).abs()
        say(f"# fixed-threshold filter A/B: one reference view, {N_SRC} sources at {H}x{W}; final mask {float(rf['mask'].float().mean()):.3f} full; "
            f"final masks differ at {int((rf['mask'].bool() != ru[0][0, 0]).sum())} of {H * W} pixels; averaged depth: median difference "
            f"{float(dd.median()):.3e}, {int((dd > 1e-3).sum())} pixels differ by more than 1e-3 (a per-view test that fell the other way), max {float(dd.max()):.3e}")
        tf, tu = [], []
        for _ in range(a.reps):                                           # alternated: both sides see the same clocks and cache state
            tf.append(timed(fused)[0])
            tu.append(timed(comp)[0])
        say(f"fused   (ops.fusion_static_filter, 2 launches)            : {stats(tf)}")
        say(f"unfused (idx_* kernels + grid_sample + tensor lines)       : {stats(tu)}")
        say(f"# ratio of the medians unfused / fused: {sorted(tu)[len(tu) // 2] / sorted(tf)[len(tf) // 2]:.2f}")
        del ru, rf
        torch.cuda.empty_cache()
        if not a.no_scan:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            from bench_fusion_scan import pair_data
            d, cams = synth.synth_depth_maps(SCAN_H, SCAN_W, SCAN_VIEWS, seed=3, noise_mm=0.05, outlier_frac=0.3)
            d, cams = d.to(dev), cams.to(dev)
            g = torch.Generator().manual_seed(10)
            conf = torch.rand(SCAN_VIEWS, SCAN_H // 2, SCAN_W // 2, generator=g).to(dev)
            img = torch.rand(SCAN_VIEWS, 3, SCAN_H, SCAN_W, generator=g).to(dev)
            pairs = pair_data(SCAN_VIEWS, N_SRC)
            scan = lambda: fusion.static_filter_scan(d, conf, cams, img, pairs, THR["prob"], THR["img_dist"], THR["depth"], THR["vthresh"])   # noqa: E731
            r = scan()
            ts = [timed(scan)[0] for _ in range(a.scan_reps)]
            say(f"static_filter_scan, {SCAN_VIEWS} reference views x {N_SRC} sources at {SCAN_H}x{SCAN_W}, {r['xyz'].shape[0]} vertices "
                f"({r['xyz'].shape[0] / (SCAN_VIEWS * SCAN_H * SCAN_W):.3f} of the pixels): {stats(ts)}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
