#!/usr/bin/env python3
"""Time of the Gipuma fusion of one DTU-sized scan (49 views at 1184x1600, every other view a source: 48 per reference view,
synth.synth_depth_maps), device maps in, compacted cloud out:

  hip       : ``gipuma.fuse_scan`` (csrc/gipuma.hip: one launch per reference view, compaction on the device);
  composite : the same specification as a per-reference-view loop of torch tensor operations on the same GPU
              (``composite`` below) -- what a user without the kernel would write.

The two sides alternate, ``--runs`` whole scans each after a warm-up of both, each scan timed by a host clock around work that ends in
a device synchronise; the report gives median (min - max) per scan and per reference view.  A further, separate pass of the hip side
runs under ``ops.KernelProfile`` (device events around each launch) for the kernel's own time per reference view, which is set
against the bytes a reference view has to read: (1 + S) h w 4 B of depth (the colours and flags come on top for fused pixels only).
The two sides round differently in places (torch's matmul against the kernel's written-out sums), so a few decisions may flip; the
share of pixels with equal masks is reported, not asserted -- the kernel's correctness is the business of tests/test_gpu_gipuma.py.
Needs a GPU; results go to --out (default out/gipuma_bench.txt).
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, N_VIEWS = 1184, 1600, 49
DEPTH_MIN, DEPTH_MAX = 0.001, 100000.0
HBM_BYTES_PER_S = 8.0e12           # MI355X peak HBM3E bandwidth


def composite(depths, cams, images, rows, thr, num):
    """DESIGN.md 7.10 in torch fp32: -> (xyz [M,3], rgb [M,3] uint8, masks [n_ref,h*w] bool).  One pass of tensor operations per
    (reference, source) pair; the flags persist over the reference views."""
    import torch
    n, h, w = depths.shape
    hw = h * w
    dev = depths.device
    D = depths.reshape(n, hw)
    I = images.reshape(n, hw, 3)
    K, R, t = cams[:, 1, :3, :3], cams[:, 0, :3, :3], cams[:, 0, :3, 3]
    Kinv = torch.linalg.inv(K.double()).float()
    C = -(R.double().transpose(1, 2) @ t.double()[:, :, None])[:, :, 0]
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(hw, device=dev)])
    ok = lambda d: (d >= DEPTH_MIN) & (d <= DEPTH_MAX)
    used = torch.zeros(n, hw, dtype=torch.bool, device=dev)
    xyz, rgb, masks = [], [], []
    for ref, srcs in rows:
        d = D[ref]
        live = ok(d) & ~used[ref]
        X = R[ref].t() @ (d * (Kinv[ref] @ pix) - t[ref][:, None])
        cnt = torch.zeros(hw, dtype=torch.int32, device=dev)
        psum, csum, kept = X.clone(), I[ref].clone(), []
        for s in srcs:
            Y = R[s] @ X + t[s][:, None]
            k = K[s] @ Y
            qx, qy = torch.floor(k[0] / k[2] + 0.5), torch.floor(k[1] / k[2] + 0.5)
            valid = (Y[2] > 0) & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            q = torch.where(valid, qy * w + qx, torch.zeros_like(qx)).long()
            ds = D[s][q]
            fb = float(K[ref, 0, 0].double() * (C[ref] - C[s]).norm())
            c = live & valid & ok(ds) & ((fb / Y[2] - fb / ds).abs() < thr)
            Xs = R[s].t() @ (ds * (Kinv[s] @ torch.stack([qx, qy, torch.ones_like(qx)])) - t[s][:, None])
            psum = psum + torch.where(c, Xs, torch.zeros_like(Xs))
            csum = csum + torch.where(c[:, None], I[s][q], torch.zeros_like(csum))
            cnt += c
            kept.append((c, q.int()))
        fused = live & (cnt >= num)
        for s, (c, q) in zip(srcs, kept):
            used[s][q[c & fused].long()] = True
        used[ref] |= fused
        div = (cnt + 1).float()
        xyz.append((psum / div)[:, fused].t())
        rgb.append(((csum / div[:, None])[fused] * 255.0).to(torch.uint8))
        masks.append(fused)
    return torch.cat(xyz), torch.cat(rgb), torch.stack(masks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=N_VIEWS)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--disp-threshold", type=float, default=0.25)
    ap.add_argument("--num-consistent", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "gipuma_bench.txt"))
    a = ap.parse_args()
    import torch
    from effi_mvs_plus_amd import gipuma, ops, synth
    if not torch.cuda.is_available():
        sys.exit("bench_gipuma: needs a GPU (nothing is measured without one)")
    dev = "cuda:0"
    n, h, w = a.views, a.height, a.width
    d, cams = synth.synth_depth_maps(h, w, n, seed=3, noise_mm=0.03, outlier_frac=0.08, pixel_center=0.0)
    depths, cams = d.to(dev), cams.to(dev)
    images = torch.rand(n, h, w, 3, generator=torch.Generator().manual_seed(10)).to(dev)
    rows = gipuma.scan_rows(n)
    S = len(rows[0][1])

    def hip():
        r = gipuma.fuse_scan(depths, None, cams, images, None, 0.5, a.disp_threshold, a.num_consistent)
        return r["xyz"], r["rgb"], r["mask"].reshape(n, -1)

    def comp():
        return composite(depths, cams, images, rows, a.disp_threshold, a.num_consistent)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    warm = {"hip": timed(hip)[1], "composite": timed(comp)[1]}        # warm-up of both sides, and the outputs to compare
    secs = {"hip": [], "composite": []}
    for _ in range(a.runs):
        for side, fn in (("hip", hip), ("composite", comp)):
            secs[side].append(timed(fn)[0])
    prof = ops.KernelProfile()
    ops.set_profile(prof)
    try:
        hip()
        torch.cuda.synchronize()
    finally:
        ops.set_profile(None)
    kern = prof.summary()
    fmt = lambda v, k=1.0: f"{statistics.median(v) * k:.4f} ({min(v) * k:.4f} - {max(v) * k:.4f})"
    view = kern["fusion_gipuma_view"]
    ms_view = view["ms"] / view["launches"]
    each = [e0.elapsed_time(e1) for key, _, e0, e1 in prof.records if key == "fusion_gipuma_view"]      # in reference order
    floor_bytes = (1 + S) * h * w * 4.0
    same = float((warm["hip"][2] == warm["composite"][2]).float().mean())
    lines = [f"# gipuma fusion: {n} views at {h}x{w}, {S} sources per reference view, disp_threshold {a.disp_threshold}, num_consistent "
             f"{a.num_consistent}; {a.runs} alternating runs after a warm-up of both sides; median (min - max)",
             f"hip       seconds per scan {fmt(secs['hip'])}   ms per reference view {fmt(secs['hip'], 1000.0 / n)}",
             f"composite seconds per scan {fmt(secs['composite'])}   ms per reference view {fmt(secs['composite'], 1000.0 / n)}",
             f"ratio composite / hip (medians) {statistics.median(secs['composite']) / statistics.median(secs['hip']):.1f}",
             f"kernel (device events, separate profiled pass): fusion_gipuma_view {view['launches']} launches, {ms_view:.3f} ms each "
             f"(prepare + pixel kernel); depth floor {(1 + S)} maps = {floor_bytes / 1e6:.0f} MB per reference view -> "
             f"{floor_bytes / (ms_view * 1e-3) / 1e12:.2f} TB/s achieved against that floor ({floor_bytes / HBM_BYTES_PER_S * 1e3:.3f} ms at "
             f"{HBM_BYTES_PER_S / 1e12:.0f} TB/s); {ms_view * 1e9 / (h * w * S):.2f} ps per (pixel, source)",
             f"per launch in reference order: first (nothing consumed yet) {each[0]:.3f} ms = {floor_bytes / (each[0] * 1e-3) / 1e12:.2f} TB/s, "
             f"second {each[1]:.3f}, median {statistics.median(each):.3f}, last {each[-1]:.3f}, largest {max(each):.3f} ms",
             "other launches of the profiled pass: " + "  ".join(f"{k} {v['launches']}x {v['ms']:.2f} ms" for k, v in kern.items()
                                                               if k != "fusion_gipuma_view"),
             f"vertices: hip {warm['hip'][0].shape[0]}  composite {warm['composite'][0].shape[0]}  of {n * h * w} pixels; pixels with equal "
             f"masks {same:.6f}"]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
