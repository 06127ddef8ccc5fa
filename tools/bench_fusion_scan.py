#!/usr/bin/env python3
"""A/B of the scan-level fusion path: one DTU-sized scan (49 reference views x 10 sources at 1152x1600, synth.synth_depth_maps) from
depth maps in device memory to the vertex arrays in host memory,

  parent : ``dtu_fusion.filter_view`` per reference view (torch.stack of its sources), mask and points ``.cpu()``, numpy boolean
           indexing, np.concatenate -- what ``filter_depth`` does between reading its files and writing the PLY;
  scan   : ``dtu_fusion.fuse_scan`` (scan-batched filter launches, compaction on the device) plus one copy of xyz and rgb.

The driver (no argument) opens no GPU itself: it writes the inputs once, then alternates the two sides, three runs each, every run a
child process under its own ``timeout``; it stops at the first child that fails.  Each child times one whole pass after a two-view
warm-up, then repeats the pass under ``ops.KernelProfile`` for the per-kernel times.  Both sides must report the same vertex count
and checksum.  Results go to --out (default out/fusion_scan_ab.txt).
"""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, N_VIEWS, N_SRC = 1152, 1600, 49, 10
CONF = 0.3


def pair_data(n_views=N_VIEWS, n_src=N_SRC):
    """Every view is a reference view; its sources are the nearest neighbours on the camera ring, nearest first."""
    out = []
    for v in range(n_views):
        srcs = []
        for k in range(1, n_src // 2 + 1):
            srcs += [(v + k) % n_views, (v - k) % n_views]
        out.append((v, srcs[:n_src]))
    return out


def write_inputs(path, h, w, n_views):
    import torch
    from effi_mvs_plus_amd import synth
    d, cams = synth.synth_depth_maps(h, w, n_views, seed=3, noise_mm=0.03, outlier_frac=0.08, pixel_center=0.0)
    g = torch.Generator().manual_seed(10)
    conf = torch.rand(n_views, h // 2, w // 2, generator=g)
    img = torch.randint(0, 256, (n_views, h, w, 3), generator=g, dtype=torch.uint8)
    torch.save({"depths": d, "cams": cams, "conf": conf, "img_u8": img}, path)


def child(side, path, n_views, n_src):
    import numpy as np
    import torch
    from effi_mvs_plus_amd import dtu_fusion, ops
    dev = "cuda:0"
    z = torch.load(path)
    depths, cams, conf = z["depths"].to(dev), z["cams"].to(dev), z["conf"].to(dev)
    img_host = z["img_u8"].numpy().astype(np.float32) / 255.             # read_img's values; the parent's way indexes them on the host
    img_dev = torch.from_numpy(img_host).to(dev) if side == "scan" else None
    pairs = pair_data(n_views, n_src)
    K = [cams[v, 1, :3, :3].cpu().numpy() for v in range(n_views)]
    E = [cams[v, 0].cpu().numpy() for v in range(n_views)]

    def parent(pd):
        xyz, rgb = [], []
        for ref, srcs in pd:
            r = dtu_fusion.filter_view(depths[ref], K[ref], E[ref], torch.stack([depths[v] for v in srcs]), [K[v] for v in srcs],
                                       [E[v] for v in srcs], conf[ref], CONF)
            m = r["final_mask"].cpu().numpy()
            p = r["xyz_world"].cpu().numpy()
            xyz.append(p[:, m].transpose((1, 0)))
            rgb.append((img_host[ref][m] * 255).astype(np.uint8))
        return np.concatenate(xyz, axis=0), np.concatenate(rgb, axis=0)

    def scan(pd):
        r = dtu_fusion.fuse_scan(depths, conf, cams, img_dev, pd, conf=CONF)
        return r["xyz"].cpu().numpy(), r["rgb"].cpu().numpy()

    run = parent if side == "parent" else scan
    run(pairs[:2])                                                        # warm-up: library load, allocator, workspace
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    xyz, rgb = run(pairs)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    prof = ops.KernelProfile()
    ops.set_profile(prof)
    try:
        run(pairs)
    finally:
        ops.set_profile(None)
    kernels = {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in prof.summary().items()}
    print(json.dumps({"side": side, "seconds": round(sec, 4), "vertices": int(xyz.shape[0]),
                      "crc": zlib.crc32(np.ascontiguousarray(xyz).tobytes() + np.ascontiguousarray(rgb).tobytes()), "kernels_ms": kernels}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=["parent", "scan"], help="child mode: time one side once (the driver starts these)")
    ap.add_argument("--inputs", default=os.path.join(ROOT, "out", "fusion_scan_inputs.pt"))
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "fusion_scan_ab.txt"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--views", type=int, default=N_VIEWS)
    ap.add_argument("--sources", type=int, default=N_SRC)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each child may take")
    a = ap.parse_args()
    if a.side:
        return child(a.side, a.inputs, a.views, a.sources)
    os.makedirs(os.path.dirname(a.inputs), exist_ok=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    write_inputs(a.inputs, a.height, a.width, a.views)
    lines = [f"# fusion scan A/B: {a.views} reference views x {a.sources} sources at {a.height}x{a.width}, device maps -> host vertex arrays, "
             f"{a.runs} alternating runs (seconds per whole scan; kernels_ms = the launches' own durations in a second, profiled pass)"]
    results = {"parent": [], "scan": []}
    try:
        for i in range(a.runs):
            for side in ("parent", "scan"):
                cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--side", side, "--inputs", a.inputs,
                       "--views", str(a.views), "--sources", str(a.sources)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                if p.returncode != 0:
                    lines.append(f"run {i} {side}: FAILED with exit status {p.returncode}; stopping\n{p.stdout[-2000:]}")
                    return 1
                rec = json.loads(p.stdout.strip().splitlines()[-1])
                results[side].append(rec)
                lines.append(f"run {i} {json.dumps(rec)}")
                print(lines[-1], flush=True)
        pa, sc = results["parent"], results["scan"]
        same = {(r["vertices"], r["crc"]) for r in pa + sc}
        lines.append(f"# same vertex arrays on both sides: {len(same) == 1} ({pa[0]['vertices']} vertices)")
        med = lambda rs: sorted(r["seconds"] for r in rs)[len(rs) // 2]
        lines.append(f"# median seconds per scan: parent {med(pa):.4f}  scan {med(sc):.4f}  ratio parent/scan {med(pa) / med(sc):.2f}")
        print("\n".join(lines[-2:]))
        return 0 if len(same) == 1 else 1
    finally:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        if os.path.exists(a.inputs):
            os.remove(a.inputs)


if __name__ == "__main__":
    sys.exit(main())
