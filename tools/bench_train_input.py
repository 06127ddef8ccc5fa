#!/usr/bin/env python3
"""The training input at the DTU training shape (640x512, N = 5 views; B = 1 and B = 4 samples):

  1. ``ops.images_prepare`` (one launch for B*N views) against B*N ``ops.image_prepare`` calls;
  2. ``ops.gt_pyramid`` (one launch, DTU and BlendedMVS mode) against the eight stock-torch launches that compute the same maps
     (three strided copies and one copy of the depth, the threshold, three strided copies of the mask);
  3. ``GraphedTrainStep.load_raw_sample`` against host preparation (the numpy restatement of tests/train_input_ref.py) followed by
     ``load_sample``, for the same decoded DTU sample.

1 and 2: every candidate is captured as a HIP graph of ``--chain`` back-to-back calls and the replay is timed by HIP events, so the
figure is device time per call without the host's launch cost; the median over ``--iters`` replays with the 10th / 90th
percentile.  3: a host clock around calls that end in a synchronise.
usage: bench_train_input.py [--iters 50] [--chain 50] [--no-step]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import train_input_ref as R  # noqa: E402
from common import build_model  # noqa: E402
from effi_mvs_plus_amd import ops, synth, train_graph  # noqa: E402
from effi_mvs_plus_amd.datasets.train_sample import prepare_train_sample  # noqa: E402

DEV = "cuda:0"
H, W, N = 512, 640, 5


def graph_times(fn, chain, iters):
    """microseconds per call of fn, from replays of a captured chain of `chain` calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(chain):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        g.replay()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) * 1e3 / chain for a, b in ev)


def show(name, us, nbytes):
    n, med = len(us), statistics.median(us)
    print(f"{name:<64s} median {med:8.2f} us   p10 {us[n // 10]:8.2f}   p90 {us[(9 * n) // 10]:8.2f}   {nbytes / med * 1e-6:7.2f} TB/s")


def torch_pyramid(depth, mask_u8, outs_d, outs_m):
    """The same eight maps by stock torch operators, written into given buffers (8+ launches)."""
    m = (mask_u8 > 10).float()
    for j, k in enumerate(R.STAGES):
        f = 8 >> j
        outs_d[k].copy_(depth[:, ::f, ::f])
        outs_m[k].copy_(m[:, ::f, ::f])


def kernels(args):
    rng = np.random.default_rng(0)
    for B in (1, 4):
        V = B * N
        x = torch.from_numpy(rng.integers(0, 256, size=(V, H, W, 3), dtype=np.uint8)).to(DEV)
        out = torch.empty(V, 3, H, W, device=DEV)
        nbytes = 15.0 * V * H * W
        show(f"images_prepare, B = {B} ({V} views, one launch)", graph_times(lambda: ops.images_prepare(x, out=out), args.chain, args.iters), nbytes)
        want = out.clone()

        def per_view():
            for v in range(V):
                ops.image_prepare(x[v], H, W, out=out[v])
        show(f"{V} x image_prepare (one launch per view)", graph_times(per_view, max(1, args.chain // V), args.iters), nbytes)
        assert torch.equal(out, want)
        depth = torch.from_numpy((425.0 + 500.0 * rng.random((B, H, W))).astype(np.float32)).to(DEV)
        mask = torch.from_numpy(rng.integers(0, 256, size=(B, H, W), dtype=np.uint8)).to(DEV)
        rng_t = torch.tensor([[425.0, 935.0]] * B, device=DEV)
        od, om = ops.gt_pyramid(depth, mask_u8=mask)
        pyr = (4.0 + 8.0 * 85 / 64) * B * H * W
        show(f"gt_pyramid DTU mode, B = {B} (one launch)", graph_times(lambda: ops.gt_pyramid(depth, mask_u8=mask, out=(od, om)), args.chain, args.iters),
             pyr + B * H * W)
        show(f"gt_pyramid BlendedMVS mode, B = {B} (one launch)",
             graph_times(lambda: ops.gt_pyramid(depth, depth_range=rng_t, out=(od, om)), args.chain, args.iters), pyr)
        td, tm = {k: torch.empty_like(v) for k, v in od.items()}, {k: torch.empty_like(v) for k, v in om.items()}
        ops.gt_pyramid(depth, mask_u8=mask, out=(od, om))
        show(f"the same maps by torch operators, B = {B} (10 launches)", graph_times(lambda: torch_pyramid(depth, mask, td, tm), max(1, args.chain // 10), args.iters),
             pyr + B * H * W)
        assert all(torch.equal(td[k], od[k]) and torch.equal(tm[k], om[k]) for k in R.STAGES)


def loading(args):
    rng = np.random.default_rng(1)
    raws = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(N)]
    depth_full = (425.0 + 500.0 * rng.random((1200, 1600))).astype(np.float32)
    mask_full = rng.integers(0, 256, size=(1200, 1600), dtype=np.uint8)
    _, pm, dv = synth.synth_sample(H, W, N, seed=10)
    oy, ox = (600 - H) // 2, (800 - W) // 2
    crop = lambda a: np.ascontiguousarray(a[2 * oy:2 * (oy + H):2, 2 * ox:2 * (ox + W):2])       # noqa: E731
    raw = {"imgs_u8": torch.from_numpy(np.stack(raws))[None], "depth_raw": torch.from_numpy(crop(depth_full))[None],
           "mask_raw": torch.from_numpy(crop(mask_full))[None], "proj_matrices": pm, "depth_values": dv, "filename": ["x"]}
    first = prepare_train_sample(raw, device=DEV)
    net, _ = build_model("48,8,8", seed=2, device=DEV)
    net.train()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-6, capturable=True)
    step = train_graph.GraphedTrainStep(net, opt, first["imgs"], first["proj_matrices"], first["depth_values"], first["depth"], first["mask"])

    def host_path():
        imgs = torch.from_numpy(R.images(raws))[None]
        d_ms, m_ms = R.dtu_ground_truth(depth_full, mask_full, (H, W))
        step.load_sample(imgs, pm, dv, {k: torch.from_numpy(v)[None] for k, v in d_ms.items()},
                         {k: torch.from_numpy(v)[None] for k, v in m_ms.items()})

    def host_prepare_only():
        R.images(raws)
        R.dtu_ground_truth(depth_full, mask_full, (H, W))

    def raw_path():
        step.load_raw_sample(raw)

    def crop_and_raw_path():          # with the dataset's strided crop of the 1200 x 1600 maps included
        raw2 = dict(raw, depth_raw=torch.from_numpy(crop(depth_full))[None], mask_raw=torch.from_numpy(crop(mask_full))[None])
        step.load_raw_sample(raw2)

    times = {}
    for _ in range(args.rounds):
        for name, fn in (("host preparation (numpy restatement) + load_sample", host_path), ("host preparation alone", host_prepare_only),
                         ("load_raw_sample", raw_path), ("strided crop of the raw maps + load_raw_sample", crop_and_raw_path)):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            times.setdefault(name, []).append((time.perf_counter() - t0) / 5 * 1e3)
    host_path()
    kept = (step.imgs.clone(), {k: v.clone() for k, v in step.gt.items()}, {k: v.clone() for k, v in step.mask.items()})
    raw_path()
    same = torch.equal(step.imgs, kept[0]) and all(torch.equal(step.gt[k], kept[1][k]) and torch.equal(step.mask[k], kept[2][k]) for k in step.gt)
    print(f"# loading one decoded DTU sample ({N} views {W}x{H}, raw maps 1600x1200) into a captured step: ms per sample, wall clock, "
          f"{args.rounds} alternated rounds of 5; buffers bitwise equal: {same}")
    for name, v in times.items():
        print(f"{name:<56s} median {statistics.median(v):8.3f} ms   min {min(v):8.3f}   max {max(v):8.3f}")
    t0 = time.perf_counter()
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    print(f"replayed step for scale: {(time.perf_counter() - t0) / 10 * 1e3:.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--chain", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured on a CPU"
    print(f"# training-input kernels at {W}x{H}, N = {N}: device time per call from replays of a captured chain of {args.chain} calls")
    kernels(args)
    if not args.no_step:
        loading(args)


if __name__ == "__main__":
    main()
