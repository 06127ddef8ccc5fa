#!/usr/bin/env python3
"""The scalar side of a training / validation step at the DTU training shape (640x512, B = 1, the 13 outputs of GRUiters 3,3,3):

  1. loss, forward + backward: ``mvs_loss_static`` (stock torch operators) against ``mvs_loss_fused`` (csrc/metrics.hip);
  2. metrics: the 12 calls of test_sample_depth written the reference's way (boolean indexing, one call per scalar, train.py:322-337)
     against one ``metrics.depth_scalars``;
  3. ``GraphedTrainStep`` replay with each loss, same process, alternated.

Times are HIP events around each call on the device (1, 2) or a host clock around replays that end in a synchronise (3); every
figure is a median over the timed calls with the 10th / 90th percentile as the spread.  Launch counts come from torch's profiler
(kernel events of one call); if the profiler is unavailable they are reported as not measured.
usage: bench_loss_metrics.py [--iters 200] [--rounds 6] [--no-step]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from common import build_model  # noqa: E402
from effi_mvs_plus_amd import metrics, synth, train_graph  # noqa: E402
from effi_mvs_plus_amd.models import mvs_loss_fused  # noqa: E402
from effi_mvs_plus_amd.models.module import mvs_loss_static  # noqa: E402

DEV = "cuda:0"
H, W = 512, 640
DLOSS = list(train_graph.DLOSS)


def targets(B, seed):
    g = torch.Generator().manual_seed(seed)
    gt, mask = {}, {}
    for k, f in (("stage1", 8), ("stage2", 4), ("stage3", 2), ("stage4", 1)):
        gt[k] = (synth.DEPTH_MIN_MM + (synth.DEPTH_MAX_MM - synth.DEPTH_MIN_MM) * torch.rand(B, H // f, W // f, generator=g)).to(DEV)
        mask[k] = (torch.rand(B, H // f, W // f, generator=g) > 0.3).float().to(DEV)
    return gt, mask


def event_times(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) * 1e3 for a, b in ev)            # microseconds


def show(name, us, launches):
    n = len(us)
    print(f"{name:<58s} median {statistics.median(us):8.1f} us   p10 {us[n // 10]:8.1f}   p90 {us[(9 * n) // 10]:8.1f}   "
          f"n={n}   launches {launches}")


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return str(n) if n else "not measured"
    except Exception as exc:      # noqa: BLE001
        return f"not measured ({type(exc).__name__})"


def reference_style_metrics(est, gt, mask):
    """The scalars of test_sample_depth computed the reference's way: per image, select the valid pixels by boolean indexing, then
    one reduction per scalar; twelve calls, each with a data-dependent shape."""
    def per_image(fn):
        return torch.stack([fn((est[b][mask[b]] - gt[b][mask[b]]).abs()) for b in range(est.shape[0])]).mean()

    def band(lo, hi):
        def fn(e):
            e = e[(e >= lo) & (e <= hi)]
            return e.mean() if e.numel() else torch.zeros((), device=e.device)
        return fn

    out = [per_image(lambda e: e.mean())]
    out += [per_image(lambda e, t=t: (e > t).float().mean()) for t in metrics.TEST_SCALARS.thresholds]
    out += [per_image(band(lo, hi)) for lo, hi in metrics.TEST_SCALARS.bands]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured on a CPU"
    gt, mask = targets(1, 1)
    g = torch.Generator().manual_seed(2)
    ests = [(gt["stage{}".format(s)].cpu() + 3.0 * torch.randn(gt["stage{}".format(s)].shape, generator=g)).to(DEV).requires_grad_(True)
            for s in DLOSS]
    print(f"# loss and metrics at {W}x{H}, B = 1, {len(ests)} outputs; times by HIP events per call")

    def loss_fwd_bwd(fn):
        def run():
            total, _ = fn(ests, gt, mask, DLOSS)
            torch.autograd.grad(total, ests)
        return run

    for name, fn in (("mvs_loss_static forward + backward (torch operators)", mvs_loss_static),
                     ("mvs_loss_fused forward + backward (effi_mvs_loss[_bwd]_f32)", mvs_loss_fused)):
        run = loss_fwd_bwd(fn)
        launches = count_launches(run)
        show(name, event_times(run, 20, args.iters), launches)
    a = mvs_loss_static(ests, gt, mask, DLOSS)[0]
    b = mvs_loss_fused(ests, gt, mask, DLOSS)[0]
    print(f"# totals: static {float(a.detach()):.7f}  fused {float(b.detach()):.7f}")

    est4, gt4, m4 = ests[-1].detach(), gt["stage4"], mask["stage4"] > 0.5
    ref_run = lambda: reference_style_metrics(est4, gt4, m4)          # noqa: E731
    one_run = lambda: metrics.depth_scalars(est4, gt4, m4, metrics.TEST_SCALARS.thresholds, metrics.TEST_SCALARS.bands)   # noqa: E731
    show("12 reference-style metric calls (boolean indexing)", event_times(ref_run, 10, args.iters), count_launches(ref_run))
    show("metrics.depth_scalars, TEST_SCALARS (effi_depth_metrics_f32)", event_times(one_run, 20, args.iters), count_launches(one_run))
    want = torch.stack(ref_run()).cpu()
    got = one_run().cpu()
    print(f"# largest relative difference of the 12 scalars: {float(((got - want).abs() / want.abs().clamp_min(1e-30)).max()):.2e}")

    if args.no_step:
        return
    net, _ = build_model("48,8,8", seed=2, device=DEV)
    net.train()
    imgs, pm, dv = synth.synth_sample(H, W, 5, seed=10)
    imgs, pm, dv = imgs.to(DEV), {k: v.to(DEV) for k, v in pm.items()}, dv.to(DEV)
    steps = {}
    for name, fn in (("static", mvs_loss_static), ("fused", mvs_loss_fused)):
        opt = torch.optim.AdamW(net.parameters(), lr=1e-6, capturable=True)
        steps[name] = train_graph.GraphedTrainStep(net, opt, imgs, pm, dv, gt, mask, loss_fn=fn)
    steps["fused+scalars"] = train_graph.GraphedTrainStep(net, torch.optim.AdamW(net.parameters(), lr=1e-6, capturable=True), imgs, pm, dv,
                                                          gt, mask, loss_fn=mvs_loss_fused, scalars=metrics.TRAIN_SCALARS)
    times = {k: [] for k in steps}
    for _ in range(args.rounds):
        for name, step in steps.items():
            step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                step()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / 10 * 1e3)
    print(f"# GraphedTrainStep replay at {W}x{H}, 5 views, 48,8,8: ms per step, {args.rounds} alternated rounds of 10 replays")
    for name, v in times.items():
        print(f"replay, loss = {name:<14s} median {statistics.median(v):7.3f} ms   min {min(v):7.3f}   max {max(v):7.3f}   rounds "
              + " ".join(f"{x:.3f}" for x in v))


if __name__ == "__main__":
    main()
