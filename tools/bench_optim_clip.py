#!/usr/bin/env python3
"""The optimizer step alone on the training model (build_model("48,8,8"): 242 parameter tensors), with and without the global-norm
clip, three legs (profiles/optim_clip_ab.txt):
    a  FusedAdamW
    b  FusedAdamW(max_grad_norm=1.0)                          (the clip inside the step: csrc/optim.hip)
    c  torch.nn.utils.clip_grad_norm_(foreach=True) + FusedAdamW
usage: bench_optim_clip.py [--replays 200] [--rounds 2]       each leg captured by itself into a graph; device events around the
                                                             replays, the legs alternated; eager enqueue / wall time beside it
       bench_optim_clip.py --trace a|b|c --steps K           K eager steps of one leg and nothing else timed: the program to put
                                                             under a kernel trace (launches per step = the difference of two
                                                             runs' kernel counts over the difference of their K)"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from common import build_model  # noqa: E402
from effi_mvs_plus_amd import synth, train_graph  # noqa: E402
from effi_mvs_plus_amd.models import mvs_loss  # noqa: E402
from effi_mvs_plus_amd.optim import FusedAdamW  # noqa: E402

DEV = "cuda:0"
MAX_NORM = 1.0


def model_with_gradients():
    """The training model after one backward at 64 x 96, N = 3: the number and sizes of the parameter tensors do not depend on the
    image size."""
    H, W, N = 64, 96, 3
    net, _ = build_model("48,8,8", seed=2, device=DEV)
    imgs, pm, dv = synth.synth_sample(H, W, N, seed=3)
    imgs, pm, dv = imgs.to(DEV), {k: v.to(DEV) for k, v in pm.items()}, dv.to(DEV)
    net.eval()
    with torch.no_grad():
        target = net(imgs, pm, dv)["depth"][-1]
    gt = {k: F.interpolate((target + 15.0).unsqueeze(1), scale_factor=1 / f, mode="nearest").squeeze(1) if f > 1 else target + 15.0
          for k, f in (("stage1", 8), ("stage2", 4), ("stage3", 2), ("stage4", 1))}
    mask = {k: torch.ones_like(v) for k, v in gt.items()}
    net.train()
    loss, _ = mvs_loss(net(imgs, pm, dv)["depth"], gt, mask, list(train_graph.DLOSS))
    loss.backward()
    return net


def make_leg(leg, params):
    if leg == "a":
        opt = FusedAdamW(params, lr=1e-5)
        return opt.step
    if leg == "b":
        opt = FusedAdamW(params, lr=1e-5, max_grad_norm=MAX_NORM)
        return opt.step
    if leg == "c":
        opt = FusedAdamW(params, lr=1e-5)

        def step():
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
            opt.step()
        return step
    raise SystemExit("leg a|b|c")


NAMES = {"a": "FusedAdamW", "b": f"FusedAdamW(max_grad_norm={MAX_NORM})", "c": "clip_grad_norm_(foreach=True) + FusedAdamW"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--trace", choices=("a", "b", "c"), default=None)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_clip: needs the GPU")
    net = model_with_gradients()
    params = [p for p in net.parameters() if p.grad is not None]
    n_el = sum(p.numel() for p in params)
    print(f"model 48,8,8: {len(params)} parameter tensors with a gradient, {n_el} elements")
    if args.trace:
        step = make_leg(args.trace, params)
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        print(f"trace leg {args.trace} ({NAMES[args.trace]}): {args.steps} eager steps")
        return

    grads0 = [p.grad.detach().clone() for p in params]

    def reset_grads():                                  # leg c scales the gradients in place: every leg starts from the same ones
        for p, g in zip(params, grads0):
            p.grad.copy_(g)

    steps, graphs = {}, {}
    for leg in "abc":
        reset_grads()
        steps[leg] = make_leg(leg, params)
        steps[leg]()                                    # creates the state; warm
        steps[leg]()
        torch.cuda.synchronize()
        graphs[leg] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[leg]):
            steps[leg]()
        for _ in range(20):
            graphs[leg].replay()
        torch.cuda.synchronize()
    out = {leg: {"replay": [], "enqueue": [], "wall": []} for leg in "abc"}
    for _ in range(args.rounds):
        for leg in "abc":
            reset_grads()
            graphs[leg].replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.replays):
                graphs[leg].replay()
            e1.record()
            torch.cuda.synchronize()
            out[leg]["replay"].append(e0.elapsed_time(e1) * 1e3 / args.replays)
            steps[leg]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.replays):
                steps[leg]()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            out[leg]["enqueue"].append((t1 - t0) * 1e6 / args.replays)
            out[leg]["wall"].append((t2 - t0) * 1e6 / args.replays)
    fmt = lambda xs: " / ".join(f"{x:7.1f}" for x in xs)                    # noqa: E731
    print(f"{args.replays} steps per figure, legs alternated, {args.rounds} rounds; us per step")
    for leg in "abc":
        r = out[leg]
        print(f"  ({leg}) {NAMES[leg]:44s} replay {fmt(r['replay'])}   eager enqueue {fmt(r['enqueue'])}   eager wall {fmt(r['wall'])}")
    med = {leg: sorted(out[leg]["replay"])[len(out[leg]["replay"]) // 2] for leg in "abc"}
    print(f"  replay, (b) - (a): {med['b'] - med['a']:+.1f} us;  (c) - (b): {med['c'] - med['b']:+.1f} us")


if __name__ == "__main__":
    main()
