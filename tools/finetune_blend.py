#!/usr/bin/env python3
"""Finetune on BlendedMVS with the captured training step (the reference's ``train.py --mode finetune --dataset blend``, argument
names as there): host-mode ``datasets.blend`` samples out of DataLoader workers -> ``GraphedTrainStep(depth_range="sample")``, which
reads every sample's own depth range on the device -> ``train_graph.train_epoch`` per epoch, a checkpoint per epoch.

usage: finetune_blend.py --trainpath DIR --trainlist FILE --logdir DIR [--loadckpt CKPT] [--ndepths 48,8,8] [--numdepth 384]
                         [--trainviews 3] [--batch_size 4] [--lr 0.001] [--wd 0.001] [--epochs 16] [--num_workers 4]
                         [--optimizer torch|fused]   (fused: optim.FusedAdamW on csrc/optim.hip; its checkpoints load into torch's AdamW)
                         [--clip-grad-norm X] [--skip-nonfinite]   (with --optimizer fused: clip the gradients by their global norm, and
                         leave the weights alone on a step whose gradient norm is not finite; both inside the captured step)"""
import argparse
import os
import sys

import torch
from torch.utils.data import DataLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from effi_mvs_plus_amd import train_graph  # noqa: E402
from effi_mvs_plus_amd.datasets import blend, prepare_train_sample  # noqa: E402
from effi_mvs_plus_amd.models import Effi_MVS_plus, mvs_loss_fused  # noqa: E402

MAX_WORKERS = 16


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--trainpath", required=True, help="train datapath")
    p.add_argument("--trainlist", required=True, help="train list")
    p.add_argument("--loadckpt", default=None, help="load a specific checkpoint")
    p.add_argument("--ndepths", type=str, default="48,8,8", help="ndepths")
    p.add_argument("--numdepth", type=int, default=384, help="the number of depth values")
    p.add_argument("--trainviews", type=int, default=3, help="trainviews")
    p.add_argument("--batch_size", type=int, default=4, help="train batch size")
    p.add_argument("--lr", type=float, default=0.001, help="learning rate")
    p.add_argument("--wd", type=float, default=0.001, help="weight decay")
    p.add_argument("--epochs", type=int, default=16, help="number of epochs to train")
    p.add_argument("--logdir", default="./checkpoints/debug/refine", help="the directory to save checkpoints/logs")
    p.add_argument("--GRUiters", type=str, default="3,3,3", help="iters")
    p.add_argument("--CostNum", type=int, default=3, help="CostNum")
    p.add_argument("--num_workers", type=int, default=4, help=f"DataLoader workers (at most {MAX_WORKERS})")
    p.add_argument("--optimizer", choices=("torch", "fused"), default="torch",
                   help="torch: torch.optim.AdamW(capturable=True); fused: effi_mvs_plus_amd.optim.FusedAdamW (the HIP kernel)")
    p.add_argument("--clip-grad-norm", type=float, default=None, metavar="X",
                   help="--optimizer fused: FusedAdamW(max_grad_norm=X), the global-norm clip of clip_grad_norm_ inside the step")
    p.add_argument("--skip-nonfinite", action="store_true",
                   help="--optimizer fused: a step whose gradient norm is inf or NaN changes nothing and is counted")
    args = p.parse_args(argv)
    if args.optimizer != "fused" and (args.clip_grad_norm is not None or args.skip_nonfinite):
        p.error("--clip-grad-norm and --skip-nonfinite need --optimizer fused: a captured step cannot clip with torch's optimizer")
    if args.clip_grad_norm is not None and not args.clip_grad_norm >= 0:
        p.error("--clip-grad-norm must be a number >= 0")
    if not 0 <= args.num_workers <= MAX_WORKERS:
        p.error(f"--num_workers must be in 0..{MAX_WORKERS}")
    if args.batch_size < 1 or args.epochs < 1:
        p.error("--batch_size and --epochs must be at least 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("finetune_blend: the training path runs on HIP kernels only; no GPU found")
    dev = torch.device("cuda:0")
    os.makedirs(args.logdir, exist_ok=True)
    model = Effi_MVS_plus(args)
    if args.loadckpt:
        print("loading model {}".format(args.loadckpt))
        model.load_state_dict(torch.load(args.loadckpt, map_location="cpu")["model"])
    model = model.to(dev).train()
    if args.optimizer == "fused":
        optimizer = train_graph.FusedAdamW(model.parameters(), lr=args.lr, weight_decay=args.wd, eps=1e-8,
                                           max_grad_norm=args.clip_grad_norm, skip_nonfinite=args.skip_nonfinite)
    else:
        optimizer = torch.optim.AdamW(model.parameters(), lr=args.lr, weight_decay=args.wd, eps=1e-8, capturable=True)   # train.py:441-442
    dataset = blend.MVSDataset(args.trainpath, args.trainlist, "finetune", args.trainviews, args.numdepth, device="host")
    loader = DataLoader(dataset, args.batch_size, shuffle=True, num_workers=args.num_workers, drop_last=True)
    if len(loader) == 0:
        raise SystemExit(f"finetune_blend: {len(dataset)} samples do not fill one batch of {args.batch_size}")
    scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer, args.lr, len(loader) * args.epochs + 100, pct_start=0.05,
                                                    cycle_momentum=False, anneal_strategy="linear")                  # train.py:510-511
    first = prepare_train_sample(next(iter(loader)), device=dev)     # shapes (and nothing else) of the captured step come from it
    step = train_graph.GraphedTrainStep(model, optimizer, first["imgs"], first["proj_matrices"], first["depth_values"], first["depth"],
                                        first["mask"], depth_range="sample", loss_fn=mvs_loss_fused)
    for epoch_idx in range(args.epochs):
        print("Epoch {}:".format(epoch_idx))
        mean_loss, steps = train_graph.train_epoch(step, loader, scheduler)
        state = optimizer.state_dict()
        # the captured step keeps lr as a device tensor; the checkpoint holds the float the reference's would (train.py:151-155)
        state["param_groups"] = [dict(g, lr=float(g["lr"])) for g in state["param_groups"]]
        torch.save({"epoch": epoch_idx, "model": model.state_dict(), "optimizer": state},
                   "{}/model_{:0>6}.ckpt".format(args.logdir, epoch_idx))
        print("Epoch {}/{}, {} steps, lr {:.6f}, mean train loss = {:.3f}".format(epoch_idx, args.epochs, steps,
                                                                                 float(optimizer.param_groups[0]["lr"]), mean_loss))
        if getattr(optimizer, "skipped_steps", None) is not None:    # (train_epoch has synchronised: these reads wait for nothing)
            print("  last gradient norm = {:.4g}, steps skipped for a non-finite norm so far = {}".format(
                float(optimizer.grad_norm), int(optimizer.skipped_steps)))


if __name__ == "__main__":
    main()
