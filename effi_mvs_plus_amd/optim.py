"""The optimizer of the reference's training loop (``optim.AdamW(model.parameters(), lr, weight_decay=args.wd, eps=1e-8)``,
train.py:441; ``optimizer.step()``, train.py:263) on the HIP kernel of csrc/optim.hip.

``FusedAdamW`` stands beside ``torch.optim.AdamW``: the same constructor defaults, the same ``param_groups`` keys and the same
``state`` layout as torch's AdamW with ``capturable=True`` (``step`` a 0-dim fp32 tensor on the parameter's device, ``exp_avg``,
``exp_avg_sq``), so ``state_dict()`` / ``load_state_dict()`` -- the base class's -- exchange checkpoints with it in both directions
(the reference's resume, train.py:454), and ``train_graph.GraphedTrainStep`` takes it as it takes torch's: its ``capturable`` check
and its conversion of a float ``lr`` into a device tensor apply unchanged.  One ``step()`` is two launches per
``ops.adamw_max_tensors()`` tensors instead of torch's chain of ``_foreach_*`` operators.

The kernel writes through raw pointers, which autograd's version counters do not see: ``step()`` increments the counters of what it
wrote itself (``torch.autograd.graph.increment_version``: host-side bookkeeping, no launch) -- the per-module caches of folded and
packed weights (``packing.PackCache``) are keyed by them -- and ends with ``ops.drop_pack_cache()``, as a replayed graph does, so
the next eager forward, in either mode, packs the new weights.
"""
from __future__ import annotations

import torch
from torch.optim import Optimizer

from . import ops


class FusedAdamW(Optimizer):
    """``FusedAdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)``: decoupled weight-decay AdamW (the defaults
    of ``torch.optim.AdamW``).  ``lr`` is a float or a 0-dim fp32 tensor on the parameters' device (read by the kernel when it runs).
    fp32 parameters with dense fp32 gradients; ``amsgrad`` and ``maximize`` are not on the HIP path."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False):
        if isinstance(lr, torch.Tensor):
            if lr.numel() != 1:
                raise ValueError("Tensor lr must be 1-element")
        elif not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # the keys of torch.optim.AdamW's groups; capturable: the step counters live on the device
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=True, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)

    @staticmethod
    def _check_group(group):
        if group.get("amsgrad", False):
            raise NotImplementedError("FusedAdamW: amsgrad=True is not on the HIP path (csrc/optim.hip keeps no running maximum)")
        if group.get("maximize", False):
            raise NotImplementedError("FusedAdamW: maximize=True is not on the HIP path")
        if group.get("differentiable", False):
            raise NotImplementedError("FusedAdamW: differentiable=True is not on the HIP path")
        if not group.get("decoupled_weight_decay", True):
            raise NotImplementedError("FusedAdamW: coupled weight decay (torch.optim.Adam's) is not on the HIP path")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])

    def __setstate__(self, state):
        # load_state_dict() ends here with the checkpoint's groups and state.  A checkpoint of torch.optim.AdamW without capturable
        # keeps its step counters on the host and says capturable=False: this class has the one form, counters on the device
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsgrad", False)
            group.setdefault("maximize", False)
            group.setdefault("foreach", None)
            group.setdefault("differentiable", False)
            group.setdefault("fused", None)
            group.setdefault("decoupled_weight_decay", True)
            group["capturable"] = True
            self._check_group(group)
            for p in group["params"]:
                st = self.state.get(p, None)
                if st and "step" in st:
                    s = st["step"]
                    if not torch.is_tensor(s):
                        st["step"] = torch.tensor(float(s), dtype=torch.float32, device=p.device)
                    elif s.device != p.device or s.dtype != torch.float32:
                        st["step"] = s.to(device=p.device, dtype=torch.float32)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            self._check_group(group)
            beta1, beta2 = group["betas"]
            # the lists are rebuilt from self.state on every call: load_state_dict() replaces the state tensors, so no address is kept
            by_device = {}
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("FusedAdamW does not support sparse gradients")
                if p.dtype != torch.float32 or g.dtype != torch.float32:
                    raise TypeError(f"FusedAdamW: fp32 parameters and gradients only (got {p.dtype} / {g.dtype})")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                lists = by_device.setdefault(p.device, ([], [], [], [], []))
                lists[0].append(p)
                lists[1].append(g if g.is_contiguous() else g.contiguous())
                lists[2].append(st["exp_avg"])
                lists[3].append(st["exp_avg_sq"])
                lists[4].append(st["step"])
            for dev, (ps, gs, ms, vs, ss) in by_device.items():
                if dev.type == "cuda":
                    with torch.cuda.device(dev):
                        ops.adamw_multi(ps, gs, ms, vs, ss, group["lr"], beta1, beta2, group["eps"], group["weight_decay"])
                else:
                    ops.adamw_multi(ps, gs, ms, vs, ss, group["lr"], beta1, beta2, group["eps"], group["weight_decay"])   # raises: no CPU path
                torch.autograd.graph.increment_version(ps + ms + vs + ss)
        ops.drop_pack_cache()
        return loss
