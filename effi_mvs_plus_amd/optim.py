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

``FusedAdamW(max_grad_norm=..., skip_nonfinite=...)`` clips by the global gradient norm and leaves the weights alone on a step whose
norm is not finite -- on the device, inside ``step()``, so also inside a captured step, which cannot look at its loss before it
updates (three more launches for the model).  ``grad_norm(parameters)`` is the same reduction on its own.
"""
from __future__ import annotations

import torch
from torch.optim import Optimizer

from . import ops


class FusedAdamW(Optimizer):
    """``FusedAdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)``: decoupled weight-decay AdamW (the defaults
    of ``torch.optim.AdamW``).  ``lr`` is a float or a 0-dim fp32 tensor on the parameters' device (read by the kernel when it runs).
    fp32 parameters with dense fp32 gradients; ``amsgrad`` and ``maximize`` are not on the HIP path.

    ``max_grad_norm`` (a number >= 0): clip by the global 2-norm over every parameter of every group that has a gradient, as
    ``torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)`` before the step would -- with one difference: ``p.grad`` stays as
    backward wrote it (``clip_grad_norm_`` scales it in place); the update kernel multiplies each gradient element by the
    coefficient as it reads it.  ``skip_nonfinite``: a step whose norm is inf or NaN (or above the largest fp32 number) changes
    nothing -- no parameter, no moment, no step counter -- and is counted; without ``max_grad_norm`` it only guards.  Both are
    decided on the device, inside ``step()``, so they hold in a captured step; the host reads nothing.  After a guarded ``step()``,
    ``grad_norm`` / ``clip_coef`` (0-dim fp32) and ``skipped_steps`` (0-dim int64) are device tensors at fixed addresses; they are
    attributes of the optimizer like the two options, not ``param_groups`` keys and not in ``state_dict()``, which stays
    ``torch.optim.AdamW``'s.  With either option the gradients must be on one device.  One guarded step adds one launch per
    ``ops.gradnorm_max_tensors()`` gradients and one more; with both options left at their defaults no launch is added."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False,
                 max_grad_norm=None, skip_nonfinite=False):
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
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm} (a number >= 0, inf included, or None)")
        # the keys of torch.optim.AdamW's groups; capturable: the step counters live on the device
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=True, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        # attributes, not group keys: the norm is global over all groups, and the groups stay those of torch.optim.AdamW
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._clip = self._skipped = None               # created by the first guarded step(); the addresses then stay

    @property
    def grad_norm(self):
        """0-dim fp32 device tensor: the global gradient norm of the last ``step()`` (None before the first guarded step)."""
        return None if self._clip is None else self._clip[0]

    @property
    def clip_coef(self):
        """0-dim fp32 device tensor: the coefficient the last ``step()`` applied, min(1, max_grad_norm / (norm + 1e-6))."""
        return None if self._clip is None else self._clip[1]

    @property
    def skipped_steps(self):
        """0-dim int64 device tensor: the steps whose gradient norm was not finite (None before the first guarded step)."""
        return self._skipped

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
        for k in ("max_grad_norm", "_clip", "_skipped"):        # an unpickled optimizer carries defaults, state and groups only
            self.__dict__.setdefault(k, None)
        self.__dict__.setdefault("skip_nonfinite", False)
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
        guarded = self.max_grad_norm is not None or self.skip_nonfinite
        work, all_grads = [], {}
        for group in self.param_groups:
            self._check_group(group)
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
                if guarded:
                    all_grads.setdefault(p.device, []).append(lists[1][-1])
            work.append((group, by_device))
        clip = None
        if guarded and all_grads:
            if len(all_grads) > 1:
                raise ValueError("FusedAdamW: max_grad_norm / skip_nonfinite take the norm over all parameters, which must then be on one "
                                 f"device (gradients on {sorted(str(d) for d in all_grads)})")
            (dev, grads), = all_grads.items()
            if self._clip is None or self._clip.device != dev:
                self._clip = torch.zeros(4, dtype=torch.float32, device=dev)
                self._skipped = torch.zeros((), dtype=torch.int64, device=dev)
            clip = self._clip
            max_norm = float("inf") if self.max_grad_norm is None else self.max_grad_norm
            if dev.type == "cuda":
                with torch.cuda.device(dev):
                    ops.grad_norm_multi(grads, max_norm, clip, self._skipped)
            else:
                ops.grad_norm_multi(grads, max_norm, clip, self._skipped)   # raises: no CPU path
        for group, by_device in work:
            beta1, beta2 = group["betas"]
            for dev, (ps, gs, ms, vs, ss) in by_device.items():
                hyper = (group["lr"], beta1, beta2, group["eps"], group["weight_decay"], clip, self.skip_nonfinite and clip is not None)
                if dev.type == "cuda":
                    with torch.cuda.device(dev):
                        ops.adamw_multi(ps, gs, ms, vs, ss, *hyper)
                else:
                    ops.adamw_multi(ps, gs, ms, vs, ss, *hyper)   # raises: no CPU path
                torch.autograd.graph.increment_version(ps + ms + vs + ss)
        ops.drop_pack_cache()
        return loss


def grad_norm(parameters):
    """The global 2-norm of the gradients of ``parameters`` (a tensor or an iterable of tensors; those without a gradient are left
    out) as a 0-dim fp32 device tensor, by the reduction ``FusedAdamW(max_grad_norm=...)`` uses: for a loop that keeps torch's
    optimizer, or only logs.  fp32 gradients on one GPU; nothing is modified and the host does not wait."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in parameters if p.grad is not None]
    if not grads:
        raise ValueError("grad_norm: no parameter has a gradient")
    if grads[0].is_cuda:
        with torch.cuda.device(grads[0].device):
            return ops.grad_norm_multi(grads)[0]
    return ops.grad_norm_multi(grads)[0]                # raises: no CPU path
