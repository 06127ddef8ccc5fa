"""A whole training step -- forward in train mode -> loss -> backward -> optimizer step, the body of the reference's
``train_sample`` (train.py:229-263) -- captured ONCE into a HIP graph and replayed per sample.

Why: the eager step issues ~3,500 kernel launches (one per operator, forward and backward); their kernels add up to ~32 ms at the DTU
training shape (640x512, 5 views) while the host needs 45-55 ms to issue them, depending on the box.  A replayed graph has no
per-launch host work: the step takes what its kernels take.

What makes the step capturable:
  * every operator of the path launches on torch's current stream through the C ABI and never synchronises (include/effi_mvs_hip.h);
  * the depth range (``depth_values[:, 0]``, ``[:, -1]``): two modes, ``depth_range=``.
    ``"static"`` (the default): the 12 inverse-depth -> depth conversions of the step and their backward take the range BY VALUE
    (``EFFI_PW_INV_TO_DEPTH`` / ``_BWD`` of ``effi_pointwise_f32``), so it is fixed at capture time (``model.static_depth_range``
    while the constructor runs) and every replayed sample must have it.  DTU training uses one range for every sample
    (datasets/dtu_yao.py: 425 mm + 192 x 2.5 mm).
    ``"sample"``: the conversions read every sample's range on the device from the captured ``depth_values`` buffer
    (``effi_inv_to_depth_ranged_f32`` / ``_bwd``: the same arithmetic, bit for bit) -- as every other operator of the step already
    does -- so any range replays and the samples of a batch may each have their own: BlendedMVS (datasets/blend.py), whose samples
    carry the range of their reference view (the reference's finetune, train.py --mode finetune, batch_size 4).  Nothing is set on
    the model; what is checked per sample is only that the range is usable (0 < first < last < inf);
  * the loss is ``mvs_loss_static`` (mean over the valid pixels as sum x mask / count: the reference's boolean indexing has a
    data-dependent shape and synchronises), or ``mvs_loss_fused``: the same loss as two HIP launches forward and one backward
    instead of ~250 small torch launches (csrc/metrics.hip; 26.5 -> 25.8 ms per replayed step at 640x512);
  * the optimizer must be constructed with ``capturable=True`` (its step counter lives on the device);
  * the learning rate must be a TENSOR: a Python-float ``lr`` would be baked into the captured kernels' arguments and every replay
    would train at the capture-time rate, whatever a scheduler sets afterwards (the reference steps ``OneCycleLR`` after every
    sample, train.py:127,510-511).  ``GraphedTrainStep`` converts each group's float ``lr`` to a 0-dim device tensor in place;
    torch's schedulers ``fill_`` a tensor ``lr`` (``_update_param_group_val``), so ``scheduler.step()`` between replays works as
    in the eager loop.  ``betas`` / ``eps`` / ``weight_decay`` ARE captured by value: a scheduler that cycles momentum
    (``OneCycleLR(cycle_momentum=True)``; the reference passes ``False``) is refused;
  * BatchNorm's ``num_batches_tracked`` is incremented by the forward kernel.

Weights are updated by the replayed optimizer on the device, which does not bump ``Tensor._version``: the packed-weight cache of
``ops`` is dropped after every replay, so an eager forward of the same model in between sees the new weights.  (The same holds for
code that writes ``p.data`` directly: call ``ops.drop_pack_cache()`` after such an update.)

The weight-gradient arena and the packed-weight cache of ``autograd`` / ``ops`` know about capture (a block / entry made outside the
graph is not reused inside it).
"""
from __future__ import annotations

import copy
from typing import Callable, Dict, Sequence

import torch

from . import metrics as _metrics
from .graph import ReplayGraph
from .models.module import mvs_loss_fused, _mvs_loss_fused_vector, mvs_loss_static  # noqa: F401  (re-exported: the losses a graphed step uses)
from .optim import FusedAdamW  # noqa: F401  (re-exported: AdamW on csrc/optim.hip, a drop-in for torch.optim.AdamW(capturable=True) here)

DLOSS = (1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4)            # train.py:246: stage of each of the 13 depth maps


class GraphedTrainStep:
    """``step = GraphedTrainStep(model, optimizer, imgs, proj_matrices, depth_values, depth_gt_ms, mask_ms)`` captures the step on
    the given sample (its tensors fix shapes and the depth range); ``loss = step(imgs, proj_matrices, depth_values, depth_gt_ms,
    mask_ms)`` copies a new sample into the captured buffers and replays.  Returns the loss tensor of the captured graph (valid
    until the next call; with ``scalars=metrics.TRAIN_SCALARS`` the step's metrics are in ``step.scalars``, a device vector in the
    order of ``scalars.keys``).  ``warmup`` eager steps run first on a side stream (allocator and lazy initialisation; PyTorch's recipe
    for whole-network capture) -- model and optimizer state are restored afterwards, so the first replay is step 1."""

    def __init__(self, model: torch.nn.Module, optimizer: torch.optim.Optimizer, imgs: torch.Tensor, proj_matrices: Dict[str, torch.Tensor],
                 depth_values: torch.Tensor, depth_gt_ms: Dict[str, torch.Tensor], mask_ms: Dict[str, torch.Tensor],
                 dloss: Sequence[int] = DLOSS, loss_fn: Callable = mvs_loss_static, warmup: int = 2, scalars=None,
                 depth_range: str = "static"):
        if depth_range not in ("static", "sample"):
            raise ValueError(f"GraphedTrainStep: depth_range must be 'static' or 'sample', got {depth_range!r}")
        self.range_mode = depth_range
        for grp in optimizer.param_groups:
            if not grp.get("capturable", False):
                raise ValueError("GraphedTrainStep: construct the optimizer with capturable=True")
            if not torch.is_tensor(grp["lr"]):
                # a float would be frozen into the graph (see the module docstring); schedulers fill_ a tensor lr in place
                grp["lr"] = torch.tensor(float(grp["lr"]), dtype=torch.float32, device=imgs.device)
            elif grp["lr"].device != imgs.device:
                raise ValueError("GraphedTrainStep: a tensor lr must live on the model's device")
        if not model.training:
            raise ValueError("GraphedTrainStep: model.train() first")
        self.model, self.optimizer, self.dloss, self.loss_fn = model, optimizer, tuple(dloss), loss_fn
        # scalars=metrics.TRAIN_SCALARS: the captured step also computes the metrics train_sample logs (train.py:268-271) on its last
        # depth map (self.depth_est) against stage4, in one metrics call; self.scalars is their device vector (keys: scalars.keys)
        self.scalar_set, self.scalars, self.depth_est = scalars, None, None
        clone = lambda t: t.detach().clone()                      # noqa: E731
        self.imgs, self.depth_values = clone(imgs), clone(depth_values)
        self.proj = {k: clone(v) for k, v in proj_matrices.items()}
        self.gt = {k: clone(v) for k, v in depth_gt_ms.items()}
        self.mask = {k: clone(v) for k, v in mask_ms.items()}
        self._betas = [tuple(grp.get("betas", ())) for grp in optimizer.param_groups]
        # samples on the device whose range differs from the captured one ("static") or is unusable ("sample") are counted here (no
        # host sync per step): check_ranges()
        self.range_mismatches = torch.zeros((), dtype=torch.int64, device=imgs.device)
        if depth_range == "sample":
            # the step reads each sample's range from self.depth_values: nothing is captured by value, nothing is set on the model
            self.depth_range = None
            if not bool(self._usable(depth_values).all()):
                raise ValueError("GraphedTrainStep: unusable depth range in the capture batch (0 < first < last < inf expected)")
            self._build(model, optimizer, imgs, warmup)
            return
        lo, hi = depth_values[:, 0], depth_values[:, -1]
        if not (bool((lo == lo[0]).all()) and bool((hi == hi[0]).all())):
            raise NotImplementedError("GraphedTrainStep: the samples of a batch must share their depth range")
        self.depth_range = (float(lo[0]), float(hi[0]))
        # the range is a constant of the CAPTURED step only: the attribute lives on the model while this constructor runs its eager
        # and captured steps and is removed again, so later eager train-mode forwards of the model read their own sample's range
        model.static_depth_range = self.depth_range
        try:
            self._build(model, optimizer, imgs, warmup)
        finally:
            model.static_depth_range = None

    def _build(self, model, optimizer, imgs, warmup):
        # warm-up on a side stream, then restore the state it changed (weights, BatchNorm buffers, optimizer moments)
        model_state = copy.deepcopy(model.state_dict())
        opt_state = copy.deepcopy(optimizer.state_dict())
        side = torch.cuda.Stream(device=imgs.device)
        side.wait_stream(torch.cuda.current_stream(imgs.device))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                self._step()
        torch.cuda.current_stream(imgs.device).wait_stream(side)
        torch.cuda.synchronize(imgs.device)
        with torch.no_grad():
            model.load_state_dict(model_state)                    # copies in place: parameter addresses stay
        optimizer.load_state_dict(opt_state)
        if not optimizer.state_dict()["state"]:
            # a fresh optimizer creates its state lazily in step(): that must not happen inside the capture with different
            # addresses per replay -- so take one eager step to create it, then zero it
            self._step()
            torch.cuda.synchronize(imgs.device)
            with torch.no_grad():
                model.load_state_dict(model_state)
                for st in optimizer.state.values():
                    for v in st.values():
                        if torch.is_tensor(v):
                            v.zero_()
        self.graph = torch.cuda.CUDAGraph()
        optimizer.zero_grad(set_to_none=True)
        self._drop_caches()
        with torch.cuda.graph(self.graph):
            self.loss = self._step()
        self._drop_caches()                                       # nothing outside the graph keeps pointing into its memory pool
        skipped = getattr(optimizer, "skipped_steps", None)       # FusedAdamW's non-finite guard: warm-up steps do not count
        if torch.is_tensor(skipped):
            skipped.zero_()
        self.replays = 0

    @staticmethod
    def _drop_caches():
        from . import autograd, ops
        ops._PACK_CACHE.clear()
        autograd.grad_arena.blocks.clear()

    def _step(self):
        self.optimizer.zero_grad(set_to_none=True)
        out = self.model(self.imgs, self.proj, self.depth_values)
        loss, _ = self.loss_fn(out["depth"], self.gt, self.mask, self.dloss)
        loss.backward()
        self.optimizer.step()
        if self.scalar_set is not None:
            self.depth_est = out["depth"][-1].detach()
            self.scalars = _metrics.depth_scalars(out["depth"][-1], self.gt["stage4"], self.mask["stage4"], self.scalar_set.thresholds,
                                                  self.scalar_set.bands)
        return loss

    def load_sample(self, imgs, proj_matrices, depth_values, depth_gt_ms, mask_ms):
        """Copy a sample into the captured buffers (asynchronous device copies on the current stream).  ``"static"`` mode: the depth
        range of the sample must be the captured one (two kernels hold it by value); ``"sample"`` mode: it must be usable (0 < first
        < last < inf).  A host tensor is checked here and refused before anything is written; a device tensor is checked on the device
        without a sync -- ``check_ranges()`` reads the count."""
        self._check_range(depth_values)
        self.imgs.copy_(imgs, non_blocking=True)
        self.depth_values.copy_(depth_values, non_blocking=True)
        for k in self.proj:
            self.proj[k].copy_(proj_matrices[k], non_blocking=True)
        for k in self.gt:
            self.gt[k].copy_(depth_gt_ms[k], non_blocking=True)
            self.mask[k].copy_(mask_ms[k], non_blocking=True)

    @staticmethod
    def _usable(depth_values):
        """Per sample: 0 < first < last < inf (NaN fails every comparison)."""
        lo, hi = depth_values[:, 0], depth_values[:, -1]
        return (lo > 0) & (lo < hi) & (hi < float("inf"))

    def _check_range(self, depth_values):
        lo, hi = depth_values[:, 0], depth_values[:, -1]
        if self.range_mode == "sample":
            ok = self._usable(depth_values)
            if not depth_values.is_cuda:
                if not bool(ok.all()):
                    b = int((~ok).nonzero()[0])
                    raise ValueError(f"GraphedTrainStep: unusable depth range ({float(lo[b])}, {float(hi[b])}) in sample {b} of the "
                                     "batch: 0 < first < last < inf expected")
            else:
                self.range_mismatches += (~ok).any().to(torch.int64)
            return
        if not depth_values.is_cuda:
            if not (bool((lo == self.depth_range[0]).all()) and bool((hi == self.depth_range[1]).all())):
                raise ValueError(f"GraphedTrainStep: sample depth range ({float(lo[0])}, {float(hi[0])}) differs from the captured "
                                 f"{self.depth_range}; capture a step per range (datasets/dtu_yao.py uses one)")
        else:
            self.range_mismatches += ((lo != self.depth_range[0]) | (hi != self.depth_range[1])).any().to(torch.int64)

    def load_raw_sample(self, sample):
        """``load_sample`` for a host-mode sample of the training datasets (``datasets.dtu_yao`` / ``datasets.blend`` with
        ``device="host"`` or out of DataLoader workers; one sample or a default-collated batch): the decoded bytes go to the device
        and the two kernels of csrc/train_input.hip write ``imgs`` and the depth / mask pyramid straight into the captured buffers;
        ``proj_matrices`` and ``depth_values`` are copied.  The depth range is checked as in ``load_sample`` (in ``"static"`` mode a
        BlendedMVS sample with another range is refused the same way; ``"sample"`` mode takes it).  ``step.load_raw_sample(s);
        step()`` is the loop body (``train_epoch``)."""
        from .datasets.train_sample import train_arrays
        dv = sample["depth_values"]
        self._check_range(dv if dv.dim() == 2 else dv.unsqueeze(0))
        train_arrays(sample, self.imgs.device, out=(self.imgs, self.gt, self.mask))
        self.depth_values.copy_(dv, non_blocking=True)                   # an unbatched sample broadcasts over the batch of one
        for k in self.proj:
            self.proj[k].copy_(sample["proj_matrices"][k], non_blocking=True)

    def check_ranges(self):
        """Synchronises; raises if any device-resident sample loaded so far had another depth range than the captured one
        (``"sample"`` mode: an unusable one)."""
        n = int(self.range_mismatches.item())
        if n and self.range_mode == "sample":
            raise ValueError(f"GraphedTrainStep: {n} loaded batch(es) had an unusable depth range (0 < first < last < inf expected)")
        if n:
            raise ValueError(f"GraphedTrainStep: {n} replayed sample(s) had a depth range other than the captured {self.depth_range}")

    def __call__(self, imgs=None, proj_matrices=None, depth_values=None, depth_gt_ms=None, mask_ms=None):
        for grp, b in zip(self.optimizer.param_groups, self._betas):
            if tuple(grp.get("betas", ())) != b:
                raise ValueError("GraphedTrainStep: betas changed after capture (a momentum-cycling scheduler?): they are captured by value")
        if imgs is not None:
            self.load_sample(imgs, proj_matrices, depth_values, depth_gt_ms, mask_ms)
        self.graph.replay()
        self.replays += 1
        from . import ops
        ops.drop_pack_cache()              # the replay updated the weights on the device without bumping their version counters
        return self.loss


def train_epoch(step, loader, scheduler=None):
    """One epoch of the reference's loop (train.py:115-127) on a captured step: for every batch of a host-mode dataset
    ``step.load_raw_sample(batch)``, ``step()``, ``scheduler.step()``; the losses are added on the device (no host sync per step).
    Ends with ``step.check_ranges()`` (the one sync) and returns (mean loss, number of steps)."""
    total, steps = None, 0
    for batch in loader:
        step.load_raw_sample(batch)
        loss = step()
        if scheduler is not None:
            scheduler.step()
        total = loss.detach().clone() if total is None else total.add_(loss.detach())
        steps += 1
    step.check_ranges()
    return (float(total) / steps if steps else float("nan")), steps


class GraphedTestStep:
    """The body of the reference's ``test_sample_depth`` (train.py:293-353) -- eval-mode forward, ``mvs_loss_fused`` forward and the
    ``TEST_SCALARS`` metrics of the last depth map against stage4 -- captured once (``graph.ReplayGraph``) and replayed per sample,
    its scalars added on the device into a ``DeviceAverageMeter`` that carries ``loss``, ``depth_loss``, the metrics and
    ``l0 .. l{K-1}``.  ``step(imgs, proj_matrices, depth_values, depth_gt_ms, mask_ms)`` copies the sample into the captured buffers
    and replays: no host synchronisation per sample.  ``step.mean()`` returns the dictionary ``test()`` prints (train.py:226; without
    its wall-clock ``time``), and is the only sync.  ``step.outputs`` are the captured forward's outputs (valid until the next call);
    ``step.loss`` / ``step.per_output`` [K] / ``step.scalars`` are the total, l0 .. l{K-1} and the metrics of the last replay.  As in
    ``GraphedTrainStep`` the eval-mode forward reads the depth range from ``depth_values`` on the device, so any range replays."""

    def __init__(self, model: torch.nn.Module, imgs: torch.Tensor, proj_matrices: Dict[str, torch.Tensor], depth_values: torch.Tensor,
                 depth_gt_ms: Dict[str, torch.Tensor], mask_ms: Dict[str, torch.Tensor], dloss: Sequence[int] = DLOSS,
                 loss_rate: float = 0.9):
        if model.training:
            raise ValueError("GraphedTestStep: model.eval() first")
        self.model, self.dloss, self.loss_rate, self.scalar_set = model, tuple(dloss), float(loss_rate), _metrics.TEST_SCALARS
        K = len(self.dloss)
        self.loss_keys = ("loss",) + tuple("l{}".format(i) for i in range(K))
        self.meter = _metrics.DeviceAverageMeter(("depth_loss",) + tuple(self.scalar_set.keys) + self.loss_keys, device=imgs.device)
        self._graph = ReplayGraph(self._body, (imgs, proj_matrices, depth_values, depth_gt_ms, mask_ms))
        self.meter.data.zero_()                                   # the warm-up and capture passes added their sample
        self.outputs, self.loss, self.per_output, self.scalars = self._graph.outputs[0]

    def _body(self, imgs, proj_matrices, depth_values, depth_gt_ms, mask_ms):
        out = self.model(imgs, proj_matrices, depth_values)
        K = len(self.dloss)
        if len(out["depth"]) != K:
            raise ValueError("GraphedTestStep: dloss names {} outputs, the model returns {}".format(K, len(out["depth"])))
        total, per = _mvs_loss_fused_vector(out["depth"], depth_gt_ms, mask_ms, self.dloss, loss_rate=self.loss_rate)
        sc = _metrics.depth_scalars(out["depth"][-1], depth_gt_ms["stage4"], mask_ms["stage4"], self.scalar_set.thresholds,
                                    self.scalar_set.bands, acc=self.meter.slots(self.scalar_set.keys[0], len(self.scalar_set.keys)))
        self.meter.slots("l0", K).add_(per)                       # fp32 values added into the fp64 sums
        self.meter.slots("depth_loss", 1).add_(per[K - 1:])       # train.py:319: depth_loss = l{iters}, the last output's
        self.meter.slots("loss", 1).add_(total.reshape(1))
        return out, total, per, sc

    def __call__(self, imgs=None, proj_matrices=None, depth_values=None, depth_gt_ms=None, mask_ms=None):
        if imgs is not None:
            self._graph.load(0, imgs, proj_matrices, depth_values, depth_gt_ms, mask_ms)
        self._graph.replay(0)
        self.meter.tick()
        return self.loss

    def mean(self) -> Dict[str, float]:
        return self.meter.mean()
