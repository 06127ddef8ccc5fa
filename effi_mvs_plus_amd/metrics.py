"""The depth metrics of the reference's drivers on the device (reference: utils.py:103-160, train.py:266-271,322-337).

``from effi_mvs_plus_amd.metrics import *`` replaces ``from utils import *`` for ``Thres_metrics`` and ``AbsDepthError_metrics``: same
signatures, same values, but each is ONE call of ``ops.depth_metrics`` (a pass over the map and a finishing launch, csrc/metrics.hip)
that returns a 0-dim DEVICE tensor -- the reference selects the valid pixels by boolean indexing (a data-dependent shape and a host
sync per metric) and ``tensor2float`` reads every scalar back.  ``depth_scalars`` computes all metrics of a sample in one such
call; ``TRAIN_SCALARS`` / ``TEST_SCALARS`` are the sets ``train_sample`` / ``test_sample_depth`` log; ``DeviceAverageMeter`` is
``DictAverageMeter`` with its sums on the device, so a validation loop synchronises once, in ``mean()``.

Values: the per-image counts are exact integers, the per-image sums fp64; every per-image value is the fp32 rounding of its fp64
quotient and the batch average is one more rounding.  The mask is either the reference's bool
(``mask > 0.5``) or the float mask itself (valid where > 0.5, compared in the kernel).
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from . import ops

__all__ = ["Thres_metrics", "AbsDepthError_metrics", "depth_scalars", "ScalarSet", "TRAIN_SCALARS", "TEST_SCALARS", "DeviceAverageMeter"]


class ScalarSet(NamedTuple):
    """A set of metrics of one depth map: ``keys`` name [abs_mean, one per threshold, one per band] in that order."""
    thresholds: Tuple[float, ...]
    bands: Tuple[Tuple[float, float], ...]
    keys: Tuple[str, ...]


# train.py:268-271
TRAIN_SCALARS = ScalarSet((2.0, 4.0, 8.0), (), ("abs_depth_error", "thres2mm_error", "thres4mm_error", "thres8mm_error"))
# train.py:324-336
TEST_SCALARS = ScalarSet((0.125, 0.25, 0.5, 1.0, 20.0), ((0.0, 2.0), (2.0, 4.0), (4.0, 8.0), (8.0, 14.0), (14.0, 20.0), (20.0, 1e5)),
                         ("abs_depth_error", "thres2mm_error", "thres4mm_error", "thres8mm_error", "thres14mm_error", "thres20mm_error",
                          "thres2mm_abserror", "thres4mm_abserror", "thres8mm_abserror", "thres14mm_abserror", "thres20mm_abserror",
                          "thres>20mm_abserror"))


@ops.on_tensor_device
def depth_scalars(depth_est: torch.Tensor, depth_gt: torch.Tensor, mask: torch.Tensor, thresholds: Sequence[float] = (),
                  bands: Sequence[Sequence[float]] = (), acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """All metrics of depth_est / depth_gt / mask [B,H,W] in one call: -> fp32 device vector [abs_mean, Thres_metrics per threshold,
    AbsDepthError_metrics per band]; ``acc`` (fp64 device vector of that length, e.g. ``DeviceAverageMeter.slots``) += it."""
    est = depth_est.detach().contiguous()
    return ops.depth_metrics(est, depth_gt.detach().contiguous(), mask.contiguous(), thresholds, bands, acc)[0]


def Thres_metrics(depth_est, depth_gt, mask, thres):
    """utils.py:139-147: mean over the images of the share of valid pixels with |est - gt| > thres -> 0-dim device tensor."""
    assert isinstance(thres, (int, float))
    return depth_scalars(depth_est, depth_gt, mask, (thres,))[1]


def AbsDepthError_metrics(depth_est, depth_gt, mask, thres=None):
    """utils.py:151-160: mean over the images of the mean |est - gt| over the valid pixels, or over those of them with
    thres[0] <= |est - gt| <= thres[1] (0 for an image without any) -> 0-dim device tensor."""
    if thres is None:
        return depth_scalars(depth_est, depth_gt, mask)[0]
    return depth_scalars(depth_est, depth_gt, mask, (), ((float(thres[0]), float(thres[1])),))[1]


class DeviceAverageMeter:
    """``DictAverageMeter`` (utils.py:103-122) with the sums in one fp64 DEVICE vector: ``update`` adds a dictionary of 0-dim device
    tensors (or floats) without reading them back, ``mean()`` is the only synchronisation.  With ``keys`` given up front, kernels and
    captured graphs can add into ``slots(first_key, n)`` themselves (``depth_scalars(..., acc=...)``) and call ``tick()`` per sample."""

    def __init__(self, keys: Optional[Sequence[str]] = None, device=None):
        self.keys = None
        self.data = None
        self.count = 0
        self.device = torch.device(device) if device is not None else None
        if keys is not None:
            self._create(keys)

    def _create(self, keys):
        self.keys = tuple(keys)
        if len(set(self.keys)) != len(self.keys):
            raise ValueError("DeviceAverageMeter: duplicate keys")
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.data = torch.zeros(len(self.keys), dtype=torch.float64, device=self.device)

    def slots(self, first_key: str, n: int) -> torch.Tensor:
        """The n consecutive sums starting at ``first_key`` (a view: what is added to it is averaged by ``mean()``)."""
        i = self.keys.index(first_key)
        if i + n > len(self.keys):
            raise ValueError("DeviceAverageMeter.slots: past the end")
        return self.data[i:i + n]

    def tick(self, n: int = 1):
        """Count n samples whose values were added into ``slots`` directly."""
        self.count += n

    def update(self, new_input: Dict[str, object]):
        if self.keys is None:
            first = next((v for v in new_input.values() if torch.is_tensor(v)), None)
            if self.device is None and first is not None:
                self.device = first.device
            self._create(new_input.keys())
        if set(new_input) != set(self.keys):
            raise ValueError("DeviceAverageMeter.update: the keys differ from the first update's")
        vals = []
        for k in self.keys:
            v = new_input[k]
            if torch.is_tensor(v):
                if v.numel() != 1:
                    raise NotImplementedError("invalid data {}: {} elements".format(k, v.numel()))
                vals.append(v.detach().reshape(()).to(device=self.device, dtype=torch.float64))
            elif isinstance(v, (int, float)):
                vals.append(torch.tensor(float(v), dtype=torch.float64, device=self.device))
            else:
                raise NotImplementedError("invalid data {}: {}".format(k, type(v)))
        self.data += torch.stack(vals)
        self.count += 1

    def mean(self) -> Dict[str, float]:
        if self.keys is None:
            return {}
        vals = (self.data / self.count).tolist() if self.count else [float("nan")] * len(self.keys)
        return dict(zip(self.keys, vals))
