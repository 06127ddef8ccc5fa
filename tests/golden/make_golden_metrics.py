"""Record what the REFERENCE computes for the training loss and the depth metrics -> tests/golden/g16_loss_metrics.npz.

Run on a machine that has the reference checkout (tests/refimport.REF_ROOT), CPU only:  python tests/golden/make_golden_metrics.py

  * ``Thres_metrics`` / ``AbsDepthError_metrics`` come from the reference's ``utils.py``, imported by file path behind a stub
    ``torchvision`` (utils.py:2 imports it for image logging only);
  * ``mvs_loss`` comes from the reference's ``models/module.py`` through tests/refimport.py.

Inputs are rebuilt from seeds by tests/loss_metrics_ref.py (``metrics_case`` / ``loss_case``); only OUTPUTS are recorded.
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import loss_metrics_ref as R  # noqa: E402
import refimport  # noqa: E402

OUT = os.path.join(HERE, "g16_loss_metrics.npz")

METRIC_CASES, LOSS_CASES = R.GOLDEN_METRIC_CASES, R.GOLDEN_LOSS_CASES


def load_utils():
    if "torchvision" not in sys.modules:
        tv = types.ModuleType("torchvision")
        tv.utils = types.ModuleType("torchvision.utils")
        sys.modules["torchvision"], sys.modules["torchvision.utils"] = tv, tv.utils
    spec = importlib.util.spec_from_file_location("reference_utils", os.path.join(refimport.REF_ROOT, "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def stage_dicts(gt, mask):
    first = {s: R.DLOSS.index(s) for s in (1, 2, 3, 4)}
    return ({"stage{}".format(s): torch.from_numpy(gt[i]) for s, i in first.items()},
            {"stage{}".format(s): torch.from_numpy(mask[i]) for s, i in first.items()})


def main():
    U = load_utils()
    ref = refimport.load_reference()
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, (shape, seed, kw) in METRIC_CASES.items():
            est, gt, valid = (torch.from_numpy(a) for a in R.metrics_case(shape, seed, **kw))
            out[name + "_abs"] = np.float32(U.AbsDepthError_metrics(est, gt, valid).item())
            out[name + "_thres"] = np.array([U.Thres_metrics(est, gt, valid, t).item() for t in R.ALL_THRES], dtype=np.float32)
            out[name + "_bands"] = np.array([U.AbsDepthError_metrics(est, gt, valid, list(b)).item() for b in R.TEST_BANDS], dtype=np.float32)
        for name, (sizes, B, seed, empty, with_grad) in LOSS_CASES.items():
            est, gt, mask = R.loss_case(sizes, B, seed, empty_output=empty)
            gt_ms, mask_ms = stage_dicts(gt, mask)
            inputs = [torch.from_numpy(e).requires_grad_(with_grad) for e in est]
            total, per = ref.module.mvs_loss(inputs, gt_ms, mask_ms, list(R.DLOSS), loss_rate=0.9)
            out[name + "_l"] = np.array([per["l{}".format(i)].item() for i in range(len(est))], dtype=np.float32)
            out[name + "_total"] = np.float32(total.item())
            if with_grad:
                total.backward()
                out[name + "_grad"] = np.concatenate([t.grad.numpy().reshape(-1) for t in inputs]).astype(np.float32)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", ", ".join(sorted(out)))


if __name__ == "__main__":
    main()
