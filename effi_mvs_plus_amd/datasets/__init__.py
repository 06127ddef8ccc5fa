"""Scope row n4: the input pipeline and on-disk formats on either side of the hot path (reference: datasets/).

``data_io``      PFM reader / writer (datasets/data_io.py:61-126)
``general_eval`` DTU-style evaluation dataset (datasets/general_eval.py:8-228)
``tank``         Tanks-and-Temples evaluation dataset (datasets/tank.py:13-183)
``dtu_yao``      DTU training dataset (datasets/dtu_yao.py:9-214)
``blend``        BlendedMVS training dataset (datasets/blend.py:20-254)
``train_sample`` what the two training datasets share; ``prepare_train_sample`` = the device half of their samples
``find_dataset_def(name)`` the reference's lookup (datasets/__init__.py:5-8): ``MVSDataset`` of the module of that name

Parsing and matrix bookkeeping are host code like the reference's; the array arithmetic is HIP kernels, so ``__getitem__`` needs
the GPU and fails loudly without it: per view / 255, bilinear resize, HWC -> CHW for evaluation (``ops.image_prepare``); for
training / 255 and HWC -> CHW of all views of a sample batch in one launch (``ops.images_prepare``) and the per-stage depth / mask
pyramid the loss reads in another (``ops.gt_pyramid``).  A DataLoader worker, or ``device="host"``, returns the decoded bytes
instead, and ``prepare_sample`` / ``prepare_train_sample`` finish the sample (or collated batch) in the main process.
"""
import importlib


def find_dataset_def(dataset_name):
    """``MVSDataset`` of ``datasets/<dataset_name>.py``, e.g. "dtu_yao" (datasets/__init__.py:5-8)."""
    module = importlib.import_module("{}.{}".format(__name__, dataset_name))
    return getattr(module, "MVSDataset")


def prepare_train_sample(sample, device="cuda", out=None):
    from .train_sample import prepare_train_sample as impl
    return impl(sample, device, out)
