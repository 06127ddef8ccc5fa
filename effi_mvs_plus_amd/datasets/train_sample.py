"""What the two training datasets (``dtu_yao``, ``blend``) share: the cam-file reader, the host form of a sample and its device
half.

A host-mode sample (``device="host"``, or inside a DataLoader worker) holds, in place of ``imgs`` / ``depth`` / ``mask``,
  ``imgs_u8``     [N,h,w,3] uint8     the decoded views
  ``depth_raw``   [h,w] fp32          the stage-4 depth map, already cut to the training size
  ``mask_raw``    [h,w] uint8         DTU: the visibility PNG at the same pixels      -- or --
  ``depth_range`` [2] fp32            BlendedMVS: depth_min, depth_max of the reference view
and default collation puts a batch dimension in front of each.  ``prepare_train_sample`` runs the two kernels of
csrc/train_input.hip on the whole sample or collated batch (``ops.images_prepare``, ``ops.gt_pyramid``: one launch each) and
returns the reference's dictionary on the device.
"""
import numpy as np
import torch

from .. import ops

RAW_KEYS = ("imgs_u8", "depth_raw", "mask_raw", "depth_range")


def parse_train_cam_file(path):
    """cam.txt -> (intrinsics [3,3] as stored, extrinsics [4,4], the fields of the depth line as floats)
    (datasets/dtu_yao.py:57-68, datasets/blend.py:71-86: neither scales the intrinsics)."""
    with open(path) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape(4, 4)
    intrinsics = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape(3, 3)
    return intrinsics, extrinsics, [float(v) for v in lines[11].split()]


def read_pair_file(path):
    """pair.txt -> [(ref_view, [src views by score])], every view kept (datasets/dtu_yao.py:38-43)."""
    out = []
    with open(path) as f:
        for _ in range(int(f.readline())):
            ref = int(f.readline().rstrip())
            out.append((ref, [int(x) for x in f.readline().rstrip().split()[1::2]]))
    return out


def stack_views(raws, what):
    """list of decoded views -> [N,h,w,3] uint8 tensor (np.stack of the reference: the views of a sample share their size)."""
    for r in raws:
        if r.ndim != 3 or r.shape[2] != 3:
            raise TypeError(f"{what}: 8-bit RGB image expected, got an array of shape {r.shape}")
    return torch.from_numpy(np.stack(raws))


def train_arrays(sample, device="cuda", out=None):
    """The device half proper: the raw entries of a host-mode sample (or collated batch) -> (imgs [B,N,3,h,w], depth_ms, mask_ms
    with [B,h_k,w_k] per stage) on ``device``, two launches.  ``out=(imgs, depth_ms, mask_ms)`` writes into given tensors of these
    (batched) shapes.  -> (imgs, depth_ms, mask_ms, batched)."""
    raws, depth = sample["imgs_u8"], sample["depth_raw"]
    batched = raws.dim() == 5
    mask, rng = sample.get("mask_raw"), sample.get("depth_range")
    if not batched:
        raws, depth = raws.unsqueeze(0), depth.unsqueeze(0)
        mask = None if mask is None else mask.unsqueeze(0)
        rng = None if rng is None else rng.unsqueeze(0)
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise ops.EffiLibraryError(f"the training input is prepared by HIP kernels and device {device} cannot run them "
                                   "(no CPU fallback); device=\"host\" returns the raw sample")
    up = lambda t: None if t is None else t.contiguous().to(device, non_blocking=True)      # noqa: E731
    o_imgs, o_depth, o_mask = out if out is not None else (None, None, None)
    with torch.cuda.device(device):
        imgs = ops.images_prepare(up(raws), out=o_imgs)
        depth_ms, mask_ms = ops.gt_pyramid(up(depth.float()), mask_u8=up(mask), depth_range=None if rng is None else up(rng.float()),
                                           out=None if o_depth is None else (o_depth, o_mask))
    return imgs, depth_ms, mask_ms, batched


def prepare_train_sample(sample, device="cuda", out=None):
    """Device half of the training datasets' ``__getitem__`` for a host-mode sample or a default-collated batch of them, in place of
    the reference's ``tocuda(sample)`` (train.py:232): -> {"imgs" [N,3,h,w], "proj_matrices" stage0..4, "depth" stage1..4 [h_k,w_k],
    "depth_values", "mask" stage1..4, "filename"} on ``device``, each with the batch dimension in front for a batch
    ([B,N,3,h,w], [B,h_k,w_k]: what the reference's collate gives and ``mvs_loss_fused`` accepts).  A sample that already holds
    ``imgs`` passes through.  ``out``: see ``train_arrays``."""
    if "imgs_u8" not in sample:
        return sample
    imgs, depth_ms, mask_ms, batched = train_arrays(sample, device, out)
    if not batched:
        imgs, depth_ms, mask_ms = imgs[0], {k: v[0] for k, v in depth_ms.items()}, {k: v[0] for k, v in mask_ms.items()}
    res = {"imgs": imgs,
           "proj_matrices": {k: v.to(imgs.device, non_blocking=True) for k, v in sample["proj_matrices"].items()},
           "depth": depth_ms,
           "depth_values": sample["depth_values"].to(imgs.device, non_blocking=True),
           "mask": mask_ms}
    res.update({k: v for k, v in sample.items() if k not in res and k not in RAW_KEYS})
    return res
