"""DTU training dataset, Yao Yao's preprocessing (reference: datasets/dtu_yao.py:9-214): same constructor, same ``metas``, same
sample dictionary {"imgs" [N,3,512,640], "proj_matrices" {"stage0".."stage4": [N,2,4,4]}, "depth" {"stage1".."stage4"},
"depth_values" [ndepths], "mask" {"stage1".."stage4"}, "filename"}.

Host side: list / pair / cam parsing, view sampling (the reference's ``random.sample`` call, so a seeded run picks the same
views), decoding, and the strided crop of the raw depth map and visibility PNG: ``prepare_img`` (dtu_yao.py:76-91:
cv2.resize(INTER_NEAREST) to half size, then the centred 512 x 640 crop) reads source pixel (2 y, 2 x) for even raw sides, so it
IS ``a[2 oy : 2 (oy + 512) : 2, 2 ox : 2 (ox + 640) : 2]`` -- a view and one copy, no arithmetic, no cv2, and the fewest bytes
through worker IPC and PCIe.  Device side (``train_sample.prepare_train_sample``): / 255 + HWC -> CHW of all views in one launch,
the depth / mask pyramid in another.  As in ``general_eval``, a DataLoader worker or ``device="host"`` stays on the host and
returns ``imgs_u8`` / ``depth_raw`` / ``mask_raw``.
"""
import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from .data_io import read_pfm
from .general_eval import STAGE_SCALES, decode_image, host_only, inverse_depth_samples, stage_projections
from .train_sample import parse_train_cam_file, prepare_train_sample, read_pair_file, stack_views  # noqa: F401  (prepare_train_sample re-exported)


class MVSDataset(Dataset):
    CROP_HW = (512, 640)                  # prepare_img's target_h, target_w (dtu_yao.py:84); multiples of 8 (ops.gt_pyramid)

    def __init__(self, datapath, listfile, mode, nviews, ndepths=192, interval_scale=1.06, dispmaxfirst="first", **kwargs):
        super().__init__()
        self.datapath = datapath
        self.listfile = listfile
        self.mode = mode
        self.nviews = nviews
        self.ndepths = ndepths
        self.interval_scale = 1.06 / (float(ndepths) / 192.0)          # the argument is ignored (dtu_yao.py:18-19)
        self.dispmaxfirst = dispmaxfirst
        self.kwargs = kwargs
        self.device = kwargs.get("device", "cuda")
        print("mvsdataset kwargs", self.kwargs)
        assert self.mode in ["train", "val", "test"]
        self.metas = self.build_list()

    def build_list(self):
        metas = []
        with open(self.listfile) as f:
            scans = [line.rstrip() for line in f.readlines()]
        for scan in scans:
            for ref_view, src_views in read_pair_file(os.path.join(self.datapath, "Cameras/pair.txt")):
                if self.mode == "train":                                # light conditions 0-6
                    for light_idx in range(7):
                        metas.append((scan, light_idx, ref_view, src_views))
                else:
                    metas.append((scan, 3, ref_view, src_views))
        print("dataset", self.mode, "metas:", len(metas))
        return metas

    def __len__(self):
        return len(self.metas)

    def read_cam_file(self, filename):
        intrinsics, extrinsics, fields = parse_train_cam_file(filename)
        return intrinsics, extrinsics, fields[0], 2.5 * self.interval_scale     # the file's own interval is ignored (dtu_yao.py:67)

    def crop(self, a, what):
        """prepare_img (dtu_yao.py:76-91) as one strided view, made contiguous."""
        H, W = a.shape
        ch, cw = self.CROP_HW
        if H % 2 or W % 2:
            raise ValueError(f"{what}: raw size {H} x {W} has an odd side (the half-size nearest resize is pinned for even sides only)")
        if H // 2 < ch or W // 2 < cw:
            raise ValueError(f"{what}: raw size {H} x {W} is smaller than twice the {ch} x {cw} crop")
        oy, ox = (H // 2 - ch) // 2, (W // 2 - cw) // 2
        return np.ascontiguousarray(a[2 * oy:2 * (oy + ch):2, 2 * ox:2 * (ox + cw):2])

    def read_depth_hr(self, filename):
        return self.crop(np.array(read_pfm(filename)[0], dtype=np.float32), filename)

    def read_mask_hr(self, filename):
        """The visibility PNG as bytes at the crop's pixels; the ``> 10`` of dtu_yao.py:96 is the kernel's."""
        arr = decode_image(filename)
        if arr.ndim != 2:
            raise TypeError(f"{filename}: single-channel 8-bit mask expected, got an array of shape {arr.shape}")
        return self.crop(arr, filename)

    def view_paths(self, scan, vid, light_idx):
        # the id in image file names is from 1 to 49 (dtu_yao.py:146-153)
        return (os.path.join(self.datapath, "Rectified/{}_train/rect_{:0>3}_{}_r5000.png".format(scan, vid + 1, light_idx)),
                os.path.join(self.datapath, "Depths_raw/{}/depth_visual_{:0>4}.png".format(scan, vid)),
                os.path.join(self.datapath, "Depths_raw/{}/depth_map_{:0>4}.pfm".format(scan, vid)),
                os.path.join(self.datapath, "Cameras/train/{:0>8}_cam.txt").format(vid))

    def __getitem__(self, idx):
        scan, light_idx, ref_view, src_views = self.metas[idx]
        if self.mode == "train":
            src_views_ids = random.sample(src_views, self.nviews - 1)
        else:
            src_views_ids = src_views[:self.nviews - 1]
        view_ids = [ref_view] + src_views_ids
        raws, proj_matrices = [], []
        for i, vid in enumerate(view_ids):
            img_filename, mask_filename, depth_filename, cam_filename = self.view_paths(scan, vid, light_idx)
            raws.append(decode_image(img_filename))
            intrinsics, extrinsics, depth_min, depth_interval = self.read_cam_file(cam_filename)
            proj_mat = np.zeros((2, 4, 4), dtype=np.float32)
            proj_mat[0, :4, :4] = extrinsics
            proj_mat[1, :3, :3] = intrinsics
            proj_matrices.append(proj_mat)
            if i == 0:
                mask_raw = self.read_mask_hr(mask_filename)
                depth_raw = self.read_depth_hr(depth_filename)
                depth_values = inverse_depth_samples(depth_min, depth_interval, self.ndepths, self.dispmaxfirst)
        sample = {"imgs_u8": stack_views(raws, img_filename),
                  "proj_matrices": stage_projections(np.stack(proj_matrices), STAGE_SCALES),
                  "depth_raw": torch.from_numpy(depth_raw),
                  "depth_values": torch.from_numpy(depth_values.copy()).contiguous().float(),
                  "mask_raw": torch.from_numpy(mask_raw),
                  "filename": scan + "/{}/" + "{:0>8}".format(view_ids[0]) + "{}"}
        return sample if host_only(self.device) else prepare_train_sample(sample, self.device)
