"""BlendedMVS training dataset (reference: datasets/blend.py:20-254): same constructor, same ``metas``, same sample dictionary
{"imgs" [N,3,h,w], "proj_matrices" {"stage0".."stage4": [N,2,4,4]}, "depth" {"stage1".."stage4"}, "depth_values" [ndepths],
"mask" {"stage1".."stage4"}, "filename"}.

Host side: list / pair / cam parsing, decoding, the inverse-depth samples.  There is no crop: images and the rendered depth map go
to the device as they are.  Device side (``train_sample.prepare_train_sample``): / 255 + HWC -> CHW of all views in one launch; the
depth pyramid and, per level, mask = depth_min <= depth <= depth_max (blend.py:208-220) in another.  A DataLoader worker or
``device="host"`` stays on the host and returns ``imgs_u8`` / ``depth_raw`` / ``depth_range``.

``mode``: the reference's constructor asserts train / val / test although ``__getitem__`` samples its source views only in mode
"finetune" (blend.py:37,143); here "finetune" is accepted too, so that branch can be reached.
"""
import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from .data_io import read_pfm
from .general_eval import decode_image, host_only, stage_projections
from .train_sample import parse_train_cam_file, prepare_train_sample, read_pair_file, stack_views  # noqa: F401  (prepare_train_sample re-exported)

STAGE_SCALES = {"stage0": 1 / 16.0, "stage1": 1 / 8.0, "stage2": 1 / 4.0, "stage3": 1 / 2.0, "stage4": 1.0}   # blend.py:226-235 (exact)
MIN_SOURCES = 7                                                                                               # blend.py:59


class MVSDataset(Dataset):
    def __init__(self, datapath, listfile, mode, nviews, ndepths=192, interval_scale=1.06, dispmaxfirst="first", **kwargs):
        super().__init__()
        self.datapath = datapath
        self.mode = mode
        self.listfile = listfile
        self.nviews = nviews
        self.ndepths = ndepths
        self.interval_scale = interval_scale
        self.device = kwargs.get("device", "cuda")
        assert self.mode in ["train", "val", "test", "finetune"]
        self.metas = self.build_list()

    def build_list(self):
        metas = []
        with open(self.listfile) as f:
            scans = [line.rstrip() for line in f.readlines()]
        for scan in scans:
            for ref_view, src_views in read_pair_file(os.path.join(self.datapath, "{}/cams/pair.txt".format(scan))):
                if len(src_views) < MIN_SOURCES:
                    print("less ref_view small {}".format(self.nviews - 1))
                    continue
                metas.append((scan, ref_view, src_views, 0))
        print("dataset", self.mode, "metas:", len(metas))
        return metas

    def __len__(self):
        return len(self.metas)

    def read_cam_file(self, filename):
        intrinsics, extrinsics, fields = parse_train_cam_file(filename)
        return intrinsics, extrinsics, fields[0], fields[3]              # depth_min, depth_max (blend.py:83-86)

    def read_depth(self, filename):
        depth = np.ascontiguousarray(read_pfm(filename)[0], dtype=np.float32)
        h, w = depth.shape
        if h % 8 or w % 8:
            raise ValueError(f"{filename}: depth map {h} x {w}: the ground-truth pyramid kernel needs h % 8 == 0 and w % 8 == 0 "
                             "(cv2's nearest rounding is pinned for these sizes only)")
        return depth

    def view_paths(self, scan, vid):
        return (os.path.join(self.datapath, "{}/blended_images/{:0>8}.jpg".format(scan, vid)),
                os.path.join(self.datapath, "{}/cams/{:0>8}_cam.txt".format(scan, vid)),
                os.path.join(self.datapath, "{}/rendered_depth_maps/{:0>8}.pfm".format(scan, vid)))

    def __getitem__(self, idx):
        scan, ref_view, src_views, _ = self.metas[idx]
        if self.mode == "finetune":
            src_views_ids = random.sample(src_views, self.nviews - 1)
        else:
            src_views_ids = src_views[:self.nviews - 1]
        view_ids = [ref_view] + src_views_ids
        raws, proj_matrices = [], []
        for i, vid in enumerate(view_ids):
            img_filename, cam_filename, depth_filename = self.view_paths(scan, vid)
            raws.append(decode_image(img_filename))
            intrinsics, extrinsics, depth_min, depth_max = self.read_cam_file(cam_filename)
            proj_mat = np.zeros((2, 4, 4), dtype=np.float32)
            proj_mat[0, :4, :4] = extrinsics
            proj_mat[1, :3, :3] = intrinsics
            proj_matrices.append(proj_mat)
            if i == 0:
                depth_values = np.linspace(1 / depth_max, 1 / depth_min, self.ndepths, endpoint=False).astype(np.float32)
                depth_raw = self.read_depth(depth_filename)
                # numpy compares the float32 map against the Python floats rounded to float32 (blend.py:215-220)
                depth_range = np.array([depth_min, depth_max], dtype=np.float32)
        sample = {"imgs_u8": stack_views(raws, img_filename),
                  "proj_matrices": stage_projections(np.stack(proj_matrices), STAGE_SCALES),
                  "depth_raw": torch.from_numpy(depth_raw),
                  "depth_values": torch.from_numpy(depth_values),
                  "depth_range": torch.from_numpy(depth_range),
                  "filename": scan + "/{}/" + "{:0>8}".format(view_ids[0]) + "{}"}
        return sample if host_only(self.device) else prepare_train_sample(sample, self.device)
