"""CPU: the host half of the training datasets (datasets/dtu_yao.py, datasets/blend.py, find_dataset_def) on synthetic trees --
metas, view sampling, the host-mode sample against the numpy restatement (tests/train_input_ref.py) bit for bit, worker
collation, the refusals, and the new symbols of the C ABI.  Nothing here touches a GPU."""
import os
import random

import numpy as np
import pytest
import torch

import train_input_ref as R
from train_input_trees import write_blend_tree, write_dtu_tree
from effi_mvs_plus_amd import _lib, datasets
from effi_mvs_plus_amd._lib import EffiLibraryError
from effi_mvs_plus_amd.datasets import blend, data_io, dtu_yao

CROP = (24, 72)
RAW = (60, 164)          # half size 30 x 82: crop offsets (30 - 24) // 2 = 3 and (82 - 72) // 2 = 5, both odd
SAMPLE_KEYS = {"imgs", "proj_matrices", "depth", "depth_values", "mask", "filename"}


class SmallDTU(dtu_yao.MVSDataset):
    CROP_HW = CROP


@pytest.fixture(scope="module")
def dtu_tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("dtu"))
    listfile, stored = write_dtu_tree(root, ["scan1", "scan7"], 6, RAW, CROP)
    return root, listfile, stored


@pytest.fixture(scope="module")
def blend_tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("blend"))
    listfile, stored = write_blend_tree(root, ["5a0271884e62597cdee0d0eb"], 9, (24, 72), ranges={2: (3.0, 9.5)})
    return root, listfile, stored


def _dtu_cams(root, ids):
    return [os.path.join(root, "Cameras", "train", f"{v:08d}_cam.txt") for v in ids]


# ---- metas and view sampling ---------------------------------------------------------------------
def test_dtu_metas_seven_lights_in_train_mode_one_otherwise(dtu_tree, capsys):
    root, listfile, stored = dtu_tree
    train = SmallDTU(root, listfile, "train", 3, 96, device="host")
    assert len(train) == 7 * 6 * 2 and "metas: 84" in capsys.readouterr().out
    assert train.metas[:8] == [("scan1", light, 0, stored["sources"][0]) for light in range(7)] + [("scan1", 0, 1, stored["sources"][1])]
    for mode in ("val", "test"):
        ds = SmallDTU(root, listfile, mode, 3, 96, device="host")
        assert len(ds) == 6 * 2 and all(m[1] == 3 for m in ds.metas) and ds.metas[7] == ("scan7", 3, 1, stored["sources"][1])
    with pytest.raises(AssertionError):
        SmallDTU(root, listfile, "finetune", 3)
    # the constructor's interval_scale is ignored (dtu_yao.py:18)
    assert SmallDTU(root, listfile, "val", 3, 96, interval_scale=0.5, device="host").interval_scale == 1.06 / (96 / 192.0)
    assert dtu_yao.MVSDataset.CROP_HW == (512, 640)


def test_blend_metas_skip_views_with_fewer_than_seven_sources(blend_tree, capsys):
    root, listfile, stored = blend_tree
    ds = blend.MVSDataset(root, listfile, "train", 5, 128, device="host")
    out = capsys.readouterr().out
    assert len(ds) == 8 and out.count("less ref_view small 4") == 1 and "metas: 8" in out
    assert [m[1] for m in ds.metas] == list(range(1, 9)) and ds.metas[0] == ("5a0271884e62597cdee0d0eb", 1, stored["sources"][1], 0)


@pytest.mark.parametrize("seed", [0, 7])
def test_seeded_sampling_picks_the_views_of_a_direct_random_sample(dtu_tree, blend_tree, seed):
    root, listfile, stored = dtu_tree
    ds = SmallDTU(root, listfile, "train", 4, 96, device="host")
    idx = 7 * 2 + 5                                      # scan1, view 2, light 5
    random.seed(seed)
    want = [2] + random.sample(stored["sources"][2], 3)
    random.seed(seed)
    s = ds[idx]
    assert s["filename"] == "scan1/{}/00000002{}"
    assert np.array_equal(s["imgs_u8"].numpy(), np.stack([stored["imgs"]["scan1", v, 5] for v in want]))
    # val mode and BlendedMVS outside "finetune": the first nviews - 1
    v = SmallDTU(root, listfile, "val", 4, 96, device="host")[2]
    assert np.array_equal(v["imgs_u8"].numpy(), np.stack([stored["imgs"]["scan1", u, 3] for u in [2] + stored["sources"][2][:3]]))
    broot, blist, bstored = blend_tree
    scan = "5a0271884e62597cdee0d0eb"
    ft = blend.MVSDataset(broot, blist, "finetune", 4, 128, device="host")
    random.seed(seed)
    want = [3] + random.sample(bstored["sources"][3], 3)
    random.seed(seed)
    assert np.array_equal(ft[2]["imgs_u8"].numpy(), np.stack([bstored["imgs"][scan, u] for u in want]))
    tr = blend.MVSDataset(broot, blist, "train", 4, 128, device="host")[2]
    assert np.array_equal(tr["imgs_u8"].numpy(), np.stack([bstored["imgs"][scan, u] for u in [3] + bstored["sources"][3][:3]]))


# ---- the host-mode sample against the restatement ------------------------------------------------
@pytest.mark.parametrize("dispmaxfirst", ["first", "last"])
def test_dtu_host_sample_equals_the_restatement(dtu_tree, dispmaxfirst):
    root, listfile, stored = dtu_tree
    ds = SmallDTU(root, listfile, "val", 3, 96, dispmaxfirst=dispmaxfirst, device="host")
    s = ds[6 + 4]                                        # scan7, view 4
    ids = [4] + stored["sources"][4][:2]
    assert set(s) == (SAMPLE_KEYS - {"imgs", "depth", "mask"}) | {"imgs_u8", "depth_raw", "mask_raw"}
    assert s["imgs_u8"].dtype == torch.uint8 and tuple(s["imgs_u8"].shape) == (3,) + CROP + (3,)
    assert np.array_equal(s["imgs_u8"].numpy(), np.stack([stored["imgs"]["scan7", v, 3] for v in ids]))
    depth_ms, mask_ms = R.dtu_ground_truth(stored["depth"]["scan7", 4], stored["mask"]["scan7", 4], CROP)
    assert s["depth_raw"].dtype == torch.float32 and s["depth_raw"].is_contiguous()
    assert np.array_equal(s["depth_raw"].numpy(), depth_ms["stage4"])
    # the crop offsets are odd here: the strided view must start at raw (2 * 3, 2 * 5)
    assert s["depth_raw"][0, 0] == stored["depth"]["scan7", 4][6, 10] and s["depth_raw"][23, 71] == stored["depth"]["scan7", 4][52, 152]
    assert s["mask_raw"].dtype == torch.uint8 and tuple(s["mask_raw"].shape) == CROP
    assert np.array_equal(s["mask_raw"].numpy(), R.dtu_prepare(stored["mask"]["scan7", 4], CROP))
    assert np.array_equal((s["mask_raw"].numpy() > 10).astype(np.float32), mask_ms["stage4"])
    assert 0.2 < mask_ms["stage1"].mean() < 1.0 and (s["mask_raw"] == 10).any() and (s["mask_raw"] == 11).any()
    want_proj = R.projections(_dtu_cams(root, ids), scales=R.DTU_SCALES)
    assert list(s["proj_matrices"]) == ["stage0", "stage1", "stage2", "stage3", "stage4"]
    for k, m in want_proj.items():
        assert s["proj_matrices"][k].dtype == torch.float32 and np.array_equal(s["proj_matrices"][k].numpy(), m)
    # the intrinsics are NOT divided by 4 (general_eval's are): stage2 holds them as stored
    assert np.array_equal(s["proj_matrices"]["stage2"][:, 1, :3, :3].numpy(), np.stack([R.read_cam(p)[0] for p in _dtu_cams(root, ids)]))
    dv = R.dtu_depth_values(425.0, 96, dispmaxfirst)
    assert s["depth_values"].dtype == torch.float32 and np.array_equal(s["depth_values"].numpy(), dv)
    assert (dv[0] > dv[-1]) == (dispmaxfirst == "first") and dv.max() == np.float32(1 / 425.0)
    assert s["filename"] == "scan7/{}/00000004{}"


def test_blend_host_sample_equals_the_restatement(blend_tree):
    root, listfile, stored = blend_tree
    scan = "5a0271884e62597cdee0d0eb"
    ds = blend.MVSDataset(root, listfile, "val", 4, 128, device="host")
    for idx in (0, 1):                                   # views 1 and 2: view 2 has its own depth range
        ref = idx + 1
        ids = [ref] + stored["sources"][ref][:3]
        s = ds[idx]
        assert set(s) == (SAMPLE_KEYS - {"imgs", "depth", "mask"}) | {"imgs_u8", "depth_raw", "depth_range"}
        assert np.array_equal(s["imgs_u8"].numpy(), np.stack([stored["imgs"][scan, v] for v in ids]))
        assert s["depth_raw"].dtype == torch.float32 and np.array_equal(s["depth_raw"].numpy(), stored["depth"][scan, ref], equal_nan=True)
        lo, hi = stored["range"][ref]
        assert s["depth_range"].dtype == torch.float32 and s["depth_range"].tolist() == [np.float32(lo), np.float32(hi)]
        cams = [os.path.join(root, scan, "cams", f"{v:08d}_cam.txt") for v in ids]
        for k, m in R.projections(cams, divisors=R.BLEND_DIVISORS).items():
            assert np.array_equal(s["proj_matrices"][k].numpy(), m)
        dv = R.blend_depth_values(lo, hi, 128)
        assert s["depth_values"].dtype == torch.float32 and np.array_equal(s["depth_values"].numpy(), dv)
        assert dv[0] == np.float32(1 / hi) and dv[-1] < np.float32(1 / lo)               # endpoint=False
        assert s["filename"] == scan + "/{}/" + f"{ref:08d}" + "{}"
    assert ds[0]["depth_range"].tolist() != ds[1]["depth_range"].tolist()


def test_restatement_nearest_rule():
    """The rule itself: for exact power-of-two ratios the source index is f * x; for others the double arithmetic decides."""
    a = np.arange(24 * 72, dtype=np.float32).reshape(24, 72)
    for f in (2, 4, 8):
        assert np.array_equal(R.resize_nearest(a, 72 // f, 24 // f), a[::f, ::f])
    assert R.nearest_index(3, 7).tolist() == [0, 2, 4] and R.nearest_index(5, 3).tolist() == [0, 0, 1, 1, 2]
    assert np.array_equal(R.dtu_prepare(np.arange(60 * 164).reshape(60, 164), CROP), np.arange(60 * 164).reshape(60, 164)[6:54:2, 10:154:2])
    m = R.blend_masks({"s": np.array([1.0, np.nextafter(np.float32(1), np.float32(0)), 2.0, np.nan, np.inf], dtype=np.float32)}, 1.0, 2.0)
    assert m["s"].tolist() == [1.0, 0.0, 1.0, 0.0, 0.0]


# ---- workers, device mode without a GPU, refusals -------------------------------------------------
def test_dataloader_workers_stay_on_the_host_and_collate(dtu_tree, blend_tree):
    from torch.utils.data import DataLoader
    root, listfile, _ = dtu_tree
    ds = SmallDTU(root, listfile, "val", 3, 96)                                # device="cuda", the default
    host = SmallDTU(root, listfile, "val", 3, 96, device="host")
    batches = list(DataLoader(ds, batch_size=2, shuffle=False, num_workers=2))
    assert len(batches) == 6
    b = batches[1]
    assert "imgs" not in b and tuple(b["imgs_u8"].shape) == (2, 3) + CROP + (3,) and b["imgs_u8"].dtype == torch.uint8
    assert tuple(b["depth_raw"].shape) == (2,) + CROP and tuple(b["mask_raw"].shape) == (2,) + CROP and b["mask_raw"].dtype == torch.uint8
    assert tuple(b["proj_matrices"]["stage3"].shape) == (2, 3, 2, 4, 4) and tuple(b["depth_values"].shape) == (2, 96)
    assert b["filename"] == ["scan1/{}/00000002{}", "scan1/{}/00000003{}"]
    for j in (0, 1):
        assert torch.equal(b["imgs_u8"][j], host[2 + j]["imgs_u8"]) and torch.equal(b["depth_raw"][j], host[2 + j]["depth_raw"])
        assert torch.equal(b["mask_raw"][j], host[2 + j]["mask_raw"])
    broot, blist, _ = blend_tree
    bb = next(iter(DataLoader(blend.MVSDataset(broot, blist, "val", 3, 64), batch_size=2, num_workers=2)))
    assert "imgs" not in bb and tuple(bb["imgs_u8"].shape) == (2, 3, 24, 72, 3) and tuple(bb["depth_range"].shape) == (2, 2)
    assert tuple(bb["depth_raw"].shape) == (2, 24, 72)


def test_device_mode_without_a_gpu_fails_loudly(dtu_tree, blend_tree):
    root, listfile, _ = dtu_tree
    broot, blist, _ = blend_tree
    for dev in ("cpu",) if torch.cuda.is_available() else ("cuda", "cpu"):     # "cuda" (the default) fails the same way without one
        with pytest.raises(EffiLibraryError):
            SmallDTU(root, listfile, "val", 3, 96, device=dev)[0]
        with pytest.raises(EffiLibraryError):
            blend.MVSDataset(broot, blist, "val", 3, 64, device=dev)[0]
    host = SmallDTU(root, listfile, "val", 3, 96, device="host")[0]
    with pytest.raises(EffiLibraryError):
        datasets.prepare_train_sample(host, device="cpu")
    done = {"imgs": torch.zeros(1)}
    assert datasets.prepare_train_sample(done) is done                         # already complete: untouched


def test_host_half_refusals(tmp_path):
    from PIL import Image
    ds = SmallDTU.__new__(SmallDTU)
    with pytest.raises(ValueError, match="odd side"):
        ds.crop(np.zeros((61, 164), dtype=np.float32), "x")
    with pytest.raises(ValueError, match="odd side"):
        ds.crop(np.zeros((60, 165), dtype=np.float32), "x")
    with pytest.raises(ValueError, match="smaller"):
        ds.crop(np.zeros((46, 164), dtype=np.float32), "x")
    with pytest.raises(ValueError, match="smaller"):
        ds.crop(np.zeros((60, 142), dtype=np.float32), "x")
    assert ds.crop(np.zeros((48, 144), dtype=np.float32), "x").shape == CROP    # exactly twice the crop
    rgb = str(tmp_path / "rgb.png")
    Image.fromarray(np.zeros((60, 164, 3), dtype=np.uint8)).save(rgb)
    with pytest.raises(TypeError, match="single-channel"):
        ds.read_mask_hr(rgb)
    deep = str(tmp_path / "deep.png")
    Image.fromarray(np.zeros((60, 164), dtype=np.uint16)).save(deep)
    with pytest.raises(TypeError, match="8-bit"):
        ds.read_mask_hr(deep)
    bl = blend.MVSDataset.__new__(blend.MVSDataset)
    for hw in ((12, 72), (24, 68)):
        p = str(tmp_path / "d.pfm")
        data_io.save_pfm(p, np.ones(hw, dtype=np.float32))
        with pytest.raises(ValueError, match="h % 8 == 0 and w % 8 == 0"):
            bl.read_depth(p)


def test_find_dataset_def_resolves_every_dataset():
    from effi_mvs_plus_amd.datasets import general_eval, tank
    assert datasets.find_dataset_def("dtu_yao") is dtu_yao.MVSDataset
    assert datasets.find_dataset_def("blend") is blend.MVSDataset
    assert datasets.find_dataset_def("general_eval") is general_eval.MVSDataset
    assert datasets.find_dataset_def("tank") is tank.MVSDataset
    with pytest.raises(ImportError):
        datasets.find_dataset_def("no_such_dataset")


def test_new_symbols_are_declared_bound_and_built():
    names = {"effi_gt_pyramid_f32", "effi_images_prepare_batch_u8_f32"}
    assert names <= set(_lib.declared_symbols()) and names <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["effi_gt_pyramid_f32"]) == 10 and len(_lib.SIGNATURES["effi_images_prepare_batch_u8_f32"]) == 6
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert "train_input.hip" in src
