"""GPU: the training input on the device -- ops.gt_pyramid / ops.images_prepare (csrc/train_input.hip), the device mode of the two
training datasets, prepare_train_sample and GraphedTrainStep.load_raw_sample -- against the numpy restatement
(tests/train_input_ref.py).  Every comparison is bitwise: the kernels move data and do one correctly rounded division."""

import numpy as np
import pytest
import torch

import train_input_ref as R
from common import build_model
from train_input_trees import write_blend_tree, write_dtu_tree
from effi_mvs_plus_amd import ops, synth
from effi_mvs_plus_amd._lib import EffiLibraryError
from effi_mvs_plus_amd.datasets import blend, dtu_yao, prepare_train_sample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (1,8,8): the smallest legal size, one thread.  (2,24,72): two different samples, 216 row-octets = four 64-lane workgroups with a
# ragged last one, rows that are no multiple of the row tile.  (1,512,640): the training shape's launch geometry, once.
SHAPES = [(1, 8, 8), (2, 24, 72), (1, 512, 640)]
CROP = (24, 72)
RAW = (60, 164)
KEYS = ("imgs", "proj_matrices", "depth", "depth_values", "mask", "filename")


def _nan_outputs(B, h, w):
    mk = lambda: {k: torch.full((B, h >> (3 - j), w >> (3 - j)), float("nan"), device=DEV) for j, k in enumerate(R.STAGES)}  # noqa: E731
    return mk(), mk()


def _stacked(per_sample):
    """[{stage: [h_k,w_k]} per sample] -> {stage: [B,h_k,w_k]}"""
    return {k: np.stack([p[k] for p in per_sample]) for k in R.STAGES}


def _assert_pyramid(got, want, what):
    for k in R.STAGES:
        g = got[k]
        assert g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == want[k].shape, (what, k)
        assert not torch.isnan(g).any() or np.isnan(want[k]).any(), (what, k, "an element was not written")
        assert np.array_equal(g.cpu().numpy(), want[k], equal_nan=True), (what, k)


def _index_depth(B, h, w):
    return (np.arange(B * h * w, dtype=np.float64) + 0.25).astype(np.float32).reshape(B, h, w)       # a wrong address shows


@pytest.mark.parametrize("shape", SHAPES)
def test_gt_pyramid_dtu_mode_equals_the_restatement(shape):
    B, h, w = shape
    rng = np.random.default_rng(h + w)
    depth = _index_depth(B, h, w)
    mask = rng.integers(0, 256, size=shape, dtype=np.uint8)
    mask[:, 0::8, 0::8] = 10                 # positions every level samples: both sides of "> 10"
    mask[:, 0::8, 8::16] = 11
    mask[:, 8::16, 0::8] = 11
    mask[:, 1::2, 1::4] = 11                 # positions only stage 4 reads
    mask[:, 1::2, 3::4] = 10
    mask[:, 2::8, 2::8], mask[:, 2::8, 6::8] = 10, 11        # stage 3 and 4 only
    if B > 1:
        mask[1] = 255 - mask[1]              # the samples differ
    want_d = _stacked([R.pyramid(depth[b]) for b in range(B)])
    want_m = _stacked([R.pyramid((mask[b].astype(np.float32) > 10).astype(np.float32)) for b in range(B)])
    out_d, out_m = _nan_outputs(B, h, w)
    got_d, got_m = ops.gt_pyramid(torch.from_numpy(depth).to(DEV), mask_u8=torch.from_numpy(mask).to(DEV), out=(out_d, out_m))
    assert all(got_d[k] is out_d[k] and got_m[k] is out_m[k] for k in R.STAGES)
    _assert_pyramid(got_d, want_d, "depth")
    _assert_pyramid(got_m, want_m, "mask")
    assert all(set(np.unique(got_m[k].cpu().numpy())) <= {0.0, 1.0} for k in R.STAGES)
    assert want_m["stage1"][0, 0, 0] == 0.0 and want_m["stage4"][0, 1, 1] == 1.0
    # without out=, and another threshold
    d2, m2 = ops.gt_pyramid(torch.from_numpy(depth).to(DEV), mask_u8=torch.from_numpy(mask).to(DEV), thresh=9)
    _assert_pyramid(d2, want_d, "depth (allocated)")
    _assert_pyramid(m2, _stacked([R.pyramid((mask[b] > 9).astype(np.float32)) for b in range(B)]), "mask, thresh 9")


@pytest.mark.parametrize("shape", SHAPES)
def test_gt_pyramid_blend_mode_masks_each_level_by_its_own_depth(shape):
    B, h, w = shape
    rng = np.random.default_rng(h * w)
    ranges = [(2.3, 11.7), (425.3, 935.7)][:B]                    # not representable in fp32: the comparison rounds them first
    depth = np.empty(shape, dtype=np.float32)
    for b, (lo, hi) in enumerate(ranges):
        lo32, hi32 = np.float32(lo), np.float32(hi)
        d = (lo32 - (hi32 - lo32) * 0.2 + (hi32 - lo32) * 1.4 * rng.random((h, w))).astype(np.float32)
        planted = [lo32, hi32, np.nextafter(lo32, np.float32(-np.inf)), np.nextafter(hi32, np.float32(np.inf)), np.float32(np.nan),
                   np.float32(np.inf), np.float32(-np.inf), np.float32(0.0)]
        # on the stage-3 grid (even coordinates; (0,0) and (4,4)-multiples reach the coarser levels) and at odd positions
        spots = [(0, 0), (0, 4), (4, 0), (4, 4), (0, 2), (2, 0), (2, 2), (2, 4)]
        for i, (y, x) in enumerate(spots):
            d[y, x] = planted[(i + b) % 8]
            d[y + 1, x + 1] = planted[(i + b + 3) % 8]
        if h >= 16:
            d[8, 8], d[8, 16], d[16, 8], d[16, 16], d[16, 24], d[8, 24] = planted[:6]
        depth[b] = d
    per = [R.blend_ground_truth(depth[b], *ranges[b]) for b in range(B)]
    want_d, want_m = _stacked([p[0] for p in per]), _stacked([p[1] for p in per])
    assert want_m["stage3"].min() == 0.0 and want_m["stage3"].max() == 1.0
    rng_t = torch.tensor([[np.float32(lo), np.float32(hi)] for lo, hi in ranges], dtype=torch.float32, device=DEV)
    out_d, out_m = _nan_outputs(B, h, w)
    got_d, got_m = ops.gt_pyramid(torch.from_numpy(depth).to(DEV), depth_range=rng_t, out=(out_d, out_m))
    _assert_pyramid(got_d, want_d, "depth")
    _assert_pyramid(got_m, want_m, "mask")
    assert not any(torch.isnan(got_m[k]).any() for k in R.STAGES)                  # NaN depth gives mask 0, never NaN
    for k in R.STAGES:                                                              # each level's mask is a function of its own depth
        assert np.array_equal(got_m[k].cpu().numpy(), _stacked_mask(got_d[k].cpu().numpy(), ranges))


def _stacked_mask(d, ranges):
    return np.stack([R.blend_masks({"s": d[b]}, *ranges[b])["s"] for b in range(len(ranges))])


def test_gt_pyramid_refusals_launch_nothing():
    depth = torch.from_numpy(_index_depth(1, 24, 72)).to(DEV)
    mask = torch.zeros(1, 24, 72, dtype=torch.uint8, device=DEV)
    rng_t = torch.tensor([[1.0, 2.0]], device=DEV)
    out_d, out_m = _nan_outputs(1, 24, 72)
    with pytest.raises(EffiLibraryError):
        ops.gt_pyramid(depth, mask_u8=mask, depth_range=rng_t, out=(out_d, out_m))          # both
    with pytest.raises(EffiLibraryError):
        ops.gt_pyramid(depth, out=(out_d, out_m))                                           # neither
    for bad in ((1, 12, 72), (1, 24, 68)):                                                  # h or w not a multiple of 8
        o_d, o_m = _nan_outputs(*bad)
        with pytest.raises(EffiLibraryError):
            ops.gt_pyramid(torch.ones(bad, device=DEV), mask_u8=torch.zeros(bad, dtype=torch.uint8, device=DEV), out=(o_d, o_m))
        torch.cuda.synchronize()
        assert all(torch.isnan(o_d[k]).all() and torch.isnan(o_m[k]).all() for k in R.STAGES)
    torch.cuda.synchronize()
    assert all(torch.isnan(out_d[k]).all() and torch.isnan(out_m[k]).all() for k in R.STAGES)
    with pytest.raises(EffiLibraryError):
        ops.gt_pyramid(depth.cpu(), mask_u8=mask.cpu())                                     # no CPU fallback
    with pytest.raises(ValueError):
        ops.gt_pyramid(depth, mask_u8=mask, out=(out_d, {k: v[:, :1] for k, v in out_m.items()}))
    with pytest.raises(TypeError):
        ops.gt_pyramid(depth, mask_u8=mask.float())


@pytest.mark.parametrize("shape", [(5, 8, 72), (3, 5, 7), (5, 512, 640)])
def test_images_prepare_is_the_correctly_rounded_division(shape):
    """(5,8,72): 144 pixel quads per view = two 128-lane workgroups, the second ragged.  (3,5,7): 35 pixels, no multiple of 4 -- the
    byte-wise kernel.  (5,512,640): the training shape."""
    V, h, w = shape
    rng = np.random.default_rng(V * h)
    x = rng.integers(0, 256, size=(V, h, w, 3), dtype=np.uint8)
    x.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)                 # every byte value
    want = R.images(list(x))
    assert want.dtype == np.float32 and want.shape == (V, 3, h, w)
    dev_x = torch.from_numpy(x).to(DEV)
    out = torch.full((V, 3, h, w), float("nan"), device=DEV)
    got = ops.images_prepare(dev_x, out=out)
    assert got is out and not torch.isnan(out).any()
    assert np.array_equal(out.cpu().numpy(), want)
    assert torch.equal(ops.images_prepare(dev_x), out)
    if h * w <= 1024:
        single = torch.stack([ops.image_prepare(dev_x[v], h, w) for v in range(V)])
        assert torch.equal(single, out)                                   # V calls of the per-view kernel at dst == src
    # [B,N,h,w,3] -> [B,N,3,h,w]
    if V == 5 and h == 8:
        two = ops.images_prepare(torch.stack([dev_x, dev_x.flip(0)]))
        assert tuple(two.shape) == (2, 5, 3, h, w) and torch.equal(two[0], out) and torch.equal(two[1], out.flip(0))
    with pytest.raises(EffiLibraryError):
        ops.images_prepare(torch.from_numpy(x))
    with pytest.raises(TypeError):
        ops.images_prepare(dev_x.float())
    with pytest.raises(ValueError):
        ops.images_prepare(dev_x, out=torch.empty(V, 3, h, w + 1, device=DEV))


# ---- datasets ------------------------------------------------------------------------------------
class SmallDTU(dtu_yao.MVSDataset):
    CROP_HW = CROP


@pytest.fixture(scope="module")
def dtu_tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("dtu"))
    listfile, stored = write_dtu_tree(root, ["scan2"], 5, RAW, CROP, lights=[3])
    return root, listfile, stored


@pytest.fixture(scope="module")
def blend_tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("blend"))
    listfile, stored = write_blend_tree(root, ["scene"], 9, CROP, ranges={2: (3.0, 9.5)})
    return root, listfile, stored


def _assert_sample(s, want_imgs, want_d, want_m, host, lead=()):
    assert set(s) == set(KEYS)
    assert s["imgs"].is_cuda and s["imgs"].dtype == torch.float32 and tuple(s["imgs"].shape) == lead + want_imgs.shape
    assert np.array_equal(s["imgs"].cpu().numpy().reshape(want_imgs.shape), want_imgs)
    for k in R.STAGES:
        for got, want in ((s["depth"][k], want_d[k]), (s["mask"][k], want_m[k])):
            assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == lead + want.shape
            assert np.array_equal(got.cpu().numpy().reshape(want.shape), want, equal_nan=True)
    assert list(s["proj_matrices"]) == ["stage0", "stage1", "stage2", "stage3", "stage4"]
    for k, m in s["proj_matrices"].items():
        assert m.dtype == torch.float32 and torch.equal(m.cpu().reshape(host["proj_matrices"][k].shape), host["proj_matrices"][k])
    assert s["depth_values"].dtype == torch.float32 and torch.equal(s["depth_values"].cpu().reshape(-1), host["depth_values"])
    assert s["filename"] == host["filename"] or s["filename"] == [host["filename"]]


def test_device_mode_samples_equal_the_host_restatement(dtu_tree, blend_tree):
    root, listfile, stored = dtu_tree
    mk = lambda dev: SmallDTU(root, listfile, "val", 3, 96, device=dev)  # noqa: E731
    ids = [1] + stored["sources"][1][:2]
    want_d, want_m = R.dtu_ground_truth(stored["depth"]["scan2", 1], stored["mask"]["scan2", 1], CROP)
    want_imgs = R.images([stored["imgs"]["scan2", v, 3] for v in ids])
    host = mk("host")[1]
    _assert_sample(mk(DEV)[1], want_imgs, want_d, want_m, host)
    assert prepare_train_sample(host, device=DEV)["depth"]["stage1"].shape == (3, 9)
    broot, blist, bstored = blend_tree
    bmk = lambda dev: blend.MVSDataset(broot, blist, "val", 4, 64, device=dev)  # noqa: E731
    for idx in (0, 1):
        ref = idx + 1
        ids = [ref] + bstored["sources"][ref][:3]
        want_d, want_m = R.blend_ground_truth(bstored["depth"]["scene", ref], *bstored["range"][ref])
        assert 0.0 < want_m["stage4"].mean() < 1.0 and np.isnan(want_d["stage4"][1, 1]) and want_m["stage1"][0, 0] == 1.0
        _assert_sample(bmk(DEV)[idx], R.images([bstored["imgs"]["scene", v] for v in ids]), want_d, want_m, bmk("host")[idx])


def test_prepare_train_sample_of_a_worker_batch_equals_the_stacked_samples(dtu_tree, blend_tree):
    from torch.utils.data import DataLoader
    from effi_mvs_plus_amd.models.module import mvs_loss, mvs_loss_fused
    root, listfile, _ = dtu_tree
    broot, blist, _ = blend_tree
    for ds in (SmallDTU(root, listfile, "val", 3, 96, device=DEV), blend.MVSDataset(broot, blist, "val", 3, 64, device=DEV)):
        batch = next(iter(DataLoader(ds, batch_size=2, shuffle=False, num_workers=2)))
        assert "imgs" not in batch and not batch["imgs_u8"].is_cuda
        got = prepare_train_sample(batch, device=DEV)
        one = [ds[0], ds[1]]                                              # main process: device mode
        assert set(got) == set(KEYS) and tuple(got["imgs"].shape) == (2, 3, 3) + CROP
        assert torch.equal(got["imgs"], torch.stack([s["imgs"] for s in one]))
        for k in R.STAGES:
            j = 3 - R.STAGES.index(k)
            assert tuple(got["depth"][k].shape) == (2, CROP[0] >> j, CROP[1] >> j) == tuple(got["mask"][k].shape)
            assert torch.equal(got["depth"][k].nan_to_num(-1.0), torch.stack([s["depth"][k] for s in one]).nan_to_num(-1.0))
            assert torch.equal(got["mask"][k], torch.stack([s["mask"][k] for s in one]))
        for k in got["proj_matrices"]:
            assert got["proj_matrices"][k].is_cuda and torch.equal(got["proj_matrices"][k], torch.stack([s["proj_matrices"][k] for s in one]))
        assert torch.equal(got["depth_values"], torch.stack([s["depth_values"] for s in one]))
        assert got["filename"] == [s["filename"] for s in one]
        assert prepare_train_sample(got) is got
        # the shapes are what the fused loss takes: one estimate per stage, the batch in front
        gt = {k: v.nan_to_num(1.0) for k, v in got["depth"].items()}
        ests = [gt[k] + 0.5 + i for i, k in enumerate(R.STAGES)]
        fused, _ = mvs_loss_fused(ests, gt, got["mask"], [1, 2, 3, 4])
        plain, _ = mvs_loss(ests, gt, got["mask"], [1, 2, 3, 4])
        assert abs(float(fused) - float(plain)) <= 1e-5 * abs(float(plain))


def test_load_raw_sample_fills_the_captured_buffers_like_load_sample(tmp_path, blend_tree):
    from torch.utils.data import default_collate
    from effi_mvs_plus_amd import train_graph
    H, W, N = 128, 160, 3

    class Dtu128(dtu_yao.MVSDataset):
        CROP_HW = (H, W)

    pm = synth.synth_cameras(H, W, N, torch.float64)["stage2"][0]        # the dataset's stage2 is the cam file as stored
    cams = [(pm[v, 0].numpy(), pm[v, 1, :3, :3].numpy()) for v in range(N)]
    root = str(tmp_path)
    listfile, _ = write_dtu_tree(root, ["scan3"], N, (2 * H + 12, 2 * W + 20), (H, W), lights=[3], cams=cams, depth_min=synth.DEPTH_MIN_MM)
    ds = Dtu128(root, listfile, "val", N, 192, dispmaxfirst="last", device="host")
    raws = [default_collate([ds[i]]) for i in (0, 1)]                    # what a DataLoader(batch_size=1) hands over
    prepared = [prepare_train_sample(r, device=DEV) for r in raws]
    args = lambda s: (s["imgs"], s["proj_matrices"], s["depth_values"], s["depth"], s["mask"])  # noqa: E731
    assert tuple(prepared[0]["imgs"].shape) == (1, N, 3, H, W) and tuple(prepared[0]["depth"]["stage1"].shape) == (1, H // 8, W // 8)
    net, _ = build_model("8,8,8", seed=4, device=DEV)
    net.train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    opt = torch.optim.AdamW(net.parameters(), lr=0.0, weight_decay=0.0, capturable=True)   # the weights stay: replays are comparable
    step = train_graph.GraphedTrainStep(net, opt, *args(prepared[0]))
    step.load_sample(*args(prepared[1]))
    kept = (step.imgs.clone(), {k: v.clone() for k, v in step.gt.items()}, {k: v.clone() for k, v in step.mask.items()},
            {k: v.clone() for k, v in step.proj.items()}, step.depth_values.clone())
    loss_a = float(step().detach())
    for t in [step.imgs, step.depth_values] + list(step.gt.values()) + list(step.mask.values()) + list(step.proj.values()):
        t.fill_(float("nan"))
    step.load_raw_sample(raws[1])
    assert torch.equal(step.imgs, kept[0]) and torch.equal(step.depth_values, kept[4])
    for k in step.gt:
        assert torch.equal(step.gt[k], kept[1][k]) and torch.equal(step.mask[k], kept[2][k]), k
    for k in step.proj:
        assert torch.equal(step.proj[k], kept[3][k]), k
    loss_b = float(step().detach())
    assert np.isfinite(loss_b) and loss_b == loss_a
    assert not torch.equal(prepared[0]["imgs"], prepared[1]["imgs"])     # the loaded sample is not the captured one
    step.load_raw_sample(ds[0])                                          # an unbatched sample fills the batch of one
    assert torch.equal(step.imgs, prepared[0]["imgs"]) and torch.equal(step.gt["stage2"], prepared[0]["depth"]["stage2"])
    # another depth range is refused as in load_sample, before anything is written
    other = dict(raws[1], depth_values=raws[1]["depth_values"] * 1.01)
    with pytest.raises(ValueError, match="depth range"):
        step.load_raw_sample(other)
    with pytest.raises(ValueError, match="depth range"):
        step.load_sample(*args(dict(prepared[1], depth_values=other["depth_values"])))
    broot, blist, _ = blend_tree
    with pytest.raises(ValueError, match="depth range"):
        step.load_raw_sample(blend.MVSDataset(broot, blist, "val", N, 192, device="host")[0])
    assert torch.equal(step.imgs, prepared[0]["imgs"])
