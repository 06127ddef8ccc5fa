"""GPU: a whole scan through the depth-fusion filters in scan-batched launches, and the ordered compaction of the survivors.

  1. ``ops.fusion_dtu_filter_scan`` / ``ops.fusion_dynamic_filter_scan``: every output of reference view r == today's single-view
     launch on that view and its stacked sources;
  2. ``ops.fusion_compact`` == numpy boolean indexing view by view, then concatenate (the reference's lines), on hand-made masks;
  3. ``dtu_fusion.fuse_scan`` / ``fusion.dynamic_filter_scan``: the same result for every ``chunk``;
  4. ``fuse_scan`` on a scan directory == ``filter_depth``'s PLY bytes and masks;
  5. launch counts: a chunk of 2 and a chunk of 5 reference views record the same launches.

The bar is BITWISE (torch.equal / byte equality) everywhere: both sides are this library, a scan launch resolves the reference
view's pointers and runs the single-view body, and the compaction only moves values (the colour is one fp32 multiply and a
truncation on both sides).
"""
import numpy as np
import pytest
import torch

from common import t
from effi_mvs_plus_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAIRS = [(0, [1, 2]), (1, [0, 2, 3]), (2, [0, 1, 3, 4, 5]), (3, [5, 4, 2, 1]), (5, [4, 3])]
SIZES = [(37, 53), (7, 9)]            # not a multiple of the 256-pixel workgroup; less than one wave
N_VIEWS = 6


def _dtu_scan(h, w, seed=3):
    d, cams = synth.synth_depth_maps(h, w, N_VIEWS, seed=seed, noise_mm=0.03, outlier_frac=0.08, pixel_center=0.0)
    g = torch.Generator().manual_seed(seed + 7)
    conf = torch.rand(N_VIEWS, h // 2, w // 2, generator=g)
    img = torch.rand(N_VIEWS, h, w, 3, generator=g)
    return t(d, DEV), t(cams, DEV), t(conf, DEV), t(img, DEV)


def _tank_scan(h, w, seed=4):
    d, cams = synth.synth_depth_maps(h, w, N_VIEWS, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    conf = torch.rand(N_VIEWS, h // 2, w // 2, generator=g)
    img = torch.rand(N_VIEWS, 3, h, w, generator=g)
    return t(d, DEV), t(cams, DEV), t(conf, DEV), t(img, DEV)


def _mixed(name, m):
    frac = float(m.float().mean())
    print(f"[fusion scan] {name}: final mask keeps {frac:.3f}")
    assert 0.0 < frac < 1.0, f"{name}: the final mask must be neither empty nor full ({frac})"


# ---------------------------------------------------------------------------------------------------------------------------
# 1. scan launch == per-view launches
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
def test_dtu_scan_launch_equals_the_per_view_launches(h, w):
    from effi_mvs_plus_amd import ops
    d, cams, conf, _ = _dtu_scan(h, w)
    table = ops.fusion_pair_table(PAIRS)
    refs = [ref for ref, _ in PAIRS]
    got = ops.fusion_dtu_filter_scan(d, cams, table, conf[refs].contiguous(), conf_threshold=0.3)
    assert tuple(got["points"].shape) == (len(PAIRS), 3, h, w)
    for r, (ref, srcs) in enumerate(PAIRS):
        want = ops.fusion_dtu_filter(d[ref].contiguous(), torch.stack([d[v] for v in srcs]), cams[ref].contiguous(),
                                     torch.stack([cams[v] for v in srcs]), conf[ref].contiguous(), conf_threshold=0.3)
        for k in ("depth", "photo_mask", "geo_mask", "mask", "points"):
            assert torch.equal(got[k][r], want[k]), (k, ref)
        _mixed(f"dtu {h}x{w} ref {ref}", want["mask"])
    # without a confidence map and without points: still row for row the single-view launch
    got = ops.fusion_dtu_filter_scan(d, cams, table, None, conf_threshold=0.3, want_points=False)
    assert got["points"] is None
    for r, (ref, srcs) in enumerate(PAIRS):
        want = ops.fusion_dtu_filter(d[ref].contiguous(), torch.stack([d[v] for v in srcs]), cams[ref].contiguous(),
                                     torch.stack([cams[v] for v in srcs]), None, conf_threshold=0.3, want_points=False)
        for k in ("depth", "photo_mask", "geo_mask", "mask"):
            assert torch.equal(got[k][r], want[k]), (k, ref)


@pytest.mark.parametrize("relative", [False, True])
@pytest.mark.parametrize("with_conf", [True, False])
@pytest.mark.parametrize("h,w", SIZES)
def test_tank_scan_launch_equals_the_per_view_launches(h, w, with_conf, relative):
    from effi_mvs_plus_amd import fusion, ops
    d, cams, conf, img = _tank_scan(h, w)
    kept = [(ref, srcs) for ref, srcs in PAIRS if len(srcs) >= 3]          # test_tank.py:478 with dh_view_num = 2
    assert [ref for ref, _ in kept] == [1, 2, 3]
    refs = [ref for ref, _ in kept]
    got = ops.fusion_dynamic_filter_scan(d, cams, ops.fusion_pair_table(kept), conf[refs].contiguous() if with_conf else None, 0.3, 2, 4.0,
                                         1.3, relative)
    drv = fusion.dynamic_filter_scan(d, conf if with_conf else None, cams, img, PAIRS, prob_threshold=0.3, dh_view_num=2,
                                     dist_filter=4.0, depth_filter=1.3, relative=relative)
    assert drv["ref_ids"] == refs                                          # the two-source views 0 and 5 contribute nothing
    xyz, rgb, offs = [], [], [0]
    for r, (ref, srcs) in enumerate(kept):
        want = ops.fusion_dynamic_filter(d[ref].contiguous(), torch.stack([d[v] for v in srcs]), cams[ref].contiguous(),
                                         torch.stack([cams[v] for v in srcs]), conf[ref].contiguous() if with_conf else None, 0.3, 2, 4.0,
                                         1.3, relative)
        for k in ("depth", "geo_mask", "prob_mask", "mask", "points"):
            assert torch.equal(got[k][r], want[k]), (k, ref)
            if k != "points":
                assert torch.equal(drv[k][r], want[k].bool() if k != "depth" else want[k]), (k, ref)
        name = f"tank {h}x{w} conf={with_conf} relative={relative} ref {ref}"
        if (h, w) == (7, 9) and not relative:
            # One pixel of a 7x9 map spans ~50 mm of the synthetic scene, so the reference's half-pixel sampling offset alone moves a
            # reprojected depth by more than the absolute thresholds (i / 1.3 mm, i = 2 .. V): the CPU oracle
            # (oracle/effi_oracle.py::fusion_dynamic_filter) keeps 0.000 of every retained view here, with and without a confidence
            # map, for seed 4 and for every noise setting of synth_depth_maps.  No input of this size can make this cell's final
            # mask mixed; what it can show is the empty mask row for row (M = 0 through the driver) and a mixed prob mask.
            assert not want["geo_mask"].any() and not want["mask"].any(), name
            if with_conf:
                _mixed(name + " (prob mask)", want["prob_mask"])
        else:
            _mixed(name, want["mask"])
        # the driver's lines test_tank.py:517-533 on this view
        m = want["mask"].cpu().numpy().astype(bool)
        p, im = want["points"].cpu().numpy(), img[ref].cpu().numpy()
        xyz.append(np.stack([p[k][m] for k in range(3)], -1))
        rgb.append((np.stack([im[k][m] for k in range(3)], -1) * 255).astype(np.uint8))
        offs.append(offs[-1] + int(m.sum()))
    assert drv["xyz"].cpu().numpy().tobytes() == np.concatenate(xyz).tobytes()
    assert drv["rgb"].cpu().numpy().tobytes() == np.concatenate(rgb).tobytes()
    assert drv["offsets"].tolist() == offs
    for chunk in (1, 2):
        again = fusion.dynamic_filter_scan(d, conf if with_conf else None, cams, img, PAIRS, prob_threshold=0.3, dh_view_num=2,
                                           dist_filter=4.0, depth_filter=1.3, relative=relative, chunk=chunk)
        for k in ("xyz", "rgb", "offsets", "depth", "prob_mask", "geo_mask", "mask"):
            assert torch.equal(again[k], drv[k]), (k, chunk)


def test_scan_launches_refuse_17_sources_and_ids_outside_the_scan():
    from effi_mvs_plus_amd import ops
    from effi_mvs_plus_amd._lib import EffiLibraryError
    d, cams, _, _ = _dtu_scan(7, 9)
    seventeen = ops.fusion_pair_table([(0, [1, 2, 3, 4, 5] * 3 + [1, 2])])
    outside = ops.fusion_pair_table([(0, [1, 2, 3]), (1, [0, N_VIEWS, 2])])
    outside_ref = ops.fusion_pair_table([(N_VIEWS, [1, 2, 3])])
    for bad in (seventeen, outside, outside_ref):
        with pytest.raises(EffiLibraryError):
            ops.fusion_dtu_filter_scan(d, cams, bad)
        with pytest.raises(EffiLibraryError):
            ops.fusion_dynamic_filter_scan(d, cams, bad)
    with pytest.raises(EffiLibraryError):                                  # a row with fewer sources than dh_view_num
        ops.fusion_dynamic_filter_scan(d, cams, ops.fusion_pair_table([(0, [1, 2, 3]), (1, [0])]), dh_view_num=2)
    ok = ops.fusion_pair_table([(0, [1, 2, 3, 4, 5] * 3 + [1])])           # 16 sources is the limit, not beyond it
    assert tuple(ops.fusion_dtu_filter_scan(d, cams, ok)["depth"].shape) == (1, 7, 9)


def test_one_row_table_is_the_single_view_launch_for_all_three_filters():
    """One kernel under its two addressings at 5x7 (one partial workgroup, odd width): the table [0, 1, 2, 3] over four views names
    what the single-view form gets as (reference, stacked sources), so every output is bitwise the same; both forms refuse h = 1."""
    from effi_mvs_plus_amd import ops
    from effi_mvs_plus_amd._lib import EffiLibraryError
    h, w = 5, 7
    table = ops.fusion_pair_table([(0, [1, 2, 3])])
    assert table.tolist() == [[0, 1, 2, 3]]
    conf = t(torch.rand(1, 3, 4, generator=torch.Generator().manual_seed(11)), DEV)
    dtu_rig = synth.synth_depth_maps(h, w, 4, seed=3, noise_mm=0.03, outlier_frac=0.08, pixel_center=0.0)
    tank_rig = synth.synth_depth_maps(h, w, 4, seed=4)
    for rig, scan, single, kw in (
            (dtu_rig, ops.fusion_dtu_filter_scan, ops.fusion_dtu_filter, dict(conf_threshold=0.3)),
            (tank_rig, ops.fusion_dynamic_filter_scan, ops.fusion_dynamic_filter, dict(prob_threshold=0.3, dh_view_num=2, rel_diff_base=1.3)),
            (tank_rig, ops.fusion_static_filter_scan, ops.fusion_static_filter, dict(prob_threshold=0.3))):
        d, cams = t(rig[0], DEV), t(rig[1], DEV)
        got = scan(d, cams, table, conf, **kw)
        want = single(d[0].contiguous(), d[1:].contiguous(), cams[0].contiguous(), cams[1:].contiguous(), conf[0].contiguous(), **kw)
        assert len(got) == 5
        for k, v in got.items():
            assert tuple(v.shape[:1]) == (1,) and torch.equal(v[0], want[k]), (single.__name__, k)
        flat = d[:, :1].contiguous()                                       # h = 1
        with pytest.raises(EffiLibraryError):
            scan(flat, cams, table, **kw)
        with pytest.raises(EffiLibraryError):
            single(flat[0].contiguous(), flat[1:].contiguous(), cams[0].contiguous(), cams[1:].contiguous(), **kw)
    # a single view of 2^31 pixels is past the kernel's int pixel index: EFFI_ERR_BADARG from every single-view entry, before any launch.
    # The pointers are one small tensor's address: nothing may read or write through them.  That holds because each entry returns from
    # fus_check (null pointers, sizes, then this limit) before fus_run launches anything; keep that order, or give these calls real maps.
    L, p, s = ops._lib.lib(), d.data_ptr(), ops._stream()
    assert L.effi_fusion_dynamic_filter_f32(p, p, p, p, 3, 65536, 32768, None, 0, 0, 0.3, 2, 4.0, 1.3, 0, p, p, None, None, None, None, None, s) == -1
    assert L.effi_fusion_dtu_filter_f32(p, p, p, p, 3, 65536, 32768, None, 0.3, 0.75, 1, 11, 0.5, 0.25, p, p, None, None, None, None, s) == -1
    assert L.effi_fusion_static_filter_f32(p, p, p, p, 3, 65536, 32768, None, 0, 0, 0.3, 1.0, 0.01, 4.0, p, p, None, None, None, None, None, None,
                                           s) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. compaction == numpy boolean indexing
# ---------------------------------------------------------------------------------------------------------------------------
def _compact_case(mask, seed=0):
    """mask [n,h,w] bool -> the inputs of both layouts and the reference's arrays.  View 0's colours walk through k/255 for all k, as
    ``read_img`` makes them (uint8 / 255. in float32); the other views hold arbitrary floats of [0, 1)."""
    n, h, w = mask.shape
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((n, 3, h, w)).astype(np.float32)
    img = rng.random((n, h, w, 3), dtype=np.float32)
    k255 = np.arange(256, dtype=np.float32) / 255
    img[0] = np.resize(k255, h * w * 3).reshape(h, w, 3)
    chw = np.ascontiguousarray(img.transpose(0, 3, 1, 2))
    xyz = [pts[v][:, mask[v]].transpose((1, 0)) for v in range(n)]                                  # test_dtu_dypcd.py:332
    rgb_hwc = [(img[v][mask[v]] * 255).astype(np.uint8) for v in range(n)]                          # test_dtu_dypcd.py:333
    rgb_chw = [(np.stack([chw[v, k][mask[v]] for k in range(3)], -1) * 255).astype(np.uint8) for v in range(n)]   # test_tank.py:529-533
    offs = np.concatenate([[0], np.cumsum(mask.reshape(n, -1).sum(1))])
    return pts, img, chw, np.concatenate(xyz), np.concatenate(rgb_hwc), np.concatenate(rgb_chw), offs


def _check_compact(mask, seed=0):
    from effi_mvs_plus_amd import ops
    pts, img, chw, xyz, rgb_hwc, rgb_chw, offs = _compact_case(mask, seed)
    assert np.array_equal(rgb_hwc, rgb_chw)
    m = torch.from_numpy(mask.astype(np.uint8)).to(DEV)
    p = torch.from_numpy(pts).to(DEV)
    for layout, im in (("hwc", img), ("chw", chw)):
        x, c, o = ops.fusion_compact(m, p, torch.from_numpy(im).to(DEV), layout)
        assert x.dtype == torch.float32 and c.dtype == torch.uint8 and tuple(x.shape) == tuple(c.shape) == (int(mask.sum()), 3)
        assert o.tolist() == offs.tolist(), layout
        assert x.cpu().numpy().tobytes() == xyz.tobytes(), layout
        assert c.cpu().numpy().tobytes() == rgb_hwc.tobytes(), layout
    return rgb_hwc


N, H, W = 3, 20, 29                   # 580 pixels per view: three workgroups, the last one partly filled


def _hand_masks():
    z = np.zeros((N, H, W), bool)
    first, last, lanes = z.copy(), z.copy(), z.copy()
    first[0, 0, 0] = True
    last[N - 1, H - 1, W - 1] = True
    lanes.reshape(N, -1)[1, 256 + 63] = lanes.reshape(N, -1)[1, 256 + 64] = True    # last lane of wave 0, first lane of wave 1
    return {"none": z, "all": ~z, "first_pixel": first, "last_pixel_of_last_view": last, "lanes_63_64": lanes,
            "half": np.random.default_rng(5).random((N, H, W)) < 0.5}


@pytest.mark.parametrize("name", ["none", "all", "first_pixel", "last_pixel_of_last_view", "lanes_63_64", "half"])
def test_compaction_equals_numpy_boolean_indexing(name):
    mask = _hand_masks()[name]
    rgb = _check_compact(mask)
    if name == "all":                                                      # every k/255 went through the colour conversion
        assert len(np.unique(rgb[:H * W].reshape(-1))) >= 200


def test_compaction_scans_more_counts_than_one_pass_of_the_scan_kernel():
    """The scan kernel walks the per-workgroup counts in tiles of ``effi_fusion_compact_scan_tile()`` (its thread count x items per
    thread) and carries the running total from tile to tile: five views whose workgroup counts together exceed one tile by ~10 %, so
    that the tile edge falls inside a view and the carry is exercised."""
    from effi_mvs_plus_amd import _lib
    L = _lib.lib()
    tile = L.effi_fusion_compact_scan_tile()
    n, w = 5, 481
    h = -(-(tile * 256 * 11 // 10) // (n * w)) + 1
    assert L.effi_fusion_compact_blocks(n, h, w) > tile and L.effi_fusion_compact_blocks(n - 1, h, w) < tile
    mask = np.random.default_rng(11).random((n, h, w)) < 0.5
    mask[2, : h // 3] = False                                              # a run of empty workgroups too
    _check_compact(mask, seed=3)


def test_compaction_refuses_2_to_the_31_pixels():
    from effi_mvs_plus_amd import _lib, ops
    L = _lib.lib()
    m = torch.zeros(1, 4, 4, dtype=torch.uint8, device=DEV)
    buf = torch.zeros(64, dtype=torch.int32, device=DEV)
    assert L.effi_fusion_compact_blocks(32768, 256, 256) == 0 and L.effi_fusion_compact_blocks(32767, 256, 256) == 32767 * 256
    rc = L.effi_fusion_compact_count_u8(m.data_ptr(), 32768, 256, 256, buf.data_ptr(), buf.data_ptr(), ops._stream())
    assert rc == -1                                                        # EFFI_ERR_BADARG, before anything is launched
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. fuse_scan: the same for every chunk
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dtu_fused():
    from effi_mvs_plus_amd import dtu_fusion
    d, cams, conf, img = _dtu_scan(37, 53)
    return (d, cams, conf, img), dtu_fusion.fuse_scan(d, conf, cams, img, PAIRS, conf=0.3)


@pytest.mark.parametrize("chunk", [1, 2, len(PAIRS)])
def test_fuse_scan_is_the_same_for_every_chunk(dtu_fused, chunk):
    from effi_mvs_plus_amd import dtu_fusion
    (d, cams, conf, img), whole = dtu_fused
    got = dtu_fusion.fuse_scan(d, conf, cams, img, PAIRS, conf=0.3, chunk=chunk)
    assert set(got) == set(whole) == {"xyz", "rgb", "offsets", "depth_est_averaged", "photo_mask", "geo_mask", "final_mask"}
    for k in whole:
        assert got[k].dtype == whole[k].dtype and torch.equal(got[k], whole[k]), (k, chunk)
    m = got["xyz"].shape[0]
    assert 0 < m < len(PAIRS) * 37 * 53 and got["offsets"].tolist()[-1] == m
    assert got["offsets"].tolist() == [0] + np.cumsum(got["final_mask"].reshape(len(PAIRS), -1).sum(1).cpu().numpy()).tolist()


def test_fuse_scan_equals_filter_view_and_numpy_indexing(dtu_fused):
    """The parent's way -- ``filter_view`` per reference view, masks and points to the host, boolean indexing, concatenate."""
    from effi_mvs_plus_amd import dtu_fusion
    (d, cams, conf, img), whole = dtu_fused
    K = [cams[v, 1, :3, :3].cpu().numpy() for v in range(N_VIEWS)]
    E = [cams[v, 0].cpu().numpy() for v in range(N_VIEWS)]
    xyz, rgb = [], []
    for r, (ref, srcs) in enumerate(PAIRS):
        one = dtu_fusion.filter_view(d[ref], K[ref], E[ref], torch.stack([d[v] for v in srcs]), [K[v] for v in srcs], [E[v] for v in srcs],
                                     conf[ref], 0.3)
        m = one["final_mask"].cpu().numpy()
        assert torch.equal(whole["final_mask"][r], one["final_mask"]) and torch.equal(whole["depth_est_averaged"][r], one["depth_est_averaged"])
        xyz.append(one["xyz_world"].cpu().numpy()[:, m].transpose((1, 0)))
        rgb.append((img[ref].cpu().numpy()[m] * 255).astype(np.uint8))
    assert whole["xyz"].cpu().numpy().tobytes() == np.concatenate(xyz).tobytes()
    assert whole["rgb"].cpu().numpy().tobytes() == np.concatenate(rgb).tobytes()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. end to end: a scan directory through filter_depth and through fuse_scan
# ---------------------------------------------------------------------------------------------------------------------------
def test_fuse_scan_writes_the_ply_filter_depth_writes(tmp_path):
    """The 4-view 64x96 scan directory of test_fusion.py::test_dtu_filter_parity_unpinned_scan_directory_end_to_end in the reference's
    formats; ``filter_depth`` reads it from disk, ``fuse_scan`` takes the same maps loaded to the device."""
    from PIL import Image
    from effi_mvs_plus_amd import dtu_fusion
    from effi_mvs_plus_amd.datasets.data_io import read_pfm, save_pfm
    H, W, N = 64, 96, 4
    d, cams = synth.synth_depth_maps(H, W, N, seed=2, noise_mm=0.03, outlier_frac=0.08, pixel_center=0.0)
    K = [cams[v, 1, :3, :3].numpy().astype(np.float32) for v in range(N)]
    E = [cams[v, 0].numpy().astype(np.float32) for v in range(N)]
    scan, pairs = tmp_path / "out" / "scan1", tmp_path / "data" / "scan1"
    for sub in ("cams", "images", "depth_est", "confidence"):
        (scan / sub).mkdir(parents=True, exist_ok=True)
    pairs.mkdir(parents=True)
    rng = np.random.default_rng(1)
    with open(pairs / "pair.txt", "w") as f:
        f.write(f"{N}\n")
        for v in range(N):
            srcs = [u for u in range(N) if u != v]
            f.write(f"{v}\n{len(srcs)} " + " ".join(f"{u} {100.0 - u}" for u in srcs) + "\n")
    for v in range(N):
        with open(scan / "cams" / f"{v:08d}_cam.txt", "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join(repr(float(x)) for x in row) for row in E[v]) + "\n\nintrinsic\n")
            f.write("\n".join(" ".join(repr(float(x)) for x in row) for row in K[v]) + "\n\n425.0 2.5\n")
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(scan / "images" / f"{v:08d}.jpg")
        save_pfm(str(scan / "depth_est" / f"{v:08d}.pfm"), d[v].numpy())
        save_pfm(str(scan / "confidence" / f"{v:08d}.pfm"), torch.rand(H // 2, W // 2, generator=torch.Generator().manual_seed(v)).numpy())
    ply = str(tmp_path / "out" / "mvsnet001_l3.ply")
    dtu_fusion.filter_depth(str(pairs), str(scan), str(scan), ply, conf=0.3, device=DEV)

    pair_data = dtu_fusion.read_pair_file(str(pairs / "pair.txt"))
    load = lambda sub, v: torch.from_numpy(np.ascontiguousarray(read_pfm(str(scan / sub / f"{v:08d}.pfm"))[0]))
    cam = [dtu_fusion.read_camera_parameters(str(scan / "cams" / f"{v:08d}_cam.txt")) for v in range(N)]
    out = dtu_fusion.fuse_scan(torch.stack([load("depth_est", v) for v in range(N)]).to(DEV),
                               torch.stack([load("confidence", v) for v in range(N)]).to(DEV),
                               torch.stack([dtu_fusion._cam_tensor(k, x, DEV) for k, x in cam]),
                               torch.stack([torch.from_numpy(dtu_fusion.read_img(str(scan / "images" / f"{v:08d}.jpg"))) for v in range(N)]).to(DEV),
                               pair_data, conf=0.3)
    ply2 = str(tmp_path / "out" / "scan_path.ply")
    dtu_fusion.write_ply(ply2, out["xyz"].cpu().numpy(), out["rgb"].cpu().numpy())
    body, body2 = (open(f, "rb").read().split(b"end_header\n", 1)[1] for f in (ply, ply2))
    m = out["xyz"].shape[0]
    assert 0 < m < N * H * W and len(body) == 15 * m
    assert body2 == body
    for r, (ref, _) in enumerate(pair_data):
        for kind in ("photo", "geo", "final"):
            png = np.array(Image.open(scan / "mask" / f"{ref:08d}_{kind}.png")) > 0
            assert np.array_equal(out[f"{kind}_mask"][r].cpu().numpy(), png), (ref, kind)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. launch counts
# ---------------------------------------------------------------------------------------------------------------------------
def _launches(fn):
    from effi_mvs_plus_amd import ops
    prof = ops.KernelProfile()
    ops.set_profile(prof)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ops.set_profile(None)
    return sum(1 for r in prof.records if r[2] is not None)


def test_fuse_scan_records_one_pass_of_launches_for_a_chunk():
    from effi_mvs_plus_amd import dtu_fusion, fusion
    d, cams, conf, img = _dtu_scan(37, 53)
    two = _launches(lambda: dtu_fusion.fuse_scan(d, conf, cams, img, PAIRS[:2], conf=0.3, chunk=2))
    five = _launches(lambda: dtu_fusion.fuse_scan(d, conf, cams, img, PAIRS, conf=0.3, chunk=5))
    assert two == five == 3, (two, five)                                   # filter, count + scan, scatter
    assert _launches(lambda: dtu_fusion.fuse_scan(d, conf, cams, img, PAIRS, conf=0.3, chunk=1)) == 5 * two
    d, cams, conf, img = _tank_scan(37, 53)
    kept = [p for p in PAIRS if len(p[1]) >= 3]
    run = lambda pairs: fusion.dynamic_filter_scan(d, conf, cams, img, pairs, 0.3, 2, 4.0, 1.3)
    assert _launches(lambda: run(kept[:1])) == _launches(lambda: run(kept)) == 3
