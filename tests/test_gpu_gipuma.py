"""The Gipuma fusion on the GPU (csrc/gipuma.hip, effi_mvs_plus_amd/gipuma.py) against the float64 interval
reference of tests/gipuma_ref.py on the cases of tests/gipuma_cases.py: every DECIDED pixel of mask and count and every KNOWN flag
exactly, every fused pixel's point and colour inside its interval; on the exact rigs nothing is undecided and everything is bitwise.
tests/test_gipuma_host.py asserts, on the CPU, that the reference meets its caps on these cases and that the checks catch planted
errors.
"""
import functools
import os

import numpy as np
import pytest
import torch

import fusion_bound as FB
import gipuma_cases as GC
import gipuma_ref as GR
from effi_mvs_plus_amd import ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = {}


def _dev(c):
    g = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(DEV)
    return g(c["depths"]), g(c["conf"]), g(c["cams"]), g(c["images"])


@functools.lru_cache(maxsize=None)
def ref_of(name):
    return GR.case_reference(GC.case(name))


@functools.lru_cache(maxsize=None)
def view_loop(name):
    """The per-view entry called in a Python loop over the case's reference views -> (views as numpy dicts, used [n,h*w] uint8)."""
    c = GC.case(name)
    depths, conf, cams, images = _dev(c)
    if conf is not None:
        depths = ops.fusion_gipuma_prob(depths, conf, c["prob_thr"])
    n, h, w = depths.shape
    used = torch.zeros(n, h, w, device=DEV, dtype=torch.uint8)
    views = []
    for ref, srcs in GC.rows_of(c):
        r = ops.fusion_gipuma_view(depths, cams, images, ref, srcs, used, c["thr"], c["num"])
        m = r["mask"].bool()
        views.append({"mask": m.reshape(-1).cpu().numpy(), "count": r["count"].reshape(-1).cpu().numpy(),
                      "points": torch.where(m[None], r["points"], torch.zeros_like(r["points"])).reshape(3, -1).cpu().numpy(),
                      "colour": torch.where(m[..., None], r["colour"], torch.zeros_like(r["colour"])).reshape(-1, 3).cpu().numpy()})
    return views, used.reshape(n, -1).cpu().numpy()


def _scan(name, chunk=None):
    from effi_mvs_plus_amd import gipuma
    c = GC.case(name)
    depths, conf, cams, images = _dev(c)
    return gipuma.fuse_scan(depths, conf, cams, images, c["pair_data"], c["prob_thr"], c["thr"], c["num"], chunk=chunk)


@pytest.mark.parametrize("name", GC.CASES)
def test_view_entry_against_the_interval_reference(name):
    c = GC.case(name)
    views, used = view_loop(name)
    rviews, flags = ref_of(name)
    st = RECORD.setdefault(name, FB.Stats(name))
    GR.check_scan(name, views, used, rviews, flags, st)
    if c["exact"] is not None:                                       # nothing undecided: every pixel of every output was compared
        plain, pused = GR.case_restate(c)
        assert np.array_equal(used, pused)
        for g, p in zip(views, plain):
            assert np.array_equal(g["mask"], p["mask"]) and np.array_equal(g["count"], p["count"])
            # the colour against the fp32 restatement in the same order, bitwise (the library is built without contraction)
            assert np.array_equal(g["colour"].view(np.uint32), p["colour"].view(np.uint32))
            if c["exact"] == "all":
                assert np.array_equal(g["points"].view(np.uint32), p["points"].view(np.uint32))
            st.bit_same += g["colour"].size
            st.bit_all += g["colour"].size
    fused = sum(int(v["mask"].sum()) for v in views)
    assert (fused == 0) == (name in GC.EMPTY)


@pytest.mark.parametrize("name", GC.CASES)
def test_fuse_scan_equals_the_view_loop(name):
    c = GC.case(name)
    views, used = view_loop(name)
    out = _scan(name)
    n, h, w = c["depths"].shape
    rows = GC.rows_of(c)
    assert out["ref_ids"] == [r for r, _ in rows]
    assert out["mask"].dtype == torch.bool and tuple(out["mask"].shape) == (len(rows), h, w)
    assert out["count"].dtype == torch.uint8 and tuple(out["count"].shape) == (len(rows), h, w)
    assert out["used"].dtype == torch.bool and tuple(out["used"].shape) == (n, h, w)
    assert out["xyz"].dtype == torch.float32 and out["rgb"].dtype == torch.uint8 and out["offsets"].dtype == torch.int32
    mask = np.stack([v["mask"] for v in views])
    assert np.array_equal(out["mask"].reshape(len(rows), -1).cpu().numpy(), mask)
    assert np.array_equal(out["count"].reshape(len(rows), -1).cpu().numpy(), np.stack([v["count"] for v in views]))
    assert np.array_equal(out["used"].reshape(n, -1).cpu().numpy(), used.astype(bool))
    assert out["offsets"].cpu().tolist() == [0] + np.cumsum(mask.sum(1)).tolist()
    xyz = np.concatenate([v["points"].T[v["mask"]] for v in views])
    rgb = np.concatenate([(v["colour"][v["mask"]] * np.float32(255.0)).astype(np.int32).astype(np.uint8) for v in views])
    assert tuple(out["xyz"].shape) == (int(mask.sum()), 3) and tuple(out["rgb"].shape) == (int(mask.sum()), 3)
    assert np.array_equal(out["xyz"].cpu().numpy().view(np.uint32), xyz.astype(np.float32).view(np.uint32))
    assert np.array_equal(out["rgb"].cpu().numpy(), rgb)


@pytest.mark.parametrize("name", ["general_37x53", "pairs", "exact_7x9"])
def test_fuse_scan_does_not_depend_on_chunk(name):
    base = _scan(name)
    for chunk in (1, 2):
        out = _scan(name, chunk)
        for k in ("xyz", "rgb", "offsets", "mask", "count", "used"):
            assert torch.equal(out[k], base[k]), (name, chunk, k)


def test_reversed_reference_order_gives_another_cloud():
    fwd, rev = _scan("exact_37x53"), _scan("exact_reversed")
    assert rev["ref_ids"] == fwd["ref_ids"][::-1]
    assert not torch.equal(fwd["mask"], rev["mask"].flip(0))
    assert fwd["xyz"].shape[0] > 0 and rev["xyz"].shape[0] > 0


def test_more_views_needed_than_sources_gives_an_empty_cloud():
    out = _scan("too_many_needed")
    n, h, w = GC.case("too_many_needed")["depths"].shape
    assert tuple(out["xyz"].shape) == (0, 3) and tuple(out["rgb"].shape) == (0, 3) and out["offsets"].cpu().tolist() == [0] * (n + 1)
    assert tuple(out["mask"].shape) == (n, h, w) and not out["mask"].any() and not out["used"].any()
    assert int(out["count"].max()) > 0                               # the counts are still reported


def test_refusals_come_before_any_launch():
    from effi_mvs_plus_amd import gipuma
    c = GC.case("exact_7x9")
    depths, _, cams, images = _dev(c)
    n, h, w = depths.shape
    used = torch.zeros(n, h, w, device=DEV, dtype=torch.uint8)
    for ref, srcs in ((1, [0, 1]), (0, [n]), (0, [-1]), (n, [0]), (0, [])):
        with pytest.raises(ValueError):
            ops.fusion_gipuma_view(depths, cams, images, ref, srcs, used)
    with pytest.raises(ValueError):
        gipuma.fuse_scan(depths, None, cams, images, [(0, [1]), (2, [2])])
    big = GC.case("full64")
    d, _, cm, im = _dev(big)
    d66, cm66, im66 = torch.cat([d, d[:1]]), torch.cat([cm, cm[:1]]), torch.cat([im, im[:1]])
    with pytest.raises(ValueError):
        gipuma.fuse_scan(d66, None, cm66, im66, [(0, list(range(1, 66)))])
    with pytest.raises(ValueError):
        gipuma.fuse_scan(d66, None, cm66, im66)                     # all-others sources: 65 per view
    assert not used.any()


def test_gipuma_filter_writes_the_ply_of_fuse_scan(tmp_path):
    """A scan directory in the reference's layout: gipuma_filter (probability filter on the host as the reference, fusion on the
    device) writes the PLY bytes that fuse_scan + write_ply give on the same maps; the folder mvsnet_to_gipuma writes fuses too."""
    from PIL import Image
    from effi_mvs_plus_amd import dtu_fusion, gipuma
    from effi_mvs_plus_amd.datasets.data_io import save_pfm
    H, W, N = 24, 40, 5
    d, cams = synth.synth_depth_maps(H, W, N, seed=2, noise_mm=0.03, outlier_frac=0.08, pixel_center=0.0)
    g = torch.Generator().manual_seed(9)
    conf = torch.rand(N, H, W, generator=g).numpy()
    scan = tmp_path / "out" / "scan1"
    for sub in ("cams", "images", "depth_est", "confidence"):
        (scan / sub).mkdir(parents=True)
    for v in range(N):
        name = "{:0>8}".format(v)
        K, E = cams[v, 1, :3, :3].numpy(), cams[v, 0].numpy()
        with open(scan / "cams" / f"{name}_cam.txt", "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join(repr(float(x)) for x in row) for row in E) + "\n\nintrinsic\n" +
                    "\n".join(" ".join(repr(float(x)) for x in row) for row in K) + "\n\n425.0 2.5\n")
        Image.fromarray((torch.rand(H, W, 3, generator=g).numpy() * 255).astype(np.uint8)).save(scan / "images" / f"{name}.png")
        save_pfm(scan / "depth_est" / f"{name}.pfm", d[v].numpy().astype(np.float32))
        save_pfm(scan / "confidence" / f"{name}.pfm", conf[v].astype(np.float32))
    plys = gipuma.gipuma_filter(["scan1"], str(tmp_path / "out"), 0.3, 0.25, 2, fusibile_exe_path="/nonexistent/fusibile")
    assert plys == [str(scan / "points_mvsnet" / "consistencyCheck-hip" / "final3d_model.ply")]
    images = np.stack([dtu_fusion.read_img(scan / "images" / "{:0>8}.png".format(v)) for v in range(N)])
    cams_read = np.stack([gipuma._cam_array(*gipuma.read_camera_parameters(scan / "cams" / "{:0>8}_cam.txt".format(v))) for v in range(N)])
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    out = gipuma.fuse_scan(tt(d.numpy()), tt(conf), tt(cams_read), tt(images), None, 0.3, 0.25, 2)
    assert 0 < out["xyz"].shape[0] < N * H * W
    dtu_fusion.write_ply(tmp_path / "want.ply", out["xyz"].cpu().numpy(), out["rgb"].cpu().numpy())
    assert open(plys[0], "rb").read() == open(tmp_path / "want.ply", "rb").read()
    # the reference's intermediate folder fuses as well (cameras recovered from the .P files by RQ)
    gipuma.mvsnet_to_gipuma(str(scan), str(scan / "points_mvsnet"))
    ply2 = gipuma.depth_map_fusion(str(scan / "points_mvsnet"), None, 0.25, 2)
    assert os.path.getsize(ply2) > 200 and b"element vertex" in open(ply2, "rb").read(200)
    # images of another size are refused
    Image.fromarray(np.zeros((H // 2, W // 2, 3), np.uint8)).save(scan / "images" / "00000000.png")
    with pytest.raises(ValueError):
        gipuma.gipuma_filter(["scan1"], str(tmp_path / "out"), 0.3, 0.25, 2)


def test_cloud_goes_straight_into_point_compare():
    from effi_mvs_plus_amd import dtu_eval
    xyz = _scan("general_lownoise")["xyz"]
    assert xyz.is_cuda and xyz.dtype == torch.float32 and xyz.shape[0] > 500
    lo, hi = xyz.amin(0).double(), xyz.amax(0).double()
    res = float((hi - lo).max()) / 38.0
    stl = (xyz[::3] + 0.5).contiguous()
    out = dtu_eval.point_compare(xyz, stl, torch.ones(40, 40, 40, dtype=torch.bool), torch.stack([lo, hi]).cpu(), res,
                                 [0.0, 0.0, 1.0, -float(xyz[:, 2].median())], dst=4.0)
    assert int(out["n_input"]) == xyz.shape[0] and 0 < int(out["n_reduced"]) <= xyz.shape[0]
    assert int(out["n_acc"]) > 0 and int(out["n_comp"]) > 0 and bool(torch.isfinite(out["overall"]))


def test_record_of_the_run():
    """Prints the per-case record that DESIGN 7.10 quotes (checks, share of the interval used, undecided) from the cases that ran
    before it.  It asserts nothing of its own: the assertions are the tests above."""
    for st in RECORD.values():
        print(st.line().replace("[fusion-bound]", "[gipuma-bound]"))
