"""GPU: the fixed-threshold visibility filter (misc/fusion.py:50-115) -- the fused kernel, the five drop-in
functions and the scan driver.

Values are gated against the float64 restatement of tests/static_fusion_ref.py within E (4 x the reference's own fp32 distance from
it, measured by tests/golden/make_golden_static_fusion.py and stored in the golden file); mask elements that E decides must equal the
float64 decision, the others may be at most 2 % of a case.  The rigs are the smallest at which each hazard exists
(static_fusion_ref.CASES): 13x17 (the +-1.1 clamp moves taps back inside; less than one workgroup), 9x20 and 33x65 with 5 % zero
depths, 16 sources, and the 96x128 golden rig.  Scan launches are compared bitwise with the single-view launch.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from common import t
import static_fusion_ref as SR
from effi_mvs_plus_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(name):
    c = SR.case(name)
    g = lambda k: t(torch.from_numpy(c[k]), DEV)                         # noqa: E731
    return c, g("ref_depth"), g("src_depths"), g("ref_cam"), g("src_cams"), g("conf")


def _np(x):
    return x.detach().cpu().numpy()


def _prob_mask(c):
    h, w = c["ref_depth"].shape
    return (F.interpolate(torch.from_numpy(c["conf"])[None, None], size=[h, w], mode="nearest") > c["prob_thr"])[0, 0].numpy()   # test_tank.py:473-474


@pytest.mark.parametrize("name", list(SR.CASES))
def test_fused_filter_and_the_drop_in_composition_pass_the_same_gates(name):
    from effi_mvs_plus_amd import fusion, ops
    c, rd, sd, rc, sc, conf = _dev(name)
    thr = (c["img_dist_thresh"], c["depth_thresh"], c["vthresh"])
    one = ops.fusion_static_filter(rd, sd, rc, sc, conf, c["prob_thr"], *thr, want_reproj=True)
    SR.check_outputs(name, dict(xyd=_np(one["reproj_xyd"]), in_range=_np(one["in_range"]), mask=_np(one["geo_mask"]),
                                depth=_np(one["depth"]), points=_np(one["points"])), "fused")
    pm = _prob_mask(c)
    assert np.array_equal(_np(one["prob_mask"]) != 0, pm) and 0.0 < pm.mean() < 1.0
    assert np.array_equal(_np(one["mask"]), _np(one["geo_mask"]) & _np(one["prob_mask"]))
    frac = float(one["mask"].float().mean())
    print(f"[static fusion] {name}: final mask keeps {frac:.3f}")
    assert 0.2 <= frac <= 0.9
    # the public form, and without the by-products: the same numbers
    pub = fusion.static_filter(rd[None, None], sd[None, :, None], rc[None], sc[None], conf[None], c["prob_thr"], *thr)
    assert tuple(pub["depth"].shape) == (1, 1) + tuple(rd.shape) and tuple(pub["points"].shape) == (1, 3) + tuple(rd.shape)
    assert pub["mask"].dtype == torch.bool and tuple(pub["mask"].shape) == (1, 1) + tuple(rd.shape)
    for k in ("depth", "points", "geo_mask", "prob_mask", "mask"):
        assert torch.equal(pub[k][0].reshape(one[k].shape).to(one[k].dtype), one[k]), k

    # the reference's lines, one function at a time
    xyd, in_range = fusion.get_reproj(rd[None, None], sd[None, :, None], rc[None], sc[None])
    v = sd.shape[0]
    assert tuple(xyd.shape) == (1, v, 3) + tuple(rd.shape) and tuple(in_range.shape) == (1, v, 1) + tuple(rd.shape)
    assert xyd.dtype == in_range.dtype == torch.float32
    masks, mask = fusion.vis_filter(rd[None, None], xyd, in_range, *thr)
    assert masks.dtype == torch.float32 and tuple(masks.shape) == (1, v, 1) + tuple(rd.shape)
    assert mask.dtype == torch.bool and tuple(mask.shape) == (1, 1) + tuple(rd.shape)
    depth = fusion.ave_fusion(rd[None, None], xyd, masks)
    assert tuple(depth.shape) == (1, 1) + tuple(rd.shape)
    idx_img = fusion.get_pixel_grids(*depth.size()[-2:]).unsqueeze(0)                                   # test_tank.py:513
    idx_cam = fusion.idx_img2cam(idx_img, depth, rc[None])                                              # :514
    points = fusion.idx_cam2world(idx_cam, rc[None])[..., :3, 0].permute(0, 3, 1, 2)                    # :515
    SR.check_outputs(name, dict(xyd=_np(xyd[0]), in_range=_np(in_range[0, :, 0]), masks=_np(masks[0, :, 0]), mask=_np(mask[0, 0]),
                                depth=_np(depth[0, 0]), points=_np(points[0])), "composition")
    # in_range does not enter the result (misc/fusion.py:106)
    masks0, mask0 = fusion.vis_filter(rd[None, None], xyd, torch.zeros_like(in_range), *thr)
    assert torch.equal(masks0, masks) and torch.equal(mask0, mask)
    same = {k: bool(torch.equal(a, b)) for k, a, b in (("depth", depth[0, 0], one["depth"]), ("mask", mask[0, 0], one["geo_mask"].bool()),
                                                       ("points", points[0].contiguous(), one["points"]))}
    print(f"[static fusion] {name}: fused == composition bitwise: {same}")


def test_seventeen_sources_and_ids_outside_the_scan_are_refused():
    from effi_mvs_plus_amd import ops
    from effi_mvs_plus_amd._lib import EffiLibraryError
    c, rd, sd, rc, sc, _ = _dev("max_16")
    assert sd.shape[0] == 16
    with pytest.raises(EffiLibraryError, match="code -2"):                 # EFFI_ERR_UNSUPPORTED, before anything is launched
        ops.fusion_static_filter(rd, torch.cat([sd, sd[:1]]), rc, torch.cat([sc, sc[:1]]))
    depths, cams = torch.cat([rd[None], sd]), torch.cat([rc[None], sc])
    n = depths.shape[0]
    seventeen = ops.fusion_pair_table([(0, list(range(1, 17)) + [1])])
    outside = ops.fusion_pair_table([(0, [1, 2, 3]), (1, [0, n, 2])])
    outside_ref = ops.fusion_pair_table([(n, [1, 2, 3])])
    for bad in (seventeen, outside, outside_ref):
        with pytest.raises(EffiLibraryError, match="code -1"):             # EFFI_ERR_BADARG from the host copy of the table
            ops.fusion_static_filter_scan(depths, cams, bad)
    for bad in (dict(img_dist_thresh=0.0), dict(depth_thresh=-1.0), dict(vthresh=float("nan"))):
        with pytest.raises(EffiLibraryError, match="code -1"):
            ops.fusion_static_filter(rd, sd, rc, sc, **bad)
    ok = ops.fusion_static_filter_scan(depths, cams, ops.fusion_pair_table([(0, list(range(1, 17)))]), None, 0.0, c["img_dist_thresh"],
                                       c["depth_thresh"], c["vthresh"])   # 16 sources is the limit, not beyond it
    one = ops.fusion_static_filter(rd, sd, rc, sc, None, 0.0, c["img_dist_thresh"], c["depth_thresh"], c["vthresh"])
    for k in ("depth", "geo_mask", "prob_mask", "mask", "points"):
        assert torch.equal(ok[k][0], one[k]), k
    torch.cuda.synchronize()


def test_golden_rig_through_the_reference_names():
    """Rig "a" (96x128, 5 sources) against what the reference returned: values within E of float64 (check_outputs) and, printed, their
    distance from the reference's own fp32 numbers; in_range equal to the reference's except where gx / gy is within E of +-1."""
    from effi_mvs_plus_amd import fusion
    g, E = SR.golden(), SR.bounds()
    c, rd, sd, rc, sc, conf = _dev("a")
    r = SR.case_ref("a")
    xyd, in_range = fusion.get_reproj(rd[None, None], sd[None, :, None], rc[None], sc[None])
    dxy, dd = np.abs(_np(xyd[0])[:, :2] - g["a_reproj_xyd"][:, :2]).max(), np.abs(_np(xyd[0])[:, 2] - g["a_reproj_xyd"][:, 2]).max()
    print(f"[static fusion] a: |get_reproj - reference fp32| x,y {dxy:.3e}  d {dd:.3e}")
    assert dxy <= 1.25 * E["xy"] and dd <= 1.25 * E["d"]                  # both sides within E and E / 4 of float64
    dec = SR.in_range_decided(r["gx"], r["gy"], E["g"])
    assert np.array_equal(_np(in_range[0, :, 0])[dec], g["a_in_range"][dec].astype(np.float32)) and dec.mean() > 0.99
    # the reference's own reproj_xyd through vis_filter / ave_fusion: the same inputs as the reference's lines had
    gx = t(torch.from_numpy(g["a_reproj_xyd"]), DEV)[None]
    masks, mask = fusion.vis_filter(rd[None, None], gx, in_range, c["img_dist_thresh"], c["depth_thresh"], c["vthresh"])
    dist, ddiff = SR.vis_quantities(c["ref_depth"], g["a_reproj_xyd"])
    t_dist, t_d, _ = SR.thresholds(c["img_dist_thresh"], c["depth_thresh"], c["vthresh"])
    tie = 8 * 2.0 ** -23 * np.maximum(1.0, np.abs(c["ref_depth"]))[None]  # the fp32 subtraction and norm of given fp32 numbers: a few ulp
    clear = (np.abs(dist - t_dist) > tie) & (np.abs(ddiff - t_d) > tie)
    print(f"[static fusion] a: vis_filter on the reference's reproj_xyd: {int((~clear).sum())} elements within a few ulp of a threshold, "
          f"{int((_np(masks[0, :, 0]) != g['a_masks']).sum())} differ from the reference")
    assert np.array_equal(_np(masks[0, :, 0])[clear], g["a_masks"][clear].astype(np.float32)) and clear.mean() > 0.999
    ave = fusion.ave_fusion(rd[None, None], gx, t(torch.from_numpy(g["a_masks"]), DEV)[None, :, None])
    e = np.abs(_np(ave[0, 0]) - SR.ave(c["ref_depth"], g["a_reproj_xyd"], g["a_masks"])).max()
    print(f"[static fusion] a: |ave_fusion - f64| on the reference's inputs {e:.3e} (E {E['ave']:.3e})")
    assert e <= E["ave"]
    if np.array_equal(_np(masks[0, :, 0]), g["a_masks"]):
        assert np.array_equal(_np(mask[0, 0]), g["a_mask"] != 0)
    # static_filter against the reference's final mask and points on the decided pixels
    out = fusion.static_filter(rd[None, None], sd[None, :, None], rc[None], sc[None], conf[None], c["prob_thr"], c["img_dist_thresh"],
                               c["depth_thresh"], c["vthresh"])
    rr = SR.case_ref("a", tuple(sorted(E.items())))
    sel = rr["mask_decided"]
    assert np.array_equal(_np(out["prob_mask"][0, 0]), g["a_prob_mask"] != 0)
    assert np.array_equal(_np(out["mask"][0, 0])[sel], (g["a_final"] != 0)[sel]) and np.array_equal(_np(out["geo_mask"][0, 0])[sel], (g["a_mask"] != 0)[sel])
    sel = rr["all_decided"]
    e = np.abs(_np(out["points"][0]) - g["a_points"])[:, sel].max()
    print(f"[static fusion] a: |static_filter points - reference fp32| {e:.3e} on {sel.mean():.4f} of the pixels")
    assert e <= 1.25 * E["pts"]


def test_prob_filter_three_channels_equals_the_reference():
    from effi_mvs_plus_amd import fusion
    g = SR.golden()
    prob = torch.rand(1, 3, 1, 96, 128, generator=torch.Generator().manual_seed(int(g["prob3_seed"])))
    both = torch.cat([prob, prob.flip(1)]).to(DEV)                        # a batch of two, the second with its channels reversed
    thr = [float(x) for x in g["prob3_thresholds"]]
    mask = fusion.prob_filter(both, thr)
    assert mask.dtype == torch.bool and tuple(mask.shape) == (2, 1, 1, 96, 128)
    assert np.array_equal(_np(mask[0, 0, 0]), g["prob3_mask"] != 0) and 0.1 < g["prob3_mask"].mean() < 0.9
    want = (both[1, 0] > thr[0]) & (both[1, 1] > thr[1]) & (both[1, 2] > thr[2])
    assert torch.equal(mask[1, 0], want)
    assert torch.equal(fusion.prob_filter(both, thr[:1], greater=False)[:, 0], both[:, 0] > thr[0])     # fewer thresholds than channels; greater is ignored
    assert fusion.prob_filter(both, []) is None


def test_project_img_five_channels_into_a_smaller_destination():
    from effi_mvs_plus_amd import fusion
    g, E = SR.golden(), SR.bounds()
    c, rd, sd, rc, sc, _ = _dev("a")
    hh, ww = g["proj_warped"].shape[-2:]
    src_img = torch.rand(1, 5, 96, 128, generator=torch.Generator().manual_seed(int(g["proj_seed"])))
    dst_depth = rd[:hh, :ww].contiguous()[None, None]
    # a batch of two: the second element with another source camera and the channels reversed
    imgs = torch.cat([src_img, src_img.flip(1)]).to(DEV)
    warped, in_range = fusion.project_img(imgs, dst_depth.expand(2, 1, hh, ww), sc[:2], rc[None].expand(2, 2, 4, 4), hh, ww)
    assert tuple(warped.shape) == (2, 5, hh, ww) and tuple(in_range.shape) == (2, 1, hh, ww) and in_range.dtype == torch.float32
    for b in range(2):
        w64, gx, gy = SR.project_img(_np(imgs[b]), c["ref_depth"][:hh, :ww], c["src_cams"][b], c["ref_cam"], hh, ww)
        e = np.abs(_np(warped[b]) - w64).max()
        dec = SR.in_range_decided(gx, gy, E["g"])
        want_in = (-1 <= gx) & (gx <= 1) & (-1 <= gy) & (gy <= 1)
        print(f"[static fusion] project_img batch {b}: |warped - f64| {e:.3e} (E {E['img']:.3e}), in_range {want_in.mean():.3f} full")
        assert e <= E["img"] and np.array_equal((_np(in_range[b, 0]) != 0)[dec], want_in[dec]) and 0.0 < want_in.mean() < 1.0
    e = np.abs(_np(warped[0]) - g["proj_warped"]).max()
    print(f"[static fusion] project_img: |warped - reference fp32| {e:.3e}")
    assert e <= 1.25 * E["img"]
    _, gx, gy = SR.project_img(_np(imgs[0]), c["ref_depth"][:hh, :ww], c["src_cams"][0], c["ref_cam"], hh, ww)
    dec = SR.in_range_decided(gx, gy, E["g"])
    assert np.array_equal((_np(in_range[0, 0]) != 0)[dec], (g["proj_in_range"] != 0)[dec])
    # default size: the source's own
    w2, r2 = fusion.project_img(imgs[:1, :, :hh, :ww].contiguous(), dst_depth, sc[:1], rc[None])
    assert tuple(w2.shape) == (1, 5, hh, ww) and tuple(r2.shape) == (1, 1, hh, ww)


# ---------------------------------------------------------------------------------------------------------------------------
# the scan: 6 views of 24x40, 1-4 sources per row, one row without sources
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan():
    from effi_mvs_plus_amd import fusion
    s = SR.SCAN
    d, cams = synth.synth_depth_maps(s["h"], s["w"], s["n"], seed=s["seed"], **SR.SYNTH)
    g = torch.Generator().manual_seed(s["seed"] + 7)
    conf = torch.rand(s["n"], 2 * s["h"], 2 * s["w"], generator=g)
    img = torch.rand(s["n"], 3, s["h"], s["w"], generator=g)
    d, cams, conf, img = t(d, DEV), t(cams, DEV), t(conf, DEV), t(img, DEV)
    thr = (s["prob_thr"], s["img_dist_thresh"], s["depth_thresh"], s["vthresh"])
    return (d, cams, conf, img, thr), fusion.static_filter_scan(d, conf, cams, img, s["pairs"], *thr)


def test_scan_rows_equal_the_single_view_launch_and_numpy_indexing(scan):
    from effi_mvs_plus_amd import fusion, ops
    (d, cams, conf, img, thr), drv = scan
    kept = fusion.static_scan_rows(SR.SCAN["pairs"])
    refs = [ref for ref, _ in kept]
    assert drv["ref_ids"] == refs == [0, 1, 3, 4, 5]                       # view 2 has no source and is dropped
    assert sorted(len(s) for _, s in kept) == [1, 2, 2, 3, 4]
    got = ops.fusion_static_filter_scan(d, cams, ops.fusion_pair_table(kept), conf[refs].contiguous(), *thr)
    xyz, rgb, offs = [], [], [0]
    for r, (ref, srcs) in enumerate(kept):
        want = ops.fusion_static_filter(d[ref].contiguous(), torch.stack([d[v] for v in srcs]), cams[ref].contiguous(),
                                        torch.stack([cams[v] for v in srcs]), conf[ref].contiguous(), *thr)
        for k in ("depth", "geo_mask", "prob_mask", "mask", "points"):
            assert torch.equal(got[k][r], want[k]), (k, ref)
            if k != "points":
                assert torch.equal(drv[k][r], want[k].bool() if k != "depth" else want[k]), (k, ref)
        frac = float(want["mask"].float().mean())
        print(f"[static fusion] scan ref {ref} ({len(srcs)} sources): final mask keeps {frac:.3f}")
        assert 0.0 < frac < 1.0, f"ref {ref}: the final mask must be neither empty nor full"
        m = _np(want["mask"]).astype(bool)
        p, im = _np(want["points"]), _np(img[ref])
        xyz.append(np.stack([p[k][m] for k in range(3)], -1))                                           # test_tank.py:527-528
        rgb.append((np.stack([im[k][m] for k in range(3)], -1) * 255).astype(np.uint8))                 # :529-533
        offs.append(offs[-1] + int(m.sum()))
    assert 0 < offs[-1] < len(kept) * d.shape[1] * d.shape[2]
    assert _np(drv["xyz"]).tobytes() == np.concatenate(xyz).tobytes()
    assert _np(drv["rgb"]).tobytes() == np.concatenate(rgb).tobytes()
    assert drv["offsets"].tolist() == offs
    # without a confidence map: the photometric mask is all ones
    bare = ops.fusion_static_filter_scan(d, cams, ops.fusion_pair_table(kept), None, *thr, want_points=False)
    assert bare["points"] is None and bool(bare["prob_mask"].all()) and torch.equal(bare["geo_mask"], got["geo_mask"])


@pytest.mark.parametrize("chunk", [1, 2, 5])
def test_scan_result_is_the_same_for_every_chunk(scan, chunk):
    from effi_mvs_plus_amd import fusion
    (d, cams, conf, img, thr), whole = scan
    again = fusion.static_filter_scan(d, conf, cams, img, SR.SCAN["pairs"], *thr, chunk=chunk)
    assert set(again) == set(whole) == {"xyz", "rgb", "offsets", "ref_ids", "depth", "prob_mask", "geo_mask", "mask"}
    for k in ("xyz", "rgb", "offsets", "depth", "prob_mask", "geo_mask", "mask"):
        assert again[k].dtype == whole[k].dtype and torch.equal(again[k], whole[k]), (k, chunk)
    assert again["ref_ids"] == whole["ref_ids"]


def test_scan_of_views_without_sources_is_empty():
    from effi_mvs_plus_amd import fusion
    d, cams = torch.zeros(2, 8, 8, device=DEV), torch.eye(4, device=DEV).expand(2, 2, 4, 4).contiguous()
    out = fusion.static_filter_scan(d, None, cams, torch.zeros(2, 3, 8, 8, device=DEV), [(0, []), (1, [])])
    assert out["ref_ids"] == [] and tuple(out["xyz"].shape) == (0, 3) and out["offsets"].tolist() == [0]
