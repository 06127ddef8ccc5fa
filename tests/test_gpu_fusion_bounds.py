"""Every pixel of the depth-fusion filters decided by a float64 interval: the kernels of csrc/fusion.hip
through the product's wrappers (ops.*, fusion.*, dtu_fusion.*) against tests/fusion_bound.py, on the cases of tests/fusion_cases.py.

Every mask pixel the reference decides must equal its value; every continuous element must lie inside its interval (exactly on the
pinned value where half = 0).  The only elements excused are the undecided and left-out ones, which the reference names before a
result is looked at and whose share is capped (fusion_bound.assert_caps).  No agreement share, no frac_ok, no peak-scaled tolerance.
The share of elements that equal the fp32 restatement bit for bit is RECORDED (the `bitwise=` figure of each line), not asserted."""
import numpy as np
import pytest
import torch

import fusion_bound as FB
import fusion_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RECORD = {}


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _n(t_):
    return None if t_ is None else t_.detach().cpu().numpy()


def _stats(family):
    return RECORD.setdefault(family, FB.Stats(family))


def _tt_out(r):
    return {"depth": _n(r["depth"]).reshape(-1), "geo": _n(r["geo_mask"]).reshape(-1), "prob": _n(r["prob_mask"]).reshape(-1),
            "mask": _n(r["mask"]).reshape(-1), "points": None if r.get("points") is None else _n(r["points"]).reshape(3, -1),
            "xyd": None if r.get("reproj_xyd") is None else _n(r["reproj_xyd"]).reshape(r["reproj_xyd"].shape[0], 3, -1)}


@pytest.mark.parametrize("name", C.TT_CASES)
def test_tt_dynamic_filter_every_pixel_and_element(name):
    from effi_mvs_plus_amd import ops
    c, ref = C.tt_case(name), C.tt_ref(name)
    FB.assert_caps(name, ref)
    r = ops.fusion_dynamic_filter(_t(c["ref_depth"]), _t(c["src_depths"]), _t(c["ref_cam"]), _t(c["src_cams"]), _t(c["conf"]), c["prob_thr"],
                                  c["dh"], c["dist_base"], c["rel_base"], c["relative"], want_points=True, want_reproj=True)
    st = FB.Stats(name)
    for s in (st, _stats("tt_filter")):
        FB.check_tt_outputs(name, _tt_out(r), ref, s, restated=C.tt_restated(name))
        FB.count_decisions(ref, s)
    print(st.line())
    # the same launch without the optional outputs writes the same depth and masks
    q = ops.fusion_dynamic_filter(_t(c["ref_depth"]), _t(c["src_depths"]), _t(c["ref_cam"]), _t(c["src_cams"]), _t(c["conf"]), c["prob_thr"],
                                  c["dh"], c["dist_base"], c["rel_base"], c["relative"], want_points=False, want_reproj=False)
    assert q["points"] is None and q["reproj_xyd"] is None
    assert all(torch.equal(torch.nan_to_num(q[k].float()), torch.nan_to_num(r[k].float())) for k in ("depth", "geo_mask", "prob_mask", "mask"))


@pytest.mark.parametrize("name", ["fixture_b", "odd_v5_conf75x101", "border_v5"])
def test_tt_driver_forms_get_reproj_and_vis_filter(name):
    """fusion.get_reproj_dynamic and fusion.vis_filter_dynamic run as the T&T driver runs them."""
    from effi_mvs_plus_amd import fusion
    c, ref = C.tt_case(name), C.tt_ref(name)
    FB.assert_caps(name, ref)
    h, w = c["ref_depth"].shape
    V, n = len(c["src_depths"]), h * w
    st = _stats("tt_driver_forms")
    xyd, ref_idx_cam, src2ref = fusion.get_reproj_dynamic(_t(c["ref_depth"][None, None]), _t(c["src_depths"][None, :, None]), _t(c["ref_cam"][None]),
                                                          _t(c["src_cams"][None]))
    g = _n(xyd)[0].reshape(V, 3, n)
    rs = C.tt_restated(name)
    for s in range(V):
        for k in range(3):
            FB.check_elements(f"{name} get_reproj_dynamic xyd[{s},{k}]", g[s, k], ref["xyd"][s][k], st, rs["xyd"][s, k])
    ys, xs = FB.pixel_grid(h, w)
    grid = np.stack([xs + 0.5, ys + 0.5, np.ones(n)], 1).astype(np.float32)
    rc, sc = _n(ref_idx_cam).reshape(V, n, 4), _n(src2ref).reshape(V, n, 4)
    want_ref = FB.points_chain(FB.BND, 0, grid, c["ref_cam"], c["ref_depth"].reshape(-1))
    for s in range(V):
        back = np.stack([g[s, 0], g[s, 1], np.ones(n, np.float32)], 1)
        want_back = FB.points_chain(FB.BND, 0, back, c["ref_cam"], g[s, 2])
        for k in range(4):
            FB.check_elements(f"{name} ref_idx_cam[{s},{k}]", rc[s, :, k], _full(want_ref[k], n), st)
            FB.check_elements(f"{name} src2ref_idx_cam[{s},{k}]", sc[s, :, k], _full(want_back[k], n), st)
    masks, mask = fusion.vis_filter_dynamic(_t(c["ref_depth"][None, None]), xyd, ref_idx_cam, src2ref, dist_base=c["dist_base"],
                                            rel_diff_base=c["rel_base"], thres_view=c["dh"], relative=c["relative"])
    m = _n(masks)[0].reshape(V, -1, n)
    # pinned: the kernel's arithmetic on ITS inputs restates exactly; and decided: the reference's comparisons on the same pixels
    want = FB.vis_filter_f32(c["ref_depth"], _n(xyd)[0], c["dist_base"], c["rel_base"], c["dh"], c["relative"]).reshape(V, -1, n)
    assert np.array_equal(m, want), f"{name}: {int((m != want).sum())} vis_masks elements differ from the exact restatement"
    st.pinned += m.size
    st.checks += m.size
    for s in range(V):
        for k in range(m.shape[1]):
            FB.check_mask(f"{name} vis_masks[{s},{k}]", m[s, k], ref["T"][s, k], ~ref["Un"][s, k], st)
    assert torch.equal(mask, masks[:, :, -1:])


def _full(b, n):
    return FB.B(np.broadcast_to(b.m, (n,)), np.broadcast_to(b.e, (n,)))


@pytest.mark.parametrize("relative", [False, True])
def test_vis_filter_planted_ties_every_element_pinned(relative):
    from effi_mvs_plus_amd import ops
    t = C.vis_ties(relative)
    got = ops.fusion_vis_filter(_t(t["ref_depth"][None, None]), _t(t["xyd"][None]), t["dist_base"], t["rel_base"], t["thres"], relative)
    want = C.vis_ties_expected(t)
    g = _n(got)[0].astype(bool)
    st = _stats("vis_filter_ties")
    st.checks += g.size
    st.pinned += g.size
    st.bit_same += int((g == want).sum())
    st.bit_all += g.size
    assert np.array_equal(g, want), f"{int((g != want).sum())} of {g.size} planted ties decided wrongly: `<` is false at equality, true one ulp below"


def test_fusion_points_four_modes_on_the_reference_intermediates():
    from effi_mvs_plus_amd import ops
    st = _stats("points_modes")
    c = C.tt_case("fixture_b")
    h, w = c["ref_depth"].shape
    n = h * w
    for mode, pts, cam, depth in C.points_inputs("fixture_b"):
        got = ops.fusion_points(mode, _t(pts.reshape(1, h, w, pts.shape[1], 1)), _t(cam[None]), None if depth is None else _t(depth.reshape(1, 1, h, w)))
        g = _n(got).reshape(n, -1)
        bound = FB.points_chain(FB.BND, mode, pts, cam, depth)
        with np.errstate(all="ignore"):
            rs = FB.points_chain(FB.F32, mode, pts, cam, depth)
        assert g.shape[1] == len(bound)
        for k, b in enumerate(bound):
            FB.check_elements(f"fusion_points mode {mode}[{k}]", g[:, k], _full(b, n), st, np.broadcast_to(rs[k], (n,)))


def test_tt_scan_rows_with_different_source_counts_against_the_reference():
    """fusion_dynamic_filter_scan: every row against the interval reference of ITS reference view and sources (not against the
    per-view launch, which tests/test_gpu_fusion_scan.py compares bitwise)."""
    from effi_mvs_plus_amd import ops
    c = C.tt_scan()
    refs = [C.tt_scan_ref(r) for r in range(len(c["rows"]))]
    for r, ref in enumerate(refs):
        FB.assert_caps(f"scan row {r}", ref)
    pairs = ops.fusion_pair_table(c["rows"])
    out = ops.fusion_dynamic_filter_scan(_t(c["depths"]), _t(c["cams"]), pairs, _t(c["conf"]), c["prob_thr"], c["dh"], c["dist_base"], c["rel_base"],
                                         c["relative"], want_points=True)
    st = _stats("tt_scan")
    for r, ref in enumerate(refs):
        row = {k: out[k][r] for k in ("depth", "geo_mask", "prob_mask", "mask", "points")}
        FB.check_tt_outputs(f"scan row {r}", _tt_out(row), ref, st, restated=FB.tt_restate(*C.tt_scan_row(c, r)))
        FB.count_decisions(ref, st)


def _dtu_out(r):
    return {"depth": _n(r["depth"]).reshape(-1), "photo": _n(r["photo_mask"]).reshape(-1), "geo": _n(r["geo_mask"]).reshape(-1),
            "final": _n(r["mask"]).reshape(-1), "points": _n(r["points"]).reshape(3, -1)}


@pytest.mark.parametrize("name", C.DTU_CASES)
def test_dtu_filter_every_pixel_and_element(name):
    from effi_mvs_plus_amd import ops
    c, ref = C.dtu_case(name), C.dtu_ref(name)
    FB.assert_caps(name, ref, "final")
    r = ops.fusion_dtu_filter(_t(c["ref_depth"]), _t(c["src_depths"]), _t(c["ref_cam"]), _t(c["src_cams"]), _t(c["conf"]), c["conf_thr"],
                              c["conf_keep"], c["s"], c["e"], c["dist_base"], c["diff_base"])
    st = FB.Stats(name)
    for s in (st, _stats("dtu_filter")):
        FB.check_dtu_outputs(name, _dtu_out(r), ref, s, restated=C.dtu_restated(name))
        FB.count_decisions(ref, s, "geo", "final")
    print(st.line() + f" log_two={ref['log_two']}")


@pytest.mark.parametrize("name", ["tiny_n2", "odd_n3_loose", "odd_n3_short", "n5_tight", "rolled_n3"])
def test_dtu_reproject_both_forms(name):
    """fusion_dtu_reproject as reproject_with_depth (no masks) and as check_geometric_consistency (masks; the first three outputs are
    zero under a false last mask, pinned where the mask is decided), for every source view of the case."""
    from effi_mvs_plus_amd import ops
    c, ref, rs = C.dtu_case(name), C.dtu_ref(name), C.dtu_restated(name)
    FB.assert_caps(name, ref, "final")
    st = _stats("dtu_reproject")
    n = c["ref_depth"].size
    for sv in range(len(c["src_depths"])):
        out5, masks = ops.fusion_dtu_reproject(_t(c["ref_depth"]), _t(c["src_depths"][sv]), _t(c["ref_cam"]), _t(c["src_cams"][sv]))
        assert masks is None
        FB.check_dtu_out5(f"{name} reproject_with_depth[{sv}]", _n(out5).reshape(5, n), None, ref, sv, st, rs["out5"][sv])
        out5, masks = ops.fusion_dtu_reproject(_t(c["ref_depth"]), _t(c["src_depths"][sv]), _t(c["ref_cam"]), _t(c["src_cams"][sv]), s=c["s"], e=c["e"],
                                               dist_base=c["dist_base"], diff_base=c["diff_base"])
        FB.check_dtu_out5(f"{name} check_geometric_consistency[{sv}]", _n(out5).reshape(5, n), _n(masks).reshape(-1, n).astype(bool), ref, sv, st,
                          FB.dtu_zeroed(rs["out5"][sv], rs["masks"][sv]))


def test_dtu_named_functions_on_numpy_arrays():
    """dtu_fusion.reproject_with_depth / check_geometric_consistency under the reference's names and argument lists."""
    from effi_mvs_plus_amd import dtu_fusion
    name = "odd_n3_loose"                                  # s, e = 1, 11 and the bases are the module's constants
    c, ref = C.dtu_case(name), C.dtu_ref(name)
    assert (dtu_fusion.s, dtu_fusion.e, dtu_fusion.dist_base, dtu_fusion.diff_base) == (c["s"], c["e"], c["dist_base"], c["diff_base"])
    st = _stats("dtu_reproject")
    n = c["ref_depth"].size
    K = lambda cam: cam[1, :3, :3]      # noqa: E731
    got = dtu_fusion.reproject_with_depth(c["ref_depth"], K(c["ref_cam"]), c["ref_cam"][0], c["src_depths"][0], K(c["src_cams"][0]), c["src_cams"][0][0])
    FB.check_dtu_out5(f"{name} dtu_fusion.reproject_with_depth", np.stack(got).reshape(5, n), None, ref, 0, st)
    masks, mask, dep, xs_, ys_, xr, yr = dtu_fusion.check_geometric_consistency(c["ref_depth"].copy(), K(c["ref_cam"]), c["ref_cam"][0], c["src_depths"][1],
                                                                               K(c["src_cams"][1]), c["src_cams"][1][0], None)
    FB.check_dtu_out5(f"{name} dtu_fusion.check_geometric_consistency", np.stack([dep, xr, yr, xs_, ys_]).reshape(5, n),
                      np.stack(masks).reshape(-1, n), ref, 1, st)
    assert np.array_equal(mask, masks[-1])


def test_dtu_scan_rows_with_different_source_counts_against_the_reference():
    from effi_mvs_plus_amd import ops
    c = C.dtu_scan()
    refs = [C.dtu_scan_ref(r) for r in range(len(c["rows"]))]
    for r, ref in enumerate(refs):
        FB.assert_caps(f"dtu scan row {r}", ref, "final")
    out = ops.fusion_dtu_filter_scan(_t(c["depths"]), _t(c["cams"]), ops.fusion_pair_table(c["rows"]), _t(c["conf"]), 0.5, 0.75, c["s"], c["e"], 0.5, 0.25)
    st = _stats("dtu_scan")
    for r, ref in enumerate(refs):
        row = {k: out[k][r] for k in ("depth", "photo_mask", "geo_mask", "mask", "points")}
        FB.check_dtu_outputs(f"dtu scan row {r}", _dtu_out(row), ref, st, restated=FB.dtu_restate(*C.dtu_scan_row(c, r)))
        FB.count_decisions(ref, st, "geo", "final")


def test_record_of_the_run():
    """Prints the per-family record that DESIGN 2.7 quotes (checks, share of the interval used, pinned, undecided, left out, bitwise
    share) from the families that ran before it.  It asserts nothing of its own: the assertions are the tests above."""
    for st in RECORD.values():
        print(st.line())
