"""CPU: the fixed-threshold visibility filter's checker and host side.

  1. what the REFERENCE returned (tests/golden/g17_static_fusion.npz, recorded by tests/golden/make_golden_static_fusion.py from
     misc/fusion.py's own functions) passes the gates of tests/static_fusion_ref.py -- the same gates the kernels face in
     tests/test_gpu_static_fusion.py;
  2. the five reference names carry the reference's parameter lists: against the recorded ones, and against the imported
     misc/fusion.py where the reference tree is present;
  3. the host part of ``static_filter_scan``: which rows of a pair list remain, and their table.
"""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import refimport
import static_fusion_ref as SR
from effi_mvs_plus_amd import _lib, fusion, ops


def test_the_reference_outputs_pass_the_checker():
    g = SR.golden()
    SR.check_outputs("a", dict(xyd=g["a_reproj_xyd"], in_range=g["a_in_range"], masks=g["a_masks"], mask=g["a_mask"], depth=g["a_depth"],
                               points=g["a_points"]), "reference")
    # without its per-view masks (what the fused call returns) the averaged depth is pinned on the decided pixels alone
    SR.check_outputs("a", dict(mask=g["a_mask"], depth=g["a_depth"], points=g["a_points"]), "reference, fused view")
    E = SR.bounds()
    assert set(E) == set(SR.KINDS) | {"g", "img"} and all(0 < v < 0.1 for v in E.values())
    r = SR.case_ref("a")
    # the reference sits at a quarter of every bound, by construction
    assert np.abs(g["a_reproj_xyd"][:, :2] - r["xyd"][:, :2]).max() <= E["xy"] / 4 and np.abs(g["a_reproj_xyd"][:, 2] - r["xyd"][:, 2]).max() <= E["d"] / 4


@pytest.mark.parametrize("name", list(SR.CASES))
def test_every_case_stays_inside_the_undecided_cap_with_mixed_masks(name):
    r = SR.case_ref(name, tuple(sorted(SR.bounds().items())))
    und, full, geo = 1.0 - r["masks_decided"].mean(), r["masks"].mean(), r["mask"].mean()
    print(f"[static fusion] {name}: undecided {und:.4f}, per-view masks {full:.3f} full, mask {geo:.3f} full, in_range {r['in_range'].mean():.3f}")
    assert und <= SR.UNDECIDED_CAP and 1.0 - r["mask_decided"].mean() <= SR.UNDECIDED_CAP
    assert 0.2 <= full <= 0.9 and np.isfinite(r["xyd"]).all() and 0.0 < r["in_range"].mean() < 1.0


def test_the_checker_refuses_a_filter_without_the_clamp_or_with_the_other_normalisation():
    """The gates are not vacuous: the two obvious 'repairs' of the reference (no +-1.1 clamp; normalising by w - 1) miss them."""
    c, E = SR.case("zeros_3"), SR.bounds()
    r = SR.case_ref("zeros_3")
    h, w = c["ref_depth"].shape
    for repair in ("no_clamp", "w_minus_1"):
        xyd = []
        for s in range(c["src_depths"].shape[0]):
            S = SR.source_map(c["src_depths"][s], c["src_cams"][s], c["ref_cam"])
            gx, gy = SR.warp_coords(c["ref_depth"], c["ref_cam"], c["src_cams"][s], h, w, clamp=repair != "no_clamp",
                                    minus_one=repair == "w_minus_1")
            xyd.append(SR.grid_sample(S, gx, gy))
        e = np.abs(np.stack(xyd) - r["xyd"])
        print(f"[static fusion] repair {repair}: {int((e[:, :2].max(1) > E['xy']).sum() + (e[:, 2] > E['d']).sum())} elements outside E")
        assert e[:, :2].max() > E["xy"] or e[:, 2].max() > E["d"], repair


def test_the_new_names_have_the_reference_parameter_lists():
    g = SR.golden()
    for name in SR.NAMES:
        assert str(inspect.signature(getattr(fusion, name))) == str(g[f"sig_{name}"][0]), name
    if os.path.isfile(os.path.join(refimport.REF_ROOT, "misc", "fusion.py")):
        sys.dont_write_bytecode = True
        import importlib.util
        spec = importlib.util.spec_from_file_location("reference_misc_fusion", os.path.join(refimport.REF_ROOT, "misc", "fusion.py"))
        ref = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ref)
        for name in SR.NAMES:
            assert inspect.signature(getattr(fusion, name)).parameters.keys() == inspect.signature(getattr(ref, name)).parameters.keys(), name
            assert str(inspect.signature(getattr(fusion, name))) == str(inspect.signature(getattr(ref, name))), name


def test_static_entries_are_declared_and_bound():
    names = {"effi_fusion_static_filter_f32", "effi_fusion_static_filter_scan_f32", "effi_fusion_project_img_f32",
             "effi_fusion_static_vis_filter_f32", "effi_fusion_prob_filter_f32"}
    assert names <= set(_lib.SIGNATURES) and names <= set(_lib.declared_symbols())
    for fn in (ops.fusion_static_filter, ops.fusion_static_filter_scan, ops.fusion_project_img, ops.fusion_static_vis_filter,
               ops.fusion_static_ave, ops.fusion_prob_filter, fusion.static_filter, fusion.static_filter_scan):
        assert callable(fn)
    assert list(inspect.signature(fusion.static_filter).parameters) == ["ref_depth", "src_depths", "ref_cam", "src_cams", "ref_conf",
                                                                        "prob_threshold", "img_dist_thresh", "depth_thresh", "vthresh"]
    assert list(inspect.signature(fusion.static_filter_scan).parameters) == ["depths", "confidences", "cams", "images", "pair_data",
                                                                             "prob_threshold", "img_dist_thresh", "depth_thresh", "vthresh", "chunk"]


def test_scan_rows_drop_the_reference_views_without_a_source():
    pairs = SR.SCAN["pairs"]
    rows = fusion.static_scan_rows(pairs)
    assert [ref for ref, _ in rows] == [0, 1, 3, 4, 5] and all(len(s) >= 1 for _, s in rows)
    assert sorted(len(s) for _, s in rows) == [1, 2, 2, 3, 4]
    assert fusion.pair_table(rows).tolist() == [[0, 1, -1, -1, -1], [1, 0, 2, -1, -1], [3, 5, 4, 2, -1], [4, 0, 1, 2, 3], [5, 4, 3, -1, -1]]
    assert fusion.static_scan_rows([(7, []), (8, ())]) == []
    with pytest.raises(ValueError):                                        # the table itself still refuses a row without sources
        fusion.pair_table(pairs)


def test_static_wrappers_refuse_cpu_tensors():
    d, cams = torch.zeros(3, 8, 8), torch.zeros(3, 2, 4, 4)
    with pytest.raises(_lib.EffiLibraryError):
        ops.fusion_static_filter_scan(d, cams, fusion.pair_table([(0, [1, 2])]))
    with pytest.raises(_lib.EffiLibraryError):
        ops.fusion_static_filter(d[0], d[1:], cams[0], cams[1:])
    with pytest.raises(_lib.EffiLibraryError):
        fusion.get_reproj(d[:1, None], d[None, 1:, None], cams[:1], cams[None, 1:])
