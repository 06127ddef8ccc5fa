"""CPU side of the Gipuma fusion tests: the float64 interval reference (tests/gipuma_ref.py) meets its own
conditions on every case of tests/gipuma_cases.py, the fp32 op-for-op restatement of the kernel lies inside every interval, planted
structural errors are caught, the file formats equal the bytes the reference wrote (tests/golden/g18_gipuma_io.npz), and the host-side
refusals.  Nothing here needs a GPU or the built library.
"""
import functools
import inspect
import os

import numpy as np
import pytest

import fusion_bound as FB
import gipuma_cases as GC
import gipuma_ref as GR
from effi_mvs_plus_amd import _lib, ops
from effi_mvs_plus_amd.datasets.data_io import read_pfm, save_pfm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g18_gipuma_io.npz")


@functools.lru_cache(maxsize=None)
def ref_of(name):
    return GR.case_reference(GC.case(name))


@functools.lru_cache(maxsize=None)
def plain_of(name):
    return GR.case_restate(GC.case(name))


def _shares(views):
    return [float(v["mask"].mean()) for v in views]


@pytest.mark.parametrize("name", GC.CASES)
def test_reference_meets_its_caps_and_is_neither_empty_nor_full(name):
    c = GC.case(name)
    views, flags = ref_of(name)
    worst = GR.assert_caps(name, views)
    fused = sum(int(v["mask"].sum()) for v in views)
    total = sum(v["mask"].size for v in views)
    print(f"[gipuma-host] {name:18s} fused per view " + " / ".join(f"{s:.2f}" for s in _shares(views)) +
          f"  undecided-or-tainted (worst view) {worst:.4f}  consumed per view " + " / ".join(f"{(f == 1).mean():.2f}" for f in flags[:6]))
    assert len(views) == len(GC.rows_of(c)) and flags.shape == (c["depths"].shape[0], views[0]["mask"].size)
    if name in GC.EMPTY:
        assert fused == 0 and not flags.any()
    else:
        assert 0 < fused < total, (name, fused, total)
    if c["exact"] is not None:                                       # exact rigs: nothing undecided, every flag known
        assert worst == 0.0 and not (flags == GR.UNKNOWN).any()
        assert all(v["mask_decided"].all() and v["count_decided"].all() for v in views)
    if c["exact"] == "all":                                          # ... and every checked value pinned
        assert all((p.e[v["clean"]] == 0).all() for v in views for p in v["points"])


@pytest.mark.parametrize("name", [n for n in GC.CASES if GC.case(n)["exact"] is not None])
def test_exact_rig_projects_onto_integers(name):
    """The claim the exact rigs rest on: every projection of a live pixel is an integer, and the disparities are dyadic enough that the
    fp32 chain equals the float64 one -- checked by running the chain in both and comparing every value."""
    c = GC.case(name)
    D = c["depths"]
    n, h, w = D.shape
    ys, xs = FB.pixel_grid(h, w)
    for ref, srcs in GC.rows_of(c):
        d = D[ref].reshape(-1)
        live = d > 0
        m32 = GR._lift(FB.F32, GR.prepare_slot(c["cams"][ref], c["cams"][ref]))
        X32 = GR.backproject(m32, xs.astype(np.float32), ys.astype(np.float32), d)
        X64 = GR.backproject({k: np.asarray(v, np.float64) for k, v in m32.items()}, xs.astype(np.float64), ys.astype(np.float64),
                             d.astype(np.float64))
        for a, b in zip(X32, X64):
            assert (a[live].astype(np.float64) == b[live]).all()
        for s in srcs:
            ms = GR._lift(FB.F32, GR.prepare_slot(c["cams"][s], c["cams"][ref]))
            with np.errstate(all="ignore"):
                z, uh, vh = GR.project(FB.F32, ms, X32)
            assert ((uh[live] - np.floor(uh[live])) == 0.5).all() and ((vh[live] - np.floor(vh[live])) == 0.5).all()
            fb = np.float64(ms["fb"])
            assert fb == 256.0 * abs(ref - s)
            for depth in np.unique(D[D > 0]):                         # every disparity the rig can form is an fp32 number
                assert np.float64(np.float32(fb / depth)) == fb / np.float64(depth)


def test_order_dependence_and_count_histogram():
    fwd, _ = ref_of("exact_37x53")
    rev, _ = ref_of("exact_reversed")
    assert _shares(fwd) != _shares(rev[::-1])
    # the first view fused claims most; later views find their pixels consumed
    assert _shares(fwd)[0] > _shares(fwd)[-1] and _shares(rev)[0] > _shares(rev)[-1]
    hist = np.bincount(np.concatenate([v["count"] for v in fwd]), minlength=6)
    assert (hist[1:4] > 0).all(), hist
    # the general scene consumes a large share of the later views' pixels
    _, flags = ref_of("general_37x53")
    assert ((flags == 1).mean(1)[1:] > 0.3).all()


@pytest.mark.parametrize("name", GC.CASES)
def test_restatement_lies_inside_every_interval(name):
    views, used = plain_of(name)
    rviews, flags = ref_of(name)
    assert GR.caught(views, used, rviews, flags) == 0
    st = FB.Stats(name)
    GR.check_scan(name, views, used, rviews, flags, st)
    assert st.checks > 0


def test_depth_range_edges_are_inside():
    c = GC.case("depth_edges")
    views, _ = plain_of("depth_edges")
    d = c["depths"]
    fused = np.stack([v["mask"] for v in views]).reshape(d.shape)
    at_edge = (d == GC.DEPTH_MIN) | (d == GC.DEPTH_MAX)
    outside = (d < GC.DEPTH_MIN) | (d > GC.DEPTH_MAX) | np.isnan(d)
    assert outside.any() and not fused[outside].any()
    assert fused[d == GC.DEPTH_MIN].any() and fused[d == GC.DEPTH_MAX].any() and at_edge.any()


def test_every_mutant_is_caught():
    """Each planted error breaks a decided pixel, a known flag, an interval or (colour order) the bitwise colour on at least one case."""
    names = ("exact_37x53", "exact_edge", "general_37x53", "general_lownoise", "pairs")
    found = {}
    for mutant in GR.MUTANTS:
        for name in names:
            views, used = GR.case_restate(GC.case(name), mutant)
            n = GR.caught(views, used, *ref_of(name), plain=plain_of(name)[0])
            if n:
                found[mutant] = (name, n)
                break
    print("[gipuma-host] mutants caught: " + "  ".join(f"{m}: {v[0]} ({v[1]})" for m, v in found.items()))
    assert set(found) == set(GR.MUTANTS), sorted(set(GR.MUTANTS) - set(found))


# ---- host-side logic ----
def test_scan_rows_and_refusals():
    from effi_mvs_plus_amd import gipuma
    assert gipuma.scan_rows(3) == [(0, [1, 2]), (1, [0, 2]), (2, [0, 1])]
    assert gipuma.scan_rows(6, GC.PAIRS) == [(r, list(s)) for r, s in GC.PAIRS]
    assert len(gipuma.scan_rows(65)[0][1]) == 64
    for n, bad in ((4, [(1, [0, 1])]), (4, [(0, [4])]), (4, [(0, [-1])]), (4, [(4, [0])]), (4, [(-1, [0])]), (4, [(0, [])]), (4, []),
                   (70, [(0, list(range(1, 66)))]), (66, None), (1, None)):
        with pytest.raises(ValueError):
            gipuma.scan_rows(n, bad)
    assert ops.GIPUMA_MAX_SOURCES == 64


def test_entries_are_bound_and_declared():
    declared = _lib.declared_symbols()
    for name in ("effi_fusion_gipuma_view_f32", "effi_fusion_gipuma_prob_f32"):
        assert name in _lib.SIGNATURES and name in declared
    header = open(_lib.HEADER_PATH).read()
    assert "misc/gipuma.py:160-236" in header and "UNPINNED" in header


def test_unpinned_boundary_is_stated():
    from effi_mvs_plus_amd import gipuma
    assert "PARITY WITH THE EXTERNAL BINARY UNPINNED" in gipuma.__doc__
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "gipuma" in text.lower() and "UNPINNED" in text[text.lower().index("gipuma"):]


# ---- file formats, byte for byte what the reference wrote ----
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_dmb_files_match_the_reference(golden, tmp_path):
    from effi_mvs_plus_amd import gipuma
    gipuma.write_gipuma_dmb(tmp_path / "one.dmb", golden["depth"])
    gipuma.write_gipuma_dmb(tmp_path / "three.dmb", golden["img3"])
    assert _bytes(tmp_path / "one.dmb") == golden["dmb1"].tobytes()
    assert _bytes(tmp_path / "three.dmb") == golden["dmb3"].tobytes()          # planar [c][h][w]: the reference's transpose
    back = gipuma.read_gipuma_dmb(tmp_path / "one.dmb")
    assert back.dtype == np.float32 and np.array_equal(back, golden["depth"]) and np.array_equal(back, golden["dmb1_read"])
    h, w = golden["depth"].shape
    planar = np.frombuffer(golden["dmb3"].tobytes()[16:], np.float32).reshape(3, h, w)
    assert np.array_equal(planar, golden["img3"].transpose(2, 0, 1))
    gipuma.fake_gipuma_normal(tmp_path / "one.dmb", tmp_path / "normals.dmb")
    assert _bytes(tmp_path / "normals.dmb") == golden["normals"].tobytes()
    n = np.frombuffer(golden["normals"].tobytes()[16:], np.float32).reshape(3, h, w)
    assert set(np.unique(n).tolist()) == {0.0, float(np.float32(1 / 1.732050808))} and ((n[0] > 0) == (golden["depth"] > 0)).all()


def test_projection_file_matches_the_reference(golden, tmp_path):
    from effi_mvs_plus_amd import gipuma
    (tmp_path / "00000003_cam.txt").write_bytes(golden["cam_txt"].tobytes())
    gipuma.mvsnet_to_gipuma_cam(tmp_path / "00000003_cam.txt", tmp_path / "00000003.jpg.P")
    assert _bytes(tmp_path / "00000003.jpg.P") == golden["cam_P"].tobytes()
    # and back: P = K [R|t] by RQ, the sign convention of decompose_projection
    K0, E0 = gipuma.read_camera_parameters(tmp_path / "00000003_cam.txt")
    K, R, t = gipuma.decompose_projection(np.loadtxt(tmp_path / "00000003.jpg.P"))
    assert (np.diag(K) > 0).all() and K[2, 2] == 1.0 and abs(np.linalg.det(R) - 1.0) < 1e-9
    assert np.abs(K - K0).max() < 1e-6 * 2892.33 and np.abs(R - E0[:3, :3]).max() < 1e-6 and np.abs(t - E0[:3, 3]).max() < 1e-6 * 191.02
    K2, R2, t2 = gipuma.decompose_projection(-np.loadtxt(tmp_path / "00000003.jpg.P"))
    assert np.allclose(K2, K) and np.allclose(R2, R) and np.allclose(t2, t)


def test_probability_filter_matches_the_reference(golden, tmp_path):
    from effi_mvs_plus_amd import gipuma
    for sub in ("images", "depth_est", "confidence", "cams"):
        (tmp_path / sub).mkdir()
    (tmp_path / "images" / "00000003.jpg").write_bytes(b"")
    (tmp_path / "images" / ".hidden").write_bytes(b"")
    save_pfm(tmp_path / "depth_est" / "00000003.pfm", golden["depth"])
    save_pfm(tmp_path / "confidence" / "00000003.pfm", golden["conf"])
    assert _bytes(tmp_path / "depth_est" / "00000003.pfm") == golden["depth_pfm"].tobytes()
    gipuma.probability_filter(str(tmp_path), float(golden["prob_threshold"]))
    assert _bytes(tmp_path / "depth_est" / "00000003_prob_filtered.pfm") == golden["prob_filtered_pfm"].tobytes()
    kept = read_pfm(tmp_path / "depth_est" / "00000003_prob_filtered.pfm")[0]
    assert np.array_equal(kept, GR.filtered_depths(golden["depth"], golden["conf"], float(golden["prob_threshold"])))
    # mvsnet_to_gipuma: the folder fusibile would have read
    (tmp_path / "cams" / "00000003_cam.txt").write_bytes(golden["cam_txt"].tobytes())
    gipuma.mvsnet_to_gipuma(str(tmp_path), str(tmp_path / "points_mvsnet"))
    pf = tmp_path / "points_mvsnet"
    assert _bytes(pf / "2333__00000003" / "disp.dmb") == golden["disp_dmb"].tobytes()
    assert _bytes(pf / "cams" / "00000003.jpg.P") == golden["cam_P"].tobytes()
    assert (pf / "images" / "00000003.jpg").exists() and (pf / "2333__00000003" / "normals.dmb").exists()


def test_signatures_are_the_references(golden):
    from effi_mvs_plus_amd import gipuma
    for fn in ("read_gipuma_dmb", "write_gipuma_dmb", "mvsnet_to_gipuma_dmb", "mvsnet_to_gipuma_cam", "fake_gipuma_normal", "mvsnet_to_gipuma",
               "probability_filter", "read_camera_parameters"):
        assert str(inspect.signature(getattr(gipuma, fn))) == str(golden[f"sig_{fn}"][0]), fn
    want = list(inspect.signature(gipuma.gipuma_filter).parameters)
    assert want[:6] == ["testlist", "outdir", "prob_threshold", "disp_threshold", "num_consistent", "fusibile_exe_path"]
    assert str(golden["sig_gipuma_filter"][0]) == "(testlist, outdir, prob_threshold, disp_threshold, num_consistent, fusibile_exe_path)"
