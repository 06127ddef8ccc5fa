"""The host proof of the fusion bounds, CPU only: for every case tests/test_gpu_fusion_bounds.py runs,
(a) the fp32 restatements of csrc/fusion.hip lie inside every interval of tests/fusion_bound.py and agree with every decided pixel,
(b) every structural mutant leaves an interval or flips a decided pixel in every case that can express it -- with, beside it, whether
    the share-of-agreement checks of tests/test_fusion.py (agree >= 0.999 / 0.998, frac_close >= 0.999) would accept it,
(c) the stated conditions hold: the undecided set is named by the reference alone and capped.

The oracle (oracle/effi_oracle.py) is not used as a second witness for the T&T branch: its point transforms are batched GEMMs whose
summation order is the BLAS's own, and its inverses are single precision -- the intervals here are counted against ONE operation
order, the kernel's.  The DTU oracle's single-precision inverse is the `inverse_fp32` mutant, whose size is printed below."""
import numpy as np
import pytest

import fusion_bound as FB
import fusion_cases as C

TT_MASKS, TT_CONT = [("geo", "geo"), ("prob", "prob"), ("mask", "mask")], [("depth", "depth"), ("points", "points"), ("xyd", "xyd")]
DTU_MASKS, DTU_CONT = [("geo", "geo"), ("photo", "photo"), ("final", "final")], [("depth", "depth"), ("points", "points")]

# the flat-bound counts the caps were set against (shares of comparisons / of pixels that a flat 2e-3 px / mm bound -- 3e-4 mm for
# DTU -- leaves undecided, measured with the float64 oracle): the caps keep at least 3x headroom over each
LISTED_COMPARISONS = [24 / 245760, 1 / 504000, 96 / 537600, 11 / 11100, 0.0012]
LISTED_PIXELS = [0.0, 0.0, 0.0, 5 / 1850, 23 / 7575]


def _bites(st, geo_means):
    print(st.line() + f" mean_geo={np.mean(geo_means):.3f}")
    assert st.near_true >= 50 and st.near_false >= 50, "too few decided comparisons within 32 bounds of a threshold: the bounds do not bite"
    assert 0.05 < np.mean(geo_means) < 0.999
    assert st.tight * 2 >= st.nonpinned, "fewer than half of the non-pinned elements have half <= 2^-10 |mid|"


def test_caps_keep_their_headroom_over_the_flat_bound_counts():
    assert all(3.0 * s <= FB.CAP_COMPARISONS for s in LISTED_COMPARISONS) and all(3.0 * s <= FB.CAP_PIXELS for s in LISTED_PIXELS)


def test_running_bound_contains_fp32_arithmetic_on_random_operands():
    """The bounded arithmetic itself: fp32 sums, products, quotients and square roots of operands that already carry an error stay
    within the carried bound of the float64 value, over magnitudes from 1e-6 to 1e6, cancellation included."""
    rng = np.random.default_rng(7)
    n = 20000
    mag = lambda: (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n))      # noqa: E731
    x64, y64, z64 = mag(), mag(), mag()
    x, y, z = (v.astype(np.float32) for v in (x64, y64, z64))
    bx, by, bz = (FB.B(v64, np.abs(v64) * FB.U32) for v64 in (x64, y64, z64))   # the float64 value and the rounding that made the fp32 one
    with np.errstate(all="ignore"):
        pairs = [((x * y + z) / (y - x), (bx * by + bz) / (by - bx)), (np.sqrt(x * x + y * y) - np.abs(x), (bx * bx + by * by).sqrt() - bx.abs()),
                 (x / y * z + np.float32(1e-9), bx / by * bz + FB.BND.lift(1e-9))]
    for got, b in pairs:
        g = got.astype(np.float64)
        ok = (g >= b.lo) & (g <= b.hi) | ~np.isfinite(b.e)
        assert ok.all(), f"{int((~ok).sum())} fp32 results outside the running bound"
        assert np.isfinite(b.e).mean() > 0.99 and np.median(b.e / np.abs(b.m).clip(1e-300)) < 1e-5


def test_inverses_restated_and_away_from_rounding_boundaries():
    """fus_invert restated is an inverse, and no inverse entry (nor an entry of the DTU products) of any case lies within 2^-40
    relative of an fp32 rounding boundary: a condition on the inputs, under which the rounded matrices are the kernel's bit for bit."""
    worst = np.inf
    for name in C.TT_CASES:
        c = C.tt_case(name)
        for cam in [c["ref_cam"], *c["src_cams"]]:
            m = FB.prepare_view(cam)
            worst = min(worst, float(FB.near_boundary(m["raw64"]).min()))
            E = np.asarray(cam[0], np.float64)
            assert np.abs(FB.gauss_jordan(E) @ E - np.eye(4)).max() < 1e-9
    for cams in [C.tt_scan()["cams"], C.dtu_scan()["cams"]]:
        for cam in cams:
            worst = min(worst, float(FB.near_boundary(FB.prepare_view(cam)["raw64"]).min()))
    for name in C.DTU_CASES:
        c = C.dtu_case(name)
        for cam in c["src_cams"]:
            worst = min(worst, float(FB.near_boundary(FB.dtu_prepare_view(c["ref_cam"], cam)["raw64"]).min()))
    sc = C.dtu_scan()
    for ref, srcs in sc["rows"]:
        for s in srcs:
            worst = min(worst, float(FB.near_boundary(FB.dtu_prepare_view(sc["cams"][ref], sc["cams"][s])["raw64"]).min()))
    print(f"[fusion-bound] closest inverse entry to an fp32 rounding boundary: {worst:.3e} relative (needs > {FB.NEAR:.3e})")
    assert worst > FB.NEAR


def test_tt_restatement_inside_every_interval_and_conditions_hold():
    st, geo_means = FB.Stats("tt_filter"), []
    for name in C.TT_CASES:
        ref, rs = C.tt_ref(name), C.tt_restated(name)
        FB.check_tt_outputs(name, rs, ref, st, restated=rs)
        a, b = FB.count_decisions(ref, st)
        geo_means.append(ref["geo"].value.mean())
        print(f"[fusion-bound] {name:20s} undecided_cmp={a:.5f} undecided_pix={b:.5f} left_out_views={int(ref['left'].sum())} "
              f"mean_geo={geo_means[-1]:.3f}")
    _bites(st, geo_means)
    # the half-widths behind the derivation table of DESIGN 2.7, on fixture_a (px and mm; median / largest finite over pixels and views)
    ref, ch = C.tt_ref("fixture_a"), C.tt_ref("fixture_a")["chain"]
    med = lambda bs: (float(np.median(np.concatenate([b.e for b in bs]))), float(np.max(np.concatenate([b.e[np.isfinite(b.e)] for b in bs]))))      # noqa: E731
    for label, bs in (("world point", list(ch["world"][:3])), ("source pixel", [xy[i] for xy in ch["src_xy"] for i in (0, 1)]), ("sample", ch["sample"]),
                      ("reproj x y", ch["x"] + ch["y"]), ("reproj depth", ch["d"]), ("cdiff", ch["cdiff"]), ("ddiff", ch["ddiff"]),
                      ("averaged depth", [ref["depth"]]), ("points", ref["points"])):
        print(f"[fusion-half] {label:16s} median {med(bs)[0]:.3e} largest {med(bs)[1]:.3e}")


def test_tt_left_out_rule_is_exercised():
    """The source camera moved into the scene and the reference depths of 0 (relative difference): the left-out comparisons are
    named by the reference, counted, and stay under the cap with the undecided ones."""
    ref = C.tt_ref("inside_v5")
    n_left = int(ref["left"].sum())
    print(f"[fusion-bound] inside_v5: left-out (pixel, view) pairs {n_left}, undecided or left-out comparisons {int(ref['Un'].sum())} of {ref['Un'].size}")
    assert n_left >= 3 * 5                               # the three planted pixels, every view
    FB.assert_caps("inside_v5", ref)


def test_tt_scan_rows_against_the_reference_and_the_shifted_table():
    c = C.tt_scan()
    st = FB.Stats("tt_scan")
    caught = accepted = 0
    for r in range(len(c["rows"])):
        ref = C.tt_scan_ref(r)
        rs = FB.tt_restate(*C.tt_scan_row(c, r))
        FB.check_tt_outputs(f"scan row {r}", rs, ref, st, restated=rs)
        FB.count_decisions(ref, st)
        mu = FB.tt_restate(*C.tt_scan_row(c, r, shift=1))
        n = FB.mutant_caught(mu, ref, TT_MASKS, [("depth", "depth"), ("points", "points")])         # what a scan launch returns
        assert n > 0, f"row {r}: the shifted table is not caught"
        caught += 1
        accepted += _present_tt(mu, rs)
    print(st.line())
    print(f"[fusion-mutant] T&T table_shifted          expressed by {len(c['rows']):2d} rows, caught in {caught:2d}, "
          f"accepted by agree >= 0.999 / frac_close >= 0.999 in {accepted:2d}")


@pytest.mark.parametrize("relative", [False, True])
def test_vis_filter_planted_ties_are_pinned(relative):
    """Exact ties: `<` is false at equality and true one ulp below.  The planted values make every operation of the kernel exact, so
    float64 arithmetic on them is the exact answer and the fp32 restatement must equal it in every element."""
    t = C.vis_ties(relative)
    got = FB.vis_filter_f32(t["ref_depth"], t["xyd"], t["dist_base"], t["rel_base"], t["thres"], relative)
    want = C.vis_ties_expected(t)
    assert np.array_equal(got, want)
    assert want.any() and not want.all()
    mu = FB.vis_filter_f32(t["ref_depth"], t["xyd"], t["dist_base"], t["rel_base"], t["thres"], relative, mutant="le_for_lt")
    flipped = int((mu != want).sum())
    print(f"[fusion-bound] vis ties relative={relative}: {want.size} pinned elements, `<=` for `<` flips {flipped} "
          f"(share {flipped / want.size:.4f}; an agreement of 0.9995 accepts {flipped / want.size <= 0.0005})")
    assert flipped > 0
    if relative:
        ig = FB.vis_filter_f32(t["ref_depth"], t["xyd"], t["dist_base"], t["rel_base"], t["thres"], relative, mutant="relative_ignored")
        assert (ig != want).any()


def test_points_modes_restated_inside_their_intervals():
    """fusion_points_kernel's four modes on the reference's own intermediates of fixture_b."""
    st = FB.Stats("points_modes")
    for mode, pts, cam, depth in C.points_inputs("fixture_b"):
        bound = FB.points_chain(FB.BND, mode, pts, cam, depth)
        with np.errstate(all="ignore"):
            rs = FB.points_chain(FB.F32, mode, pts, cam, depth)
        for k, (b, r) in enumerate(zip(bound, rs)):
            FB.check_elements(f"points mode {mode}[{k}]", np.broadcast_to(r, (pts.shape[0],)), FB.B(np.broadcast_to(b.m, (pts.shape[0],)), np.broadcast_to(b.e, (pts.shape[0],))), st, restated=np.broadcast_to(r, (pts.shape[0],)))
    print(st.line())
    assert st.tight * 2 >= st.nonpinned


def test_dtu_restatement_inside_every_interval_and_conditions_hold():
    st, st5, geo_means, log_two = FB.Stats("dtu_filter"), FB.Stats("dtu_reproject"), [], 0
    for name in C.DTU_CASES:
        ref, rs = C.dtu_ref(name), C.dtu_restated(name)
        FB.check_dtu_outputs(name, rs, ref, st, restated=rs)
        a, b = FB.count_decisions(ref, st, "geo", "final")
        geo_means.append(ref["geo"].value.mean())
        log_two += ref["log_two"]
        for sv in range(len(ref["out5"])):
            FB.check_dtu_out5(f"{name} reproject {sv}", rs["out5"][sv], None, ref, sv, st5, rs["out5"][sv])
            FB.check_dtu_out5(f"{name} consistency {sv}", FB.dtu_zeroed(rs["out5"][sv], rs["masks"][sv]), rs["masks"][sv], ref, sv, st5,
                              FB.dtu_zeroed(rs["out5"][sv], rs["masks"][sv]))
        print(f"[fusion-bound] {name:20s} undecided_cmp={a:.5f} undecided_pix={b:.5f} mean_geo={geo_means[-1]:.3f}")
    sc = C.dtu_scan()
    for r in range(len(sc["rows"])):
        ref, rs = C.dtu_scan_ref(r), FB.dtu_restate(*C.dtu_scan_row(sc, r))
        FB.check_dtu_outputs(f"dtu scan row {r}", rs, ref, st, restated=rs)
    print(f"[fusion-bound] thresholds log10(max(i, 1.05)) * diff_base with two admissible fp32 neighbours: {log_two} (0 expected)")
    print(st5.line())
    _bites(st, geo_means)
    # the DTU chain is double rounded to fp32: almost every element is pinned or one ulp wide, so the 2^-10 yardstick is met trivially
    assert st5.tight * 2 >= st5.nonpinned


def _present_tt(out, rs):
    agree = min(float((out[k] == rs[k]).mean()) for k in ("geo", "prob", "mask"))
    with np.errstate(all="ignore"):
        close = float((np.abs(out["depth"] - rs["depth"]) <= 2e-3).mean())
    return agree >= 0.999 and close >= 0.999


def _present_dtu(out, rs):
    agree = min(float((out[k] == rs[k]).mean()) for k in ("geo", "photo", "final"))
    same = out["geo"] == rs["geo"]
    with np.errstate(all="ignore"):
        dd = np.abs(out["depth"].astype(np.float64) - rs["depth"])
    return agree >= 0.998 and dd[same].max() <= 2e-3 and np.median(dd) <= 1e-4


def _differs(out, rs, keys):
    return any(not np.array_equal(np.asarray(out[k]), np.asarray(rs[k]), equal_nan=True) for k in keys)


def test_every_tt_mutant_is_caught_where_a_case_can_express_it():
    """A case can express a mutant when the mutated restatement differs from the plain one in any output."""
    rows = []
    for mu, kind in FB.MUTANTS.items():
        if kind != "tt":
            continue
        expressed = caught = accepted = 0
        for name in C.TT_CASES:
            ref, rs = C.tt_ref(name), C.tt_restated(name)
            out = FB.tt_restate(*C.tt_args(C.tt_case(name)), mutant=mu)
            if not _differs(out, rs, ("geo", "prob", "mask", "depth", "points", "xyd")):
                continue
            expressed += 1
            n = FB.mutant_caught(out, ref, TT_MASKS, TT_CONT)
            caught += n > 0
            accepted += _present_tt(out, rs)
            assert n > 0, f"mutant {mu} is expressed by case {name} and not caught"
        rows.append((mu, expressed, caught, accepted))
        assert expressed >= 2, f"mutant {mu}: fewer than two cases can express it"
    for mu, e, c_, a in rows:
        print(f"[fusion-mutant] T&T {mu:22s} expressed by {e:2d} cases, caught in {c_:2d}, accepted by agree >= 0.999 / frac_close >= 0.999 in {a:2d}")


def test_every_dtu_mutant_is_caught_where_a_case_can_express_it():
    rows = []
    for mu, kind in FB.MUTANTS.items():
        if not kind.startswith("dtu"):
            continue
        expressed = caught = accepted = 0
        moved, biggest = 0, 0.0
        for name in C.DTU_CASES:
            ref, rs = C.dtu_ref(name), C.dtu_restated(name)
            if kind == "dtu_reproject":
                for sv in range(len(ref["out5"])):
                    z = FB.dtu_zeroed(rs["out5"][sv], rs["masks"][sv], mutant=mu)
                    if np.array_equal(z, FB.dtu_zeroed(rs["out5"][sv], rs["masks"][sv])):
                        continue
                    expressed += 1
                    with pytest.raises(AssertionError):
                        FB.check_dtu_out5(f"{name} {mu}", z, rs["masks"][sv], ref, sv, FB.Stats("mutant"))
                    caught += 1
                    # tests/test_fusion.py asserts (gdep[~gmask] == 0).all() on the library's own mask: the present check rejects it too
                continue
            out = FB.dtu_restate(*C.dtu_args(C.dtu_case(name)), mutant=mu)
            if not _differs(out, rs, ("geo", "photo", "final", "depth", "points", "out5")):
                continue
            expressed += 1
            n = FB.mutant_caught(out, ref, DTU_MASKS, DTU_CONT)
            n5 = sum(FB.mutant_caught({"o": out["out5"][sv]}, {"o": ref["out5"][sv]}, [], [("o", "o")]) for sv in range(len(ref["out5"])))
            caught += (n + n5) > 0
            accepted += bool(_present_dtu(out, rs))
            if mu == "inverse_fp32":
                d = np.abs(out["out5"].astype(np.float64) - rs["out5"])
                moved, biggest = moved + int((d > 0).sum()), max(biggest, float(np.nanmax(d)))
            assert n + n5 > 0, f"mutant {mu} is expressed by case {name} and not caught"
        rows.append((mu, expressed, caught, accepted))
        assert expressed >= 1, f"mutant {mu}: no case can express it"
        if mu == "inverse_fp32":
            print(f"[fusion-mutant] inverse_fp32 moves {moved} reprojected elements, the largest by {biggest:.3e} (px / mm): the gap the "
                  "agreement share of 0.998 was covering")
    for mu, e, c_, a in rows:
        print(f"[fusion-mutant] DTU {mu:22s} expressed by {e:2d} cases, caught in {c_:2d}, accepted by agree >= 0.998 / 2e-3 mm in {a:2d}")
