"""CPU proof that the GetCost read-out rig (tests/getcost_cases.py, tests/getcost_readout.py) would notice: the fp32 restatement
of ``effi_getcost_pixel`` (tests/getcost_pixel_ref.py) stands in for the kernel.  Unmutated it lies inside every float64 interval of
every case, with nothing left out, and the selection-weight read-out returns its costs bit for bit; with ONE defect switched on it
leaves at least one interval on the case named for that defect.  No GPU, no reference tree."""
import pytest
import torch

import getcost_cases as G
import getcost_pixel_ref as R
import getcost_readout as RO
import interval_ref as IR


def ref_cost(c, layout="planar", mutant=None, views=None):
    """The restatement on a case of getcost_cases -> cost [2 nq, h, w]."""
    h, w, nq = c["h"], c["w"], c["nq"]
    cur_t, reg_t = views if views is not None else G.layout(c["cur"], c["reg"], layout)
    cf, cstr, Dc = G.flat_and_strides(cur_t, h, w)
    rf, rstr, Dr = G.flat_and_strides(reg_t, h, w)
    rng = [v.reshape(-1) if v.numel() > 1 else v.reshape(()) for v in (c["dmin"], c["dmax"])]
    out = R.getcost_pixel(c["x"].reshape(-1), c["input_is_depth"], c["disp_range"], c["itv"][0], cf, cstr, Dc, rf, rstr, Dr,
                          rng[0], rng[1], nq, mutant)
    return out.view(2 * nq, h, w)


def check(name, cost, c):
    nq = c["nq"]
    return [IR.check_inside(f"{name} {half}", part, **iv.args(), max_left_out=0.0)
            for half, part, iv in (("cur", cost[:nq], c["iv"][0]), ("reg", cost[nq:], c["iv"][1]))]


def violations(cost, c):
    """Elements that ``check_inside`` would refuse (outside the interval, not exactly 0 where they must be, not finite) -> bool mask."""
    nq = c["nq"]
    bad = []
    for part, iv in ((cost[:nq], c["iv"][0]), (cost[nq:], c["iv"][1])):
        g = part.double()
        assert not iv.left_out.any()
        bad.append(~torch.isfinite(g) | ~((g >= iv.lo - iv.tol) & (g <= iv.hi + iv.tol)) | (iv.must_be_zero & (g != 0)))
    return torch.cat(bad)


def assert_readout_exact(name, cost):
    """The selection matrices of getcost_readout.py, applied in fp32 as the kernel applies them, give the costs back bit for bit."""
    n2 = cost.shape[0]
    flat = cost.reshape(n2, -1)
    w, b = RO.selection_plain(n2 // 2)
    assert torch.equal(RO.recover_plain(name, RO.conv1x1_fp32(flat, w, b, relu=False), n2 // 2), flat)
    if n2 == 6:
        for cout in RO.RELU_COUTS:
            w, b = RO.selection_relu(3, cout)
            assert torch.equal(RO.recover_relu(f"{name} cout={cout}", RO.conv1x1_fp32(flat, w, b, relu=True), 3), flat)


@pytest.mark.parametrize("input_is_depth", [False, True])
@pytest.mark.parametrize("Dcur,Dreg,nq,h,w,per_pixel", G.INSIDE_CASES)
def test_restatement_inside_every_interval_in_every_layout(Dcur, Dreg, nq, h, w, per_pixel, input_is_depth):
    c = G.inside_case(Dcur, Dreg, nq, h, w, per_pixel, input_is_depth)
    G.shares(c["cur"], c["qd"], c["dmin"], c["dmax"])
    first = None
    for lay in G.LAYOUTS:
        cost = ref_cost(c, lay)
        check(f"restatement D={Dcur}/{Dreg} nq={nq} {h}x{w} depth={int(input_is_depth)} {lay}", cost, c)
        first = cost if first is None else first
        assert torch.equal(cost, first), f"{lay}: the layout changes a bit"
    assert_readout_exact("read-out", first)


@pytest.mark.parametrize("input_is_depth", [False, True])
@pytest.mark.parametrize("nq", [2, 3, 4])
@pytest.mark.parametrize("D", [2, 8, 48])
def test_restatement_inside_on_every_tap_class(D, nq, input_is_depth):
    c = G.rig_case(D, nq, input_is_depth)
    cls = G.assert_every_class(c, D)
    print(f"[taps] D={D} nq={nq} depth={int(input_is_depth)} classes per query {cls}")
    for lay in G.LAYOUTS:
        cost = ref_cost(c, lay)
        s = check(f"restatement tap classes D={D} nq={nq} depth={int(input_is_depth)} {lay}", cost, c)
        assert s[0]["must_be_zero"] > 0
    assert_readout_exact("read-out, tap classes", cost)


@pytest.mark.parametrize("nq", [3, 4])
@pytest.mark.parametrize("D", [2, 8, 48])
def test_restatement_ignores_nan_taps_it_does_not_select(D, nq):
    far = G.rig_case(D, nq, True, kinds=("far",), nan="all")
    G.assert_all_outside(far, D)
    cost = ref_cost(far)
    assert torch.equal(cost, torch.zeros_like(cost)), "a tap outside the volume reached the result"
    assert_readout_exact("read-out, NaN volume", cost)
    edge = G.rig_case(D, nq, True, kinds=G.NAN_EDGE_KINDS, nan="edges", seed=17)
    G.assert_off_the_edge_planes(edge, D)
    check(f"restatement NaN edge planes D={D} nq={nq}", ref_cost(edge), edge)


def test_restatement_on_strided_views_is_bitwise_the_compact_copy():
    """The layout of section "volumes that span 2^31 bytes" at a small stride: cur and reg interleaved in one buffer."""
    c = G.rig_case(8, 4, True)
    buf = torch.full((G.H * G.W * 40,), float("nan"))
    strided = ref_cost(c, views=G.interleaved_views(buf, 40, c["cur"], c["reg"]))
    check("restatement, interleaved strided views", strided, c)
    assert torch.equal(strided, ref_cost(c, views=G.compact_views(c["cur"], c["reg"])))
    assert int(torch.isfinite(buf).sum()) == 2 * 8 * G.H * G.W, "only the views' elements are written"


def test_big_pixel_strides_sit_on_both_sides_of_two_to_the_31():
    npix, D = G.H * G.W, 8
    below, above = G.big_pixel_strides(npix, D)
    assert (below, above) == (11422785, 11422786)
    assert G.span_bytes(npix, below, D, 1) == (1 << 31) - 36 and G.span_bytes(npix, above, D, 1) == (1 << 31) + 152
    assert G.BIG_REG_OFFSET + (npix - 1) * above + D <= G.BIG_ELEMS < (1 << 29) + (1 << 20)


# ---- the mutants ------------------------------------------------------------------------------------------------------------------
def _rig83():
    return G.rig_case(8, 3, True)


MUTANT_CASES = [
    ("second_batch_index", "nq = 4: (48, 8, 4, 20, 29), per-pixel range", lambda: G.inside_case(48, 8, 4, 20, 29, True, False), "planar"),
    ("second_batch_index", "nq = 4 on the tap-class rig, D = 8", lambda: G.rig_case(8, 4, True), "planar"),
    ("reg_at_cur_position", "Dreg != Dcur: (8, 48, 4, 9, 13)", lambda: G.inside_case(8, 48, 4, 9, 13, True, False), "planar"),
    ("reg_at_cur_position", "Dreg != Dcur: (2, 48, 3, 9, 13), depth input", lambda: G.inside_case(2, 48, 3, 9, 13, True, True), "planar"),
    ("outside_tap_weighted", "tap-class rig, D = 8, nq = 3", _rig83, "planar"),
    ("reg_with_cur_strides", "mixed layout, cur pixel-major: (8, 8, 3, 9, 13)", lambda: G.inside_case(8, 8, 3, 9, 13, False, False),
     "cur_pixel_major"),
    ("reg_with_cur_strides", "mixed layout, reg pixel-major: (8, 8, 3, 9, 13)", lambda: G.inside_case(8, 8, 3, 9, 13, False, False),
     "reg_pixel_major"),
    ("pixel_offset_dropped", "(8, 8, 3, 9, 13)", lambda: G.inside_case(8, 8, 3, 9, 13, False, False), "planar"),
    ("pixel_offset_dropped", "pixel-major view, (48, 48, 4, 20, 29)", lambda: G.inside_case(48, 48, 4, 20, 29, False, True), "view"),
    ("halves_swapped", "(8, 8, 3, 9, 13)", lambda: G.inside_case(8, 8, 3, 9, 13, False, False), "planar"),
    ("halves_swapped", "(8, 8, 2, 9, 13), depth input", lambda: G.inside_case(8, 8, 2, 9, 13, False, True), "planar"),
]


@pytest.mark.parametrize("mutant,named,make,lay", MUTANT_CASES, ids=[f"{m}-{i}" for i, (m, *_) in enumerate(MUTANT_CASES)])
def test_mutant_leaves_an_interval(mutant, named, make, lay):
    c = make()
    assert not violations(ref_cost(c, lay), c).any()
    bad = violations(ref_cost(c, lay, mutant), c)
    print(f"[mutant] {mutant} ({R.MUTANTS[mutant]}): caught by {named} [{lay}], {int(bad.sum())} of {bad.numel()} elements outside")
    assert bad.any(), f"{mutant} passes on {named}"
    # and through the read-out: what the GPU test sees is the mutant's cost itself
    assert_readout_exact(f"read-out of {mutant}", torch.nan_to_num(ref_cost(c, lay, mutant)))


def test_mutant_weighted_tap_is_caught_in_the_upper_and_in_the_lower_class():
    c = _rig83()
    x0 = G.first_tap(c["qd"], 8)
    bad = violations(ref_cost(c, "planar", "outside_tap_weighted"), c)
    for name, sel in (("upper", x0 == -1), ("lower", x0 == 7)):
        n = int((bad & torch.cat([sel, sel])).sum())
        print(f"[mutant] outside_tap_weighted: {n} of {2 * int(sel.sum())} {name}-class elements outside their interval")
        assert n > 0, f"the weighted out-of-range tap passes in the {name} class"


def test_every_mutant_has_a_case():
    assert {m for m, *_ in MUTANT_CASES} == set(R.MUTANTS)
