"""GPU: every element of the GetCost that the update block actually runs -- ``effi_getcost_pixel`` (csrc/common.hpp) behind
``getcost_conv1x1``, ``encoder_inputs`` and, bit for bit with these, ``encoder_inputs_sr`` / ``encoder_pair_gen_sr`` -- inside the
float64 interval of tests/interval_ref.py, nothing left out.  The costs are read out of the fused entries EXACTLY with selection
weights (tests/getcost_readout.py); the cases (tests/getcost_cases.py) reach both query batches of NQ = 4, Dreg != Dcur, every tap
class, NaN beside the selected taps, volumes whose strides differ, and both sides of the 2^31-byte boundary between 32-bit tap
offsets and 64-bit addressing.  tests/test_getcost_pixel_host.py proves on the CPU that these cases notice a defect of each kind."""
import contextlib

import pytest
import torch

import getcost_cases as G
import getcost_readout as RO
import interval_ref as IR
from common import build_model, t
from test_gpu_sr import assert_sr_equals

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def model():
    return build_model("8,8,8", seed=11, device=DEV)


@pytest.fixture(scope="module")
def big():
    """ONE uninitialised buffer of a little over 2^31 bytes; the tests write only the elements their views touch."""
    free, _ = torch.cuda.mem_get_info()
    if free < (4 << 30):
        pytest.skip(f"{free >> 20} MiB of device memory free: the 2^31-byte volume needs 4 GiB")
    buf = torch.empty(G.BIG_ELEMS, device=DEV, dtype=torch.float32)
    yield buf
    del buf
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _precision(p):
    from effi_mvs_plus_amd import ops
    before = ops.get_precision()
    ops.set_precision(p)
    try:
        yield
    finally:
        ops.set_precision(before)


def _dev(c):
    d = dict(c)
    for k in ("cur", "reg", "x", "disp_range", "itv", "dmin", "dmax"):
        d[k] = t(c[k], DEV)
    return d


_W7 = {}


def _w7(cout):
    if cout not in _W7:
        from effi_mvs_plus_amd import packing
        g = torch.Generator().manual_seed(70 + cout)
        _W7[cout] = packing.pack_conv2d_c1k7(t(0.2 * torch.randn(cout, 1, 7, 7, generator=g), DEV), t(0.1 * torch.randn(cout, generator=g), DEV))
    return _W7[cout]


def _inside(name, cost, c):
    nq = c["nq"]
    return [IR.check_inside(f"fused getcost {half} {name}", part, **iv.args(), max_left_out=0.0)
            for half, part, iv in (("cur", cost[:nq], c["iv"][0]), ("reg", cost[nq:], c["iv"][1]))]


def _conv1x1_cost(name, d, cur_t, reg_t):
    return RO.readout_conv1x1(name, d["x"], d["disp_range"], d["itv"], cur_t, reg_t, d["dmin"], d["dmax"], d["nq"], d["h"], d["w"],
                              d["input_is_depth"])


def _encoder_costs(name, d, cur_t, reg_t):
    """The read-out of ``encoder_inputs`` in both precisions for the three cout -> [(tag, cost)]."""
    out = []
    for precision in ("fp32", "split"):
        for cout in RO.RELU_COUTS:
            w7, b7 = _w7(cout)
            with _precision(precision):
                cost = RO.readout_encoder_inputs(f"{name} {precision} cout={cout}", d["x"], d["disp_range"], d["itv"], cur_t, reg_t, d["dmin"],
                                                 d["dmax"], d["h"], d["w"], cout, w7, b7)
            out.append((f"encoder_inputs {precision} cout={cout}", cost))
    return out


def _every_entry_inside(name, c, d, cur_t, reg_t):
    """``getcost_conv1x1`` and, where the case is one of theirs (nq = 3, normalised inverse depth), ``encoder_inputs``: every element of
    the read-out inside its interval -> the cost of ``getcost_conv1x1``."""
    cost = _conv1x1_cost(name, d, cur_t, reg_t)
    stats = _inside(f"conv1x1 {name}", cost, c)
    if c["nq"] == 3 and not c["input_is_depth"]:
        for tag, ce in _encoder_costs(name, d, cur_t, reg_t):
            _inside(f"{tag} {name}", ce, c)
            assert torch.equal(ce, cost), f"{name}: {tag} and getcost_conv1x1 see different costs"
    return cost, stats


# ---------------------------------------------------------------------------------------------
# 2. every element of the read-out inside its interval
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("input_is_depth", [False, True])
@pytest.mark.parametrize("Dcur,Dreg,nq,h,w,per_pixel", G.INSIDE_CASES)
def test_fused_getcost_inside(Dcur, Dreg, nq, h, w, per_pixel, input_is_depth):
    c = G.inside_case(Dcur, Dreg, nq, h, w, per_pixel, input_is_depth)
    G.shares(c["cur"], c["qd"], c["dmin"], c["dmax"])
    d = _dev(c)
    first = None
    for lay in G.LAYOUTS:
        cur_t, reg_t = G.layout(d["cur"], d["reg"], lay)
        cost, _ = _every_entry_inside(f"D={Dcur}/{Dreg} nq={nq} {h}x{w} depth={int(input_is_depth)} {lay}", c, d, cur_t, reg_t)
        first = cost if first is None else first
        assert torch.equal(cost, first), f"{lay}: the layout changes a bit"


@pytest.mark.parametrize("input_is_depth", [False, True])
@pytest.mark.parametrize("nq", [3, 4])
@pytest.mark.parametrize("D", [2, 8, 48])
def test_fused_getcost_every_tap_class_inside(D, nq, input_is_depth):
    """The rig of test_gpu_lookup_taps.py: every tap class at every query index (nq = 4: in both batches of two)."""
    c = G.rig_case(D, nq, input_is_depth)
    cls = G.assert_every_class(c, D)
    print(f"[taps] fused getcost D={D} nq={nq} depth={int(input_is_depth)} classes per query {cls}")
    d = _dev(c)
    for lay in G.LAYOUTS:
        _, stats = _every_entry_inside(f"tap classes D={D} nq={nq} depth={int(input_is_depth)} {lay}", c, d, *G.layout(d["cur"], d["reg"], lay))
        assert stats[0]["must_be_zero"] > 0


@pytest.mark.parametrize("nq", [3, 4])
@pytest.mark.parametrize("D", [2, 8, 48])
def test_fused_getcost_ignores_nan_taps_it_does_not_select(D, nq):
    """NaN volumes, every tap outside: the read-out is exactly 0.  NaN in planes 0 and D - 1, every selected tap off them: finite
    and inside the interval of the volume with these planes 0.  (A product with a zero weight would give NaN, and one NaN cost
    would reach every channel of the read-out.)"""
    for input_is_depth in ([False, True] if nq == 3 else [True]):
        far = G.rig_case(D, nq, input_is_depth, kinds=("far",), nan="all")
        G.assert_all_outside(far, D)
        d = _dev(far)
        cost, _ = _every_entry_inside(f"NaN volume D={D} nq={nq} depth={int(input_is_depth)}", far, d, d["cur"], d["reg"])
        assert torch.equal(cost.cpu(), torch.zeros(2 * nq, G.H, G.W)), "a tap outside the volume reached the result"
        edge = G.rig_case(D, nq, input_is_depth, kinds=G.NAN_EDGE_KINDS, nan="edges", seed=17)
        G.assert_off_the_edge_planes(edge, D)
        d = _dev(edge)
        _every_entry_inside(f"NaN edge planes D={D} nq={nq} depth={int(input_is_depth)}", edge, d, d["cur"], d["reg"])


# ---------------------------------------------------------------------------------------------
# 4. the split-resident forms: bitwise the forms bounded above
# ---------------------------------------------------------------------------------------------
def _sr_forms(tag, net, d, cur_t, reg_t):
    """For the three hd: ``encoder_inputs_sr`` == the SR form of ``encoder_inputs``' outputs, ``encoder_pair_gen_sr`` ==
    ``encoder_inputs_sr`` + ``conv2d_k3_pair_sr`` (the comparisons of test_gpu_sr.py / test_gpu_lookup_taps.py) -> the four maps
    per hd, for a caller that compares two layouts of the same values."""
    from effi_mvs_plus_amd import ops
    from effi_mvs_plus_amd.models.update import _pack
    assert d["nq"] == 3 and not d["input_is_depth"]
    assert sorted(net.hdim_stage) == [16, 32, 48]
    h, w = d["h"], d["w"]
    x = d["x"].view(1, h, w)
    args = (x, d["disp_range"], d["itv"], cur_t, reg_t, d["dmin"], d["dmax"], 3, h, w)
    out = []
    with _precision("split"):
        for s, hd in enumerate(net.hdim_stage):
            e = net.update_block[s].encoder
            wc1, bc1 = e.convc1_raw()
            w7, b7 = e.conv7_packed()
            wd2, bd2 = _pack(e._caches["d2"], e.convd2)
            wc2, bc2 = _pack(e._caches["c2"], e.convc2)
            maps = ops.sr_alloc(6, hd, h, w, DEV, clear=False)
            for m in maps:
                m.t.fill_(5.0)
            ops.sr_clear_border([maps])
            A, B, C1, D1, C2, D2 = maps
            c1, d1 = ops.encoder_inputs(*args, wc1, bc1, w7, b7, hd)
            ops.encoder_inputs_sr(*args, wc1, bc1, w7, b7, hd, A, B)
            assert_sr_equals(A, c1, f"{tag} hd={hd}: relu(convc1(cost))")
            assert_sr_equals(B, d1, f"{tag} hd={hd}: relu(convd1(inv))")
            ops.conv2d_k3_pair_sr([A], wc2.wx, bc2, C1, [B], wd2.wx, bd2, D1, hd, act=ops.ACT_RELU)
            ops.encoder_pair_gen_sr(*args, wc1, bc1, w7, b7, hd, wc2.wx, bc2, C2, wd2.wx, bd2, D2, hd, act=ops.ACT_RELU)
            torch.cuda.synchronize()
            assert float(C1.t.float().abs().max()) > 0 and float(D1.t.float().abs().max()) > 0
            assert torch.equal(C1.t, C2.t), f"{tag} hd={hd}: relu(convc2(cor1)) differs"
            assert torch.equal(D1.t, D2.t), f"{tag} hd={hd}: relu(convd2(dfm1)) differs"
            out.append([m.t.clone() for m in (A, B, C2, D2)])
    return out


@pytest.mark.parametrize("D", [2, 8, 48])
def test_sr_forms_bitwise_on_every_tap_class(model, D):
    c = G.rig_case(D, 3, False)
    G.assert_every_class(c, D)
    d = _dev(c)
    _sr_forms(f"tap classes D={D}", model[0], d, d["cur"], d["reg"])


@pytest.mark.parametrize("lay", G.MIXED)
def test_sr_forms_bitwise_on_mixed_layouts_and_unequal_volumes(model, lay):
    """13 x 20, Dcur = 8 and Dreg = 48, one volume pixel-major in memory and the other planar."""
    c = G.inside_case(8, 48, 3, 13, 20, True, False)
    d = _dev(c)
    cur_t, reg_t = G.layout(d["cur"], d["reg"], lay)
    _inside(f"conv1x1 D=8/48 nq=3 13x20 {lay}", _conv1x1_cost(lay, d, cur_t, reg_t), c)
    got = _sr_forms(f"D=8/48 13x20 {lay}", model[0], d, cur_t, reg_t)
    want = _sr_forms(f"D=8/48 13x20 planar", model[0], d, d["cur"], d["reg"])
    assert all(torch.equal(a, b) for ga, wa in zip(got, want) for a, b in zip(ga, wa)), f"{lay}: the layout changes a bit"


# ---------------------------------------------------------------------------------------------
# 3. the 64-bit offset branch and the boundary of effi_vol_fits32
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["below", "at_or_above"])
def test_fused_getcost_on_volumes_spanning_two_to_the_31_bytes(model, big, side):
    """Pixel-major views [h*w,1,1,8] of the 6 x 8 rig laid over the large buffer, cur and reg interleaved, with the pixel stride whose
    extent is the largest below 2^31 bytes (32-bit tap offsets at their largest) and the smallest at or above it (64-bit addressing).
    Every entry: inside the intervals, and bit for bit what the compact copy of the same values gives."""
    D, npix = 8, G.H * G.W
    ps = G.big_pixel_strides(npix, D)[side == "at_or_above"]
    span = G.span_bytes(npix, ps, D, 1)
    assert (span < (1 << 31)) == (side == "below")
    c3, c4 = G.rig_case(D, 3, False), G.rig_case(D, 4, True)
    assert torch.equal(c3["cur"], c4["cur"]) and torch.equal(c3["reg"], c4["reg"])
    G.assert_every_class(c3, D), G.assert_every_class(c4, D)
    d3, d4 = _dev(c3), _dev(c4)
    views = G.interleaved_views(big, ps, d3["cur"], d3["reg"])
    assert (views[0].stride(0), views[0].stride(3)) == (ps, 1) and views[1].data_ptr() - views[0].data_ptr() == 4 * G.BIG_REG_OFFSET
    compact = G.compact_views(d3["cur"], d3["reg"])
    print(f"[big] pixel stride {ps}: extent {span} bytes = 2^31 {span - (1 << 31):+d}")
    for c, d in ((c3, d3), (c4, d4)):
        tag = f"nq={c['nq']} extent 2^31{span - (1 << 31):+d}"
        cost, _ = _every_entry_inside(tag, c, d, *views)
        assert torch.equal(cost, _conv1x1_cost(f"{tag} compact", d, *compact)), f"{tag}: the layout changes a bit"
    got = _sr_forms(f"extent 2^31{span - (1 << 31):+d}", model[0], d3, *views)
    want = _sr_forms("compact copy", model[0], d3, *compact)
    assert all(torch.equal(a, b) for ga, wa in zip(got, want) for a, b in zip(ga, wa)), "SR forms: the layout changes a bit"


# ---------------------------------------------------------------------------------------------
# 5. a dense 1x1 on top of the kernel's own costs
# ---------------------------------------------------------------------------------------------
def _dense_inside(name, got, cost, wgt, bias, nq):
    """relu(b + sum_k cost_k w_k) in float64 from the costs the kernel itself read out; tol = (2 nq + 1) u (|b| + sum_k |cost_k w_k|):
    one rounding per fmaf of a partial sum no larger than that magnitude, and one spare.  The ReLU is 1-Lipschitz, so an element
    whose float64 value is within tol of 0 is inside on either side of it."""
    c64, w64, b64 = cost.double().cpu(), wgt.double().cpu(), bias.double().cpu()
    terms = c64.unsqueeze(1) * w64.view(2 * nq, -1, 1, 1)
    val = b64.view(-1, 1, 1) + terms.sum(0)
    tol = (2 * nq + 1) * IR.U * (b64.abs().view(-1, 1, 1) + terms.abs().sum(0))
    err = (got.double().cpu() - val.clamp(min=0)).abs()
    print(f"[dense] {name}: elements={err.numel()} max_err={float(err.max()):.3e} used={float((err / tol).max()):.3f} "
          f"near_zero={int((val.abs() <= tol).sum())} positive={float((val > 0).double().mean()):.3f}")
    assert torch.isfinite(got).all()
    bad = err > tol
    assert not bad.any(), f"{name}: {int(bad.sum())} elements off by more than (2 nq + 1) u of their magnitude; largest {float(err.max()):.3e}"
    assert bool((val > tol).any()) and bool((val < -tol).any()), f"{name}: the case must reach both sides of the ReLU"


def test_dense_conv1x1_on_the_kernels_own_costs():
    from effi_mvs_plus_amd import ops
    nq, h, w, cout = 4, 20, 29, 24
    c = G.inside_case(48, 8, nq, h, w, True, False)
    d = _dev(c)
    cost = _conv1x1_cost("dense", d, d["cur"], d["reg"])
    g = torch.Generator().manual_seed(5)
    wgt, bias = t(0.5 * torch.randn(2 * nq, cout, generator=g), DEV), t(0.1 * torch.randn(cout, generator=g), DEV)
    got = ops.getcost_conv1x1(d["x"], d["disp_range"], d["itv"], d["cur"], d["reg"], d["dmin"], d["dmax"], nq, h, w, wgt, bias, cout, relu=True)
    _dense_inside(f"getcost_conv1x1 nq={nq} cout={cout}", got, cost, wgt, bias, nq)


@pytest.mark.parametrize("cout", RO.RELU_COUTS)
def test_dense_encoder_inputs_on_the_kernels_own_costs(cout):
    from effi_mvs_plus_amd import ops
    h, w = 20, 29
    c = G.inside_case(48, 8, 3, h, w, True, False)
    d = _dev(c)
    w7, b7 = _w7(cout)
    with _precision("fp32"):
        cost = RO.readout_encoder_inputs("dense", d["x"], d["disp_range"], d["itv"], d["cur"], d["reg"], d["dmin"], d["dmax"], h, w, cout, w7, b7)
        g = torch.Generator().manual_seed(6 + cout)
        wgt, bias = t(0.5 * torch.randn(6, cout, generator=g), DEV), t(0.1 * torch.randn(cout, generator=g), DEV)
        got, _ = ops.encoder_inputs(d["x"], d["disp_range"], d["itv"], d["cur"], d["reg"], d["dmin"], d["dmax"], 3, h, w, wgt, bias, w7, b7, cout)
    _dense_inside(f"encoder_inputs cout={cout}", got, cost, wgt, bias, 3)
