"""GPU: the volume look-ups load both taps of a position unconditionally and SELECT (csrc/common.hpp: lookup1d_fetch,
effi_getcost_pixel; the generated-input convolution of csrc/conv2d_x3.hpp issues the twelve taps of a staged pixel together).
Checked here: every tap class of a look-up (both taps inside, only the upper, only the lower, both outside at either end) against
the float64 interval of tests/interval_ref.py; taps that are not selected never reach the result (NaN volumes);
``encoder_pair_gen_sr`` bit for bit against the two launches it replaces on maps smaller than, or cutting, a tile."""
import pytest
import torch

import interval_ref as IR
from common import build_model, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

H, W, NQ = 6, 8, 3
DMIN, DMAX = 800.0, 935.0          # a narrow range: positions down to -4.6 of a 2-long volume are still positive depths
SPREAD = 0.1                       # the three hypotheses of a pixel lie at its target position -0.1 / +0 / +0.1: one class per pixel


@pytest.fixture(scope="module")
def O():
    from oracle import effi_oracle
    return effi_oracle


@pytest.fixture(scope="module")
def model():
    return build_model("8,8,8", seed=11, device=DEV)


def _den():
    return (1.0 / DMIN - 1.0 / DMAX) + 1e-10


def _targets(kinds, D):
    """One target position per pixel, cycling through the classes asked for.  Positions keep a fractional part of 0.5 +- 0.1: the class
    of every query is certain (asserted in _classes)."""
    pos = {"both": [0.5 + j for j in sorted({0, (D - 2) // 2, D - 2})], "upper": [-0.5], "lower": [D - 0.5],
           "out_low": [-1.5, -4.5], "out_high": [D + 0.5, D + 3.5], "far": [-4.5, D + 3.5],
           "inner": [0.5 + j for j in sorted({1, (D - 2) // 2, D - 3})] if D >= 4 else []}
    vals = [p for k in kinds for p in pos[k]]
    return torch.tensor([vals[i % len(vals)] for i in range(H * W)], dtype=torch.float64).view(H, W)


def _depth_at(tpos, D):
    return 1.0 / (1.0 / DMAX + tpos * _den() / (D - 1))


def _lookup_queries(kinds, D):
    tm = _targets(kinds, D)
    tq = torch.stack([tm + (k - 1) * SPREAD for k in range(NQ)])
    return _depth_at(tq, D).float()


def _getcost_inputs(kinds, D):
    """-> (depth map of the middle hypothesis, interval): GetCost puts its NQ hypotheses one interval of inverse depth apart."""
    return _depth_at(_targets(kinds, D), D).float(), torch.tensor([SPREAD * _den() / (D - 1)], dtype=torch.float32)


def _first_tap(q, D):
    """First tap x0 of every query from its float64 position; certain: the bound on the fp32 position's error does not reach a
    whole position."""
    tpos, dt = IR.lookup_box(q, DMIN, DMAX, D)
    x0 = torch.floor(tpos - dt)
    assert torch.equal(x0, torch.floor(tpos + dt)), "a query whose first tap is uncertain"
    return x0


def _classes(q, D):
    x0 = _first_tap(q, D)
    return {"both": int(((x0 >= 0) & (x0 <= D - 2)).sum()), "upper": int((x0 == -1).sum()), "lower": int((x0 == D - 1).sum()),
            "out_low": int((x0 <= -2).sum()), "out_high": int((x0 >= D).sum())}


def _run_lookup(vol, q):
    from effi_mvs_plus_amd import ops
    lo, hi = torch.tensor([DMIN], device=DEV), torch.tensor([DMAX], device=DEV)
    return ops.vol_lookup1d(t(vol, DEV), t(q, DEV), lo, hi, H, W)


def _disp_range():
    return torch.linspace(1 / DMAX, 1 / DMIN, 48)


def _run_getcost(cur, reg, x, itv):
    from effi_mvs_plus_amd import ops
    lo, hi = torch.tensor([DMIN], device=DEV), torch.tensor([DMAX], device=DEV)
    return ops.getcost(t(x, DEV), t(_disp_range(), DEV), t(itv, DEV), t(cur, DEV), t(reg, DEV), lo, hi, NQ, H, W, input_is_depth=True)


def _getcost_q(O, x, itv):
    return IR.getcost_queries(O, x, _disp_range(), itv, NQ, True)


ALL = ("both", "upper", "lower", "out_low", "out_high")


@pytest.mark.parametrize("D", [2, 8, 48])
def test_lookup_every_tap_class_inside(O, D):
    """``vol_lookup1d`` and ``getcost`` on a 6x8 map whose queries cover every tap class; bounded as in test_gpu_intervals.py."""
    g = torch.Generator().manual_seed(31 * D)
    cur, reg = torch.randn(D, H, W, generator=g), torch.randn(D, H, W, generator=g)
    dmin, dmax = torch.tensor([DMIN]), torch.tensor([DMAX])
    q = _lookup_queries(ALL, D)
    cls = _classes(q, D)
    print(f"[taps] vol_lookup1d D={D} classes {cls}")
    assert all(v > 0 for v in cls.values()), cls
    s = IR.check_inside(f"vol_lookup1d tap classes D={D}", _run_lookup(cur, q), **IR.lookup_interval(cur, q, dmin, dmax).args())
    assert s["must_be_zero"] > 0
    x, itv = _getcost_inputs(ALL, D)
    qd = _getcost_q(O, x, itv)
    cls = _classes(qd, D)
    print(f"[taps] getcost      D={D} classes {cls}")
    assert all(v > 0 for v in cls.values()), cls
    got = _run_getcost(cur, reg, x, itv)
    for name, vol, part in (("cur", cur, got[:NQ]), ("reg", reg, got[NQ:])):
        iv = IR.lookup_interval(vol, qd, dmin, dmax, n_round=IR.GETCOST_ROUNDINGS)
        IR.check_inside(f"getcost {name} tap classes D={D}", part, **iv.args())


@pytest.mark.parametrize("D", [2, 8, 48])
def test_lookup_of_nan_volume_far_outside_is_exactly_zero(O, D):
    """Every tap outside the volume: the loaded (clamped) values are NaN and must be dropped by a select -- a product with a zero
    weight would give NaN."""
    vol = torch.full((D, H, W), float("nan"))
    q = _lookup_queries(("far",), D)
    cls = _classes(q, D)
    assert cls["both"] == cls["upper"] == cls["lower"] == 0 and cls["out_low"] > 0 and cls["out_high"] > 0, cls
    got = _run_lookup(vol, q)
    assert torch.equal(got.cpu(), torch.zeros(NQ, H, W)), "vol_lookup1d: a tap outside the volume reached the result"
    x, itv = _getcost_inputs(("far",), D)
    cls = _classes(_getcost_q(O, x, itv), D)
    assert cls["both"] == cls["upper"] == cls["lower"] == 0 and cls["out_low"] > 0 and cls["out_high"] > 0, cls
    got = _run_getcost(vol, vol, x, itv)
    assert torch.equal(got.cpu(), torch.zeros(2 * NQ, H, W)), "getcost: a tap outside the volume reached the result"


@pytest.mark.parametrize("D", [2, 8, 48])
def test_lookup_beside_nan_planes_is_finite_and_inside(O, D):
    """NaN in planes 0 and D - 1 only; every query either has both taps in planes 1 .. D - 2 or both outside the volume (D = 2 has
    no plane between the two: outside queries only).  No selected tap reads a NaN plane, so the interval is that of the volume with
    those planes set to 0 (the reference multiplies a clamped tap by its mask and would turn the NaN it must ignore into NaN)."""
    g = torch.Generator().manual_seed(17 * D)
    cur, reg = torch.randn(D, H, W, generator=g), torch.randn(D, H, W, generator=g)
    for v in (cur, reg):
        v[0] = float("nan")
        v[D - 1] = float("nan")
    dmin, dmax = torch.tensor([DMIN]), torch.tensor([DMAX])
    kinds = ("inner", "out_low", "out_high")

    def avoids(q):
        x0 = _first_tap(q, D)
        inner = (x0 >= 1) & (x0 <= D - 3)
        assert bool((inner | (x0 <= -2) | (x0 >= D)).all()), "a query touches a NaN plane"
        assert D < 4 or int(inner.sum()) > 0

    q = _lookup_queries(kinds, D)
    avoids(q)
    IR.check_inside(f"vol_lookup1d NaN edge planes D={D}", _run_lookup(cur, q),
                    **IR.lookup_interval(torch.nan_to_num(cur), q, dmin, dmax).args())
    x, itv = _getcost_inputs(kinds, D)
    qd = _getcost_q(O, x, itv)
    avoids(qd)
    got = _run_getcost(cur, reg, x, itv)
    for name, vol, part in (("cur", cur, got[:NQ]), ("reg", reg, got[NQ:])):
        iv = IR.lookup_interval(torch.nan_to_num(vol), qd, dmin, dmax, n_round=IR.GETCOST_ROUNDINGS)
        IR.check_inside(f"getcost {name} NaN edge planes D={D}", part, **iv.args())


@pytest.mark.parametrize("precision", ["split", "bf16"])
@pytest.mark.parametrize("force_mr", [1, 2, 4])
@pytest.mark.parametrize("h,w", [(3, 4), (5, 36), (13, 20)])
def test_generated_encoder_pair_small_maps_bitwise_twice(model, precision, h, w, force_mr):
    """``encoder_pair_gen_sr`` against ``encoder_inputs_sr`` + ``conv2d_k3_pair_sr``: every bit of both outputs for the three ``hd``,
    on maps smaller than a tile (3x4), one tile high and cutting the third across (5x36), and cutting tiles both ways (13x20); called
    twice in a row on different inputs into the same maps (a window image left over from the first call would show in the second).
    force_mr 4 runs the 3-row form the rule takes for it and the 4-row form behind enc_gen_mr3 = 0."""
    from effi_mvs_plus_amd import ops
    from effi_mvs_plus_amd.models.update import _pack
    net, _ = model
    g = torch.Generator().manual_seed(1000 * h + 10 * w + force_mr)
    D = 8
    before = ops.get_precision()
    try:
        ops.set_precision(precision)
        for s, hd in enumerate(net.hdim_stage):
            e = net.update_block[s].encoder
            wc1, bc1 = e.convc1_raw()
            w7, b7 = e.conv7_packed()
            wd2, bd2 = _pack(e._caches["d2"], e.convd2)
            wc2, bc2 = _pack(e._caches["c2"], e.convc2)
            dr = torch.linspace(1 / 935.0, 1 / 425.0, 384).to(DEV)
            itv = torch.tensor([(dr[-1] - dr[0]).item() / 384], device=DEV)
            lo, hi = torch.full((1,), 425.0, device=DEV), torch.full((1,), 935.0, device=DEV)
            maps = ops.sr_alloc(6, hd, h, w, DEV, clear=False)
            for m in maps:
                m.t.fill_(5.0)
            ops.sr_clear_border([maps])
            A, B, C1, D1, C2, D2 = maps
            for mr3 in ((None, 0) if force_mr == 4 else (None,)):
                for call in range(2):
                    inv = (torch.rand(1, h, w, generator=g) * 1.2 - 0.1).to(DEV)      # some estimates outside [0, 1]: taps off the volume
                    cur, reg = torch.randn(D, h, w, generator=g).to(DEV), torch.randn(D, h, w, generator=g).to(DEV)
                    with ops.options(force_mr=force_mr, enc_gen_mr3=mr3):
                        ops.encoder_inputs_sr(inv, dr, itv, cur, reg, lo, hi, 3, h, w, wc1, bc1, w7, b7, hd, A, B)
                        ops.conv2d_k3_pair_sr([A], wc2.wx, bc2, C1, [B], wd2.wx, bd2, D1, hd, act=ops.ACT_RELU)
                        ops.encoder_pair_gen_sr(inv, dr, itv, cur, reg, lo, hi, 3, h, w, wc1, bc1, w7, b7, hd, wc2.wx, bc2, C2, wd2.wx, bd2,
                                                D2, hd, act=ops.ACT_RELU)
                    torch.cuda.synchronize()
                    tag = f"stage {s + 1} (hd {hd}), call {call + 1}, enc_gen_mr3 {mr3}"
                    assert float(C1.t.float().abs().max()) > 0 and float(D1.t.float().abs().max()) > 0
                    assert torch.equal(C1.t, C2.t), f"{tag}: relu(convc2(cor1)) differs"
                    assert torch.equal(D1.t, D2.t), f"{tag}: relu(convd2(dfm1)) differs"
    finally:
        ops.set_precision(before)
