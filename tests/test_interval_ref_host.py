"""CPU: the interval reference (tests/interval_ref.py) has teeth.  The fp32 oracle stands in for the kernels: every element of it lies
inside its interval with nothing left out, and mutants of its output -- the defects the outlier fractions of the parity tests would
let through -- are caught.  No GPU; nothing here makes a kernel fail."""
import pytest
import torch
import torch.nn.functional as F

import interval_cases as cases
import interval_ref as IR
from common import check_close
from oracle import effi_oracle as O


def _rel(pm):
    """Projection pairs [1,N,2,4,4] -> per source view (rot [1,3,3], trans [1,3,1]) as the fp32 oracle composes them, and the twelve
    values as the interval reference takes them."""
    P = [O.compose_projection(pm[:, v]) for v in range(pm.shape[1])]
    out = []
    for v in range(1, len(P)):
        rot, trans = O.relative_projection(P[v], P[0])
        out.append((rot, trans, torch.cat([rot.reshape(-1), trans.reshape(-1)])))
    return out


def _sim_fp32(ref, src, rot, trans, depth, shift_px=0.0, drop_band=False):
    """The fp32 oracle's similarity of one view at explicit (rot, trans): ref / src [C,h,w], depth [D] or [D,h,w] -> [D,h,w].
    Mutants: `shift_px` moves every source x coordinate; `drop_band` zeroes the taps of the half-covered border columns, ix in (-1, 0)
    or (W-1, W) (there the only tap column inside the image is the border one)."""
    C, h, w = ref.shape
    D = depth.shape[0]
    dv = depth.reshape(1, D, 1, 1).expand(1, D, h, w) if depth.dim() == 1 else depth.unsqueeze(0)
    grid = O.warp_grid(rot, trans, dv, h, w).clone()
    grid[..., 0] += shift_px * 2.0 / (w - 1)
    warped = F.grid_sample(src.unsqueeze(0), grid.view(1, D * h, w, 2), mode="bilinear", padding_mode="zeros", align_corners=True)
    sim = (warped.view(1, C, D, h, w) * ref.view(1, C, 1, h, w)).mean(1)[0]
    if drop_band:
        ix = ((grid[..., 0] + 1) / 2 * (w - 1)).view(D, h, w)
        sim = torch.where(((ix > -1) & (ix < 0)) | ((ix > w - 1) & (ix < w)), torch.zeros_like(sim), sim)
    return sim


@pytest.fixture(scope="module")
def stage1():
    """rig x shape -> (stand-in similarities [S,D,h,w], the intervals per view), built once."""
    out = {}
    for kind in cases.RIGS:
        for h, w, D, N in cases.STAGE1_SHAPES:
            feats, pm, samples = cases.stage1_case(kind, h, w, D, N)
            rel = _rel(pm)
            sims = torch.stack([_sim_fp32(feats[0], feats[v + 1], rel[v][0], rel[v][1], samples) for v in range(N - 1)])
            ivs = [IR.warp_sim_interval(feats[0], feats[v + 1], rel[v][2], samples) for v in range(N - 1)]
            out[kind, h, w, D, N] = (sims, ivs, feats, rel, samples)
    return out


def _stack(ivs):
    return IR.stack(ivs).args()


@pytest.mark.parametrize("kind", cases.RIGS)
@pytest.mark.parametrize("h,w,D,N", cases.STAGE1_SHAPES)
def test_oracle_lies_inside_every_interval(stage1, kind, h, w, D, N):
    sims, ivs, *_ = stage1[kind, h, w, D, N]
    s = IR.check_inside(f"oracle [{kind} {h}x{w} D={D}]", sims, **_stack(ivs), max_left_out=0.0)
    if kind == "far":
        assert s["live"] == 0.0 and s["must_be_zero"] == s["elements"], "the view that looks away sees nothing: every element is pinned to 0"
    elif not (kind == "inside" and D == 1):          # `inside` at 20x24, D = 1: 0.4 % of the single plane is live
        assert s["live"] >= 0.05, f"{kind}: only {s['live']:.4f} of the similarities are live"


def test_entropy_of_the_oracle_matches_entropy_from(stage1):
    sims = stage1["rig", 37, 50, 48, 4][0]
    p = F.softmax(sims, dim=1)
    ent = (-p * torch.log(p + 1e-7)).sum(1)
    err = float((ent.double() - IR.entropy_from(sims)).abs().max())
    print(f"[interval] entropy of the fp32 oracle vs entropy_from: max abs {err:.3e}, bound {IR.entropy_atol(48):.3e}")
    assert err <= IR.entropy_atol(48)


# ---------------------------------------------------------------------------------------------
# mutants of the stage-1 similarities
# ---------------------------------------------------------------------------------------------
def _caught(name, got, ivs):
    with pytest.raises(AssertionError, match="outside their interval|must be exactly 0"):
        IR.check_inside(name, got, **_stack(ivs))


def test_mutant_one_16_lane_row_of_one_hypothesis(stage1):
    """The recorded defect's shape: 16 consecutive pixels of one row of one hypothesis of one view too small by a quarter.  Today's
    parity check accepts it -- 16 of 266 400 elements, far inside the 0.2 % allowance, bounded only by the peak: that is the gap."""
    sims, ivs, *_ = stage1["rig", 37, 50, 48, 4]
    v, d = 1, 20
    run = sims[v, d].abs().unfold(1, 16, 1).min(-1).values            # [h, w-15]: the weakest of each run of 16
    y, x = divmod(int(run.argmax()), run.shape[1])
    assert float(run[y, x]) > IR.LIVE, "the mutated run must be live"
    bad = sims.clone()
    bad[v, d, y, x:x + 16] *= 0.75
    check_close("mutant (a) under the parity check", bad, sims, rtol=1e-4, atol=2e-4, frac_ok=0.998)      # accepted: the gap
    _caught("mutant (a)", bad, ivs)


@pytest.mark.parametrize("kind", ["rolled", "wide"])
def test_mutant_border_band_taps_dropped(stage1, kind):
    sims, ivs, feats, rel, samples = stage1[kind, 37, 50, 48, 4]
    bad = torch.stack([_sim_fp32(feats[0], feats[v + 1], rel[v][0], rel[v][1], samples, drop_band=True) for v in range(len(ivs))])
    assert int(((bad != sims) & (sims.abs() > IR.LIVE)).sum()) > 0, "the band must hold live samples"
    _caught(f"mutant (b) [{kind}]", bad, ivs)


@pytest.mark.parametrize("kind", ["rig", "rolled", "wide", "inside"])
def test_mutant_coordinates_shifted_by_a_hundredth_of_a_pixel(stage1, kind):
    sims, ivs, feats, rel, samples = stage1[kind, 16, 20, 8, 3]
    bad = torch.stack([_sim_fp32(feats[0], feats[v + 1], rel[v][0], rel[v][1], samples, shift_px=0.01) for v in range(len(ivs))])
    _caught(f"mutant (c) [{kind}]", bad, ivs)


# ---------------------------------------------------------------------------------------------
# stage 2/3: the weighted combination
# ---------------------------------------------------------------------------------------------
def _dyn_fp32(feats, rel, cur, itv, view_w, shift, D, extra_shift=0):
    h, w = cur.shape
    samples = 1.0 / O.cur_depth_range_samples(1.0 / cur.unsqueeze(0), D, itv)[0]
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    vh, vw = view_w.shape[1:]
    wv = view_w[:, (ys >> (shift + extra_shift)).clamp(max=vh - 1), (xs >> (shift + extra_shift)).clamp(max=vw - 1)]
    acc = sum(wv[v] * _sim_fp32(feats[0], feats[v + 1], rel[v][0], rel[v][1], samples) for v in range(len(rel)))
    return acc / (wv.sum(0) + 1e-6), samples


@pytest.mark.parametrize("kind,h,w,shift,depth", [("rig", 16, 20, 1, "smooth"), ("rolled", 24, 40, 2, "noisy"), ("inside", 17, 23, 0, "clamps")])
def test_dyn_oracle_inside_and_weight_mutant_caught(kind, h, w, shift, depth):
    C, D, S = 8, 8, 3
    from effi_mvs_plus_amd import synth
    feats = [f[0] for f in synth.smooth_features(S + 1, C, h, w, seed=11)]
    rel = _rel(cases.dyn_cameras(h, w, S + 1, kind).unsqueeze(0))
    g = torch.Generator().manual_seed(5)
    view_w = 0.2 + torch.rand(S, h >> shift, w >> shift, generator=g)
    cur, itv = cases.dyn_depth(h, w, depth), torch.tensor(2.0e-5)
    sim, samples = _dyn_fp32(feats, rel, cur, itv, view_w, shift, D)
    iv = IR.dyn_sim_interval(feats[0], feats[1:], [r[2] for r in rel], samples, view_w, shift)
    s = IR.check_inside(f"dyn oracle [{kind} {h}x{w} shift {shift} {depth}]", sim, **iv.args(), max_left_out=0.0)
    assert s["live"] >= 0.05
    bad, _ = _dyn_fp32(feats, rel, cur, itv, view_w, shift, D, extra_shift=1)
    with pytest.raises(AssertionError, match="outside their interval"):
        IR.check_inside("mutant (d): view weights upsampled one level too far", bad, **iv.args())


def test_warp_interval_holds_the_warped_volume(stage1):
    _, _, feats, rel, samples = stage1["rolled", 9, 13, 6, 2]
    src = feats[1][:8]
    h, w = src.shape[1:]
    grid = O.warp_grid(rel[0][0], rel[0][1], samples.view(1, -1, 1, 1).expand(1, 6, h, w), h, w)
    got = F.grid_sample(src.unsqueeze(0), grid.view(1, 6 * h, w, 2), mode="bilinear", padding_mode="zeros", align_corners=True)
    iv = IR.warp_interval(src, rel[0][2], samples)
    IR.check_inside("warped volume of the oracle", got.view(8, 6, h, w), **iv.args())
    with pytest.raises(AssertionError, match="outside their interval"):
        IR.check_inside("warped volume, channels rolled", got.view(8, 6, h, w).roll(1, 0), **iv.args())


# ---------------------------------------------------------------------------------------------
# look-ups
# ---------------------------------------------------------------------------------------------
def _range_shares(vol, q, dmin, dmax):
    t, _ = IR.lookup_position(q, dmin, dmax, vol.shape[0])
    inside = ((t >= 0) & (t <= vol.shape[0] - 1)).double().mean()
    return float(inside), 1.0 - float(inside)


@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("Dp,nq,h,w", [(2, 1, 9, 13), (8, 3, 9, 13), (48, 4, 20, 29), (8, 4, 20, 29), (48, 1, 9, 13), (2, 3, 20, 29)])
def test_lookup_interval_holds_the_oracle_and_catches_an_index_off_by_one(Dp, nq, h, w, per_pixel):
    vol, q, dmin, dmax = cases.lookup_case(Dp, nq, h, w, per_pixel)
    inside, outside = _range_shares(vol, q, dmin, dmax)
    assert inside >= 0.5 and outside >= 0.05, (inside, outside)
    got = O.volume_lookup_1d_explicit(vol.unsqueeze(0), q.unsqueeze(0), dmin, dmax)[0]
    iv = IR.lookup_interval(vol, q, dmin, dmax)
    s = IR.check_inside(f"lookup oracle Dp={Dp} nq={nq} {'per-pixel' if per_pixel else 'global'}", got, **iv.args())
    assert s["must_be_zero"] > 0, "queries far outside the range pin exact zeros"
    bad = O.volume_lookup_1d_explicit(vol.roll(1, 0).unsqueeze(0), q.unsqueeze(0), dmin, dmax)[0]
    with pytest.raises(AssertionError, match="outside their interval|must be exactly 0"):
        IR.check_inside("lookup, index off by one", bad, **iv.args())


@pytest.mark.parametrize("input_is_depth", [False, True])
@pytest.mark.parametrize("Dcur,Dreg,nq,per_pixel", [(8, 8, 3, False), (48, 8, 4, True), (2, 48, 3, True)])
def test_getcost_interval_holds_the_oracle(Dcur, Dreg, nq, per_pixel, input_is_depth):
    h, w = 9, 13
    cur, reg, x, disp_range, itv, dmin, dmax = cases.getcost_case(Dcur, Dreg, nq, h, w, per_pixel, input_is_depth)
    depth = x if input_is_depth else O.disp_to_depth(x, 1.0 / disp_range[-1], 1.0 / disp_range[0])[1]
    pro = [reg.permute(1, 2, 0).reshape(h * w, 1, 1, Dreg), cur.permute(1, 2, 0).reshape(h * w, 1, 1, Dcur)]
    got = O.getcost(depth.view(1, 1, h, w), pro, itv.view(1, 1), nq, dmax, dmin, [1, h, w])[0]
    qd = IR.getcost_queries(O, x, disp_range, itv, nq, input_is_depth)
    inside, outside = _range_shares(cur, qd, dmin, dmax)
    assert inside >= 0.5 and outside >= 0.05, (inside, outside)
    for name, vol, part in (("cur", cur, got[:nq]), ("reg", reg, got[nq:])):
        iv = IR.lookup_interval(vol, qd, dmin, dmax, n_round=IR.GETCOST_ROUNDINGS)
        IR.check_inside(f"getcost oracle {name} D={vol.shape[0]} nq={nq}", part, **iv.args())
        with pytest.raises(AssertionError, match="outside their interval|must be exactly 0"):
            IR.check_inside("getcost, hypotheses in reverse order", part.flip(0), **iv.args())


# ---------------------------------------------------------------------------------------------
# soft-argmin
# ---------------------------------------------------------------------------------------------
def _conf_fp32(logits, shift=0, rounding=torch.trunc):
    """The torch expression of test_softmax_regress_conf; mutants: the padded window one plane off, round() for the truncation."""
    D = logits.shape[0]
    p = F.softmax(logits.unsqueeze(0), dim=1)
    s4 = 4 * F.avg_pool3d(F.pad(p.unsqueeze(1), pad=(0, 0, 0, 0, 1 + shift, 2 - shift)), (4, 1, 1), stride=1, padding=0).squeeze(1)
    idx = rounding(O.depth_regression(p, torch.arange(D, dtype=torch.float32))).long().clamp(0, D - 1)
    return torch.gather(s4, 1, idx.unsqueeze(1)).squeeze(1)[0]


@pytest.mark.parametrize("D", [8, 16, 32, 48, 64, 96, 2, 3, 5, 7, 47, 97])
def test_confidence_set_holds_the_oracle_and_catches_the_mutants(D):
    logits = cases.softmax_logits(D, 13, 17)
    cs = IR.confidence_set(logits, D)
    two = float(cs.two.double().mean())
    assert two >= 0.05 and 1.0 - two >= 0.5, f"two-element sets: {two:.3f}"
    assert bool((cs.idx == 0).any()) and bool((cs.idx == D - 1).any())
    IR.check_confidence(f"confidence oracle D={D}", _conf_fp32(logits), cs)
    if D > 2:                                   # (D = 2: the window covers both planes whatever the index and wherever it starts)
        with pytest.raises(AssertionError, match="match no admissible index"):
            IR.check_confidence("window one plane off", _conf_fp32(logits, shift=1), cs)
        with pytest.raises(AssertionError, match="match no admissible index"):
            IR.check_confidence("round() for trunc()", _conf_fp32(logits, rounding=torch.round), cs)
