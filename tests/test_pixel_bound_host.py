"""CPU: the reference of tests/pixel_bound.py proves itself.  For every operation and every case of
tests/test_gpu_pixel_bounds.py:

  (a) the fp32 restatement of the kernel lies inside every interval, nothing is left out, and the share of the interval used is printed;
  (b) every structural mutant leaves an interval in every case that can express it;
  (c) every precision mutant is run and reported (caught or not at these small shapes: not asserted, DESIGN.md says which);
  (d) one soft-argmin mutant that moves only elements below 2e-5 of the peak passes the old yardstick (rel <= max(2e-5, 4 e_ref))
      and fails the interval: the gap this series closes.

The conditions on the inputs (both sides of inv_to_depth's clamp and of the ReLU's kink, the planted zeros, the share of elements
whose interval is narrower than 2^-10 of the element) are asserted here, on the CPU, so the reference alone meets them.
"""
import contextlib
import functools
import math

import pytest
import torch

import pixel_bound as PB
from conv_bound import OutOfBound, check_bounded
from test_gpu_train import rel
from test_gpu_train_scale import launch_shape

USED = {}


def nsplit_of(shape, chunk):
    """The split count the library chooses (ops._reduce_split through launch_shape) under reduce_chunk = chunk (None: the default)."""
    from effi_mvs_plus_amd import ops
    with (ops.options(reduce_chunk=chunk) if chunk is not None else contextlib.nullcontext()):
        return launch_shape("reduce", B=shape[0], n=math.prod(shape[2:]))


def inside(family, name, got, iv):
    rep = check_bounded(name, got, iv.mid, iv.half, quiet=True)
    USED[family] = max(USED.get(family, 0.0), rep["used"])
    print(f"[pixel-host] {name:64s} used {rep['used']:.3f}  pinned {rep['pinned']}/{rep['checked']}")
    return rep


def caught(got, iv):
    try:
        check_bounded("mutant", got, iv.mid, iv.half, quiet=True)
    except OutOfBound:
        return True
    return False


def assert_tight(family, ivs, share=0.5):
    got, n = PB.tight_share(ivs)
    print(f"[pixel-host] {family}: {got:.3f} of {n} non-pinned elements have half <= 2^-10 |mid|; largest share used {USED.get(family, 0):.3f}")
    assert got >= share, f"{family}: only {got:.3f} of the elements are bound to 2^-10 of themselves"


# ==============================================================================================================================
# BatchNorm
# ==============================================================================================================================
BN_PARAMS = [(i, relu) for i in range(len(PB.BN_CASES)) for relu in (False, True)]
BN_FWD, BN_BWD = ("y", "mean", "invstd", "rm", "rv"), ("gx", "s1", "s2")


@functools.lru_cache(maxsize=None)
def bn_case(i, relu):
    shape, chunk, kind = PB.BN_CASES[i]
    ns = nsplit_of(shape, chunk)
    x, gy, par = PB.bn_inputs(shape, kind, seed=(chunk or 0) + sum(shape))
    args = (x, par["weight"], par["bias"], par["running_mean"], par["running_var"], 1e-5, 0.1, relu, ns)
    fwd = PB.bn_fwd_emulate(*args)
    bargs = (gy, fwd["y"], x, fwd["mean"], fwd["invstd"], par["weight"], relu, ns)
    return dict(shape=shape, chunk=chunk, kind=kind, ns=ns, args=args, fwd=fwd, ifwd=PB.bn_fwd_interval(*args), bargs=bargs,
                bwd=PB.bn_bwd_emulate(*bargs), ibwd=PB.bn_bwd_interval(*bargs), name=f"bn {shape} chunk={chunk} {kind} relu={relu} ns={ns}")


@pytest.mark.parametrize("i,relu", BN_PARAMS)
def test_batch_norm_restatement_inside(i, relu):
    c = bn_case(i, relu)
    if c["chunk"] is not None:
        assert c["ns"] > 1
    if c["shape"] == (2, 4, 40, 52):
        assert c["ns"] == 2                                         # 4160 elements per channel over the default chunk of 2048
    for k in BN_FWD:
        inside("batch norm", f"{c['name']} {k}", c["fwd"][k], c["ifwd"][k])
    for k in BN_BWD:
        inside("batch norm", f"{c['name']} {k}", c["bwd"][k], c["ibwd"][k])
    y = c["fwd"]["y"]
    if relu:
        if c["kind"] == "planted":                                  # the planted zeros: a whole channel, with a gradient behind each
            assert bool((y[:, 0] == 0).all()) and bool((c["bargs"][0][:, 0] != 0).any())
            assert int((c["ibwd"]["gx"].half[:, 0] == 0).sum()) == y[:, 0].numel()
            rest = y[:, 1:]
        else:
            rest = y
        on, off = float((rest > 0).float().mean()), float((rest == 0).float().mean())
        assert on >= 0.05 and off >= 0.05, f"{c['name']}: {on:.3f} / {off:.3f} of the elements on the two sides of the kink"


def test_batch_norm_structural_mutants_caught():
    for i, relu in BN_PARAMS:
        c = bn_case(i, relu)
        B = c["shape"][0]
        muts = [("biased_running_var", "fwd", ("rv",)), ("drop_tail", "fwd", BN_FWD), ("drop_tail", "bwd", BN_BWD)]
        if B > 1:
            muts.append(("first_sample_mean", "fwd", ("mean", "y")))
        if relu:
            muts.append(("mask_ge", "bwd", BN_BWD))
        for mut, side, keys in muts:
            emu, args, ivs = (PB.bn_fwd_emulate, c["args"], c["ifwd"]) if side == "fwd" else (PB.bn_bwd_emulate, c["bargs"], c["ibwd"])
            bad = emu(*args, mutant=mut)
            hit = [k for k in keys if caught(bad[k], ivs[k])]
            assert hit, f"{c['name']}: mutant {mut} ({side}) stays inside every interval"


def test_batch_norm_precision_mutants_reported():
    for i, relu in BN_PARAMS:
        c = bn_case(i, relu)
        bad = PB.bn_bwd_emulate(*c["bargs"], mutant="s12_fp32")
        hit = [k for k in BN_BWD if caught(bad[k], c["ibwd"][k])]
        print(f"[pixel-host] precision mutant s1/s2 in fp32, {c['name']}: {'caught on ' + ', '.join(hit) if hit else 'not caught'}")
        if c["kind"] == "offset":
            bad = PB.bn_fwd_emulate(*c["args"], mutant="mean_fp32")
            hit = [k for k in BN_FWD if caught(bad[k], c["ifwd"][k])]
            print(f"[pixel-host] precision mutant mean from an fp32 sum, {c['name']}: {'caught on ' + ', '.join(hit) if hit else 'not caught'}")


def test_batch_norm_intervals_are_tight():
    ivs = [iv for i, relu in BN_PARAMS for c in [bn_case(i, relu)] for iv in list(c["ifwd"].values()) + list(c["ibwd"].values())]
    assert_tight("batch norm", ivs)


# ==============================================================================================================================
# soft-argmin backward
# ==============================================================================================================================
@functools.lru_cache(maxsize=None)
def sam_case(i):
    D, hw, hk, lk = PB.SAM_CASES[i]
    logits, hyp, g = PB.sam_inputs(D, hw, hk, lk, seed=100 + i)
    smp = [(logits[b], hyp[b], g[b]) for b in range(logits.shape[0])]
    return dict(D=D, hw=hw, hk=hk, lk=lk, smp=smp, iv=[PB.softargmin_bwd_interval(*s) for s in smp], name=f"softargmin_bwd D={D} {hw} {hk} {lk}")


@pytest.mark.parametrize("i", range(len(PB.SAM_CASES)))
def test_softargmin_bwd_restatement_inside(i):
    c = sam_case(i)
    for b, (s, iv) in enumerate(zip(c["smp"], c["iv"])):
        rep = inside("soft-argmin bwd", f"{c['name']} sample {b}", PB.softargmin_bwd_emulate(*s), iv)
        assert (rep["pinned"] == rep["checked"]) == (c["D"] == 1)
    if c["hk"] == "pixel" and c["hw"] != (1, 1):
        assert not torch.equal(c["smp"][0][1][:, 0, 0], c["smp"][0][1][:, -1, -1])     # the hypotheses differ per pixel
    assert not torch.equal(c["smp"][0][1], c["smp"][1][1])                             # and per sample


def test_softargmin_bwd_structural_mutants_caught():
    flushed = 0
    for i in range(len(PB.SAM_CASES)):
        c = sam_case(i)
        for s, iv in zip(c["smp"], c["iv"]):
            assert caught(PB.softargmin_bwd_emulate(*s, mutant="dep_short"), iv), f"{c['name']}: dep over D - 1 hypotheses passes"
            if c["hk"] == "pixel" and c["hw"] != (1, 1) and c["D"] > 1:          # (D = 1: every element is 0 whatever hyp is)
                assert caught(PB.softargmin_bwd_emulate(*s, mutant="no_dps"), iv), f"{c['name']}: dps ignored passes"
            p = torch.softmax(s[0].double(), 0)
            if bool((p < 9e-7).any()):
                flushed += 1
                assert caught(PB.softargmin_bwd_emulate(*s, mutant="flush"), iv), f"{c['name']}: the flush passes"
    assert flushed >= 2                                             # the underflow case, both samples


def test_softargmin_bwd_precision_mutant_reported():
    for i in range(len(PB.SAM_CASES)):
        c = sam_case(i)
        hit = [b for b, (s, iv) in enumerate(zip(c["smp"], c["iv"])) if caught(PB.softargmin_bwd_emulate(*s, mutant="fp32"), iv)]
        print(f"[pixel-host] precision mutant dep and difference in fp32, {c['name']}: {'caught' if hit else 'not caught'}")


def test_softargmin_bwd_intervals_are_tight():
    assert_tight("soft-argmin bwd", [iv for i in range(len(PB.SAM_CASES)) for iv in sam_case(i)["iv"]])


def test_the_gap_flush_passes_the_peak_yardstick_and_fails_the_interval():
    """(d): probabilities below 1e-6 flushed to 0 at D = 48, 16 x 20.  Every element the mutant moves is below 2e-5 of the tensor's
    peak, so rel(got, fp64) <= max(2e-5, 4 e_ref) -- the yardstick of tests/test_gpu_train.py -- accepts it; the interval does not."""
    logits, hyp, g = (t_[0] for t_ in PB.sam_inputs(48, (16, 20), "plane", "underflow", seed=7))
    iv = PB.softargmin_bwd_interval(logits, hyp, g)
    good, bad = PB.softargmin_bwd_emulate(logits, hyp, g), PB.softargmin_bwd_emulate(logits, hyp, g, mutant="flush")
    leaf = logits.clone().requires_grad_(True)                      # e_ref: torch's own fp32 autograd of the same operation
    (torch.softmax(leaf, 0) * hyp.view(-1, 1, 1)).sum(0).backward(g)
    moved = bad != good
    peak = float(iv.mid.abs().max())
    assert int(moved.sum()) >= 2 * 16 * 20 and float(iv.mid[moved].abs().max()) < 2e-5 * peak
    e_mut, e_ref = rel(bad, iv.mid), rel(leaf.grad, iv.mid)
    print(f"[pixel-host] the gap: {int(moved.sum())} elements moved, largest {float(iv.mid[moved].abs().max()) / peak:.2e} of the peak; "
          f"e_mutant {e_mut:.3e}  e_ref {e_ref:.3e}  old bound {max(2e-5, 4 * e_ref):.3e}")
    assert e_mut <= max(2e-5, 4 * e_ref)                            # accepted: the gap
    check_bounded("the restatement", good, iv.mid, iv.half, quiet=True)
    assert caught(bad, iv)


# ==============================================================================================================================
# view aggregate
# ==============================================================================================================================
@functools.lru_cache(maxsize=None)
def va_case(i):
    S, D, hw, kind = PB.VA_CASES[i]
    sim, wts, g = PB.va_inputs(S, D, hw, kind, seed=200 + i)
    smp = [(sim[b], wts[b], g[b]) for b in range(sim.shape[0])]
    return dict(S=S, kind=kind, smp=smp, name=f"view_aggregate S={S} D={D} {hw} {kind}",
                fwd=[PB.view_aggregate_interval(s[0], s[1]) for s in smp], mean=[PB.view_aggregate_interval(s[0], None) for s in smp],
                bwd=[PB.view_aggregate_bwd_interval(*s) for s in smp])


@pytest.mark.parametrize("i", range(len(PB.VA_CASES)))
def test_view_aggregate_restatement_inside(i):
    c = va_case(i)
    for b, s in enumerate(c["smp"]):
        inside("view aggregate", f"{c['name']} sample {b} forward", PB.view_aggregate_emulate(s[0], s[1]), c["fwd"][b])
        rep = inside("view aggregate", f"{c['name']} sample {b} forward, no weights", PB.view_aggregate_emulate(s[0], None), c["mean"][b])
        assert (rep["pinned"] == rep["checked"]) == (c["S"] == 1)
        gsim, gw = PB.view_aggregate_bwd_emulate(*s)
        rep = inside("view aggregate", f"{c['name']} sample {b} gsim", gsim, c["bwd"][b][0])
        inside("view aggregate", f"{c['name']} sample {b} gw", gw, c["bwd"][b][1])
        if c["kind"] == "zero":
            assert rep["pinned"] == gsim[1].numel() and bool((s[1][1] == 0).all())
        if c["kind"] == "tiny":
            assert float(s[1].max()) <= 2e-6


def test_view_aggregate_structural_mutants_caught():
    for i in range(len(PB.VA_CASES)):
        c = va_case(i)
        for b, s in enumerate(c["smp"]):
            fwd, (igs, igw) = c["fwd"][b], c["bwd"][b]
            if c["kind"] == "tiny":                                 # den without the 1e-6
                assert caught(PB.view_aggregate_emulate(s[0], s[1], mutant="no_eps"), fwd)
                gsim, gw = PB.view_aggregate_bwd_emulate(*s, mutant="no_eps")
                assert caught(gsim, igs) and caught(gw, igw)
            if c["S"] > 1:
                assert caught(PB.view_aggregate_emulate(s[0], s[1], mutant="short_wsum"), fwd), f"{c['name']}: short wsum passes (forward)"
                gsim, gw = PB.view_aggregate_bwd_emulate(*s, mutant="short_wsum")
                assert caught(gsim, igs) and caught(gw, igw), f"{c['name']}: short wsum passes (backward)"
                assert caught(PB.view_aggregate_bwd_emulate(*s, mutant="gw_shift")[1], igw), f"{c['name']}: gw of view v - 1 passes"


def test_view_aggregate_precision_mutant_reported():
    for i in range(len(PB.VA_CASES)):
        c = va_case(i)
        hit = [b for b, s in enumerate(c["smp"]) if caught(PB.view_aggregate_bwd_emulate(*s, mutant="gw_fp32")[1], c["bwd"][b][1])]
        print(f"[pixel-host] precision mutant gw summed in fp32, {c['name']}: {'caught' if hit else 'not caught'}")


def test_view_aggregate_intervals_are_tight():
    ivs = [iv for i in range(len(PB.VA_CASES)) for c in [va_case(i)] for b in range(2) for iv in (c["fwd"][b], c["mean"][b]) + c["bwd"][b]]
    assert_tight("view aggregate", ivs)


# ==============================================================================================================================
# convex upsampling
# ==============================================================================================================================
@functools.lru_cache(maxsize=None)
def cu_case(i):
    hw, mk, gk = PB.CU_CASES[i]
    inv, mask, gup = PB.cu_inputs(hw, mk, gk, seed=300 + i)
    smp = [(inv[b, 0], mask[b], gup[b]) for b in range(inv.shape[0])]
    return dict(hw=hw, mk=mk, gk=gk, smp=smp, name=f"convex_upsample2x {hw} mask={mk} gup={gk}",
                fwd=[PB.convex_up_interval(s[0], s[1]) for s in smp], bwd=[PB.convex_up_bwd_interval(*s) for s in smp])


@pytest.mark.parametrize("i", range(len(PB.CU_CASES)))
def test_convex_upsample_restatement_inside(i):
    c = cu_case(i)
    h, w = c["hw"]
    for b, s in enumerate(c["smp"]):
        inside("convex upsample", f"{c['name']} sample {b} inv", PB.convex_up_emulate(s[0], s[1]), c["fwd"][b])
        gmask, ginv = PB.convex_up_bwd_emulate(*s)
        inside("convex upsample", f"{c['name']} sample {b} gmask", gmask, c["bwd"][b][0])
        rep = inside("convex upsample", f"{c['name']} sample {b} ginv", ginv, c["bwd"][b][1])
        if c["gk"] == "corners":                                    # ginv is pinned to 0 away from the corners' 2 x 2 neighbourhoods
            assert rep["pinned"] == h * w - 16 and int((c["bwd"][b][1].mid != 0).sum()) == 16
        if c["mk"] == "dominant":
            assert float(s[1].max()) == 30.0


def test_convex_upsample_structural_mutants_caught():
    for i in range(len(PB.CU_CASES)):
        c = cu_case(i)
        h, w = c["hw"]
        for b, s in enumerate(c["smp"]):
            fwd, (igm, igi) = c["fwd"][b], c["bwd"][b]
            for mut in ("mask_layout", "clamp_nb"):
                assert caught(PB.convex_up_emulate(s[0], s[1], mutant=mut), fwd), f"{c['name']}: {mut} passes (forward)"
                gmask, ginv = PB.convex_up_bwd_emulate(*s, mutant=mut)
                assert caught(gmask, igm), f"{c['name']}: {mut} passes (gmask)"
                if mut == "mask_layout":
                    assert caught(ginv, igi), f"{c['name']}: {mut} passes (ginv)"
            if h >= 2 and w >= 2 and c["gk"] == "dense":
                assert caught(PB.convex_up_bwd_emulate(*s, mutant="gather_skip8")[1], igi), f"{c['name']}: the gather without tap 8 passes"


def test_convex_upsample_intervals_are_tight():
    ivs = [iv for i in range(len(PB.CU_CASES)) for c in [cu_case(i)] for b in range(2) for iv in (c["fwd"][b],) + c["bwd"][b]]
    assert_tight("convex upsample", ivs)


# ==============================================================================================================================
# pointwise
# ==============================================================================================================================
@functools.lru_cache(maxsize=None)
def pw_case(n):
    t_ = PB.pw_inputs(n, seed=400 + n)
    return t_, PB.pw_calls(t_, n)


@pytest.mark.parametrize("n", PB.PW_NS)
def test_pointwise_restatement_inside(n):
    _, calls = pw_case(n)
    for op, kw, n_out in calls:
        ivs, got = PB.pw_interval(op, **kw), PB.pw_emulate(op, **kw)
        assert len(ivs) == len(got) == n_out
        for k in range(n_out):
            inside("pointwise", f"pointwise {op} n={n} {kw.get('inner', '')} {kw.get('C', '')} out {k}", got[k], ivs[k])


def test_inv_to_depth_inputs_are_decided_and_reach_both_sides_of_the_clamp():
    lo, hi = PB.PW_RANGE
    sides = [0, 0]
    for n in PB.PW_NS:
        t_, _ = pw_case(n)
        s, ds, clamped, _, _ = PB.inv_to_depth_terms(t_["inv"], lo, hi)
        assert bool(((s - PB.THR).abs() > ds).all()), "an input sits within the rounding of s of the clamp's threshold"
        sides[0] += int(clamped.sum())
        sides[1] += int((~clamped).sum())
        if n >= 255:
            assert bool(clamped.any()) and bool((~clamped).any())
    extra = PB.pw_inputs(2 * 5 * 7 * 11, seed=77)["inv"]             # the input of the GPU test's pass through the autograd Functions
    s, ds, clamped, _, _ = PB.inv_to_depth_terms(extra, lo, hi)
    assert bool(((s - PB.THR).abs() > ds).all()) and bool(clamped.any()) and bool((~clamped).any())
    print(f"[pixel-host] inv_to_depth: {sides[0]} clamped, {sides[1]} live inputs")
    assert min(sides) > 0


def test_pointwise_structural_mutants_caught():
    for n in PB.PW_NS:
        _, calls = pw_case(n)
        for op, kw, _ in calls:
            if op == "act_bwd_sigmoid":
                assert caught(PB.pw_emulate(op, **kw, mutant="sigmoid_plus")[0], PB.pw_interval(op, **kw)[0])
            if op == "scale_ch" and kw["C"] > 1 and n > kw["inner"] + 1:
                assert caught(PB.pw_emulate(op, **kw, mutant="inner_off")[0], PB.pw_interval(op, **kw)[0]), f"inner off by one passes: n={n} {kw['inner']} {kw['C']}"
    # the clamp at >=: shown where the kernel's s IS 1e-4f (inv = 0 and a lo that round-trips to it): the reference pins 0 there
    lo = PB.clamp_edge_lo()
    t_, _ = pw_case(257)
    inv = t_["inv"].clone()
    inv[::5] = 0.0
    kw = dict(a=t_["g"], b=inv, s0=lo, s1=PB.PW_RANGE[1])
    iv = PB.pw_interval("inv_to_depth_bwd", **kw)[0]
    assert bool((iv.half[::5] == 0).all()) and bool((iv.mid[::5] == 0).all())
    inside("pointwise", "pointwise inv_to_depth_bwd on the threshold", PB.pw_emulate("inv_to_depth_bwd", **kw)[0], iv)
    inside("pointwise", "pointwise inv_to_depth on the threshold", PB.pw_emulate("inv_to_depth", a=inv, s0=lo, s1=PB.PW_RANGE[1])[0],
           PB.pw_interval("inv_to_depth", a=inv, s0=lo, s1=PB.PW_RANGE[1])[0])
    assert caught(PB.pw_emulate("inv_to_depth_bwd", **kw, mutant="clamp_ge")[0], iv)


def test_pointwise_intervals_are_tight():
    ivs = [iv for n in PB.PW_NS for op, kw, _ in pw_case(n)[1] for iv in PB.pw_interval(op, **kw)]
    assert_tight("pointwise", ivs)
