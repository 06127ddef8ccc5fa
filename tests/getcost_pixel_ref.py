"""fp32 torch restatement of ``effi_getcost_pixel`` (effi_mvs_plus_amd/csrc/common.hpp), op for op and in its order: the batches of
``QB`` queries, the position of ``cur`` reused for ``reg`` unless the volumes differ in length, both taps loaded at clamped indices
and SELECTED, element strides (ds, ps) per volume.  Every torch op on fp32 CPU tensors rounds once like the C operator it stands
for (no contraction: the library is built with -ffp-contract=off); the refined reciprocal ``effi_lk_rcp`` / quotient ``effi_lk_div``
are written 1 / x and a / b (they differ from these by at most 1 ulp: the K = 2 of tests/interval_ref.py).  All pixels at once.

``mutant`` switches ONE defect on; tests/test_getcost_pixel_host.py shows that the cases of tests/getcost_cases.py notice each."""
import torch

MUTANTS = {
    "second_batch_index": "the second QB batch of NQ = 4 uses k for k0 + k",
    "reg_at_cur_position": "reg is looked up at cur's position although Dreg != Dcur",
    "outside_tap_weighted": "an out-of-range tap enters as clamped value x weight instead of being selected away",
    "reg_with_cur_strides": "reg's taps are addressed with cur's strides",
    "pixel_offset_dropped": "the pixel offset is dropped: every pixel reads pixel 0",
    "halves_swapped": "the cur and reg halves of the cost are swapped",
}


def inv_to_depth(inv, lo, hi):
    """effi_inv_to_depth: lo / hi = disp_range[0] / disp_range[-1] (0-dim fp32)."""
    max_depth, min_depth = 1.0 / lo, 1.0 / hi
    min_disp, max_disp = 1.0 / max_depth, 1.0 / min_depth
    s = min_disp + (max_disp - min_disp) * inv
    return 1.0 / s.clamp(min=1e-4)


def lookup1d_index(Dp, q, dmin, dmax):
    """lookup1d_index -> x0 (int64), w0, w1."""
    scaled = 1.0 / q
    min_disp, max_disp = 1.0 / dmax, 1.0 / dmin
    den = (max_disp - min_disp) + 1e-10
    disp = (scaled - min_disp) / den
    dm1 = float(Dp - 1)
    t = disp * dm1
    g = (2.0 * t) / dm1 - 1.0
    ix = (((g + 1.0) * 0.5) * dm1).clamp(-2.0, dm1 + 2.0)
    x0f = torch.floor(ix)
    return x0f.long(), (x0f + 1.0) - ix, ix - x0f


def _blend(Dp, x0, w0, w1, v0, v1, weighted):
    """lookup1d_blend; weighted: the mutant that multiplies where the kernel selects."""
    if weighted:
        return v0 * w0 + v1 * w1
    in0, in1 = (x0 >= 0) & (x0 <= Dp - 1), (x0 + 1 >= 0) & (x0 + 1 <= Dp - 1)
    r = torch.where(in0, v0 * w0, torch.zeros_like(v0))
    return torch.where(in1, r + v1 * w1, r)


def getcost_pixel(x, input_is_depth, disp_range, itv, cur, cstr, Dcur, reg, rstr, Dreg, rlo, rhi, nq, mutant=None):
    """x [npix]: normalised inverse depth (or depth); itv: 0-dim; cur / reg: FLAT fp32 storage of each volume with its element
    strides cstr / rstr = (ds, ps); rlo / rhi: [npix] or 0-dim -> cost [2 * nq, npix]."""
    assert mutant is None or mutant in MUTANTS
    assert all(v.dtype == torch.float32 for v in (x, itv, cur, reg, rlo, rhi))
    npix = x.numel()
    depth = x if input_is_depth else inv_to_depth(x, disp_range[0], disp_range[-1])
    dv = 1.0 / depth
    half = float(nq // 2) * itv
    smin = (dv - half).clamp(min=1e-4)
    smax = (dv + half).clamp(min=1e-4).clamp(max=1e4)
    step = (smax - smin) / float(nq - 1)
    (cds, cps), (rds, rps) = cstr, rstr
    if mutant == "reg_with_cur_strides":
        rds, rps = cds, cps
    pix = torch.zeros(npix, dtype=torch.int64) if mutant == "pixel_offset_dropped" else torch.arange(npix)
    weighted = mutant == "outside_tap_weighted"

    def tap(vol, off, ds, Dp, i):
        idx = off + i.clamp(0, Dp - 1) * ds
        return vol[idx.clamp(max=vol.numel() - 1)] if mutant == "reg_with_cur_strides" else vol[idx]

    cost = [None] * (2 * nq)
    QB = nq if nq <= 3 else 2
    assert nq % QB == 0
    for k0 in range(0, nq, QB):
        for k in range(QB):
            kk = k if mutant == "second_batch_index" else k0 + k
            s = (smin + float(kk) * step).clamp(min=1e-5)
            qd = 1.0 / s
            xc, wc0, wc1 = lookup1d_index(Dcur, qd, rlo, rhi)
            xr, wr0, wr1 = xc, wc0, wc1
            if Dreg != Dcur and mutant != "reg_at_cur_position":
                xr, wr0, wr1 = lookup1d_index(Dreg, qd, rlo, rhi)
            vc0, vc1 = tap(cur, pix * cps, cds, Dcur, xc), tap(cur, pix * cps, cds, Dcur, xc + 1)
            vr0, vr1 = tap(reg, pix * rps, rds, Dreg, xr), tap(reg, pix * rps, rds, Dreg, xr + 1)
            cost[k0 + k] = _blend(Dcur, xc, wc0, wc1, vc0, vc1, weighted)
            cost[nq + k0 + k] = _blend(Dreg, xr, wr0, wr1, vr0, vr1, weighted)
    out = torch.stack(cost)
    return torch.cat([out[nq:], out[:nq]]) if mutant == "halves_swapped" else out
