"""Interval reference for the warp, look-up and soft-argmin kernels: for every output element an interval that an fp32 evaluation
of the operator must fall into, computed in float64 on the CPU, so that a test can bound EVERY element instead of tolerating a
fraction of outliers.

The idea.  These operators sample a piecewise (bi)linear function of a coordinate that the kernel computes in fp32.  The value is
continuous in the coordinate (zeros padding included: the weight of a tap that leaves the image goes to 0), so an fp32 kernel's
result is  f(x + e) + rounding of the sum  with |e| <= delta, the coordinate's rounding error.  A bilinear function takes its
extremes over a rectangle at the rectangle's corners, a piecewise bilinear one at the corners or on a lattice line inside, so
[min, max] of f over {x - delta, x + delta, the lattice point between them} (per axis) is exact for delta < 0.5.  What remains is
`tol`, the rounding of the sum itself.  Nothing is excluded by a fraction: an element is either inside its interval, or exactly 0
where every tap is provably outside the image, or `left_out` (delta > 0.25 px: the projection is ill-conditioned, Z ~ 0) -- and the
left-out ones are counted and bounded.

Rounding model: u = 2^-24 per fp32 operation (round to nearest), first order in u.  Every constant below carries its count of
roundings against the kernel code it covers (effi_mvs_plus_amd/csrc/warpcorr.hip, common.hpp, volume_ops.hip).  A constant changes
only with its derivation; it is never fitted to a kernel's output.
"""
import torch

U = 2.0 ** -24          # unit roundoff of fp32
# The default kernels divide by a refined reciprocal + one residual step (project_xy / div_by, effi_lk_rcp / effi_lk_div): correctly
# rounded except for rare 1-ulp cases, i.e. at most 2u instead of u per division.  K = 2 scales the whole coordinate term, which
# covers the divisions twice over and leaves the other roundings a margin of 2.
K = 2.0
LEFT_OUT_PX = 0.25      # coordinate uncertainty above which an element is bounded by the peak only (and counted)
LIVE = 1e-3             # |value| above which an element is called live
X3_REL = 2.0 * 2.0 ** -16   # split-precision product (three bf16 partial products per fp32 product), relative to the sum of magnitudes


class Interval:
    """lo / hi: the float64 range of the operator over the coordinate box; tol: rounding of the sum; must_be_zero: every tap is
    outside the image for every coordinate of the box; left_out: the box is wider than LEFT_OUT_PX and meets the image."""

    def __init__(self, lo, hi, tol, must_be_zero=None, left_out=None, mag=None):
        self.lo, self.hi, self.tol, self.mag = lo, hi, tol, mag
        self.must_be_zero = torch.zeros_like(lo, dtype=torch.bool) if must_be_zero is None else must_be_zero
        self.left_out = torch.zeros_like(lo, dtype=torch.bool) if left_out is None else left_out

    def args(self, x3=False):
        """The keyword arguments of check_inside; x3: with the matrix-core form's tol (see warp_sim_interval)."""
        tol = self.tol + X3_REL * self.mag if x3 else self.tol
        return dict(lo=self.lo, hi=self.hi, tol=tol, must_be_zero=self.must_be_zero, left_out=self.left_out)


def stack(ivs):
    """Intervals of several views as one of [S, ...]."""
    cat = lambda k: torch.stack([getattr(iv, k) for iv in ivs])      # noqa: E731
    return Interval(cat("lo"), cat("hi"), cat("tol"), cat("must_be_zero"), cat("left_out"), cat("mag") if ivs[0].mag is not None else None)


# ---------------------------------------------------------------------------------------------
# projection: source coordinates of every (hypothesis, reference pixel) and their fp32 uncertainty
# ---------------------------------------------------------------------------------------------
def project(rt, depth, h, w):
    """rt: the 12 fp32 values of one view (rot row-major, then trans); depth [D] or [D,h,w] -> px, py, dx, dy [D,h,w] float64:
    source position (models/module.py:318-337; (W-1)/2 normalisation followed by the align_corners=True un-normalisation is the
    identity, so ix == px) and the bound on what an fp32 evaluation of it can be off by.

    Roundings, counted against warpcorr_views_body / project_xy / make_taps (all forms evaluate  rx = r0*x + r1*y + r2,
    X = rx*d + tx  in this order, -ffp-contract=off):
      rx: two products (u each on its own term), two adds (u on the partial sums, each <= A_x)       -> <= 3u A_x
      rx*d: the inherited 3u A_x |d| and one rounding                                                -> <= 4u A_x |d|
      + tx: one rounding of X, |X| <= A_x |d| + |tx|                                                 -> E_X = u (5 A_x |d| + |tx|)
    (the first proposal of this scheme, 4u (A_x |d| + |tx|), misses the last rounding's share of A_x |d| and charges tx four times; this is
    the re-count).  The hypothesis d is an INPUT of the projection (shared list, or the `samples` the kernel returns): exact.
      px = X / Z: (E_X + |px| E_Z) / (|Z| - E_Z)  -- exact propagation, not first order: near the pole Z ~ 0 it must not be
      under-estimated; a relative Z error >= 1/2 makes the coordinate unknown (delta = inf) --  plus one rounding of the division.
      normalise / un-normalise (px / hw2 - 1, + 1, * 0.5, * (W-1); hw2 = (W-1)/2 and the halving are exact): division u|px|,
      subtraction u|g| hw2 <= u (|px| + W/2), addition u|px|, product u|px|; with the division X/Z: 5u |px| + u W/2 <= 8u (|px| + W),
      the proposal's count, kept.
    """
    rt = torch.as_tensor(rt).double().reshape(12)
    d = torch.as_tensor(depth).double()
    D = d.shape[0]
    d = d.reshape(D, 1, 1).expand(D, h, w) if d.dim() == 1 else d
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    comp, err = [], []
    for r in range(3):
        a, b, c, tr = rt[3 * r], rt[3 * r + 1], rt[3 * r + 2], rt[9 + r]
        rot = a * xs + b * ys + c
        mag = (a * xs).abs() + (b * ys).abs() + c.abs()
        comp.append(rot * d + tr)
        err.append(U * (5.0 * mag * d.abs() + tr.abs()))
    X, Y, Z = comp
    Z = torch.where(Z == 0, Z + 1e-8, Z)                        # models/module.py:328-329
    px, py = X / Z, Y / Z
    rho = err[2] / Z.abs()
    room = (Z.abs() - err[2]).clamp(min=1e-300)
    inf = torch.full_like(px, float("inf"))
    dx = torch.where(rho < 0.5, K * ((err[0] + px.abs() * err[2]) / room + 8.0 * U * (px.abs() + w)), inf)
    dy = torch.where(rho < 0.5, K * ((err[1] + py.abs() * err[2]) / room + 8.0 * U * (py.abs() + h)), inf)
    return px, py, dx, dy


def _axis_points(p, delta, size):
    """The three abscissae of one axis: both ends of [p - delta, p + delta] and the lattice point nearest to p clamped into it
    (where the piecewise-linear function can have its kink), clamped to [-2, size + 1]: beyond that both taps of the axis are outside
    the image anyway, the value is 0 either way (the kernels' own neutral clamp)."""
    lo, hi = p - delta, p + delta
    mid = torch.minimum(torch.maximum(torch.round(p), lo), hi)
    return [torch.nan_to_num(v, nan=-2.0).clamp(-2.0, size + 1.0) for v in (lo, hi, mid)]


def _tap_products(refp, srcp, pix, x0, y0, h, w):
    """sum_c ref[pix, c] * src[tap, c] for the four taps (x0 + i, y0 + j) of each element, 0 for a tap outside the image ->
    [4, n] in the order nw, ne, sw, se.  refp / srcp: [h*w, C] float64."""
    out = []
    r = refp[pix]
    for j in (0, 1):
        for i in (0, 1):
            xx, yy = x0 + i, y0 + j
            ok = (xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)
            tap = srcp[yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)]
            out.append((r * tap).sum(-1) * ok)
    return torch.stack(out)


def _blend(G, x0, y0, x, y):
    wx1, wy1 = x - x0, y - y0
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    return G[0] * wx0 * wy0 + G[1] * wx1 * wy0 + G[2] * wx0 * wy1 + G[3] * wx1 * wy1


def _sampled_range(refp, srcp, pix, px, py, dx, dy, h, w):
    """min / max over the 3 x 3 points of  sum_c ref_c * bilinear(src_c)  for n elements (flat tensors), and the same sum of
    absolute values at the centre (the scale of the sum's rounding)."""
    xs_, ys_ = _axis_points(px, dx, w), _axis_points(py, dy, h)
    fx = [torch.floor(v) for v in xs_]
    fy = [torch.floor(v) for v in ys_]
    # elements whose nine points share one cell of the lattice: the four tap products once, nine blends
    same = (fx[0] == fx[1]) & (fy[0] == fy[1])
    lo = torch.full_like(px, float("inf"))
    hi = torch.full_like(px, float("-inf"))
    if same.any():
        s = same.nonzero().squeeze(1)
        x0, y0 = fx[0][s].long(), fy[0][s].long()
        G = _tap_products(refp, srcp, pix[s], x0, y0, h, w)
        vals = torch.stack([_blend(G, x0, y0, xv[s], yv[s]) for xv in xs_ for yv in ys_])
        lo[s], hi[s] = vals.min(0).values, vals.max(0).values
    if (~same).any():
        s = (~same).nonzero().squeeze(1)
        vals = []
        for xv, fxv in zip(xs_, fx):
            for yv, fyv in zip(ys_, fy):
                x0, y0 = fxv[s].long(), fyv[s].long()
                vals.append(_blend(_tap_products(refp, srcp, pix[s], x0, y0, h, w), x0, y0, xv[s], yv[s]))
        vals = torch.stack(vals)
        lo[s], hi[s] = vals.min(0).values, vals.max(0).values
    cx = torch.nan_to_num(px, nan=-2.0).clamp(-2.0, w + 1.0)
    cy = torch.nan_to_num(py, nan=-2.0).clamp(-2.0, h + 1.0)
    x0, y0 = torch.floor(cx).long(), torch.floor(cy).long()
    mag = _blend(_tap_products(refp.abs(), srcp.abs(), pix, x0, y0, h, w), x0, y0, cx, cy)
    return lo, hi, mag


def _box_flags(px, py, dx, dy, h, w):
    """must_be_zero: the box lies wholly outside (-1, W) x (-1, H) (no tap of any of its points is inside the image);
    left_out: wider than LEFT_OUT_PX in an axis and not must_be_zero."""
    outside = (px + dx <= -1.0) | (px - dx >= w) | (py + dy <= -1.0) | (py - dy >= h)
    left_out = ((dx > LEFT_OUT_PX) | (dy > LEFT_OUT_PX)) & ~outside
    return outside, left_out


def warp_sim_interval(ref, src, rt, depth):
    """Interval of  sim[d, y, x] = mean_c ref[c, y, x] * bilinear(src[c])(project(x, y, depth[d]))  (one source view).
    ref, src [C,h,w] fp32; rt: the 12 fp32 values the kernel receives; depth [D] or [D,h,w] fp32 -> Interval of [D,h,w].

    tol = (C + 8) u mean_c |ref_c| bilinear(|src_c|): a C-term fp32 sum in any order is off by at most (C - 1) u of the sum of
    magnitudes, the products add 1, and 8 covers the tap weights (two subtractions, one product each) and the four-term blend.
    Matrix-core form (x3=True in split precision; Interval.args(x3=True)): three bf16 partial products per fp32 product -- hi and lo
    are rounded to nearest, the dropped lo*lo term is <= 2^-18 and the two residuals <= 2^-17 each of the product: + 2 * 2^-16 of the
    same mean (X3_REL)."""
    C, h, w = ref.shape
    px, py, dx, dy = project(rt, depth, h, w)
    D = px.shape[0]
    refp = ref.double().permute(1, 2, 0).reshape(h * w, C)
    srcp = src.double().permute(1, 2, 0).reshape(h * w, C)
    pix = torch.arange(h * w).repeat(D)
    lo, hi, mag = _sampled_range(refp, srcp, pix, px.reshape(-1), py.reshape(-1), dx.reshape(-1), dy.reshape(-1), h, w)
    lo, hi, mag = (v.reshape(D, h, w) / C for v in (lo, hi, mag))
    zero, left = _box_flags(px, py, dx, dy, h, w)
    return Interval(lo, hi, (C + 8) * U * mag, zero, left, mag)


def warp_interval(src, rt, depth):
    """Interval of the warped volume itself (homo_warping_new): [C,D,h,w], per channel.  tol = 8 u bilinear(|src_c|): the tap
    weights and the four-term blend of homo_warp_kernel (three roundings per weight, one per product, three adds)."""
    C, h, w = src.shape
    px, py, dx, dy = project(rt, depth, h, w)
    D = px.shape[0]
    n = D * h * w
    pix = torch.arange(n)                                    # the "reference" is a one-hot per channel: refp row = 1
    zero, left = _box_flags(px, py, dx, dy, h, w)
    los, his, tols = [], [], []
    one = torch.ones(n, 1, dtype=torch.float64)
    for c in range(C):
        srcp = src[c].double().reshape(h * w, 1)
        lo, hi, mag = _sampled_range(one, srcp, pix, px.reshape(-1), py.reshape(-1), dx.reshape(-1), dy.reshape(-1), h, w)
        los.append(lo.reshape(D, h, w))
        his.append(hi.reshape(D, h, w))
        tols.append(8.0 * U * mag.reshape(D, h, w))
    ex = lambda m: m.unsqueeze(0).expand(C, D, h, w)      # noqa: E731
    return Interval(torch.stack(los), torch.stack(his), torch.stack(tols), ex(zero), ex(left))


def dyn_sim_interval(ref, srcs, rts, samples, view_w, shift):
    """Interval of the stage-2/3 volume  sum_v w_v sim_v / (sum_v w_v + 1e-6)  at the hypotheses `samples` [D,h,w] the kernel itself
    returned (they are compared separately with the module's formula), w_v = view_w[v, y >> shift, x >> shift] > 0.
    tol = the weighted per-view tol + (S + 4) u |value|: S products and S adds of the weighted sum share (S - 1) + 1 roundings per
    term with the weight sum's, and 4 covers + 1e-6, the division by C and the division by the weight sum."""
    C, h, w = ref.shape
    S = len(srcs)
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    wv = view_w.double()[:, ys >> shift, xs >> shift]                     # [S,h,w]
    assert (wv > 0).all(), "the weighted interval needs positive view weights"
    den = wv.sum(0) + 1e-6
    lo = hi = tol = 0.0
    zero, left = None, None
    for v in range(S):
        iv = warp_sim_interval(ref, srcs[v], rts[v], samples)
        lo, hi, tol = lo + wv[v] * iv.lo, hi + wv[v] * iv.hi, tol + wv[v] * iv.tol
        zero = iv.must_be_zero if zero is None else zero & iv.must_be_zero
        left = iv.left_out if left is None else left | iv.left_out
    lo, hi, tol = lo / den, hi / den, tol / den
    tol = tol + (S + 4) * U * torch.maximum(lo.abs(), hi.abs())
    return Interval(lo, hi, tol, zero, left & ~zero)


# ---------------------------------------------------------------------------------------------
# 1-D look-ups
# ---------------------------------------------------------------------------------------------
LOOKUP_ROUNDINGS = 4        # vol_lookup1d (lookup1d_index): 1/q, 1/dmax, their difference (u on a sum of magnitudes <= |1/q| + |1/dmax|), + 1 spare
# getcost (getcost_kernel; effi_getcost_pixel is the same arithmetic with refined reciprocals), relative to the query's inverse depth s,
# valid while the half range is at most a quarter of the inverse depth (no cancellation in dv -+ half; `getcost_queries` asserts it):
#   scale_inv_depth (effi_inv_to_depth, inv in [0, 1]): 1/lo, 1/(1/lo) and the same for hi (2u each end), the difference, its product
#   with inv, the sum: <= 5u;  1/s0, dv = 1/depth: 7u of dv.   smin / smax = dv -+ half (half = (nq/2) itv, exact for nq <= 5): 8u.
#   step = (smax - smin) / (nq - 1), k * step, smin + k * step: 3 roundings of terms <= the sum: 11u of (dv + half) <= 11 * (5/3) u of
#   s >= dv - half = 3/4 dv, i.e. 19u; hypothesis depth 1/s, then the look-up's own 1/q, 1/dmax, difference: 23u.  With K = 2 in front
#   the proposed count of 12 stands for 24u: kept.
# Re-counted against effi_getcost_pixel (common.hpp), the GetCost of the fused entries (tests/test_gpu_getcost_readout.py), whose three
# reciprocals on the way (dv, 1/s, 1/q) and 1/dmax are effi_lk_rcp, <= 1 ulp = 2u each, a = dv, H = half <= a / 4, n = nq:
#   depth: 5u (scale_inv_depth as above) + 1/s0 (IEEE, u) = 6u; dv = rcp(depth): 8u a.
#   smin = (dv - H)(1 + d1), smax = (dv + H)(1 + d2): the error of dv is COMMON to both, so smax - smin = 2H + d2 (dv + H) - d1 (dv - H) is
#   off by 2u a, + u 2H of the subtraction; step: the division (IEEE) and k * step add 2u of k * step <= 2H.  The largest error, at
#   k = n - 1: 8u a + u (a - H) [smin] + 2u a + 2u H + 4u H [k * step] + u (a + H) [the sum] = u (12 a + 6 H) <= 13.5u a.
#   Relative to s = a - H + 2 H k / (n - 1) it is largest at k = 0: (8 a + (a - H) + (a - H)) / (a - H) <= 8 * 4/3 + 2 = 12.7u
#   (k = n - 1: (12 a + 6 H) / (a + H) <= 12u): <= 13u of s.
#   1/s and the look-up's 1/q: 2u each, 17u of |1/q|; 1/dmax: 2u of |1/dmax|; the difference: u (|1/q| + |1/dmax|):
#   <= 18u (|1/q| + |1/dmax|) <= K * 12 u = 24u.  The count of 12 with K = 2 stands for effi_getcost_pixel as well; depth input
#   (input_is_depth) starts from dv = rcp(x), 2u instead of 8u.
#   den's two reciprocals are effi_lk_rcp too: K u (|1/dmin| + |1/dmax|) / den, the second term of lookup_box, is their 1 ulp exactly.
#   The grid chain of lookup1d_index with effi_lk_div (<= 1 ulp) for both quotients: den's two roundings, the quotient (2u), * (Dp-1)
#   = 5u |t|; 2t / (Dp-1) (2u |t|), - 1 (u |t - (Dp-1)/2|), + 1 and * (Dp-1) (u |t| each): 10u |t| + u Dp / 2 against the
#   8u (|t| + Dp) of lookup_box; the 2u |t| it may lack come out of the 6u (|1/q| + |1/dmax|) (Dp-1) / den >= 6u |t| that the
#   numerator's 24u leave over its 18u.
GETCOST_ROUNDINGS = 12


def _lerp_padded(vol, t):
    """Zero-padded linear interpolation of vol [Dp, ...] (float64) at positions t [nq, ...] along dim 0."""
    Dp = vol.shape[0]
    t = torch.nan_to_num(t, nan=-2.0).clamp(-2.0, Dp + 1.0)
    i0 = torch.floor(t)
    w1 = t - i0
    i0 = i0.long()
    i1 = i0 + 1
    v0 = torch.gather(vol, 0, i0.clamp(0, Dp - 1)) * ((i0 >= 0) & (i0 <= Dp - 1))
    v1 = torch.gather(vol, 0, i1.clamp(0, Dp - 1)) * ((i1 >= 0) & (i1 <= Dp - 1))
    return v0 * (1.0 - w1) + v1 * w1


def lookup_position(query, dmin, dmax, Dp):
    """t = depth_to_disp(q) * (Dp - 1) in float64 (models/Effi_MVS_plus.py:151-164, :123)."""
    q, lo, hi = query.double(), torch.as_tensor(dmin).double(), torch.as_tensor(dmax).double()
    den = (1.0 / lo - 1.0 / hi) + 1e-10
    return (1.0 / q - 1.0 / hi) / den * (Dp - 1), den


def lookup_box(query, dmin, dmax, Dp, n_round=LOOKUP_ROUNDINGS):
    """-> (t, delta_t): the float64 position of every query and what an fp32 evaluation of it can be off by (the formula derived in
    lookup_interval; shared with the backward's hat ranges, tests/scatter_ref.py)."""
    t, den = lookup_position(query, dmin, dmax, Dp)
    q, lo, hi = query.double(), torch.as_tensor(dmin).double(), torch.as_tensor(dmax).double()
    dm1 = float(Dp - 1)
    rel_den = ((1.0 / lo).abs() + (1.0 / hi).abs()) / den
    dt = K * U * (n_round * dm1 * ((1.0 / q).abs() + (1.0 / hi).abs()) / den + rel_den * t.abs()) + 8.0 * U * (t.abs() + Dp)
    return t, dt


def lookup_interval(vol, query, dmin, dmax, n_round=LOOKUP_ROUNDINGS):
    """Interval of the zero-padded 1-D look-up (pro_bilinear_sampler): vol [Dp,h,w], query [nq,h,w] (fp32 depths, or float64 depths
    rebuilt from the module's formula for getcost), dmin / dmax scalar or [h,w] -> Interval of [nq,h,w].

    delta_t = K u (Dp-1) [n_round (|1/q| + |1/dmax|) + (|1/dmin| + |1/dmax|) |t| / (Dp-1)] / den + 8u (|t| + Dp), counted against
    lookup1d_index:
      numerator 1/q - 1/dmax: n_round roundings of magnitude <= |1/q| + |1/dmax| (see LOOKUP_ROUNDINGS / GETCOST_ROUNDINGS), scaled
      to positions by (Dp-1)/den;
      den = (1/dmin - 1/dmax) + 1e-10: its two reciprocals are off by u (|1/dmin| + |1/dmax|), a RELATIVE error of t of that over
      den -- the second term in the bracket, which the first proposal's formula leaves out (it matters for a narrow range, where den is a
      difference of close numbers); den's own two roundings, the division, * (Dp-1), 2t / (Dp-1), - 1 (u of |t - (Dp-1)/2|), + 1,
      * (Dp-1): 8 roundings of magnitude <= |t| + Dp (first proposed as 4: re-counted).
    tol = 4u (|v0| + |v1|): the two weights (one subtraction each, exact or 1 rounding), two products, one add."""
    vol = vol.double()
    Dp = vol.shape[0]
    t, dt = lookup_box(query, dmin, dmax, Dp, n_round)
    pts = [t - dt, t + dt, torch.minimum(torch.maximum(torch.round(t), t - dt), t + dt)]
    vals = torch.stack([_lerp_padded(vol, p) for p in pts])
    i0 = torch.floor(torch.nan_to_num(t, nan=-2.0).clamp(-2.0, Dp + 1.0)).long()
    mag = torch.gather(vol, 0, i0.clamp(0, Dp - 1)).abs() + torch.gather(vol, 0, (i0 + 1).clamp(0, Dp - 1)).abs()
    zero = (t + dt <= -1.0) | (t - dt >= Dp)
    return Interval(vals.min(0).values, vals.max(0).values, 4.0 * U * mag, zero, (dt > LEFT_OUT_PX) & ~zero)


def getcost_queries(O, x, disp_range, interval, nq, input_is_depth):
    """The nq query depths of GetCost per pixel in float64, from the module's formula (oracle.cur_depth_range_samples), not from the
    kernel: x [h,w] normalised inverse depth (or depth), disp_range: inverse-depth range, interval: scalar -> [nq,h,w] float64."""
    x = x.double()
    if not input_is_depth:
        lo, hi = float(disp_range[0]), float(disp_range[-1])
        x = O.disp_to_depth(x, 1.0 / hi, 1.0 / lo)[1]
    inv = 1.0 / x
    assert float((nq // 2) * float(interval) / inv.abs().min()) <= 0.25, "GETCOST_ROUNDINGS assumes half range <= inverse depth / 4"
    return 1.0 / O.cur_depth_range_samples(inv.unsqueeze(0), nq, torch.tensor(float(interval), dtype=torch.float64))[0]


# ---------------------------------------------------------------------------------------------
# soft-argmin + confidence
# ---------------------------------------------------------------------------------------------
class ConfidenceSet:
    """Per pixel: the one or two admissible truncated indices and the window sum of each."""

    def __init__(self, idx, conf, tol, idxf, D):
        self.idx, self.conf, self.tol, self.idxf, self.D = idx, conf, tol, idxf, D          # idx / conf: [2,h,w]
        self.two = idx[0] != idx[1]


def confidence_set(logits, D):
    """logits [D,h,w] -> ConfidenceSet.  The confidence is the only true jump of these operators: sum of p over idx-1 .. idx+2 with
    idx = trunc(sum_d p_d d).  eps = 4 (D + 8) u (D - 1), counted against softmax_regress_conf_body / _reg_body:
      p_d = expf(x_d) / sum, x_d = l_d - m <= 0: the subtraction moves the exponent by u |x_d|, i.e. p_d by u |x_d| e^x_d / sum
      <= 0.37 u ABSOLUTE per term (|x| e^x <= 1/e, sum >= 1), <= 0.37 D u over the volume; expf (2 ulp = 4u), the D-term sum
      ((D - 1) u) and the division (u) are relative: (D + 4) u;
      sum_d p_d * d: a product and up to D - 1 adds per term, of a value <= D - 1: in all (0.37 D + D + 4 + D) u (D - 1)
      <= 4 (D + 8) u (D - 1), since 2.37 D + 4 <= 4 D + 32.
    The admissible indices are trunc(idxf -+ eps) clamped to [0, D-1]; the confidence must be within 4 (D + 8) u of the window sum of
    one of them: 4 * 0.37 u + (D + 4) u of the four p, the window's three adds and the / 4 * 4 pair, < (D + 11) u of a sum <= 1."""
    assert logits.shape[0] == D
    p = torch.softmax(logits.double(), dim=0)
    ar = torch.arange(D, dtype=torch.float64).reshape(D, 1, 1)
    idxf = (p * ar).sum(0)
    eps = 4.0 * (D + 8) * U * (D - 1)
    idx = torch.stack([torch.trunc(idxf - eps), torch.trunc(idxf + eps)]).long().clamp(0, D - 1)
    pad = torch.nn.functional.pad(p, (0, 0, 0, 0, 1, 2))                            # window idx-1 .. idx+2 of the padded volume
    win = pad[0:D] + pad[1:D + 1] + pad[2:D + 2] + pad[3:D + 3]
    conf = torch.gather(win, 0, idx)
    return ConfidenceSet(idx, conf, 4.0 * (D + 8) * U, idxf, D)


def check_confidence(name, got, cs):
    g = got.detach().double().cpu()
    err = (g.unsqueeze(0) - cs.conf).abs()
    best = err.min(0).values
    print(f"[interval] {name:42s} pixels={g.numel()} two_element_sets={float(cs.two.double().mean()):.4f} "
          f"idx_first={int((cs.idx == 0).any(0).sum())} idx_last={int((cs.idx == cs.D - 1).any(0).sum())} "
          f"used={float(best.max()) / cs.tol:.3f}")
    assert torch.isfinite(g).all(), f"{name}: non-finite confidence"
    bad = (best > cs.tol).nonzero()
    assert bad.numel() == 0, f"{name}: {bad.shape[0]} confidences match no admissible index; first: " + "; ".join(
        f"(y={int(y)}, x={int(x)}) got={float(g[y, x]):.9g} want one of {[float(c) for c in cs.conf[:, y, x]]} idxf={float(cs.idxf[y, x]):.9g}"
        for y, x in bad[:10])


def entropy_from(sim):
    """Softmax entropy over the hypothesis axis (dim -3) of the kernel's own returned similarities, in float64
    (models/Effi_MVS_plus.py:43-44).  The kernel's entropy is asserted against it with atol 17 (D + 8) u, no rtol:
    |d(p ln(p + 1e-7)) / dp| <= 17 for p >= 0 (|ln 1e-7| + 1), the relative error of p is (D + 6) u, logf adds 2 ulp, sum_d p_d = 1."""
    s = sim.detach().double().cpu()
    p = torch.softmax(s, dim=-3)
    return (-p * torch.log(p + 1e-7)).sum(-3)


def entropy_atol(D):
    return 17.0 * (D + 8) * U


# ---------------------------------------------------------------------------------------------
# the assertion
# ---------------------------------------------------------------------------------------------
def check_inside(name, got, lo, hi, tol, must_be_zero=None, left_out=None, max_left_out=0.0):
    """Every element of `got` inside [lo - tol, hi + tol], exactly 0 where `must_be_zero`; `left_out` elements are bounded by the peak
    of `hi` and their share by `max_left_out`.  Prints one [interval] line; returns its figures."""
    g = got.detach().double().cpu()
    assert tuple(g.shape) == tuple(lo.shape), f"{name}: shape {tuple(g.shape)} vs {tuple(lo.shape)}"
    zero = torch.zeros_like(g, dtype=torch.bool) if must_be_zero is None else must_be_zero
    left = torch.zeros_like(g, dtype=torch.bool) if left_out is None else left_out
    half = 0.5 * (hi - lo)
    mid = 0.5 * (hi + lo)
    keep = ~left
    width = float((hi - lo)[keep].max()) if keep.any() else 0.0
    used = ((g - mid).abs() / (half + tol).clamp(min=1e-300))
    used = torch.where(keep & torch.isfinite(mid), used, torch.zeros_like(used))
    used = torch.where((half + tol == 0) & (g == mid), torch.zeros_like(used), used)
    live = float((g.abs() > LIVE).double().mean())
    n_left = int(left.sum())
    stats = {"elements": g.numel(), "live": live, "widest": width, "used": float(used.max()) if g.numel() else 0.0,
             "left_out": n_left, "must_be_zero": int(zero.sum())}
    print(f"[interval] {name:42s} elements={g.numel()} live={live:.4f} widest={width:.3e} used={stats['used']:.3f} "
          f"must_be_zero={stats['must_be_zero']} left_out={n_left}")
    assert torch.isfinite(g).all(), f"{name}: non-finite values"

    def where(mask):
        return "; ".join(f"{tuple(int(i) for i in ix)} got={float(g[tuple(ix)]):.9g} lo={float(lo[tuple(ix)]):.9g} hi={float(hi[tuple(ix)]):.9g}"
                         for ix in mask.nonzero()[:10])
    bad = keep & ~((g >= lo - tol) & (g <= hi + tol))
    assert not bad.any(), f"{name}: {int(bad.sum())} elements outside their interval (index: view/channel, d, y, x); first: {where(bad)}"
    nz = zero & (g != 0)
    assert not nz.any(), f"{name}: {int(nz.sum())} elements must be exactly 0 (every tap outside the image); first: {where(nz)}"
    if n_left:
        finite = torch.isfinite(hi) & torch.isfinite(lo)
        peak = float(torch.maximum(hi[finite].abs(), lo[finite].abs()).max()) if finite.any() else 0.0
        wild = left & (g.abs() > peak + float(tol[finite].max() if finite.any() else 0.0))
        assert not wild.any(), f"{name}: {int(wild.sum())} left-out elements exceed the peak {peak:.3e}; first: {where(wild)}"
    share = n_left / max(1, g.numel())
    assert share <= max_left_out, f"{name}: {n_left} elements ({share:.6f}) left out, allowed {max_left_out}"
    return stats
