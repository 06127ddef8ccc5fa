"""Interval reference for the backward kernels that scatter (warp, look-up, GetCost): the sibling of tests/interval_ref.py, same
`Interval`s, same `check_inside`, float64 on the CPU.

The idea.  These gradients are linear in the upstream gradient and the sampling grid carries none, so the contribution of reference
pixel p at hypothesis d to lattice pixel q of a source map is  a * hat(px - qx) * hat(py - qy),  hat(t) = max(0, 1 - |t|):
continuous in the sampling coordinate, no floor, no flip, and zeros padding is "q outside the image receives nothing".  Over the
coordinate box [px -+ dx] x [py -+ dy] of interval_ref.project() the weight onto q ranges, per axis, over
[min(hat at both ends), hat at the point of the box nearest to q] (hat is concave on its support and 0 outside); the two axes
multiply, both factors being non-negative.  For dx, dy <= 0.25 only the 3 x 3 lattice neighbourhood of (round(px), round(py)) can
receive anything: a point of the box is within 0.75 of the rounded centre, so |q - point| < 1 leaves q = centre - 1, centre, centre + 1.
An element's interval is the sum of min / max of a w_lo, a w_hi over its contributions;  tol = (n + k) u sum |a| w_hi  with n the
number of contributions (any summation order or tree of n fp32 terms is off by at most (n - 1) u of the sum of magnitudes: LDS
partial sums flushed by atomics are one such tree) and k the roundings per term; an element with n = 0 must be exactly 0 (the outputs
are zero-filled and the kernels skip zero weights).

Every constant carries its count of roundings against effi_mvs_plus_amd/csrc/warpcorr.hip and train_ops.hip (u = 2^-24 per fp32
operation, first order); a constant changes only with its derivation, never to fit a kernel's output.
"""
import torch

import interval_ref as IR
from interval_ref import LEFT_OUT_PX, U, Interval

# A bilinear tap weight (make_taps, make_taps_win): wx = ix - x0f or (x0f + 1) - ix (x0f + 1 is exact; one rounding), wy likewise,
# and their product: 3 roundings, relative to the weight.  The rounding of ix itself is the coordinate box, not counted here.
TAP_ROUNDINGS = 3
# stage 1, grad_src  (warpcorr_views_bwd_kernel: g = grad_sim / C [1, exact for C = 2^n], gw = g * w [1], gw * ref [1], the tap weight
# [3] = 6;  warpcorr_views_bwd_win_kernel: g = grad_sim * (1/32) [exact], gw [1], gw * ref [1], the tap weight [3] = 5).  The first
# proposal of this scheme used 8; the re-count against both kernels gives 6.
STAGE1_K = TAP_ROUNDINGS + 3
# stage 1, grad_ref: both kernels run  gr = fmaf(gw, src[tap], gr)  over the FOUR taps of every (view, hypothesis) one after the other
# (the window kernel per view, then one atomic add per view), so the running sum has 4 S D terms, not S D blended ones: n = 4 S D.
# Per term: g [1], gw [1], the tap weight [3], the fused product [counted as 1] = 6.
STAGE1_REF_K = TAP_ROUNDINGS + 3
# homo_warp_bwd_kernel: w * grad_out: the tap weight [3] and the product [1].
HOMO_K = TAP_ROUNDINGS + 1
# 1-D look-ups (lookup1d_bwd behind lookup1d_index): w = ix - x0f or (x0f + 1) - ix [1], g * w [1].
LOOKUP_BWD_K = 2


def dyn_src_k(S):
    """warpcorr_dyn_bwd_kernel, grad_src: coef = g * wv / (den * C): g * wv [1], den = the S-term running sum of the weights + 1e-6
    [S], den * C [1, exact for C = 2^n], the division [1] = S + 3;  cw = coef * w [1], cw * ref [1], the tap weight [3]: S + 8."""
    return S + 3 + 2 + TAP_ROUNDINGS


def dyn_ref_k(S):
    """warpcorr_dyn_bwd_kernel, grad_ref: the four taps are blended FIRST (wp = fmaf(w, tap, wp), 4 roundings relative to the sum of
    magnitudes, the tap weight [3]), then gr = fmaf(coef, wp, gr) [1] with coef as above [S + 3]: S + 11; the sum has S D terms."""
    return S + 3 + 4 + TAP_ROUNDINGS + 1


def _hat(t):
    return (1.0 - t.abs()).clamp(min=0.0)


def hat_range(p, delta, q):
    """[min, max] of hat(p' - q) over p' in [p - delta, p + delta]."""
    lo_p, hi_p = p - delta, p + delta
    near = torch.minimum(torch.maximum(q, lo_p), hi_p)
    return torch.minimum(_hat(lo_p - q), _hat(hi_p - q)), _hat(near - q)


# ---------------------------------------------------------------------------------------------
# the 2-D scatter: gradient w.r.t. a source map
# ---------------------------------------------------------------------------------------------
def scatter_interval(px, py, dx, dy, a, live, h, w, k):
    """px, py, dx, dy [n]: positions and their uncertainty (interval_ref.project, flattened); a [n, C] float64: the coefficient of
    every contribution per channel; live [n]: the upstream gradient is not exactly 0 -> Interval of [h, w, C].
    A live contribution whose box is wider than LEFT_OUT_PX and meets the image could land anywhere: the whole map is `left_out`
    then (the tests run with max_left_out = 0, so this is a condition on the inputs)."""
    C = a.shape[1]
    outside, left = IR._box_flags(px, py, dx, dy, h, w)
    left_any = bool((left & live).any())
    idx = (live & ~outside).nonzero().squeeze(1)
    p_x, p_y = px[idx], py[idx]
    d_x, d_y = dx[idx].clamp(max=LEFT_OUT_PX), dy[idx].clamp(max=LEFT_OUT_PX)
    rx = torch.round(torch.nan_to_num(p_x, nan=-4.0).clamp(-4.0, w + 3.0))
    ry = torch.round(torch.nan_to_num(p_y, nan=-4.0).clamp(-4.0, h + 3.0))
    lo = torch.zeros(h * w, C, dtype=torch.float64)
    hi, mag = torch.zeros_like(lo), torch.zeros_like(lo)
    cnt = torch.zeros(h * w, dtype=torch.float64)
    for oy in (-1.0, 0.0, 1.0):
        qy = ry + oy
        wy_lo, wy_hi = hat_range(p_y, d_y, qy)
        for ox in (-1.0, 0.0, 1.0):
            qx = rx + ox
            wx_lo, wx_hi = hat_range(p_x, d_x, qx)
            w_lo, w_hi = wx_lo * wy_lo, wx_hi * wy_hi
            s = ((qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1) & (w_hi > 0)).nonzero().squeeze(1)
            if s.numel() == 0:
                continue
            q = (qy[s] * w + qx[s]).long()
            a_s = a[idx[s]]
            c_lo, c_hi = a_s * w_lo[s, None], a_s * w_hi[s, None]
            lo.index_add_(0, q, torch.minimum(c_lo, c_hi))
            hi.index_add_(0, q, torch.maximum(c_lo, c_hi))
            mag.index_add_(0, q, a_s.abs() * w_hi[s, None])
            cnt.index_add_(0, q, torch.ones(s.numel(), dtype=torch.float64))
    n = (cnt + k).unsqueeze(1)
    tol = n * U * mag
    zero = (cnt == 0).unsqueeze(1).expand(h * w, C)
    left_out = torch.full((h * w, C), left_any) & ~zero
    sh = (h, w, C)
    return Interval(lo.reshape(sh), hi.reshape(sh), tol.reshape(sh), zero.reshape(sh), left_out.reshape(sh), mag.reshape(sh))


def warp_scatter_interval(ref, rt, depth, G, k=STAGE1_K):
    """Interval of grad_src [h,w,C] of ONE view of the stage-1 warp + correlation: grad_src[q][c] = sum_{d,p} G[d,p] / C * ref[c][p] *
    weight of (d, p) onto q.  ref [C,h,w] fp32, rt: the 12 fp32 values, depth [D] or [D,h,w], G [D,h,w] fp32."""
    C, h, w = ref.shape
    px, py, dx, dy = (v.reshape(-1) for v in IR.project(rt, depth, h, w))
    D = px.numel() // (h * w)
    g = G.double().reshape(D, h * w)
    a = (g.unsqueeze(2) / C * ref.double().permute(1, 2, 0).reshape(1, h * w, C)).reshape(D * h * w, C)
    return scatter_interval(px, py, dx, dy, a, g.reshape(-1) != 0, h, w, k)


def homo_warp_bwd_interval(rt, depth, grad_out):
    """Interval of grad_src [h,w,C] of homo_warp: the same scatter with a = grad_out[c][d][p] (no reference map, no 1/C)."""
    C, D, h, w = grad_out.shape
    px, py, dx, dy = (v.reshape(-1) for v in IR.project(rt, depth, h, w))
    a = grad_out.double().permute(1, 2, 3, 0).reshape(D * h * w, C)
    return scatter_interval(px, py, dx, dy, a, (a != 0).any(1), h, w, HOMO_K)


# ---------------------------------------------------------------------------------------------
# the gather: gradient w.r.t. the reference map
# ---------------------------------------------------------------------------------------------
def _taps_all(srcp, x0, y0, h, w):
    """The four taps (x0 + i, y0 + j) of n positions, all channels, 0 outside the image -> [4, n, C] (nw, ne, sw, se)."""
    out = []
    for j in (0, 1):
        for i in (0, 1):
            xx, yy = x0 + i, y0 + j
            ok = (xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)
            out.append(srcp[yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)] * ok.unsqueeze(1))
    return torch.stack(out)


def _blend_all(T, x0, y0, x, y):
    wx1, wy1 = (x - x0).unsqueeze(1), (y - y0).unsqueeze(1)
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    return T[0] * wx0 * wy0 + T[1] * wx1 * wy0 + T[2] * wx0 * wy1 + T[3] * wx1 * wy1


def bilinear_range_all(srcp, px, py, dx, dy, h, w):
    """min / max over the coordinate box of bilinear(src_c) for every channel, and the max of bilinear(|src_c|): srcp [h*w, C]
    float64, n positions -> lo, hi, mag [n, C].  The points are those of interval_ref._sampled_range: both ends and the lattice
    point between them per axis (a box inside one cell of the lattice needs its four corners only: bilinear there)."""
    n, C = px.numel(), srcp.shape[1]
    xs_, ys_ = IR._axis_points(px, dx, w), IR._axis_points(py, dy, h)
    fx = [torch.floor(v) for v in xs_]
    fy = [torch.floor(v) for v in ys_]
    same = (fx[0] == fx[1]) & (fy[0] == fy[1])
    lo = torch.full((n, C), float("inf"), dtype=torch.float64)
    hi, mag = -lo, torch.zeros(n, C, dtype=torch.float64)

    def merge(s, pts):
        l_, h_, m_ = lo[s], hi[s], mag[s]
        for T, x0, y0, xv, yv in pts:
            v = _blend_all(T, x0, y0, xv, yv)
            l_, h_, m_ = torch.minimum(l_, v), torch.maximum(h_, v), torch.maximum(m_, _blend_all(T.abs(), x0, y0, xv, yv))
        lo[s], hi[s], mag[s] = l_, h_, m_

    if same.any():
        s = same.nonzero().squeeze(1)
        x0, y0 = fx[0][s].long(), fy[0][s].long()
        T = _taps_all(srcp, x0, y0, h, w)
        merge(s, [(T, x0, y0, xv[s], yv[s]) for xv in xs_[:2] for yv in ys_[:2]])
    if (~same).any():
        s = (~same).nonzero().squeeze(1)
        pts = []
        for xv, fxv in zip(xs_, fx):
            for yv, fyv in zip(ys_, fy):
                x0, y0 = fxv[s].long(), fyv[s].long()
                pts.append((_taps_all(srcp, x0, y0, h, w), x0, y0, xv[s], yv[s]))
        merge(s, pts)
    return lo, hi, mag


def warp_gather_interval(srcs, rts, depth, coefs, n_terms, k):
    """Interval of grad_ref [h,w,C]:  grad_ref[p][c] = sum_{v,d} coefs[v][d,p] * bilinear(src_v[c])(project_v(p, d)),  summed with
    the sign of the coefficient.  srcs: S maps [C,h,w]; coefs: S tensors [D,h,w] float64 (g / C at stage 1).
    tol = (n_terms + k) u sum |coef| bilinear(|src_c|)."""
    C, h, w = srcs[0].shape
    lo = torch.zeros(h * w, C, dtype=torch.float64)
    hi, mag = torch.zeros_like(lo), torch.zeros_like(lo)
    cnt = torch.zeros(h * w, dtype=torch.float64)
    left = torch.zeros(h * w, dtype=torch.bool)
    for src, rt, coef in zip(srcs, rts, coefs):
        srcp = src.double().permute(1, 2, 0).reshape(h * w, C)
        px, py, dx, dy = IR.project(rt, depth, h, w)
        outside, lft = IR._box_flags(px, py, dx, dy, h, w)
        D = px.shape[0]
        for d in range(D):                                    # one hypothesis at a time: [h*w, C] working set
            cf = coef[d].reshape(-1)
            use = ((cf != 0) & ~outside[d].reshape(-1)).nonzero().squeeze(1)
            left[use] |= lft[d].reshape(-1)[use]
            if use.numel() == 0:
                continue
            b_lo, b_hi, b_mag = bilinear_range_all(srcp, px[d].reshape(-1)[use], py[d].reshape(-1)[use], dx[d].reshape(-1)[use],
                                                   dy[d].reshape(-1)[use], h, w)
            c = cf[use].unsqueeze(1)
            lo[use] += torch.minimum(c * b_lo, c * b_hi)
            hi[use] += torch.maximum(c * b_lo, c * b_hi)
            mag[use] += c.abs() * b_mag
            cnt[use] += 1
    tol = (n_terms + k) * U * mag
    zero = (cnt == 0).unsqueeze(1).expand(h * w, C)
    left_out = left.unsqueeze(1).expand(h * w, C) & ~zero
    sh = (h, w, C)
    return Interval(lo.reshape(sh), hi.reshape(sh), tol.reshape(sh), zero.reshape(sh), left_out.reshape(sh), mag.reshape(sh))


def stage1_bwd_intervals(feats, rts, depth, G):
    """feats: N maps [C,h,w] (reference first), rts [S,12], depth [D] or [D,h,w], G [S,D,h,w] -> (grad_ref, [grad_src_v])."""
    C = feats[0].shape[0]
    S, D = G.shape[:2]
    g_src = [warp_scatter_interval(feats[0], rts[v], depth, G[v]) for v in range(S)]
    g_ref = warp_gather_interval(feats[1:], rts, depth, [G[v].double() / C for v in range(S)], 4 * S * D, STAGE1_REF_K)
    return g_ref, g_src


# ---------------------------------------------------------------------------------------------
# stages 2/3: the view-weighted volume
# ---------------------------------------------------------------------------------------------
def _fine_weights(view_w, h, w, shift):
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    vw = view_w.shape[2]
    return view_w.double()[:, ys >> shift, xs >> shift], ((ys >> shift) * vw + (xs >> shift)).reshape(-1)


def dyn_bwd_intervals(feats, rts, samples, view_w, shift, sim, G):
    """Backward of the stage-2/3 volume  sim_d = sum_v w_v s_vd / den,  den = sum_v w_v + 1e-6,  at the hypotheses `samples` [D,h,w]
    the forward kernel returned for the same inputs, `sim` [D,h,w] the very tensor handed to the kernel, G [D,h,w]
    -> (grad_ref [h,w,C], [grad_src_v [h,w,C]], grad_view_w [S,vh,vw]).
      grad_ref / grad_src: the stage-1 forms with the coefficient  g_d w_v / (den C)  (dyn_ref_k / dyn_src_k);
      grad_view_w[v][cell] = sum over d and the fine pixels of the cell of  g ([s_lo - tol, s_hi + tol] - sim) / den  with s_vd from
      interval_ref.warp_sim_interval.  The kernel sums in float64 (atomics included); what is fp32 is s_vd (its tol), den (S roundings:
      S - 1 adds and + 1e-6) and the wrapper's final cast [1]: + (S + 1) u of the sum of magnitudes."""
    C, h, w = feats[0].shape
    S, D = len(feats) - 1, samples.shape[0]
    wv, cell = _fine_weights(view_w, h, w, shift)
    den = wv.sum(0) + 1e-6
    g = G.double()
    coefs = [g * wv[v] / (den * C) for v in range(S)]
    refp = feats[0].double().permute(1, 2, 0).reshape(1, h * w, C)
    g_src = []
    for v in range(S):
        px, py, dx, dy = (t_.reshape(-1) for t_ in IR.project(rts[v], samples, h, w))
        a = (coefs[v].reshape(D, h * w, 1) * refp).reshape(D * h * w, C)
        g_src.append(scatter_interval(px, py, dx, dy, a, g.reshape(-1) != 0, h, w, dyn_src_k(S)))
    g_ref = warp_gather_interval(feats[1:], rts, samples, coefs, S * D, dyn_ref_k(S))
    n_cell = view_w.shape[1] * view_w.shape[2]
    los, his, tols, lefts = [], [], [], []
    sim64 = sim.double()
    for v in range(S):
        iv = IR.warp_sim_interval(feats[0], feats[v + 1], rts[v], samples)
        e_lo, e_hi = g / den * (iv.lo - iv.tol - sim64), g / den * (iv.hi + iv.tol - sim64)
        t_lo, t_hi = torch.minimum(e_lo, e_hi).sum(0).reshape(-1), torch.maximum(e_lo, e_hi).sum(0).reshape(-1)
        t_mag = torch.maximum(e_lo.abs(), e_hi.abs()).sum(0).reshape(-1)
        t_left = (iv.left_out & (g != 0)).any(0).reshape(-1).double()
        z = torch.zeros(n_cell, dtype=torch.float64)
        los.append(z.index_add(0, cell, t_lo))
        his.append(z.index_add(0, cell, t_hi))
        tols.append((S + 1) * U * z.index_add(0, cell, t_mag))
        lefts.append(z.index_add(0, cell, t_left) > 0)
    sh = tuple(view_w.shape)
    g_vw = Interval(torch.stack(los).reshape(sh), torch.stack(his).reshape(sh), torch.stack(tols).reshape(sh), None,
                    torch.stack(lefts).reshape(sh))
    return g_ref, g_src, g_vw


# ---------------------------------------------------------------------------------------------
# 1-D look-ups
# ---------------------------------------------------------------------------------------------
def lookup_bwd_interval(gout, Dp, query, dmin, dmax, n_round=IR.LOOKUP_ROUNDINGS):
    """Interval of the gradient of the zero-padded 1-D look-up w.r.t. its volume: gvol[x][p] = sum_k gout[k][p] hat(t_k[p] - x).
    gout [nq,h,w]; query [nq,h,w] or [nq,2h,2w] (read at the even pixels, as the kernel does); dmin / dmax scalar or [h,w]
    -> Interval of [Dp,h,w].  t_k and its uncertainty: interval_ref.lookup_box.  tol = (n + LOOKUP_BWD_K) u sum |g| w_hi; the
    accumulation is a read-modify-write in a fixed order, bounded as a sum in any order all the same."""
    nq, h, w = gout.shape
    if tuple(query.shape[1:]) != (h, w):
        assert (query.shape[1] // 2, query.shape[2] // 2) == (h, w)
        query = query[:, 0:2 * h:2, 0:2 * w:2]
    t, dt = IR.lookup_box(query, dmin, dmax, Dp, n_round)
    g = gout.double().unsqueeze(0)
    x = torch.arange(Dp, dtype=torch.float64).reshape(Dp, 1, 1, 1)
    box_out = (t + dt <= -1.0) | (t - dt >= Dp)
    live = (g[0] != 0) & ~box_out
    w_lo, w_hi = hat_range(t.unsqueeze(0), dt.clamp(max=LEFT_OUT_PX).unsqueeze(0), x)          # [Dp,nq,h,w]
    w_lo, w_hi = w_lo * live, w_hi * live
    c_lo, c_hi = g * w_lo, g * w_hi
    lo, hi = torch.minimum(c_lo, c_hi).sum(1), torch.maximum(c_lo, c_hi).sum(1)
    mag = (g.abs() * w_hi).sum(1)
    cnt = (w_hi > 0).sum(1).double()
    tol = (cnt + LOOKUP_BWD_K) * U * mag
    zero = cnt == 0
    left = ((dt > LEFT_OUT_PX) & live).any(0).unsqueeze(0).expand(Dp, h, w) & ~zero
    return Interval(lo, hi, tol, zero, left, mag)


def getcost_bwd_intervals(gcost, Dcur, Dreg, queries, dmin, dmax):
    """GetCost backward: gcost [2 nq,h,w], queries [nq,h,w] float64 (interval_ref.getcost_queries) -> (gcur [Dcur,h,w], greg [Dreg,h,w])."""
    nq = queries.shape[0]
    return (lookup_bwd_interval(gcost[:nq], Dcur, queries, dmin, dmax, n_round=IR.GETCOST_ROUNDINGS),
            lookup_bwd_interval(gcost[nq:], Dreg, queries, dmin, dmax, n_round=IR.GETCOST_ROUNDINGS))
