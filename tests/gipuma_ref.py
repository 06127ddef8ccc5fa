"""Float64 reference of the Gipuma fusion (csrc/gipuma_pixel.hpp) that DECIDES each comparison instead of
tolerating a share of wrong pixels, on the interval types of tests/fusion_bound.py (`B`: a float64 value with a running bound on the
fp32 computation's distance from it, carried operation by operation).

One statement of the kernel's arithmetic (`backproject`, `project`, `disparity`, in gipuma_pixel.hpp's operation order) runs under two
arithmetics: numpy float32 (`restate`: the op-for-op RESTATEMENT, with a `mutant=` switch that plants one structural error) and `B`
(`reference`).  A (pixel, source) comparison is decided true, decided false or UNDECIDED -- undecided when the bound on u + 0.5 or
v + 0.5 straddles an integer, the bound on z straddles 0, or the bound on |f b / z - f b / d_s| - threshold straddles 0.  The flags are
tri-state (0, 1, unknown): a pixel whose own flag is unknown, or whose count could fall on either side of num_consistent, is undecided
and everything it might mark becomes unknown; a fused pixel with an undecided source is fused for certain but its count, point and
the marks of those sources are not.  Unknown flags taint the later reference views, and the share of undecided-or-tainted pixels per
reference view is what CAP_PIXELS (fusion_bound) limits -- a condition on the inputs, asserted from the reference alone.

`exact="all"`: the rig makes every operation exact in fp32, so the chain runs with unit roundoff 0, nothing is undecided and every
value is pinned (half-width 0: bitwise).  `exact="decisions"`: the same for the decisions, the averages are bounded as usual.
"""
import numpy as np

import fusion_bound as FB
from fusion_bound import B, BND, F32, U32, f32

MUTANTS = ("floor_u", "flags_ignored", "flags_unfused", "le_for_lt", "n_for_n_plus_1", "d_for_z", "colour_order")


# ---------------------------------------------------------------------------------------------------------------------------
# gip_prepare_slot
# ---------------------------------------------------------------------------------------------------------------------------
def prepare_slot(cam, ref_cam):
    """-> dict K[9] Ki[9] R[9] t[3] fb, fp32 values: the adjugate inverse and f b in float64, rounded once."""
    cam, ref_cam = np.asarray(cam, f32).reshape(32).astype(np.float64), np.asarray(ref_cam, f32).reshape(32).astype(np.float64)
    K = np.array([cam[16 + r * 4 + k] for r in range(3) for k in range(3)])
    a00, a01, a02 = K[4] * K[8] - K[5] * K[7], K[5] * K[6] - K[3] * K[8], K[3] * K[7] - K[4] * K[6]
    det = K[0] * a00 + K[1] * a01 + K[2] * a02
    adj = np.array([a00, K[2] * K[7] - K[1] * K[8], K[1] * K[5] - K[2] * K[4], a01, K[0] * K[8] - K[2] * K[6], K[2] * K[3] - K[0] * K[5],
                    a02, K[1] * K[6] - K[0] * K[7], K[0] * K[4] - K[1] * K[3]])

    def centre(m):
        return np.array([-(m[k] * m[3] + m[4 + k] * m[7] + m[8 + k] * m[11]) for k in range(3)])
    dx, dy, dz = centre(ref_cam) - centre(cam)
    fb = ref_cam[16] * np.sqrt(dx * dx + dy * dy + dz * dz)
    with np.errstate(all="ignore"):
        return {"K": K.astype(f32), "Ki": (adj / det).astype(f32), "R": np.array([cam[r * 4 + k] for r in range(3) for k in range(3)], f32),
                "t": np.array([cam[3], cam[7], cam[11]], f32), "fb": f32(fb)}


def _lift(A, m):
    return {k: ([A.lift(v) for v in m[k]] if k != "fb" else A.lift(m[k])) for k in m}


# ---------------------------------------------------------------------------------------------------------------------------
# the chain, in gipuma_pixel.hpp's operation order
# ---------------------------------------------------------------------------------------------------------------------------
def backproject(m, x, y, d):
    Ki, R, t = m["Ki"], m["R"], m["t"]
    rx, ry, rz = Ki[0] * x + Ki[1] * y + Ki[2], Ki[3] * x + Ki[4] * y + Ki[5], Ki[6] * x + Ki[7] * y + Ki[8]
    cx, cy, cz = d * rx - t[0], d * ry - t[1], d * rz - t[2]
    return (R[0] * cx + R[3] * cy + R[6] * cz, R[1] * cx + R[4] * cy + R[7] * cz, R[2] * cx + R[5] * cy + R[8] * cz)


def project(A, m, X):
    """-> (z, u + 0.5, v + 0.5)"""
    K, R, t = m["K"], m["R"], m["t"]
    yx, yy = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0], R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1]
    yz = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]
    kx, ky, kz = K[0] * yx + K[1] * yy + K[2] * yz, K[3] * yx + K[4] * yy + K[5] * yz, K[6] * yx + K[7] * yy + K[8] * yz
    half = A.lift(0.5)
    return yz, kx / kz + half, ky / kz + half


def disparity(A, fb, z, ds):
    return A.abs(fb / z - fb / ds)


def ok(d, dmin, dmax):
    with np.errstate(all="ignore"):
        return (d >= f32(dmin)) & (d <= f32(dmax))


def filtered_depths(depths, conf, prob_thr):
    depths = np.asarray(depths, f32)
    if conf is None:
        return depths
    with np.errstate(all="ignore"):
        return np.where(np.asarray(conf, f32) > f32(prob_thr), depths, f32(0.0))


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement: gip_thread op for op in numpy float32, reference views in order
# ---------------------------------------------------------------------------------------------------------------------------
def restate(depths, cams, images, rows, thr, num, conf=None, prob_thr=0.5, dmin=0.001, dmax=100000.0, mutant=None):
    """-> (views, used [n,h*w] uint8) with views[i] = dict(mask, count [h*w], points [3,h*w], colour [h*w,3]; the last two hold 0
    where the pixel is not fused)."""
    assert mutant is None or mutant in MUTANTS, mutant
    D = filtered_depths(depths, conf, prob_thr)
    n_views, h, w = D.shape
    hw = h * w
    D = D.reshape(n_views, hw)
    I = np.asarray(images, f32).reshape(n_views, hw, 3)
    used = np.zeros((n_views, hw), np.uint8)
    ys, xs = FB.pixel_grid(h, w)
    x, y = xs.astype(f32), ys.astype(f32)
    lt = np.less_equal if mutant == "le_for_lt" else np.less
    views = []
    with np.errstate(all="ignore"):
        for ref, srcs in rows:
            mr = _lift(F32, prepare_slot(cams[ref], cams[ref]))
            d = D[ref]
            live = ok(d, dmin, dmax)
            if mutant != "flags_ignored":
                live = live & (used[ref] == 0)
            X = backproject(mr, x, y, d)
            cons, qs, slots = [], [], []
            for s in srcs:
                ms = _lift(F32, prepare_slot(cams[s], cams[ref]))
                z, uh, vh = project(F32, ms, X)
                if mutant == "floor_u":
                    uh = uh - f32(0.5)
                qx, qy = np.floor(uh), np.floor(vh)
                valid = (z > 0) & (qx >= 0) & (qx < f32(w)) & (qy >= 0) & (qy < f32(h))
                q = np.where(valid, qy * f32(w) + qx, 0).astype(np.int64)
                ds = D[s][q]
                c = live & valid & ok(ds, dmin, dmax) & lt(disparity(F32, ms["fb"], d if mutant == "d_for_z" else z, ds), f32(thr))
                cons.append(c), qs.append((q, qx, qy)), slots.append(ms)
            n = np.sum(cons, 0).astype(np.int64) if cons else np.zeros(hw, np.int64)
            fused = live & (n >= num)
            sx, sy, sz = X
            col = I[ref].copy()
            order = list(range(len(srcs)))
            for k in order:
                inc = cons[k] & fused
                q, qx, qy = qs[k]
                Xs = backproject(slots[k], qx, qy, D[srcs[k]][q])
                sx, sy, sz = np.where(inc, sx + Xs[0], sx), np.where(inc, sy + Xs[1], sy), np.where(inc, sz + Xs[2], sz)
                mark = cons[k] if mutant == "flags_unfused" else inc
                used[srcs[k]][q[mark]] = 1
            for k in (reversed(order) if mutant == "colour_order" else order):
                inc = cons[k] & fused
                col = np.where(inc[:, None], col + I[srcs[k]][qs[k][0]], col)
            used[ref][fused] = 1
            div = (n if mutant == "n_for_n_plus_1" else n + 1).astype(f32)
            pts = np.stack([np.where(fused, c / div, f32(0)) for c in (sx, sy, sz)]).astype(f32)
            views.append({"mask": fused, "count": n.astype(np.uint8), "points": pts,
                          "colour": np.where(fused[:, None], col / div[:, None], f32(0)).astype(f32)})
    return views, used


# ---------------------------------------------------------------------------------------------------------------------------
# the interval reference
# ---------------------------------------------------------------------------------------------------------------------------
UNKNOWN = 2


def _exact_floor(b):
    """floor of a bounded value where the whole interval has one floor -> (floor at the midpoint, decided)."""
    with np.errstate(all="ignore"):
        lo, hi = np.floor(b.lo), np.floor(b.hi)
        return np.floor(b.m), np.isfinite(b.e) & (lo == hi), lo, hi


def reference(depths, cams, images, rows, thr, num, conf=None, prob_thr=0.5, dmin=0.001, dmax=100000.0, exact=None):
    """-> (views, flags [n,h*w] in {0, 1, UNKNOWN}); views[i] = dict(mask / mask_decided, count / count_decided [h*w], points [3] B and
    colour [3] B (half-width inf where the pixel is not checked), undecided [h*w]: the pixel is undecided or tainted,
    cmp_undecided / cmp: undecided and all (live pixel, source) comparisons)."""
    D = filtered_depths(depths, conf, prob_thr)
    n_views, h, w = D.shape
    hw = h * w
    D = D.reshape(n_views, hw)
    I = np.asarray(images, f32).reshape(n_views, hw, 3).astype(np.float64)
    flags = np.zeros((n_views, hw), np.uint8)
    ys, xs = FB.pixel_grid(h, w)
    x, y = BND.lift(xs), BND.lift(ys)
    u_dec = 0.0 if exact in ("all", "decisions") else U32
    u_avg = 0.0 if exact == "all" else U32
    views = []
    for ref, srcs in rows:
        mr = _lift(BND, prepare_slot(cams[ref], cams[ref]))
        d = D[ref]
        own = flags[ref].copy()
        dok = ok(d, dmin, dmax)
        live_t, live_u = dok & (own == 0), dok & (own == UNKNOWN)
        with FB.unit(u_dec):
            X = backproject(mr, x, y, BND.lift(d))
        T, U, Q, QV, CAND, slots = [], [], [], [], [], []
        for s in srcs:
            ms = _lift(BND, prepare_slot(cams[s], cams[ref]))
            with FB.unit(u_dec):
                z, uh, vh = project(BND, ms, X)
            qx, dx, xlo, xhi = _exact_floor(uh)
            qy, dy, ylo, yhi = _exact_floor(vh)
            z_t, z_f = z.lo > 0, z.hi <= 0
            q_dec = dx & dy
            inside = q_dec & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            q = np.where(inside, qy * w + qx, 0).astype(np.int64)
            ds = D[s][q]
            ds_ok = inside & ok(ds, dmin, dmax)
            with FB.unit(u_dec):
                disp = disparity(BND, ms["fb"], z, BND.lift(np.where(ds_ok, ds, f32(1.0))))
            c_t, c_f = FB._tri(disp, np.float64(f32(thr)))
            if u_dec == 0.0:                                         # exact values: a tie is decided (|a| < thr is false at equality)
                c_t, c_f = disp.m < np.float64(f32(thr)), disp.m >= np.float64(f32(thr))
            known = np.isfinite(disp.e)
            true = z_t & ds_ok & c_t & known
            false = z_f | (q_dec & ~inside) | (inside & ~ds_ok) | (ds_ok & c_f & known)
            T.append(true), U.append(~(true | false)), Q.append(q), QV.append((qx, qy)), slots.append(ms)
            CAND.append((xlo, xhi, ylo, yhi, np.isfinite(uh.e) & np.isfinite(vh.e) & (xhi - xlo <= 1) & (yhi - ylo <= 1)))
        S = len(srcs)
        Tm, Um = np.array(T).reshape(S, hw), np.array(U).reshape(S, hw)
        any_live = live_t | live_u
        Um = Um & any_live
        Tm = Tm & any_live
        nT, nU = Tm.sum(0), Um.sum(0)
        fused_t = live_t & (nT >= num)
        fused_f = ~any_live | (nT + nU < num)
        fused_u = ~(fused_t | fused_f)
        clean = fused_t & (nU == 0)                                  # point, colour and count are checked
        # the marks
        new = flags
        new[ref][fused_t] = 1
        new[ref][fused_u & (own != 1)] = UNKNOWN
        for k, s in enumerate(srcs):
            sure = fused_t & Tm[k]
            new[s][Q[k][sure]] = 1
            maybe = (fused_u & (Tm[k] | Um[k])) | (fused_t & Um[k])
            if maybe.any():
                xlo, xhi, ylo, yhi, narrow = CAND[k]
                if (maybe & ~narrow).any():
                    new[s][new[s] == 0] = UNKNOWN                    # a projection without a usable bound: anything may be marked
                for cx in (xlo, xhi):
                    for cy in (ylo, yhi):
                        with np.errstate(all="ignore"):
                            okq = maybe & narrow & (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
                            idx = (np.where(okq, cy * w + cx, 0)).astype(np.int64)[okq]
                        new[s][idx[new[s][idx] == 0]] = UNKNOWN
        # the averages of the clean pixels, sums in source order
        with FB.unit(u_avg):
            sm = [B(np.where(clean, c.m, 0.0), np.where(clean, c.e, 0.0)) for c in X]
            col = [B(I[ref][:, c]) for c in range(3)]
            for k, s in enumerate(srcs):
                inc = clean & Tm[k]
                qx, qy = QV[k]
                Xs = backproject(slots[k], BND.lift(np.where(inc, qx, 0.0)), BND.lift(np.where(inc, qy, 0.0)),
                                 BND.lift(np.where(inc, D[s][Q[k]], f32(1.0))))
                for c in range(3):
                    t_ = sm[c] + Xs[c]
                    sm[c] = B(np.where(inc, t_.m, sm[c].m), np.where(inc, t_.e, sm[c].e))
            div = B((nT + 1).astype(np.float64))
            pts = [c / div for c in sm]
        with FB.unit(U32):                                           # the colours are arbitrary fp32 numbers on every rig
            for k, s in enumerate(srcs):
                inc = clean & Tm[k]
                for c in range(3):
                    t_ = col[c] + B(np.where(inc, I[s][Q[k]][:, c], 0.0))
                    col[c] = B(np.where(inc, t_.m, col[c].m), np.where(inc, t_.e, col[c].e))
            col = [c / div for c in col]
        hide = lambda b: B(b.m, np.where(clean, b.e, np.inf))
        undecided = live_u | fused_u | (fused_t & (nU > 0))
        views.append({"mask": fused_t, "mask_decided": ~fused_u, "count": nT.astype(np.uint8), "count_decided": ~live_u & (nU == 0),
                      "points": [hide(p) for p in pts], "colour": [hide(c) for c in col], "clean": clean, "undecided": undecided,
                      "cmp_undecided": int(Um.sum()), "cmp": int(any_live.sum()) * S})
    return views, flags


def case_reference(c):
    import gipuma_cases as GC
    return reference(c["depths"], c["cams"], c["images"], GC.rows_of(c), c["thr"], c["num"], c["conf"], c["prob_thr"], exact=c["exact"])


def case_restate(c, mutant=None):
    import gipuma_cases as GC
    return restate(c["depths"], c["cams"], c["images"], GC.rows_of(c), c["thr"], c["num"], c["conf"], c["prob_thr"], mutant=mutant)


# ---------------------------------------------------------------------------------------------------------------------------
# the assertions
# ---------------------------------------------------------------------------------------------------------------------------
def assert_caps(name, views):
    """The condition on the inputs, from the reference alone: at most CAP_PIXELS of a reference view's pixels undecided or tainted."""
    for i, v in enumerate(views):
        share = float(v["undecided"].mean())
        assert share <= FB.CAP_PIXELS, f"{name} view {i}: {int(v['undecided'].sum())} of {v['undecided'].size} pixels undecided ({share:.5f})"
    return max(float(v["undecided"].mean()) for v in views)


def check_view(name, got, ref, st):
    """got: dict(mask, count [h*w], points [3,h*w], colour [h*w,3] or None) of one reference view against its reference: every decided
    pixel of mask and count exactly, every clean pixel's point and colour inside its interval."""
    FB.check_mask(f"{name} mask", got["mask"], ref["mask"], ref["mask_decided"], st)
    cnt = np.asarray(got["count"]).reshape(-1)
    bad = ref["count_decided"] & (cnt != ref["count"])
    st.checks += cnt.size
    assert not bad.any(), f"{name} count: {int(bad.sum())} decided pixels wrong; first {np.nonzero(bad)[0][:8].tolist()}"
    for c in range(3):
        FB.check_elements(f"{name} points[{c}]", got["points"][c], ref["points"][c], st)
        if got.get("colour") is not None:
            FB.check_elements(f"{name} colour[{c}]", np.asarray(got["colour"])[:, c], ref["colour"][c], st)
    st.pix += ref["undecided"].size
    st.und_pix += int(ref["undecided"].sum())
    st.cmp += ref["cmp"]
    st.und_cmp += ref["cmp_undecided"]


def check_used(name, used, flags, st=None):
    used = np.asarray(used).reshape(flags.shape).astype(np.uint8)
    known = flags != UNKNOWN
    bad = known & (used != flags)
    if st is not None:
        st.checks += used.size
    assert not bad.any(), f"{name} used: {int(bad.sum())} known flags wrong; first {np.argwhere(bad)[:8].tolist()}"


def check_scan(name, got_views, got_used, ref_views, flags, st):
    assert len(got_views) == len(ref_views), name
    for i, (g, r) in enumerate(zip(got_views, ref_views)):
        check_view(f"{name} view {i}", g, r, st)
    check_used(name, got_used, flags, st)


def caught(views, used, ref_views, flags, plain=None):
    """Does a (mutated) restatement break a check?  -> number of decided pixels, known flags and interval elements it breaks, plus --
    given the unmutated restatement `plain` -- the colours that are not bitwise its (the GPU tests compare them so on the exact rigs)."""
    n = int(((flags != UNKNOWN) & (used != flags)).sum())
    for g, r in zip(views, ref_views):
        n += int((r["mask_decided"] & (g["mask"] != r["mask"])).sum()) + int((r["count_decided"] & (g["count"] != r["count"])).sum())
        for c in range(3):
            for got, b in ((g["points"][c], r["points"][c]), (g["colour"][:, c], r["colour"][c])):
                got = np.asarray(got, np.float64)
                with np.errstate(all="ignore"):
                    inside = np.where(b.e == 0, got == b.m, (got >= b.lo) & (got <= b.hi)) | ~np.isfinite(b.e)
                n += int((~inside).sum())
    if plain is not None:
        for g, p in zip(views, plain):
            both = g["mask"] & p["mask"]
            n += int((g["colour"][both].view(np.uint32) != p["colour"][both].view(np.uint32)).sum())
    return n
