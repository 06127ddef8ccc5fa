"""Float64 interval reference for the depth-fusion filters of csrc/fusion.hip: for every continuous output a
`mid` and a `half`, for every mask pixel a three-valued decision (must be 1, must be 0, undecided), so that a test can hold EVERY
element and EVERY pixel instead of a share of them.

How the bound is made.  One statement of each kernel's arithmetic (the functions `img2cam`, `xform`, `cam2img`, `tt_chain`,
`dtu_reproject`, ... below follow csrc/fusion.hip line for line, in its operation order) is evaluated with two arithmetics:
  * `F32` / `F64`: numpy float32 (float64 for the DTU chain, rounded to float32 where the kernel rounds) -- the RESTATEMENT, with a
    `mutant=` switch that plants one structural error;
  * `BND`: every value is a pair (m, e): m the float64 value of the same expression on the same fp32 inputs, e a bound on
    |computed - m| carried op by op (a running error bound): a sum adds the operands' e, a product |x| e_y + |y| e_x + e_x e_y, a
    quotient (e_x + |q| e_y) / (|y| - e_y) -- exact propagation, not first order, and unbounded (the element is LEFT OUT) when the
    denominator is within its own error of 0 -- and EVERY fp32 operation of the source adds u (|m| + e), u = 2^-24 (2^-53 for the
    DTU chain's double operations).  So `half` is the count of the source's roundings times the magnitudes behind the element, with
    the count taken by the code that mirrors the source rather than by hand; no constant here comes from a kernel's output.
The bilinear samples are bounded as tests/interval_ref.py does: zero-padded bilinear sampling is continuous, so its range over the
coordinate box is the min / max over {x - e, x + e, the lattice point between} per axis, plus the blend's own roundings.  (That
file's own routine is not reused: it bounds a feature correlation summed over channels, in torch, with the warp kernels' K = 2
factor for their refined reciprocals; here one depth map is sampled with IEEE divisions.)
"""
import contextlib

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
TINY32 = 2.0 ** -149          # fp32 underflow: absolute error of an operation whose result is subnormal
NEAR = 2.0 ** -40             # a float64 value this close (relative) to an fp32 rounding boundary may round either way
JMAX = 4                      # at most 2^JMAX admissible averaging sets are enumerated per pixel; more: the depth is left out
_UNIT = [U32]
f32 = np.float32


@contextlib.contextmanager
def unit(u):
    """The unit roundoff charged by the B operations inside the block."""
    _UNIT.append(u)
    try:
        yield
    finally:
        _UNIT.pop()


class B:
    """A bounded value: |computed - m| <= e, element-wise.  e = inf: left out (nothing is known)."""
    __array_ufunc__ = None

    def __init__(self, m, e=0.0):
        m, e = np.broadcast_arrays(np.asarray(m, np.float64), np.asarray(e, np.float64))
        bad = ~(np.isfinite(m) & np.isfinite(e))
        self.m, self.e = np.where(bad, 0.0, m), np.where(bad, np.inf, e)

    @staticmethod
    def of(x):
        return x if isinstance(x, B) else B(x)

    @staticmethod
    def _r(m, e):
        u = _UNIT[-1]
        with np.errstate(all="ignore"):
            return B(m, e + u * (np.abs(m) + e) + (TINY32 if u == U32 else 0.0))

    @property
    def lo(self):
        return self.m - self.e - 2.0 ** -52 * np.abs(self.m)

    @property
    def hi(self):
        return self.m + self.e + 2.0 ** -52 * np.abs(self.m)

    def __add__(self, o):
        o = B.of(o)
        return B._r(self.m + o.m, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = B.of(o)
        return B._r(self.m - o.m, self.e + o.e)

    def __rsub__(self, o):
        return B.of(o) - self

    def __mul__(self, o):
        o = B.of(o)
        with np.errstate(all="ignore"):
            return B._r(self.m * o.m, np.abs(self.m) * o.e + np.abs(o.m) * self.e + self.e * o.e)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = B.of(o)
        with np.errstate(all="ignore"):
            room = np.abs(o.m) - o.e
            q = self.m / o.m
            e = np.where(room > 0, (self.e + np.abs(q) * o.e) / room, np.inf)
            return B._r(q, e)

    def __rtruediv__(self, o):
        return B.of(o) / self

    def abs(self):
        return B(np.abs(self.m), self.e)

    def sqrt(self):
        with np.errstate(all="ignore"):
            m = np.sqrt(np.maximum(self.m, 0.0))
            e = np.maximum(np.sqrt(np.maximum(self.m + self.e, 0.0)) - m, m - np.sqrt(np.maximum(self.m - self.e, 0.0)))
            return B._r(m, e)

    def __getitem__(self, i):
        return B(self.m[i], self.e[i])

    def round32(self):
        """The fp32 rounding of a double: one admissible value, or both neighbours where the double lies within its own error (at
        least NEAR, relative) of a rounding boundary.  The result's lo / hi are those fp32 values."""
        e = np.maximum(self.e, NEAR * np.abs(self.m))
        with np.errstate(all="ignore"):
            lo, hi = (self.m - e).astype(f32).astype(np.float64), (self.m + e).astype(f32).astype(np.float64)
        return B(0.5 * (lo + hi), np.where(np.isfinite(self.e), 0.5 * (hi - lo), np.inf))

    def ends(self):
        """(lo, hi) without the float64 slack: the two admissible fp32 values after round32."""
        return self.m - self.e, self.m + self.e


class F32:
    """The restatement's arithmetic: numpy float32, one rounding per operation, as the kernels' (-ffp-contract=off, IEEE division)."""
    @staticmethod
    def lift(x):
        return np.asarray(x, f32)
    sqrt = staticmethod(np.sqrt)
    abs = staticmethod(np.abs)


class BND:
    @staticmethod
    def lift(x):
        return B(np.asarray(np.asarray(x, f32), np.float64))

    @staticmethod
    def sqrt(x):
        return x.sqrt()

    @staticmethod
    def abs(x):
        return x.abs()


# ---------------------------------------------------------------------------------------------------------------------------
# matrices: fus_invert / fus_prepare_view / fus_dtu_prepare_view restated in numpy float64
# ---------------------------------------------------------------------------------------------------------------------------
def gauss_jordan(A, dtype=np.float64):
    """fus_invert (fusion.hip:16-40) op for op: Gauss-Jordan with partial pivoting in float64 (dtype: the mutant's float32)."""
    A = np.asarray(A, dtype)
    n = A.shape[0]
    M = np.zeros((n, 2 * n), dtype)
    M[:, :n] = A
    M[:, n:] = np.eye(n, dtype=dtype)
    for col in range(n):
        piv, best = col, abs(M[col, col])
        for r in range(col + 1, n):
            if abs(M[r, col]) > best:
                best, piv = abs(M[r, col]), r
        if piv != col:
            M[[col, piv]] = M[[piv, col]]
        d = dtype(1.0) / M[col, col]
        for c in range(2 * n):
            M[col, c] = M[col, c] * d
        for r in range(n):
            if r == col:
                continue
            f = M[r, col]
            for c in range(2 * n):
                M[r, c] = M[r, c] - f * M[col, c]
    return M[:, n:].copy()


def _inv32(A):
    """The mutant's inverse: the same elimination in single precision (the reference inverts its float32 matrices in single
    precision; its LAPACK's operation order is not restated, any single-precision elimination shows the size of the gap)."""
    return gauss_jordan(A, f32).astype(np.float64)


def near_boundary(x64):
    """Relative distance of float64 values from the nearest fp32 rounding boundary (the midpoint of two neighbouring fp32 values)."""
    x64 = np.asarray(x64, np.float64)
    r = x64.astype(f32)
    nxt = np.where(r.astype(np.float64) <= x64, np.nextafter(r, f32(np.inf)), np.nextafter(r, f32(-np.inf))).astype(np.float64)
    mid = 0.5 * (r.astype(np.float64) + nxt)
    with np.errstate(all="ignore"):
        return np.where(x64 == 0, np.inf, np.abs(x64 - mid) / np.abs(x64))


def prepare_view(cam, inv=gauss_jordan):
    """fus_prepare_view: cam [2,4,4] fp32 -> dict K[9] Ki[9] E[16] Ei[16] fp32, and the float64 inverses before rounding."""
    cam = np.asarray(cam, f32)
    K, E = cam[1, :3, :3].astype(np.float64), cam[0].astype(np.float64)
    Ki, Ei = inv(K), inv(E)
    return {"K": K.astype(f32).reshape(-1), "Ki": Ki.astype(f32).reshape(-1), "E": E.astype(f32).reshape(-1),
            "Ei": Ei.astype(f32).reshape(-1), "raw64": np.concatenate([Ki.reshape(-1), Ei.reshape(-1)])}


def dtu_prepare_view(ref_cam, src_cam, inv=gauss_jordan):
    """fus_dtu_prepare_view: the reference's own slot (src_cam None: K Ki E Ei) or a source's: K Ki, T_ref->src = E_s . E_ref^-1 and
    T_src->ref = E_ref . E_s^-1, fp32 operands accumulated in double in k order, rounded."""
    ref_cam = np.asarray(ref_cam, f32)
    Kr, Er = ref_cam[1, :3, :3].astype(np.float64), ref_cam[0].astype(np.float64)
    Eri = inv(Er)
    if src_cam is None:
        Ki = inv(Kr)
        return {"K": Kr.astype(f32).reshape(-1), "Ki": Ki.astype(f32).reshape(-1), "E": Er.astype(f32).reshape(-1),
                "Ei": Eri.astype(f32).reshape(-1), "raw64": np.concatenate([Ki.reshape(-1), Eri.reshape(-1)])}
    src_cam = np.asarray(src_cam, f32)
    K, E = src_cam[1, :3, :3].astype(np.float64), src_cam[0].astype(np.float64)
    Ki, Ei = inv(K), inv(E)
    a, b = np.zeros((4, 4)), np.zeros((4, 4))
    E32, Eri32, Er32, Ei32 = (m.astype(f32).astype(np.float64) for m in (E, Eri, Er, Ei))
    for r in range(4):
        for c in range(4):
            sa = sb = np.float64(0.0)
            for k in range(4):
                sa = sa + E32[r, k] * Eri32[k, c]
                sb = sb + Er32[r, k] * Ei32[k, c]
            a[r, c], b[r, c] = sa, sb
    return {"K": K.astype(f32).reshape(-1), "Ki": Ki.astype(f32).reshape(-1), "E": a.astype(f32).reshape(-1),
            "Ei": b.astype(f32).reshape(-1), "raw64": np.concatenate([Ki.reshape(-1), Ei.reshape(-1), Eri.reshape(-1), a.reshape(-1), b.reshape(-1)])}


def _lift_mats(A, m):
    return {k: [A.lift(v) for v in m[k]] for k in ("K", "Ki", "E", "Ei")}


# ---------------------------------------------------------------------------------------------------------------------------
# T&T branch: the point transforms, in the source's operation order (fusion.hip:84-126)
# ---------------------------------------------------------------------------------------------------------------------------
def mul3(M, x, y, z):
    return (M[0] * x + M[1] * y + M[2] * z, M[3] * x + M[4] * y + M[5] * z, M[6] * x + M[7] * y + M[8] * z)


def mul4(M, p):
    x, y, z, w = p
    return (M[0] * x + M[1] * y + M[2] * z + M[3] * w, M[4] * x + M[5] * y + M[6] * z + M[7] * w,
            M[8] * x + M[9] * y + M[10] * z + M[11] * w, M[12] * x + M[13] * y + M[14] * z + M[15] * w)


def img2cam(A, Kinv, u, v, depth, exact, z=None):
    one, eps = A.lift(1.0), A.lift(1e-9)
    c = mul3(Kinv, u, v, one if z is None else z)
    d = c[2] + eps
    if exact:
        return (c[0] / d * depth, c[1] / d * depth, c[2] / d * depth, one)
    r = one / d
    return (c[0] * r * depth, c[1] * r * depth, c[2] * r * depth, one)


def xform(A, M, p, exact):
    q = mul4(M, p)
    d = q[3] + A.lift(1e-9)
    if exact:
        return (q[0] / d, q[1] / d, q[2] / d, q[3] / d)
    r = A.lift(1.0) / d
    return (q[0] * r, q[1] * r, q[2] * r, q[3] * r)


def cam2img(A, K, c, exact):
    d = c[3] + A.lift(1e-9)
    if exact:
        i = mul3(K, c[0] / d, c[1] / d, c[2] / d)
        e = i[2] + A.lift(1e-9)
        return (i[0] / e, i[1] / e, i[2] / e)
    r = A.lift(1.0) / d
    i = mul3(K, c[0] * r, c[1] * r, c[2] * r)
    e = A.lift(1.0) / (i[2] + A.lift(1e-9))
    return (i[0] * e, i[1] * e, i[2] * e)


def _unnormalise(A, u, size):
    """sample_bilinear_zero's round trip (fusion.hip:130-131): u / ((size-1)/2) - 1, then ((g + 1) / 2) * (size-1)."""
    g = u / (A.lift(size - 1) / A.lift(2.0)) - A.lift(1.0)
    return ((g + A.lift(1.0)) / A.lift(2.0)) * A.lift(size - 1)


def sample_f32(img, h, w, u, v, clamp=False):
    """sample_bilinear_zero restated in float32; clamp=True: the mutant that replicates the border instead of padding with zeros."""
    one = f32(1.0)
    with np.errstate(all="ignore"):
        ix, iy = _unnormalise(F32, u, w), _unnormalise(F32, v, h)
        fx, fy = np.floor(ix), np.floor(iy)
        x0 = np.nan_to_num(fx, nan=-4.0).clip(-4, w + 4).astype(np.int64)
        y0 = np.nan_to_num(fy, nan=-4.0).clip(-4, h + 4).astype(np.int64)
        tx, ty = ix - fx, iy - fy

        def at(yy, xx):
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            val = img[yy.clip(0, h - 1), xx.clip(0, w - 1)]
            return val if clamp else np.where(ok, val, f32(0.0))
        nw, ne, sw, se = (one - tx) * (one - ty), tx * (one - ty), (one - tx) * ty, tx * ty
        return at(y0, x0) * nw + at(y0, x0 + 1) * ne + at(y0 + 1, x0) * sw + at(y0 + 1, x0 + 1) * se


def bilinear_zero64(img64, h, w, x, y):
    """Zero-padded bilinear interpolation in float64 at positions clamped to [-2, size + 1] (beyond: every tap is outside anyway)."""
    x, y = np.clip(x, -2.0, w + 1.0), np.clip(y, -2.0, h + 1.0)
    x0, y0 = np.floor(x), np.floor(y)
    tx, ty = x - x0, y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def at(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return np.where(ok, img64[yy.clip(0, h - 1), xx.clip(0, w - 1)], 0.0)
    return at(y0, x0) * (1 - tx) * (1 - ty) + at(y0, x0 + 1) * tx * (1 - ty) + at(y0 + 1, x0) * (1 - tx) * ty + at(y0 + 1, x0 + 1) * tx * ty


def sample_bound(img, h, w, u, v):
    """Bound of sample_bilinear_zero at the bounded coordinates (u, v).  Range over the box as interval_ref does; the blend's own
    roundings: each weight is a product of two factors that carry one subtraction each (3u), its product with the tap (u), and three
    sums of partial sums no larger than the sum of magnitudes (3u): 7u, taken as 8u of the largest sum of magnitudes over the box."""
    ix, iy = _unnormalise(BND, u, w), _unnormalise(BND, v, h)
    img64 = np.asarray(img, np.float64)
    aimg = np.abs(img64)
    wide = ~((ix.e < 0.5) & (iy.e < 0.5))                      # more than one lattice line per axis inside the box: left out
    ex, ey = np.where(wide, 0.0, ix.e), np.where(wide, 0.0, iy.e)
    px = [ix.m - ex, ix.m + ex, np.clip(np.round(ix.m), ix.m - ex, ix.m + ex)]
    py = [iy.m - ey, iy.m + ey, np.clip(np.round(iy.m), iy.m - ey, iy.m + ey)]
    vals = np.stack([bilinear_zero64(img64, h, w, x, y) for x in px for y in py])
    mags = np.stack([bilinear_zero64(aimg, h, w, x, y) for x in px for y in py]).max(0)
    lo, hi = vals.min(0), vals.max(0)
    e = 0.5 * (hi - lo) + 8.0 * U32 * mags * (1.0 + 2.0 ** -10)
    # every tap of every point of the box is outside the image (floor(ix) <= -2 or >= size): the kernel's sample is exactly 0,
    # however wide the box
    outside = (ix.m + ix.e < -1.0) | (ix.m - ix.e >= w) | (iy.m + iy.e < -1.0) | (iy.m - iy.e >= h)
    return B(np.where(outside, 0.0, 0.5 * (lo + hi)), np.where(outside, 0.0, np.where(wide, np.inf, e)))


def pixel_grid(h, w):
    p = np.arange(h * w)
    return p // w, p % w


def tt_chain(A, ref_depth, src_depths, mats, relative, mutant=None):
    """FusDynamic::pixel (fusion.hip) up to the comparisons, for all pixels at once.  mats: prepare_view of the
    reference view, then of the sources.  -> dict of per-view lists (reprojected x, y, depth; cdiff; ddiff) and the pixel's own."""
    h, w = ref_depth.shape
    ys, xs = pixel_grid(h, w)
    off = 0.0 if mutant == "half_pixel_dropped" else 0.5
    u, vv = A.lift(xs + off), A.lift(ys + off)
    dref = A.lift(ref_depth.reshape(-1))
    Mr = _lift_mats(A, mats[0])
    ref_pt = img2cam(A, Mr["Ki"], u, vv, dref, True)
    world = xform(A, Mr["Ei"], ref_pt, True)
    out = {"u": u, "v": vv, "dref": dref, "x": [], "y": [], "d": [], "cdiff": [], "ddiff": [], "src_xy": [], "sample": [], "ref_pt": ref_pt,
           "world": world}
    for s, src in enumerate(src_depths):
        Ms = _lift_mats(A, mats[s + 1])
        c = xform(A, Ms["E"], world, True)
        im = cam2img(A, Ms["K"], c, True)
        if A is F32:
            ds = sample_f32(np.asarray(src, f32), h, w, im[0], im[1], clamp=(mutant == "border_clamp"))
        else:
            ds = sample_bound(src, h, w, im[0], im[1])
        sc = img2cam(A, Ms["Ki"], im[0], im[1], ds, False)
        sw = xform(A, Ms["Ei"], sc, False)
        rc = xform(A, Mr["E"], sw, False)
        ri = cam2img(A, Mr["K"], rc, False)
        dx, dy = ri[0] - u, ri[1] - vv
        cdiff = A.sqrt(dx * dx + dy * dy)
        ddiff = A.abs(dref - rc[2])
        if relative and mutant != "relative_ignored":
            ddiff = ddiff / dref
        for k, val in (("x", ri[0]), ("y", ri[1]), ("d", rc[2]), ("cdiff", cdiff), ("ddiff", ddiff), ("src_xy", (im[0], im[1])), ("sample", ds)):
            out[k].append(val)
    return out


def tt_thresholds(V, dh, dist_base, rel_base):
    """step / dist_base and step / rel_base as the fp32 quotients the kernel forms (fusion.hip:184-185)."""
    steps = [f32(dh + k) for k in range(V + 1 - dh)]
    return [s / f32(dist_base) for s in steps], [s / f32(rel_base) for s in steps]


def prob_mask_exact(conf, h, w, prob_thr, rounded=False):
    """The nearest-neighbour confidence look-up of fusion.hip:200-204, bit for bit: floorf(y * (ch / h)) in fp32, clamped."""
    if conf is None:
        return np.ones(h * w, bool)
    conf = np.asarray(conf, f32)
    ch, cw = conf.shape
    ys, xs = pixel_grid(h, w)
    fy, fx = ys.astype(f32) * (f32(ch) / f32(h)), xs.astype(f32) * (f32(cw) / f32(w))
    fn = np.rint if rounded else np.floor
    sy, sx = np.minimum(fn(fy).astype(np.int64), ch - 1), np.minimum(fn(fx).astype(np.int64), cw - 1)
    return conf[sy, sx] > f32(prob_thr)


def tt_restate(ref_depth, src_depths, ref_cam, src_cams, conf=None, prob_thr=0.0, dh=2, dist_base=4.0, rel_base=1300.0,
               relative=False, mutant=None, mats=None):
    """FusDynamic::pixel op for op in numpy float32.  -> dict(depth [n], geo / prob / mask [n] bool, points [3,n],
    xyd [V,3,n], m [V,nthr,n] bool).  mutant: None or one of the T&T names of MUTANTS."""
    ref_depth, src_depths = np.asarray(ref_depth, f32), np.asarray(src_depths, f32)
    h, w = ref_depth.shape
    V = len(src_depths)
    if mats is None:
        mats = [prepare_view(ref_cam)] + [prepare_view(c) for c in src_cams]
    with np.errstate(all="ignore"):
        ch = tt_chain(F32, ref_depth, src_depths, mats, relative, mutant)
        thr_c, thr_d = tt_thresholds(V, dh, dist_base, rel_base)
        nthr = V + 1 - dh
        lt = np.less_equal if mutant == "le_for_lt" else np.less
        m = np.stack([np.stack([lt(ch["cdiff"][s], thr_c[k]) & lt(ch["ddiff"][s], thr_d[k]) for k in range(nthr)]) for s in range(V)])
        if mutant == "run16_dropped":                          # one 16-pixel run of view 0's contribution to the loosest threshold
            p0 = (h // 2) * w + max(0, (w - 16) // 2)
            m[0, nthr - 1, p0:p0 + 16] = False
        counts = m.sum(0)
        vis = m[:, nthr - 2 if (mutant == "vis_second_loosest" and nthr >= 2) else nthr - 1]
        dsum, nvis = np.zeros(h * w, f32), vis.sum(0)
        for s in range(V):
            dsum = np.where(vis[s], dsum + ch["d"][s], dsum)
        div = f32(V + 1) if mutant == "average_by_v_plus_1" else (nvis + 1).astype(f32)
        davg = (dsum + ch["dref"]) / div
        need = dh + np.arange(nthr) + (1 if mutant == "count_ge_plus_1" else 0)
        geo = (counts >= need[:, None]).any(0)
        prob = prob_mask_exact(conf, h, w, prob_thr, rounded=(mutant == "conf_index_rounded"))
        Mr = _lift_mats(F32, mats[0])
        pw = xform(F32, Mr["Ei"], img2cam(F32, Mr["Ki"], ch["u"], ch["v"], davg, True), True)
    return {"depth": davg, "geo": geo, "prob": prob, "mask": geo & prob, "points": np.stack(pw[:3]),
            "xyd": np.stack([np.stack([ch["x"][s], ch["y"][s], ch["d"][s]]) for s in range(V)]), "m": m}


def _tri(val, thr):
    """(true, false) of `val < thr` for a bounded value against an exact threshold; neither: undecided."""
    return val.hi < thr, val.lo >= thr


def union_average(vals, Tm, Um, finish):
    """The interval of  finish(sum in view order of vals[s] over the included views, their number)  where the included set is
    {decided true} plus ANY subset of the undecided views: the union over the 2^j admissible sets, j <= JMAX (more: left out).
    -> (lo, hi, j)."""
    V, n = Tm.shape

    def run(inc, idx):
        sm, se = np.zeros(len(idx)), np.zeros(len(idx))
        for s in range(V):
            t_ = B(sm, se) + vals[s][idx]
            sm, se = np.where(inc[s], t_.m, sm), np.where(inc[s], t_.e, se)
        return finish(B(sm, se), inc.sum(0), idx)
    base = run(Tm, np.arange(n))
    lo, hi = base.lo.copy(), base.hi.copy()
    j = Um.sum(0)
    und = np.nonzero(j > 0)[0]
    if len(und):
        rank = np.cumsum(Um[:, und], 0) - 1
        for b in range(1, 2 ** int(min(j.max(), JMAX))):
            inc = Tm[:, und] | (Um[:, und] & (((b >> np.clip(rank, 0, JMAX - 1)) & 1) == 1))
            r = run(inc, und)
            lo[und], hi[und] = np.minimum(lo[und], r.lo), np.maximum(hi[und], r.hi)
    lo[j > JMAX], hi[j > JMAX] = -np.inf, np.inf
    return lo, hi, j


def _from_range(lo, hi):
    with np.errstate(all="ignore"):
        return B(0.5 * (lo + hi), 0.5 * (hi - lo))


class Decision:
    """A mask with its decided set: value where decided, anything where not."""

    def __init__(self, lo, hi):
        self.value, self.decided = lo, lo == hi


def tt_reference(ref_depth, src_depths, ref_cam, src_cams, conf=None, prob_thr=0.0, dh=2, dist_base=4.0, rel_base=1300.0,
                 relative=False):
    """The float64 interval reference of FusDynamic::pixel.  -> dict: xyd B [V][3], T / Un [V,nthr,n] (comparison true /
    undecided), left [V,n] (left-out views), geo / mask Decision, prob bool (pinned), depth B, points [3] B, nund [n] (undecided
    views of the averaging set), near: (value - threshold, bound) of every component comparison, for the bite statistics."""
    ref_depth, src_depths = np.asarray(ref_depth, f32), np.asarray(src_depths, f32)
    h, w = ref_depth.shape
    V = len(src_depths)
    mats = [prepare_view(ref_cam)] + [prepare_view(c) for c in src_cams]
    ch = tt_chain(BND, ref_depth, src_depths, mats, relative)
    thr_c, thr_d = tt_thresholds(V, dh, dist_base, rel_base)
    nthr, n = V + 1 - dh, h * w
    T, Un = np.zeros((V, nthr, n), bool), np.zeros((V, nthr, n), bool)
    near = []
    for s in range(V):
        for k in range(nthr):
            ct, cf = _tri(ch["cdiff"][s], np.float64(thr_c[k]))
            dt, df = _tri(ch["ddiff"][s], np.float64(thr_d[k]))
            T[s, k] = ct & dt
            Un[s, k] = ~(T[s, k] | cf | df)
            near.append((ch["cdiff"][s].m - np.float64(thr_c[k]), ch["cdiff"][s].e, ct | cf))
            near.append((ch["ddiff"][s].m - np.float64(thr_d[k]), ch["ddiff"][s].e, dt | df))
    left = np.stack([~(np.isfinite(ch["cdiff"][s].e) & np.isfinite(ch["ddiff"][s].e)) for s in range(V)])
    need = (dh + np.arange(nthr))[:, None]
    geo_lo, geo_hi = (T.sum(0) >= need).any(0), ((T | Un).sum(0) >= need).any(0)
    prob = prob_mask_exact(conf, h, w, prob_thr)
    geo, mask = Decision(geo_lo, geo_hi), Decision(geo_lo & prob, geo_hi & prob)
    dref = ch["dref"]
    lo, hi, nund = union_average(ch["d"], T[:, nthr - 1], Un[:, nthr - 1], lambda sm, cnt, idx: (sm + dref[idx]) / B((cnt + 1).astype(np.float64)))
    depth = _from_range(lo, hi)
    Mr = _lift_mats(BND, mats[0])
    pts = xform(BND, Mr["Ei"], img2cam(BND, Mr["Ki"], ch["u"], ch["v"], depth, True), True)[:3]
    return {"xyd": [[ch["x"][s], ch["y"][s], ch["d"][s]] for s in range(V)], "T": T, "Un": Un, "left": left, "geo": geo, "mask": mask,
            "prob": prob, "depth": depth, "points": list(pts), "nund": nund, "near": near, "chain": ch}


def vis_filter_f32(ref_depth, xyd, dist_base, rel_base, thres, relative, mutant=None):
    """fusion_vis_filter_kernel restated in float32: its inputs are given, its arithmetic (two subtractions, two products, a sum, a
    correctly rounded sqrtf, an IEEE quotient) restates exactly, so EVERY element is pinned.  ref_depth [h,w]; xyd [V,3,h,w]
    -> masks [V, V+1-thres, h, w] bool."""
    ref_depth, xyd = np.asarray(ref_depth, f32), np.asarray(xyd, f32)
    V, _, h, w = xyd.shape
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    u, vv = xs.astype(f32) + f32(0.5), ys.astype(f32) + f32(0.5)
    lt = np.less_equal if mutant == "le_for_lt" else np.less
    out = np.zeros((V, V + 1 - thres, h, w), bool)
    with np.errstate(all="ignore"):
        for s in range(V):
            dx, dy = xyd[s, 0] - u, xyd[s, 1] - vv
            cdiff = np.sqrt(dx * dx + dy * dy)
            ddiff = np.abs(ref_depth - xyd[s, 2])
            if relative and mutant != "relative_ignored":
                ddiff = ddiff / ref_depth
            for k in range(V + 1 - thres):
                step = f32(thres + k)
                out[s, k] = lt(cdiff, step / f32(dist_base)) & lt(ddiff, step / f32(rel_base))
    return out


def points_chain(A, mode, pts, cam, depth=None):
    """fusion_points_kernel<MODE> (fusion.hip:551-572) for one camera: pts [n, 3 or 4] -> tuple of 4 (3 for mode 3) components."""
    m = _lift_mats(A, prepare_view(cam))
    q = [A.lift(pts[:, i]) for i in range(pts.shape[1])]
    if mode == 0:
        return img2cam(A, m["Ki"], q[0], q[1], A.lift(depth), True, z=q[2])
    if mode in (1, 2):
        return xform(A, m["Ei" if mode == 1 else "E"], tuple(q), True)
    return cam2img(A, m["K"], tuple(q), True)


# ---------------------------------------------------------------------------------------------------------------------------
# DTU branch (fusion.hip:312-501): the chain in double, rounded to fp32 where the kernel rounds
# ---------------------------------------------------------------------------------------------------------------------------
class F64:
    """The DTU restatement's arithmetic: numpy float64, with the kernel's float32 islands."""
    @staticmethod
    def lift(x):
        return np.asarray(np.asarray(x, f32), np.float64)

    @staticmethod
    def r32(x):
        with np.errstate(all="ignore"):
            return np.asarray(x, np.float64).astype(f32).astype(np.float64)

    @staticmethod
    def sub32(a, b):
        return (np.asarray(a, f32) - np.asarray(b, f32)).astype(np.float64)
    sqrt = staticmethod(np.sqrt)
    abs = staticmethod(np.abs)


class BND64(BND):
    exact = staticmethod(lambda x: B(np.asarray(x, np.float64)))

    @staticmethod
    def r32(x):
        return x.round32()

    @staticmethod
    def sub32(a, b):
        with unit(U32):
            return a - b


def dmul3(M, x, y, z):
    return (M[0] * x + M[1] * y + M[2] * z, M[3] * x + M[4] * y + M[5] * z, M[6] * x + M[7] * y + M[8] * z)


def dmul4_xyz(M, p):
    return (M[0] * p[0] + M[1] * p[1] + M[2] * p[2] + M[3], M[4] * p[0] + M[5] * p[1] + M[6] * p[2] + M[7],
            M[8] * p[0] + M[9] * p[1] + M[10] * p[2] + M[11])


def _cv_cell(x32, mutant=None):
    """cv_remap_linear's fix(): rint(x * 32) (x an fp32 value, the product exact in double) -> (cell, fraction index)."""
    with np.errstate(all="ignore"):
        f = np.asarray(x32, np.float64) * 32.0
        f = np.where(np.isnan(f), -2147483648.0, np.clip(f, -2147483648.0, 2147483647.0))
        s = (np.floor(f) if mutant == "floor_for_rint" else np.rint(f)).astype(np.int64)
    return np.clip(s >> 5, -32768, 32767), s & 31


def cv_remap_f32(img, h, w, mx, my, mutant=None):
    """cv_remap_linear (fusion.hip:324-338) in float32: weights k/32 and their products exact, four products, three sums."""
    img = np.asarray(img, f32)
    one = f32(1.0)

    def at(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return np.where(ok, img[yy.clip(0, h - 1), xx.clip(0, w - 1)], f32(0.0))
    if mutant == "quantisation_dropped":                      # plain bilinear at the unquantised coordinate
        with np.errstate(all="ignore"):
            mx, my = np.nan_to_num(np.asarray(mx, f32), nan=-4.0).clip(-4, w + 4), np.nan_to_num(np.asarray(my, f32), nan=-4.0).clip(-4, h + 4)
            fx, fy = np.floor(mx), np.floor(my)
            x0, y0, tx, ty = fx.astype(np.int64), fy.astype(np.int64), mx - fx, my - fy
    else:
        (x0, ax), (y0, ay) = _cv_cell(mx, mutant), _cv_cell(my, mutant)
        tx, ty = ax.astype(f32) * f32(1.0 / 32.0), ay.astype(f32) * f32(1.0 / 32.0)
    wx0, wy0 = one - tx, one - ty
    return (at(y0, x0) * (wy0 * wx0) + at(y0, x0 + 1) * (wy0 * tx) + at(y0 + 1, x0) * (ty * wx0) + at(y0 + 1, x0 + 1) * (ty * tx)).astype(f32)


def cv_remap_bound(img, h, w, bx, by):
    """The admissible values of cv_remap_linear at fp32 coordinates that are one or two admissible values each: rint(x * 32) is a true
    jump, so each axis has one or two admissible cells; per cell pair the blend is bounded (weights exact, four products and three sums
    in fp32, charged by the B operations), and the result is the union."""
    img = np.asarray(img, f32)

    def at(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return B(np.where(ok, img[yy.clip(0, h - 1), xx.clip(0, w - 1)], f32(0.0)).astype(np.float64))
    lo = hi = None
    with unit(U32):
        for x32 in bx.ends():
            for y32 in by.ends():
                (x0, ax), (y0, ay) = _cv_cell(x32), _cv_cell(y32)
                tx, ty = ax / 32.0, ay / 32.0
                v = at(y0, x0) * B((1 - ty) * (1 - tx)) + at(y0, x0 + 1) * B((1 - ty) * tx) + at(y0 + 1, x0) * B(ty * (1 - tx)) \
                    + at(y0 + 1, x0 + 1) * B(ty * tx)
                lo, hi = (v.lo, v.hi) if lo is None else (np.minimum(lo, v.lo), np.maximum(hi, v.hi))
    e = np.where(np.isfinite(bx.e) & np.isfinite(by.e), 0.5 * (hi - lo), np.inf)
    return B(0.5 * (lo + hi), e)


def dtu_reproject(A, Mr, Ms, src, h, w, xd, yd, dref, mutant=None):
    """dtu_reproject_pixel (fusion.hip:347-367).  -> dict x_src y_src samp depth_rep x_rep y_rep (fp32 values held in the arithmetic's type)."""
    xyz = dmul3(Mr["Ki"], xd * dref, yd * dref, dref)
    xs = dmul4_xyz(Ms["E"], xyz)
    kx = dmul3(Ms["K"], xs[0], xs[1], xs[2])
    u, v = kx[0] / kx[2], kx[1] / kx[2]
    x_src, y_src = A.r32(u), A.r32(v)
    if A is F64:
        samp = cv_remap_f32(src, h, w, x_src, y_src, mutant).astype(np.float64)
    else:
        samp = cv_remap_bound(src, h, w, x_src, y_src)
    s3 = dmul3(Ms["Ki"], u * samp, v * samp, samp)
    rp = dmul4_xyz(Ms["Ei"], s3)
    kr = dmul3(Mr["K"], rp[0], rp[1], rp[2])
    krz = np.where(kr[2] == 0.0, kr[2] + 0.00001, kr[2]) if A is F64 else kr[2]
    return {"x_src": x_src, "y_src": y_src, "samp": samp, "depth_rep": A.r32(rp[2]), "x_rep": A.r32(kr[0] / krz), "y_rep": A.r32(kr[1] / krz)}


def dtu_thresholds(A, s_lo, e_hi, dist_base, diff_base, mutant=None):
    """thr_dist[k] = i * dist_base (exact in double), thr_diff[k] = (float)(log(max(i, 1.05)) / log(10) * diff_base): the device's
    double log is taken as correct to NEAR relative, so the fp32 value is pinned unless the double lies that close to a boundary."""
    dist, diff, two = [], [], 0
    for i in range(s_lo, e_hi):
        dist.append(np.float64(i) * np.float64(f32(dist_base)))
        arg = np.float64(i) if mutant == "log_floor_dropped" else max(np.float64(i), 1.05)
        val = np.log(arg) / np.log(10.0) * np.float64(f32(diff_base))
        if A is F64:
            diff.append(np.float64(f32(val)))
        else:
            b = B(val, 0.0).round32()
            two += int(b.e > 0)
            diff.append(b)
    return dist, diff, two


def _dtu_mats(A, ref_cam, src_cams, inv=gauss_jordan):
    return [_lift_mats(A, dtu_prepare_view(ref_cam, None, inv))] + [_lift_mats(A, dtu_prepare_view(ref_cam, c, inv)) for c in src_cams]


def dtu_restate(ref_depth, src_depths, ref_cam, src_cams, conf=None, conf_thr=0.5, conf_keep=0.75, s_lo=1, e_hi=11, dist_base=0.5,
                diff_base=0.25, mutant=None):
    """FusDtu::pixel op for op (float64 chain, float32 islands).  -> dict(depth f32 [n], photo / geo / final bool, points
    f32 [3,n], out5 [V,5,n] f32 (reproject outputs per view, unzeroed), masks [V,nthr,n] bool)."""
    ref_depth, src_depths = np.asarray(ref_depth, f32), np.asarray(src_depths, f32)
    h, w = ref_depth.shape
    V, n, nthr = len(src_depths), h * w, e_hi - s_lo
    mats = _dtu_mats(F64, ref_cam, src_cams, _inv32 if mutant == "inverse_fp32" else gauss_jordan)
    ys, xs = pixel_grid(h, w)
    xd, yd, dref = xs.astype(np.float64), ys.astype(np.float64), F64.lift(ref_depth.reshape(-1))
    thr_dist, thr_diff, _ = dtu_thresholds(F64, s_lo, e_hi, dist_base, diff_base, mutant)
    num, nlast, counts = np.zeros(n, f32), np.zeros(n, np.int64), np.zeros((nthr, n), np.int64)
    out5, masks = [], []
    with np.errstate(all="ignore"):
        for sv in range(V):
            r = dtu_reproject(F64, mats[0], mats[sv + 1], src_depths[sv], h, w, xd, yd, dref, mutant)
            dxr, dyr = r["x_rep"] - xd, r["y_rep"] - yd
            dist = np.sqrt(dxr * dxr + dyr * dyr)
            ddiff = np.abs(F64.sub32(r["depth_rep"], dref))
            m = np.stack([(dist < thr_dist[k]) & (ddiff < thr_diff[k]) for k in range(nthr)])
            counts += m
            num = np.where(m[-1], num + r["depth_rep"].astype(f32), num)
            nlast += m[-1]
            out5.append(np.stack([r[k] for k in ("depth_rep", "x_rep", "y_rep", "x_src", "y_src")]).astype(f32))
            masks.append(m)
        davg = (num + dref.astype(f32)).astype(np.float64) / (nlast + 1).astype(np.float64)
        c = np.ones(n, f32) if conf is None else np.asarray(conf, f32).reshape(-1)
        if mutant != "conf_keep_ignored":
            davg = np.where(c > f32(conf_keep), dref, davg)
        geo = nlast >= e_hi
        geo = geo | (counts >= (s_lo + np.arange(nthr))[:, None]).any(0)
        photo = c > f32(conf_thr)
        pc = dmul3(mats[0]["Ki"], xd * davg, yd * davg, davg)
        pw = dmul4_xyz(mats[0]["Ei"], pc)
    return {"depth": davg.astype(f32), "photo": photo, "geo": geo, "final": photo & geo, "points": np.stack(pw).astype(f32),
            "out5": np.stack(out5), "masks": np.stack(masks)}


def dtu_zeroed(out5, masks, mutant=None):
    """check_geometric_consistency's outputs from reproject's: the first three zeroed where the LAST mask is false (fusion.hip:494)."""
    out = out5.copy()
    if mutant != "zeroing_left_out":
        out[:3, ~masks[-1]] = 0.0
    return out


def dtu_reference(ref_depth, src_depths, ref_cam, src_cams, conf=None, conf_thr=0.5, conf_keep=0.75, s_lo=1, e_hi=11, dist_base=0.5,
                  diff_base=0.25):
    """The interval reference of the DTU branch.  -> dict like tt_reference: out5 [V][5] B (unzeroed), T / Un [V,nthr,n], geo / final
    Decision, photo bool (pinned), depth B (fp32 values: half = 0 is a pinned element), points [3] B, log_two: thresholds whose
    fp32 value has two admissible neighbours."""
    ref_depth, src_depths = np.asarray(ref_depth, f32), np.asarray(src_depths, f32)
    h, w = ref_depth.shape
    V, n, nthr = len(src_depths), h * w, e_hi - s_lo
    ys, xs = pixel_grid(h, w)
    near = []
    with unit(U64):
        mats = _dtu_mats(BND64, ref_cam, src_cams)
        xd, yd, dref = BND64.exact(xs), BND64.exact(ys), BND64.lift(ref_depth.reshape(-1))
        thr_dist, thr_diff, log_two = dtu_thresholds(BND64, s_lo, e_hi, dist_base, diff_base)
        T, Un = np.zeros((V, nthr, n), bool), np.zeros((V, nthr, n), bool)
        out5, dreps = [], []
        for sv in range(V):
            r = dtu_reproject(BND64, mats[0], mats[sv + 1], src_depths[sv], h, w, xd, yd, dref)
            dxr, dyr = r["x_rep"] - xd, r["y_rep"] - yd
            dist = (dxr * dxr + dyr * dyr).sqrt()
            dist = B(dist.m, np.maximum(dist.e, NEAR * np.abs(dist.m)))
            ddiff = BND64.sub32(r["depth_rep"], dref).abs()
            for k in range(nthr):
                ct, cf = _tri(dist, thr_dist[k])
                dt, df = ddiff.hi < thr_diff[k].ends()[0], ddiff.lo >= thr_diff[k].ends()[1]
                T[sv, k] = ct & dt
                Un[sv, k] = ~(T[sv, k] | cf | df)
                near.append((dist.m - thr_dist[k], dist.e, ct | cf))
                near.append((ddiff.m - thr_diff[k].m, ddiff.e + thr_diff[k].e, dt | df))
            out5.append([r[k] for k in ("depth_rep", "x_rep", "y_rep", "x_src", "y_src")])
            dreps.append(r["depth_rep"])
        need = (s_lo + np.arange(nthr))[:, None]
        lastT, lastU = T[:, -1], Un[:, -1]
        geo_lo = (lastT.sum(0) >= e_hi) | (T.sum(0) >= need).any(0)
        geo_hi = ((lastT | lastU).sum(0) >= e_hi) | ((T | Un).sum(0) >= need).any(0)
        c = np.ones(n, f32) if conf is None else np.asarray(conf, f32).reshape(-1)
        photo, keep = c > f32(conf_thr), c > f32(conf_keep)
        geo, final = Decision(geo_lo, geo_hi), Decision(geo_lo & photo, geo_hi & photo)

        def finish(sm, cnt, idx):
            with unit(U32):
                tot = sm + dref[idx]
            with unit(U64):
                return tot / B((cnt + 1).astype(np.float64))
        with unit(U32):
            lo, hi, nund = union_average(dreps, lastT, lastU, finish)
        lo, hi = np.where(keep, dref.m, lo), np.where(keep, dref.m, hi)
        nund = np.where(keep, 0, nund)
        davg = _from_range(lo, hi)
        pc = dmul3(mats[0]["Ki"], xd * davg, yd * davg, davg)
        pw = dmul4_xyz(mats[0]["Ei"], pc)
        # a wide davg (undecided set) makes round32's two ends the hull of the admissible fp32 values
        depth, points = davg.round32(), [p.round32() for p in pw]
    return {"out5": out5, "T": T, "Un": Un, "geo": geo, "final": final, "photo": photo, "depth": depth, "points": points, "nund": nund,
            "near": near, "log_two": log_two}


# ---------------------------------------------------------------------------------------------------------------------------
# the assertions
# ---------------------------------------------------------------------------------------------------------------------------
class Stats:
    """Accumulates one family's record: checks, largest share of an interval used, pinned, left-out, bitwise share."""

    def __init__(self, family):
        self.family, self.checks, self.used, self.pinned, self.left, self.tight, self.nonpinned = family, 0, 0.0, 0, 0, 0, 0
        self.bit_same, self.bit_all, self.und_cmp, self.cmp, self.und_pix, self.pix = 0, 0, 0, 0, 0, 0
        self.near_true, self.near_false = 0, 0

    def line(self):
        bit = f"{self.bit_same / self.bit_all:.6f}" if self.bit_all else "n/a"
        return (f"[fusion-bound] {self.family:18s} checks={self.checks} used={self.used:.3f} pinned={self.pinned} "
                f"undecided_cmp={self.und_cmp}/{self.cmp} undecided_pix={self.und_pix}/{self.pix} left_out={self.left} "
                f"tight={self.tight}/{self.nonpinned} near_thr_true={self.near_true} near_thr_false={self.near_false} bitwise={bit}")


def check_elements(name, got, b, st, restated=None, either_zero=None):
    """Every element of `got` inside [m - e, m + e] (exactly m where e = 0); e = inf: left out, counted.  either_zero: elements that
    may instead be exactly 0 (an undecided zeroing mask).  restated: the fp32 restatement, for the recorded bitwise share."""
    g = np.asarray(got, np.float64).reshape(-1)
    m, e = b.m.reshape(-1), b.e.reshape(-1)
    assert g.shape == m.shape, f"{name}: {g.shape} vs {m.shape}"
    left = ~np.isfinite(e)
    with np.errstate(all="ignore"):
        ok = (g >= b.lo.reshape(-1)) & (g <= b.hi.reshape(-1))
        ok = np.where(e == 0, g == m, ok)
    inside = ok
    if either_zero is not None:
        ok = ok | (either_zero.reshape(-1) & (g == 0))
    bad = ~ok & ~left
    with np.errstate(all="ignore"):
        used = np.where(left | (e == 0) | ~inside, 0.0, np.abs(g - m) / e)
    st.checks += g.size
    st.used = max(st.used, float(used.max()) if g.size else 0.0)
    st.pinned += int((e == 0).sum())
    st.left += int(left.sum())
    live = ~left & (e > 0)
    st.nonpinned += int(live.sum())
    st.tight += int((e[live] <= 2.0 ** -10 * np.abs(m[live])).sum())
    if restated is not None:
        r = np.asarray(restated, f32).reshape(-1)
        st.bit_same += int((np.asarray(got, f32).reshape(-1).view(np.uint32) == r.view(np.uint32)).sum())
        st.bit_all += g.size
    assert not bad.any(), f"{name}: {int(bad.sum())} of {g.size} elements outside their interval; first: " + "; ".join(
        f"[{i}] got={g[i]:.9g} mid={m[i]:.9g} half={e[i]:.3g}" for i in np.nonzero(bad)[0][:8])
    return int(bad.sum())


def check_mask(name, got, value, decided, st=None):
    """Every DECIDED pixel of a mask equals its value."""
    g = np.asarray(got).reshape(-1).astype(bool)
    bad = decided.reshape(-1) & (g != value.reshape(-1))
    if st is not None:
        st.checks += g.size
    assert not bad.any(), f"{name}: {int(bad.sum())} decided pixels of {g.size} are wrong; first: {np.nonzero(bad)[0][:8].tolist()}"


def count_decisions(ref, st, geo_key="geo", final_key="mask"):
    """Adds a reference's undecided / left-out comparisons and pixels and its near-threshold decided comparisons to the record."""
    st.cmp += ref["Un"].size
    st.und_cmp += int(ref["Un"].sum())
    und_pix = ~ref[geo_key].decided | ~ref[final_key].decided | (ref["nund"] > 0)
    st.pix += und_pix.size
    st.und_pix += int(und_pix.sum())
    for diff, e, decided in ref["near"]:
        with np.errstate(all="ignore"):
            close = decided & np.isfinite(e) & (np.abs(diff) <= 32.0 * e)
        st.near_true += int((close & (diff < 0)).sum())
        st.near_false += int((close & (diff >= 0)).sum())
    return int(ref["Un"].sum()) / ref["Un"].size, float(und_pix.mean())


CAP_COMPARISONS = 0.005        # undecided + left-out comparisons, share of a case's (pixel, view, threshold) triples
CAP_PIXELS = 0.01              # pixels whose geo / mask / final decision or averaging set is undecided, share of a case's pixels

# structural mutants: name -> (branch, the form that can express it)
MUTANTS = {
    "run16_dropped": "tt", "count_ge_plus_1": "tt", "vis_second_loosest": "tt", "average_by_v_plus_1": "tt", "half_pixel_dropped": "tt",
    "border_clamp": "tt", "relative_ignored": "tt", "conf_index_rounded": "tt", "le_for_lt": "vis", "table_shifted": "scan",
    "quantisation_dropped": "dtu", "floor_for_rint": "dtu", "log_floor_dropped": "dtu", "conf_keep_ignored": "dtu",
    "zeroing_left_out": "dtu_reproject", "inverse_fp32": "dtu",
}


def assert_caps(name, ref, final_key="mask"):
    """The conditions of DESIGN 2.7 on the inputs, from the reference alone: they are asserted before any result is looked at."""
    cmp_share = float(ref["Un"].mean())
    und_pix = ~ref["geo"].decided | ~ref[final_key].decided | (ref["nund"] > 0)
    assert cmp_share <= CAP_COMPARISONS, f"{name}: {int(ref['Un'].sum())} of {ref['Un'].size} comparisons undecided or left out ({cmp_share:.5f})"
    assert float(und_pix.mean()) <= CAP_PIXELS, f"{name}: {int(und_pix.sum())} of {und_pix.size} pixels undecided ({und_pix.mean():.5f})"
    return und_pix


def check_tt_outputs(name, out, ref, st, restated=None):
    """out: dict of numpy arrays over the flattened pixels -- depth [n], geo / prob / mask [n], points [3,n] or None, xyd [V,3,n] or
    None -- against a tt_reference.  Every mask pixel that is decided, every continuous element."""
    assert_caps(name, ref)
    check_mask(f"{name} prob_mask", out["prob"], ref["prob"], np.ones_like(ref["prob"]), st)
    check_mask(f"{name} geo_mask", out["geo"], ref["geo"].value, ref["geo"].decided, st)
    check_mask(f"{name} mask", out["mask"], ref["mask"].value, ref["mask"].decided, st)
    rs = restated or {}
    check_elements(f"{name} depth", out["depth"], ref["depth"], st, rs.get("depth"))
    if out.get("points") is not None:
        for c in range(3):
            check_elements(f"{name} points[{c}]", out["points"][c], ref["points"][c], st, rs["points"][c] if restated else None)
    if out.get("xyd") is not None:
        for s, v in enumerate(ref["xyd"]):
            for c in range(3):
                check_elements(f"{name} reproj_xyd[{s},{c}]", out["xyd"][s, c], v[c], st, rs["xyd"][s, c] if restated else None)


def check_dtu_outputs(name, out, ref, st, restated=None):
    """out: depth [n], photo / geo / final [n], points [3,n] against a dtu_reference."""
    assert_caps(name, ref, "final")
    check_mask(f"{name} photo_mask", out["photo"], ref["photo"], np.ones_like(ref["photo"]), st)
    check_mask(f"{name} geo_mask", out["geo"], ref["geo"].value, ref["geo"].decided, st)
    check_mask(f"{name} final_mask", out["final"], ref["final"].value, ref["final"].decided, st)
    rs = restated or {}
    check_elements(f"{name} depth", out["depth"], ref["depth"], st, rs.get("depth"))
    if out.get("points") is not None:
        for c in range(3):
            check_elements(f"{name} points[{c}]", out["points"][c], ref["points"][c], st, rs["points"][c] if restated else None)


def check_dtu_out5(name, out5, masks, ref, sv, st, restated5=None):
    """fusion_dtu_reproject for source view sv of a dtu_reference: out5 [5,n]; masks [nthr,n] or None (reproject_with_depth).  With
    masks the first three outputs are exactly 0 where the last mask is decided false, inside their interval where it is decided
    true, either where it is undecided."""
    b5 = ref["out5"][sv]
    if masks is not None:
        for k in range(masks.shape[0]):
            check_mask(f"{name} masks[{k}]", masks[k], ref["T"][sv, k], ~ref["Un"][sv, k], st)
    for c in range(5):
        b, either = b5[c], None
        if masks is not None and c < 3:
            false_ = ~ref["T"][sv, -1] & ~ref["Un"][sv, -1]
            b = B(np.where(false_, 0.0, b.m), np.where(false_, 0.0, b.e))
            either = ref["Un"][sv, -1]
        check_elements(f"{name} out5[{c}]", out5[c], b, st, None if restated5 is None else restated5[c], either_zero=either)


def mutant_caught(out, ref, keys_masks, keys_cont):
    """Does `out` (a restatement's dict) flip a decided pixel or leave an interval?  -> number of such pixels / elements."""
    n = 0
    for k, rk in keys_masks:
        r = ref[rk]
        value, decided = (r.value, r.decided) if isinstance(r, Decision) else (r, np.ones_like(r))
        n += int((decided & (np.asarray(out[k]).astype(bool) != value)).sum())
    for k, rk in keys_cont:
        got, bs = np.asarray(out[k], np.float64), ref[rk]
        if isinstance(bs, B):
            got, bs = [got], [bs]
        else:
            got = got.reshape(-1, got.shape[-1])
            bs = [b for v in bs for b in (v if isinstance(v, list) else [v])]
        for g, b in zip(got, bs):
            with np.errstate(all="ignore"):
                inside = np.where(b.e == 0, g == b.m, (g >= b.lo) & (g <= b.hi)) | ~np.isfinite(b.e)
            n += int((~inside).sum())
    return n
