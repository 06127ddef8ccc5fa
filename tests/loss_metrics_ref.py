"""Float64 restatement of the training loss and the depth metrics (reference: models/module.py:526-552, utils.py:139-160), the
inputs the tests share, the derived bounds, and a numpy emulation of the block structure of csrc/metrics.hip.

The restatement keeps what the kernels keep in fp32 -- d = est - gt, z = |d| and the per-pixel smooth-L1 term
(0.5f z) z / z - 0.5f -- and forms every sum in float64 and every weight as the double 0.9 ** j.  Bounds (DESIGN.md section 2.4;
derived from the number formats, not from what the kernels return):

  * integer tables: exact;
  * fp64 sums of N terms: (N - 1) 2^-53 sum|x|  (any order of additions);
  * a fp32 scalar or l_i: ONE rounding of its fp64 quotient, 2^-24 (1 + 2^-10) relative (the 2^-10 covers the fp64 sums);
  * total: 2.5 2^-24 sum w_i |l_i|  (one rounding of each l_i, one of the total, the rest fp64);
  * gradient element: 2.5 2^-24 |want|  (two roundings: s_i, and s_i c(d));  masked elements: exactly 0.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24
SCALAR_REL = U24 * (1 + 2.0 ** -10)
TOTAL_REL = 2.5 * U24
GRAD_REL = 2.5 * U24
CHUNK, THREADS = 2048, 256                      # csrc/metrics.hip: MT_CHUNK, MT_THREADS

DLOSS = (1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4)
TRAIN_THRES = (2.0, 4.0, 8.0)
TEST_THRES = (0.125, 0.25, 0.5, 1.0, 20.0)
TEST_BANDS = ((0.0, 2.0), (2.0, 4.0), (4.0, 8.0), (8.0, 14.0), (14.0, 20.0), (20.0, 1e5))
ALL_THRES = TRAIN_THRES + TEST_THRES            # the eight thresholds of train.py


# --------------------------------------------------------------------------------------------- cases recorded from the reference
# name -> (shape, seed, keyword arguments of metrics_case)
GOLDEN_METRIC_CASES = {
    "m2": ((2, 37, 50), 11, {}),
    "m1": ((1, 37, 50), 12, {}),
    "m3e": ((3, 16, 24), 13, {"empty_image": 1}),
    "m1n": ((1, 16, 24), 14, {"nan_valid": True}),
}
SMALL = [(5, 7), (11, 13), (21, 27), (43, 53)]
MID = [(16, 20), (32, 40), (64, 80), (128, 160)]
FULL = [(64, 80), (128, 160), (256, 320), (512, 640)]
# name -> (sizes, B, seed, empty_output, record gradients)
GOLDEN_LOSS_CASES = {
    "la": (SMALL, 1, 21, None, True),
    "lb": (MID, 2, 22, None, False),
    "lc": (FULL, 1, 23, None, False),
    "le": (SMALL, 1, 24, 12, True),
}


# --------------------------------------------------------------------------------------------- inputs
def metrics_case(shape, seed, planted=True, nan_masked=True, nan_valid=False, empty_image=None):
    """est / gt / valid [B,H,W]: gt on a 0.25 grid in the DTU range, errors log-uniform over 0.01 .. 40 (every band of train.py is
    hit), ~70 % valid.  Planted at valid pixels of image 0: e exactly 0, 0.125, 2.0, 4.0, 20.0 (the comparisons' equalities); a NaN
    estimate at a masked pixel; optionally one at a valid pixel; optionally one image fully masked."""
    B, H, W = shape
    r = np.random.RandomState(seed)
    gt = (425.0 + 0.25 * r.randint(0, 2040, size=shape)).astype(F32)
    mag = np.exp(r.uniform(np.log(0.01), np.log(40.0), size=shape))
    est = (gt + (mag * r.choice([-1.0, 1.0], size=shape)).astype(F32)).astype(F32)
    valid = r.uniform(size=shape) < 0.7
    flat_e, flat_g, flat_v = est.reshape(B, -1), gt.reshape(B, -1), valid.reshape(B, -1)
    n = H * W
    if planted:
        for j, e in enumerate((0.0, 0.125, 2.0, 4.0, 20.0, -2.0, -20.0)):
            p = (3 + 5 * j) % n
            flat_e[0, p] = flat_g[0, p] + F32(e)
            flat_v[0, p] = True
    if nan_masked:
        p = n - 1 if n - 1 not in [(3 + 5 * j) % n for j in range(7)] else n - 2
        flat_e[0, p] = np.nan
        flat_v[0, p] = False
        if n > 20:
            flat_e[B - 1, 1] = np.inf
            flat_v[B - 1, 1] = False
    if nan_valid:
        flat_e[B - 1, n // 2] = np.nan
        flat_v[B - 1, n // 2] = True
    if empty_image is not None:
        valid[empty_image] = False
    return est, gt, valid


def loss_case(sizes, B, seed, K=13, dloss=DLOSS, empty_output=None):
    """K estimates over the stages' sizes [(h, w)] * 4: lists est / gt / mask (fp32 0 / 1, shared per stage) of K arrays [B,h,w].
    Errors straddle the kink (|d| from 0.01 to 30); planted in every output: d = +1 and d = -1 exactly at valid pixels, a NaN and
    an Inf estimate at masked pixels.  ``empty_output``: that output gets a mask of its own without a valid pixel."""
    r = np.random.RandomState(seed)
    gts, masks = {}, {}
    for s, (h, w) in enumerate(sizes, start=1):
        gts[s] = (425.0 + 0.25 * r.randint(0, 2040, size=(B, h, w))).astype(F32)
        masks[s] = (r.uniform(size=(B, h, w)) < 0.7).astype(F32)
        m = masks[s].reshape(-1)
        m[[0, 1]] = 1.0
        m[[2, 3]] = 0.0
    est, gt, mask = [], [], []
    for i in range(K):
        s = dloss[i]
        g = gts[s]
        mag = np.exp(r.uniform(np.log(0.01), np.log(30.0), size=g.shape))
        e = (g + (mag * r.choice([-1.0, 1.0], size=g.shape)).astype(F32)).astype(F32)
        fe, fg = e.reshape(-1), g.reshape(-1)
        fe[0], fe[1] = fg[0] + F32(1.0), fg[1] - F32(1.0)
        fe[2], fe[3] = np.nan, np.inf
        est.append(e), gt.append(g), mask.append(masks[s])
    if empty_output is not None:
        mask[empty_output] = np.zeros_like(mask[empty_output])
    return est, gt, mask


def loss_weights(K, loss_rate=0.9):
    return [1.0 if i == 0 else loss_rate ** (K - i - 1) for i in range(K)]


# --------------------------------------------------------------------------------------------- restatement
def smooth_l1_terms(est, gt):
    with np.errstate(invalid="ignore"):
        d = (est.astype(F32) - gt.astype(F32)).astype(F32)
        z = np.abs(d)
        t = np.where(z < 1, (F32(0.5) * z) * z, z - F32(0.5)).astype(F32)
    return d, t


def loss_ref(est, gt, valid, weights):
    """-> dict: q [K] fp64 quotients (NaN for an empty output), abs_sum [K] (for the fp64-sum bound), count [K], l32 [K] =
    fl32(q), total (fp64 of sum w_i l32_i), total_scale = sum w_i |l32_i| (finite terms)."""
    K = len(est)
    q, cnt = np.zeros(K), np.zeros(K, dtype=np.int64)
    for i in range(K):
        _, t = smooth_l1_terms(est[i], gt[i])
        v = valid[i].astype(bool)
        cnt[i] = int(v.sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            q[i] = np.float64(math.fsum(t[v].astype(F64))) / np.float64(cnt[i])
    l32 = q.astype(F32)
    w = np.asarray(weights, dtype=F64)
    total = float(np.sum(w * l32.astype(F64)))
    return {"q": q, "count": cnt, "l32": l32, "total": total, "total_scale": float(np.nansum(w * np.abs(l32.astype(F64))))}


def loss_grad_ref(est, gt, valid, weights, g=1.0):
    """fp64 gradients of the total: g w_i / count_i * c(d) at the valid pixels (d in fp32), 0 elsewhere."""
    out = []
    for i in range(len(est)):
        d, _ = smooth_l1_terms(est[i], gt[i])
        v = valid[i].astype(bool)
        c = np.where(np.abs(d) < 1, d, np.sign(d)).astype(F64)
        n = int(v.sum())
        s = np.float64(F32(g)) * np.float64(weights[i]) / np.float64(n) if n else 0.0
        out.append(np.where(v, s * c, 0.0))
    return out


def metrics_ref(est, gt, valid, thresholds, bands):
    """-> dict: counts [B, 1 + T + R] int64, sums [B, 1 + R] fp64, per_image [B, 1 + T + R] fp64 quotients, want [1 + T + R] = the
    fp64 mean over the images of fl32(per_image) (what one more rounding turns into the scalar)."""
    B = est.shape[0]
    T, R = len(thresholds), len(bands)
    counts, sums = np.zeros((B, 1 + T + R), dtype=np.int64), np.zeros((B, 1 + R))
    per = np.zeros((B, 1 + T + R))
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            v = valid[b].astype(bool)
            e = np.abs((est[b].astype(F32) - gt[b].astype(F32)).astype(F32))[v]
            counts[b, 0], sums[b, 0] = e.size, math.fsum(e.astype(F64))
            per[b, 0] = sums[b, 0] / np.float64(e.size)
            for t, th in enumerate(thresholds):
                counts[b, 1 + t] = int((e > F32(th)).sum())
                per[b, 1 + t] = np.float64(counts[b, 1 + t]) / np.float64(e.size)
            for r_, (lo, hi) in enumerate(bands):
                sel = e[(e >= F32(lo)) & (e <= F32(hi))]
                counts[b, 1 + T + r_], sums[b, 1 + r_] = sel.size, math.fsum(sel.astype(F64))
                per[b, 1 + T + r_] = sums[b, 1 + r_] / np.float64(sel.size) if sel.size else 0.0
        want = per.astype(F32).astype(F64).mean(axis=0)
    return {"counts": counts, "sums": sums, "per_image": per, "want": want}


# --------------------------------------------------------------------------------------------- checks
def check_scalars(got, want, what, extra_abs=0.0):
    """Every element: NaN where want is NaN, else |got - want| <= SCALAR_REL |want| + extra_abs.  Returns the worst ratio."""
    got, want = np.asarray(got, dtype=F64).reshape(-1), np.asarray(want, dtype=F64).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern {np.isnan(got)} vs {nan}"
    err = np.abs(got - want)[~nan]
    bound = SCALAR_REL * np.abs(want[~nan]) + extra_abs
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outside the bound; worst err {err.max():.3e} vs bound {bound[np.argmax(err)]:.3e}"
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


def check_sums(got, want, n_terms, abs_sum, what):
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern"
    bound = np.maximum(n_terms - 1, 0) * 2.0 ** -53 * np.asarray(abs_sum, dtype=F64)      # want is exact (math.fsum)
    err = np.abs(got - want)
    bad = (err > bound) & ~nan
    assert not bad.any(), f"{what}: fp64 sums off by {err[bad].max():.3e}"


def check_grads(got, want, valid, what):
    """Per element: masked -> exactly 0 (not even -0.0 matters: compared as a value); valid -> within GRAD_REL |want|."""
    worst = 0.0
    for i, (g, w, v) in enumerate(zip(got, want, valid)):
        g, v = np.asarray(g, dtype=F64), np.asarray(v).astype(bool)
        assert g.shape == w.shape
        assert (g[~v] == 0.0).all(), f"{what}: output {i}: {int((g[~v] != 0).sum() + np.isnan(g[~v]).sum())} masked elements are not 0"
        err, bound = np.abs(g[v] - w[v]), GRAD_REL * np.abs(w[v])
        nan = np.isnan(w[v])
        assert np.array_equal(np.isnan(g[v]), nan), f"{what}: output {i}: NaN pattern"
        bad = (err > bound) & ~nan
        assert not bad.any(), f"{what}: output {i}: {int(bad.sum())} of {bad.size} outside 2.5 x 2^-24; worst {np.nanmax(err / np.maximum(np.abs(w[v]), 1e-300)) / U24:.2f} x 2^-24"
        if err.size and (~nan).any():
            worst = max(worst, float(np.nanmax(err[~nan] / np.maximum(np.abs(w[v][~nan]), 1e-300)) / U24))
    return worst


def check_loss(got_l, got_count, got_total, ref, what):
    assert np.array_equal(np.asarray(got_count), ref["count"]), f"{what}: counts {got_count} vs {ref['count']}"
    check_scalars(got_l, ref["q"], what + " l_i")
    got_total, want = float(got_total), ref["total"]
    if np.isnan(want):
        assert np.isnan(got_total), f"{what}: total {got_total}, NaN expected"
    else:
        assert abs(got_total - want) <= TOTAL_REL * ref["total_scale"], f"{what}: total {got_total} vs {want}"


# --------------------------------------------------------------------------------------------- emulation of the kernels' block structure
def _wave_sum(v):
    """__shfl_xor butterfly over 64 lanes, v [..., 64] -> lane 0's value."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def _block_sums(x, mutant=None):
    """x [n] (float64 terms, or integer counts) -> the per-workgroup rows: thread t adds elements t, t + 256, ... of its 2048-element
    chunk in order, the wave butterfly, then ((w0 + w1) + w2) + w3."""
    n = x.size
    if mutant == "drop_tail64":
        x = x[:n - n % 64]
        n = x.size
    blocks = -(-n // CHUNK) if n else 0
    if mutant == "drop_last_block" and n % CHUNK and blocks > 0:
        blocks -= 1
    pad = np.zeros(max(blocks, 0) * CHUNK, dtype=x.dtype)
    m = min(n, pad.size)
    pad[:m] = x[:m]
    per_thread = pad.reshape(blocks, CHUNK // THREADS, THREADS)
    acc = np.zeros((blocks, THREADS), dtype=x.dtype)
    for k in range(CHUNK // THREADS):
        acc = acc + per_thread[:, k]
    waves = _wave_sum(acc.reshape(blocks, 4, 64))
    return ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]


def _ascending(rows):
    s = rows.dtype.type(0)
    for v in rows:
        s = s + v
    return s


def emulate_loss(est, gt, mask, weights, mask_u8=False, mutant=None):
    """-> (l [K] fp32, count [K] int64, total fp32) as the two launches of effi_mvs_loss_f32 form them."""
    K = len(est)
    l, cnt = np.zeros(K, dtype=F32), np.zeros(K, dtype=np.int64)
    w = list(weights)[::-1] if mutant == "weights_reversed" else list(weights)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(K):
            _, t = smooth_l1_terms(est[i], gt[i])
            v = (mask[i] != 0) if mask_u8 else (mask[i] > F32(0.5))
            if mutant == "mask_multiply":
                terms = (t * v.astype(F32)).astype(F64)
            else:
                terms = np.where(v, t, F32(0)).astype(F64)
            if mutant == "count_per_image":
                per = []
                for b in range(terms.shape[0]):
                    per.append(_ascending(_block_sums(terms[b].reshape(-1))) / np.float64(int(v[b].sum())))
                l[i], cnt[i] = F32(np.mean(per)), int(v.sum())
                continue
            s = _ascending(_block_sums(terms.reshape(-1), mutant))
            c = int(_ascending(_block_sums(v.reshape(-1).astype(np.int64), mutant)))
            if mutant == "mean_all_pixels":
                c = v.size
            l[i], cnt[i] = F32(s / np.float64(c)), c
        total = F32(_ascending(np.asarray(w, dtype=F64) * l.astype(F64)))
    return l, cnt, total


def emulate_loss_bwd(est, gt, mask, weights, count, g, mask_u8=False, mutant=None):
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(len(est)):
            d, _ = smooth_l1_terms(est[i], gt[i])
            v = (mask[i] != 0) if mask_u8 else (mask[i] > F32(0.5))
            s = F32(np.float64(F32(g)) * np.float64(weights[i]) / np.float64(count[i]))
            c = d if mutant == "quadratic_gradient" else np.where(d < -1, F32(-1), np.where(d > 1, F32(1), d)).astype(F32)
            gr = (s * c).astype(F32)
            out.append((gr * v.astype(F32)).astype(F32) if mutant == "mask_multiply" else np.where(v, gr, F32(0)))
    return out


def emulate_metrics(est, gt, mask, thresholds, bands, mask_u8=True, mutant=None):
    """-> (scalars [1 + T + R] fp32, counts, sums) as the two launches of effi_depth_metrics_f32 form them."""
    B = est.shape[0]
    T, R = len(thresholds), len(bands)
    counts, sums = np.zeros((B, 1 + T + R), dtype=np.int64), np.zeros((B, 1 + R))
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            v = ((mask[b] != 0) if mask_u8 else (mask[b] > F32(0.5))).reshape(-1)
            e = np.abs((est[b].astype(F32) - gt[b].astype(F32)).astype(F32)).reshape(-1)

            def cnt(sel):
                return int(_ascending(_block_sums((sel & v).astype(np.int64), mutant)))

            def fsum(sel):
                if mutant == "mask_multiply":
                    return _ascending(_block_sums((e * (sel & v).astype(F32)).astype(F64), mutant))
                return _ascending(_block_sums(np.where(sel & v, e, F32(0)).astype(F64), mutant))

            every = np.ones_like(v)
            counts[b, 0], sums[b, 0] = cnt(every), fsum(every)
            if mutant == "mean_all_pixels":
                counts[b, 0] = v.size
            for t, th in enumerate(thresholds):
                counts[b, 1 + t] = cnt(e >= F32(th)) if mutant == "threshold_ge" else cnt(e > F32(th))
            for r_, (lo, hi) in enumerate(bands):
                sel = (e >= F32(lo)) & ((e < F32(hi)) if mutant == "band_exclusive" else (e <= F32(hi)))
                counts[b, 1 + T + r_], sums[b, 1 + r_] = cnt(sel), fsum(sel)
        c, s = counts.astype(F64), sums
        if mutant == "one_mean_over_batch":
            c, s = c.sum(axis=0, keepdims=True), s.sum(axis=0, keepdims=True)
        per = np.zeros((c.shape[0], 1 + T + R), dtype=F32)
        per[:, 0] = (s[:, 0] / c[:, 0]).astype(F32)
        per[:, 1:1 + T] = (c[:, 1:1 + T] / c[:, :1]).astype(F32)
        band = np.where(c[:, 1 + T:] > 0, s[:, 1:] / np.where(c[:, 1 + T:] > 0, c[:, 1 + T:], 1.0), 0.0)
        per[:, 1 + T:] = band.astype(F32)
        mean = np.zeros(1 + T + R)
        for b in range(per.shape[0]):
            mean = mean + per[b].astype(F64)
        scalars = (mean / np.float64(per.shape[0])).astype(F32)
    return scalars, counts, sums


MUTANTS_METRICS = ("threshold_ge", "band_exclusive", "one_mean_over_batch", "drop_last_block", "drop_tail64", "mean_all_pixels",
                   "mask_multiply")
MUTANTS_LOSS = ("drop_last_block", "drop_tail64", "mean_all_pixels", "mask_multiply", "count_per_image", "weights_reversed")
MUTANTS_LOSS_BWD = ("quadratic_gradient", "mask_multiply")
