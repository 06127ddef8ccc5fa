"""Float64 reference, per-element half-widths and fp32 restatements of the per-pixel training kernels and BatchNorm (DESIGN.md
section 2.6).  CPU only: nothing here imports the HIP library or touches a GPU, and nothing on the product path imports this module.

For each operation: ``*_interval`` gives (mid, half) per element -- mid = the operation in float64 from the same fp32 inputs, half = a
count of the roundings of the kernel's source in units of u = 2^-24, scaled by the magnitudes of the terms behind THAT element (never
by the tensor's peak); ``*_emulate`` restates the kernel op for op in torch fp32 on the CPU (double where the kernel accumulates in
double), with ``mutant=`` for the structural and precision mutants of tests/test_pixel_bound_host.py.  half == 0 pins an element
bit for bit (conv_bound.check_bounded).

Figures used for the library functions (the kernels are built with -ffp-contract=off, so no product is fused into a sum):

  expf       1 ulp = 2u relative (the figure tests/test_gpu_conv_bounds.py::_up2x_interval uses); expf(0) = 1 exactly.
  tanhf, effi_sigmoid   conv_bound.ACT_ERR["exact"] = 4u absolute (values <= 1).
  a / b      csrc/common.hpp and csrc/train_ops.hip write the plain C++ quotient; hipcc's default for HIP is the correctly rounded
             fp32 division (-fhip-fp32-correctly-rounded-divide-sqrt is on unless switched off; csrc/Makefile does not): u.
  rsqrtf     ASSUMED 1 ulp = 2u.  The ROCm device-library documentation is not installed with the toolchain this was written
             against; 1 ulp is the figure OpenCL's full profile requires of rsqrt and the accuracy of the hardware instruction the
             device library builds it on.
  fp32 results below the normal range: an absolute 2^-126 on top of every half-width that ends in an exponential (a library may
             flush there; relative counts say nothing below the normal range).
  double sums: depth * 2^-53 of the sum of magnitudes (never visible next to u, kept so that no term is dropped silently).

Sums follow the kernels' order (EFFI_FOR_BATCH_RANGE, csrc/train_ops.hip:33-35): nsplit workgroups take per = ceil(total / nsplit)
consecutive elements of the flattened (sample, position) range of a channel; thread t chains elements t, t + 256, ...; a six-level
xor butterfly per wave; four wave partials added left to right; the nsplit partials added ascending.  ``split_sum`` does exactly
that; its rounding depth is (K - 1) + 6 + 3 + (nsplit - 1) with K = ceil(per / 256) (the first addition of every chain is 0 + v).
"""
import numpy as np
import torch
import torch.nn.functional as F

from conv_bound import ACT_ERR, U, Interval, act_interval, check_bounded  # noqa: F401  (re-exported for the tests)

SLACK = 1.0 + 2.0 ** -10            # second-order terms of every first-order count
TPB = 256
DBL = 2.0 ** -53
TINY = 2.0 ** -126
EXP_ERR = 2.0 * U
RSQRT_ERR = 2.0 * U                 # assumed: see the module docstring
EPS6 = float(np.float32(1e-6))      # the kernels' 1e-6f
THR32 = np.float32(1e-4)            # the kernels' 1e-4f
THR = float(THR32)


def d64(t_):
    return t_.detach().double().cpu()


def tight_share(ivs, factor=2.0 ** -10):
    """Share of the non-pinned elements of the intervals ``ivs`` with half <= factor * |mid|."""
    ok = n = 0
    for iv in ivs:
        live = iv.half != 0
        ok += int((live & (iv.half <= factor * iv.mid.abs())).sum())
        n += int(live.sum())
    return ok / max(n, 1), n


def widest_relative(iv):
    """Largest half / |mid| over the non-pinned elements with mid != 0."""
    live = (iv.half != 0) & (iv.mid != 0)
    return float((iv.half[live] / iv.mid[live].abs()).max()) if live.any() else 0.0


# ==============================================================================================================================
# the split reductions
# ==============================================================================================================================
def _chan(x):
    """[B, C, ...] -> [C, B * n]: the flattened (sample, position) range of each channel."""
    B, C = x.shape[:2]
    return x.reshape(B, C, -1).transpose(0, 1).reshape(C, -1)


def _bshape(x):
    return (1, x.shape[1]) + (1,) * (x.dim() - 2)


def split_layout(total, nsplit):
    """(per, K, rounding depth) of a split reduction over ``total`` elements."""
    per = -(-total // nsplit)
    K = -(-per // TPB)
    return per, K, (K - 1) + 6 + 3 + (nsplit - 1)


def split_sum(v, nsplit, drop_tail=False):
    """v [C, total] (float32 or float64: the accumulator's type) -> the nsplit workgroup sums [C, nsplit] in the kernels' order.
    ``drop_tail``: the mutant that loses the elements behind the last full 256-stride of the last non-empty split."""
    C, total = v.shape
    per, K, _ = split_layout(total, nsplit)
    P = torch.zeros(C, nsplit, K * TPB, dtype=v.dtype)              # zero padding: x + 0 is exact
    last = (total - 1) // per
    for j in range(nsplit):
        i0, i1 = j * per, min(total, (j + 1) * per)                 # train_ops.hip:174
        if i1 <= i0:
            continue
        if drop_tail and j == last:
            i1 -= ((i1 - i0) % TPB) or min(i1 - i0, TPB)
        P[:, j, :i1 - i0] = v[:, i0:i1]
    P = P.view(C, nsplit, K, TPB)
    s = torch.zeros(C, nsplit, TPB, dtype=v.dtype)
    for k in range(K):                                              # thread t: elements t, t + 256, ... (train_ops.hip:34-35)
        s = s + P[:, :, k]
    s = s.view(C, nsplit, TPB // 64, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):                                  # wave_sum (train_ops.hip:20-29)
        s = s + s[..., lane ^ o]
    r = s[..., 0]
    return ((r[..., 0] + r[..., 1]) + r[..., 2]) + r[..., 3]        # red[0] + red[1] + red[2] + red[3] (train_ops.hip:192)


def _ascending(part):
    """[C, nsplit] -> [C]: s = 0; s += part[j], j ascending (train_ops.hip:178, 270, 344-347)."""
    s = torch.zeros(part.shape[0], dtype=part.dtype)
    for j in range(part.shape[1]):
        s = s + part[:, j]
    return s


def _split_abs(v64, nsplit):
    """sum_j |P_j| of the float64 split sums of v64 [C, total]: what the fp32 cast of each partial sum is relative to."""
    C, total = v64.shape
    per = -(-total // nsplit)
    pad = torch.zeros(C, nsplit * per, dtype=torch.float64)
    pad[:, :total] = v64
    return pad.view(C, nsplit, per).sum(2).abs().sum(1)


# ==============================================================================================================================
# BatchNorm, training mode
# ==============================================================================================================================
def bn_fwd_emulate(x, gamma, beta, rm, rv, eps, momentum, relu, nsplit, mutant=None):
    """effi_bn_train_fwd_f32 (bn_moment_kernel<1>, <2>, bn_apply_kernel) restated.  Mutants: "biased_running_var",
    "drop_tail", "first_sample_mean" (structural); "mean_fp32" (precision)."""
    v = _chan(x.float())
    C, total = v.shape
    n = total // x.shape[0]
    tail = mutant == "drop_tail"
    if mutant == "first_sample_mean":
        sh = (v[:, :n].double().sum(1) / float(n)).float()
    elif mutant == "mean_fp32":
        sh = _ascending(split_sum(v, nsplit)) / torch.tensor(float(total), dtype=torch.float32)
    else:
        part1 = split_sum(v.double(), nsplit, tail).float()          # Acc = double, (float) of the workgroup's sum (:192)
        sh = (_ascending(part1.double()) / float(total)).float()    # :177-179
    dlt = v - sh[:, None]                                           # :184
    part2 = split_sum(dlt * dlt, nsplit, tail)                      # Acc = float (:185)
    var = _ascending(part2) / torch.tensor(float(total), dtype=torch.float32)      # :270-271
    inv = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))                # :272
    mom = torch.tensor(momentum, dtype=torch.float32)
    keep = torch.tensor(1.0, dtype=torch.float32) - mom             # :276
    unbias = torch.tensor(1.0 if mutant == "biased_running_var" else float(total) / float(max(total - 1, 1)), dtype=torch.float32)
    new_rm = rm * keep + mom * sh                                   # :277
    new_rv = rv * keep + mom * (var * unbias)                       # :278
    bs = _bshape(x)
    y = (x - sh.view(bs)) * inv.view(bs) * gamma.view(bs) + beta.view(bs)          # :288
    if relu:
        y = y.clamp_min(0.0)
    return dict(y=y, mean=sh, invstd=inv, rm=new_rm, rv=new_rv)


def bn_fwd_interval(x, gamma, beta, rm, rv, eps, momentum, relu, nsplit):
    """-> {"y", "mean", "invstd", "rm", "rv"}: Intervals.  Counts (u = 2^-24), line numbers of csrc/train_ops.hip:

    mean    every workgroup's double sum is cast to fp32 (:192): u |P_j| each; the partial sums are added in double and divided by N
            in double (:178-179), one cast: u |mean|.  dmean = u |mean| + u sum_j |P_j| / N + depth 2^-53 sum |x| / N.
    var     sum (x - mean)^2 = sum (x - mu)^2 + N (mean - mu)^2 exactly, so the shift's error enters as dmean^2 only; each term is
            fl(fl(x - mean)^2): 3u of itself (:184-185); the fp32 sum in the kernel's order: depth u of the sum (all terms are
            positive); the division by N (:271): u.  dvar = (3 + depth + 1) u var + dmean^2.
    invstd  var + eps (u of it), rsqrtf (RSQRT_ERR): (var + eps)^-1/2 moves by half the relative error of its argument:
            dis = invstd (dvar / (2 (var + eps)) + u / 2 + RSQRT_ERR).
    y       (x - mean) is ga + be (:288): the subtraction u |x - mu| + dmean, two products 2u, the carried dis / is, the sum u |y|:
            |ga| is dmean + |(x - mu) is ga| (3u + dis / is) + u |y|; ReLU through act_interval (max is exact).
    running_mean  rm keep + m mean (:276-277): keep = fl(1 - m) (u), two products, one sum: 2u |rm keep| + u |m mean| + m dmean + u |.|.
    running_var   rv keep + m (var unbias) (:278), unbias = (float)(N / (N - 1)) (u): 2u |rv keep| + 3u |m var unbias| + m unbias dvar
            + u |.|.   m, eps: the fp32 values the entry receives."""
    xd = d64(x)
    v = _chan(xd)
    C, total = v.shape
    _, _, depth = split_layout(total, nsplit)
    ga, be, rmd, rvd = d64(gamma), d64(beta), d64(rm), d64(rv)
    m32, eps32 = float(np.float32(momentum)), float(np.float32(eps))
    mu = v.mean(1)
    s_abs = v.abs().sum(1)
    dmean = (U * mu.abs() + U * _split_abs(v, nsplit) / total + depth * DBL * s_abs / total) * SLACK
    var = ((v - mu[:, None]) ** 2).mean(1)
    dvar = (3 + depth + 1) * U * var * SLACK + dmean ** 2
    is_ = (var + eps32) ** -0.5
    dis = is_ * (dvar / (2 * (var + eps32)) + 0.5 * U + RSQRT_ERR) * SLACK
    bs = _bshape(x)
    xc = xd - mu.view(bs)
    core = xc * (is_ * ga).view(bs)
    ymid = core + be.view(bs)
    yhalf = ((ga.abs() * is_ * dmean).view(bs) + core.abs() * (3 * U + dis / is_).view(bs) + U * ymid.abs()) * SLACK
    y = act_interval(ymid, yhalf, "relu" if relu else "none")
    keep = 1.0 - m32
    rm_mid = rmd * keep + m32 * mu
    rm_half = (2 * U * (rmd * keep).abs() + U * (m32 * mu).abs() + m32 * dmean + U * rm_mid.abs()) * SLACK
    unb = float(total) / float(max(total - 1, 1))
    rv_mid = rvd * keep + m32 * var * unb
    rv_half = (2 * U * (rvd * keep).abs() + 3 * U * m32 * var * unb + m32 * unb * dvar + U * rv_mid.abs()) * SLACK
    return dict(y=y, mean=Interval(mu, dmean), invstd=Interval(is_, dis), rm=Interval(rm_mid, rm_half), rv=Interval(rv_mid, rv_half))


def bn_bwd_emulate(gy, y, x, mean, invstd, gamma, relu, nsplit, mutant=None):
    """effi_bn_bwd_f32 (bn_bwd_reduce_kernel, bn_bwd_apply_kernel) restated.  Mutants: "mask_ge", "drop_tail" (structural);
    "s12_fp32" (precision)."""
    bs = _bshape(x)
    g = gy
    if relu:
        keep = (y >= 0) if mutant == "mask_ge" else (y > 0)         # :311, :358
        g = torch.where(keep, gy, torch.zeros_like(gy))
    xh = (x - mean.view(bs)) * invstd.view(bs)                      # :313, :359
    N = float(x.numel() // x.shape[1])
    acc = torch.float32 if mutant == "s12_fp32" else torch.float64
    tail = mutant == "drop_tail"
    pa = split_sum(_chan(g).to(acc), nsplit, tail)                  # :312
    pb = split_sum(_chan(g * xh).to(acc), nsplit, tail)             # :313: the product is fp32
    if nsplit > 1:
        t1, t2 = _ascending(pa).double(), _ascending(pb).double()   # :344-347
        s1, s2 = t1.float(), t2.float()                             # :348
    else:
        s1, s2 = pa[:, 0].float(), pb[:, 0].float()                 # :326-327
        t1, t2 = s1.double(), s2.double()                           # :350-351
    a1, a2 = (t1 / N).float(), (t2 / N).float()                     # :353
    gx = (gamma * invstd).view(bs) * ((g - a1.view(bs)) - xh * a2.view(bs))        # :360
    return dict(gx=gx, s1=s1, s2=s2)


def bn_bwd_interval(gy, y, x, mean, invstd, gamma, relu, nsplit):
    """-> {"gx", "s1", "s2"}.  mean, invstd are the fp32 INPUTS of the entry (its forward's outputs), y the forward output whose sign
    is the mask (given to both sides: the mask is exact).  Counts:

    g'      gy where y > 0, else 0 (:311, :358): an exact select.
    xhat    fl(fl(x - mean) is): 2u of itself.
    s1      double sum of fp32 values, rounded once (:326 / :348): u |s1| + depth 2^-53 sum |g'|.
    s2      the products g' xhat are fp32 (:313): 3u of each (xhat's two, the product's one), then as s1.
    a1, a2  (float)(t / N) (:353); without splits t is the fp32 s1 read back (:350): 2u |a| + the sum's term / N.
    gx      ga is (g' - a1 - xhat a2) (:360): the first difference u (|g'| + |a1|), the product 3u |xhat a2|, the second difference
            and the two outer products 3u of at most the sum of the three magnitudes: 6u (|g'| + |a1| + |xhat a2|) + da1 + |xhat| da2,
            times |ga is|.
    A channel whose g' is 0 everywhere has s1 = s2 = 0 and gx = ga is (0 - 0 - xhat 0) = 0 exactly: pinned."""
    bs = _bshape(x)
    gd, xd = d64(gy), d64(x)
    if relu:
        gd = torch.where(d64(y) > 0, gd, torch.zeros_like(gd))
    mu, is_, ga = d64(mean), d64(invstd), d64(gamma)
    xh = (xd - mu.view(bs)) * is_.view(bs)
    total = x.numel() // x.shape[1]
    _, _, depth = split_layout(total, nsplit)
    gv, pv = _chan(gd), _chan(gd * xh)
    s1, s2 = gv.sum(1), pv.sum(1)
    h1 = (U * s1.abs() + depth * DBL * gv.abs().sum(1)) * SLACK
    h2 = (U * s2.abs() + (3 * U + depth * DBL) * pv.abs().sum(1)) * SLACK
    N = float(total)
    a1, a2 = s1 / N, s2 / N
    da1 = (2 * U * a1.abs() + depth * DBL * gv.abs().sum(1) / N) * SLACK
    da2 = (2 * U * a2.abs() + (3 * U + depth * DBL) * pv.abs().sum(1) / N) * SLACK
    a1b, a2b = a1.view(bs), a2.view(bs)
    mid = (ga * is_).view(bs) * (gd - a1b - xh * a2b)
    half = (ga * is_).abs().view(bs) * (6 * U * (gd.abs() + a1b.abs() + (xh * a2b).abs()) + da1.view(bs) + xh.abs() * da2.view(bs)) * SLACK
    dead = gv.abs().sum(1) == 0                                     # every g' of the channel is 0
    half = torch.where(dead.view(bs), torch.zeros_like(half), half)
    zero = torch.zeros_like(h1)
    return dict(gx=Interval(mid, half), s1=Interval(s1, torch.where(dead, zero, h1)), s2=Interval(s2, torch.where(dead, zero, h2)))


# ==============================================================================================================================
# softmax weights (shared by the soft-argmin backward and the convex upsampling)
# ==============================================================================================================================
def _seq_sum(t_):
    """s = 0; s += t[k], k ascending, in the tensor's own type."""
    s = torch.zeros(t_.shape[1:], dtype=t_.dtype)
    for k in range(t_.shape[0]):
        s = s + t_[k]
    return s


def softmax_weights(v):
    """v [K, ...] float64 logits -> (s_k, rho_k): the softmax and the relative error of the kernels' fp32 weight k,
    expf(v_k - max) / sum (train_ops.hip:463-473, 532-543; volume_ops.hip:531-545):
      a_k = v_k - max: u |a_k|, which moves the exponential by that much relatively; expf: EXP_ERR: eps_k = (|a_k| + 2) u;
      the K-term fp32 sum (the first addition is 0 + e): eps-weighted mean + (K - 1) u;  the division: u
      -> rho_k = eps_k + sum_j s_j eps_j + K u."""
    K = v.shape[0]
    a = v - v.max(0, keepdim=True).values
    s = torch.softmax(v, 0)
    eps = a.abs() * U + EXP_ERR
    rho = (eps + (s * eps).sum(0, keepdim=True) + K * U) * SLACK
    return s, rho


# ==============================================================================================================================
# soft-argmin backward
# ==============================================================================================================================
def _hyp_full(hyp, D, h, w):
    return hyp.view(D, 1, 1).expand(D, h, w) if hyp.dim() == 1 else hyp


def softargmin_bwd_emulate(logits, hyp, g, mutant=None):
    """softargmin_bwd_kernel restated: logits [D,h,w], hyp [D] or [D,h,w], g [h,w].  Mutants: "dep_short", "flush", "no_dps"
    (structural); "fp32" (precision)."""
    D, h, w = logits.shape
    H = _hyp_full(hyp, D, h, w)
    if mutant == "no_dps":                                          # per-pixel hypotheses read as per-plane ones
        H = H[:, :1, :1].expand(D, h, w)
    m = logits.max(0).values                                        # :464
    e = torch.exp(logits - m)                                       # :466
    pr = e / _seq_sum(e)                                            # :470, :473
    if mutant == "fp32":
        dep = _seq_sum(pr * H)
        return g * pr * (H - dep)
    prd, Hd = pr.double(), H.double()
    dep = _seq_sum((prd * Hd)[:D - 1] if mutant == "dep_short" else prd * Hd)      # :470
    if mutant == "flush":                                           # the output loop's probability (:473) flushed below 1e-6
        prd = torch.where(pr < 1e-6, torch.zeros_like(prd), prd)
    return (g.double() * prd * (Hd - dep)).float()                  # :474


def softargmin_bwd_interval(logits, hyp, g):
    """glogits_d = g p_d (hyp_d - dep), dep = sum_d p_d hyp_d.  The probabilities are fp32 (relative error rho_d, softmax_weights with
    D terms); dep, the difference and the products are double (:469-474), rounded once:
      ddep = sum_d rho_d p_d |hyp_d|;   half_d = |g| (rho_d p_d |hyp_d - dep| + p_d ddep) + u |mid| + 2^-126.
    D = 1: expf(0) = 1, 1 / 1 = 1, dep = hyp_0 and hyp_0 - dep = 0: exactly 0, pinned."""
    D, h, w = logits.shape
    H = d64(_hyp_full(hyp, D, h, w))
    p, rho = softmax_weights(d64(logits))
    dep = (p * H).sum(0)
    gd = d64(g)
    mid = gd * p * (H - dep)
    if D == 1:
        return Interval(torch.zeros_like(mid), torch.zeros_like(mid))
    ddep = (rho * p * H.abs()).sum(0) + D * DBL * (p * H.abs()).sum(0)
    half = (gd.abs() * (rho * p * (H - dep).abs() + p * ddep) + U * mid.abs()) * SLACK + TINY
    return Interval(mid, half)


# ==============================================================================================================================
# view-weighted aggregation
# ==============================================================================================================================
def _den_terms(wd):
    """(den, dden) of den = fl(fl(sum_v w_v) + 1e-6f): S - 1 roundings of the sum (the first addition is 0 + w), one of the last
    addition (volume_ops.hip:191-197, train_ops.hip:484-486)."""
    S = wd.shape[0]
    den = wd.sum(0) + EPS6
    return den, ((S - 1) * U * wd.abs().sum(0) + U * den.abs()) * SLACK


def view_aggregate_emulate(sim, weights, mutant=None):
    """view_aggregate_body restated (fp32 throughout): sim [S,D,h,w], weights [S,h,w] or None.  Mutants: "no_eps", "short_wsum"."""
    S = sim.shape[0]
    if weights is None:
        return _seq_sum(sim) / torch.tensor(float(S), dtype=torch.float32)        # volume_ops.hip:185-186
    wsum = _seq_sum(weights[:S - 1] if mutant == "short_wsum" and S > 1 else weights)
    den = wsum if mutant == "no_eps" else wsum + torch.tensor(1e-6, dtype=torch.float32)
    return _seq_sum(sim * weights[:, None]) / den                    # :202-203


def view_aggregate_interval(sim, weights):
    """weights None: acc = sum_v s_v in fp32 (S - 1 roundings), / (float)S: (S - 1) u sum |s| + u |out|; S = 1: 0 + s and s / 1 are exact,
    pinned.  With weights: every product rounds, S - 1 additions: S u sum |s w| on the numerator; the quotient u; the carried dden:
    half = S u sum_v |s_v w_v| / den + |out| (u + dden / den)."""
    sd = d64(sim)
    S = sd.shape[0]
    if weights is None:
        mid = sd.mean(0)
        half = ((S - 1) * U * sd.abs().sum(0) + U * mid.abs()) * SLACK
        if S == 1:
            mid, half = sd[0], torch.zeros_like(mid)
        return Interval(mid, half)
    wd = d64(weights)
    den, dden = _den_terms(wd)
    mid = (sd * wd[:, None]).sum(0) / den
    half = (S * U * (sd * wd[:, None]).abs().sum(0) / den + mid.abs() * (U + dden / den)) * SLACK
    return Interval(mid, half)


def view_aggregate_bwd_emulate(sim, weights, g, mutant=None):
    """view_aggregate_bwd_kernel restated -> (gsim [S,D,h,w], gw [S,h,w]).  Mutants: "no_eps", "short_wsum", "gw_shift" (structural);
    "gw_fp32" (precision)."""
    S = sim.shape[0]
    wsum = _seq_sum(weights[:S - 1] if mutant == "short_wsum" and S > 1 else weights)                   # :484-485
    den = wsum if mutant == "no_eps" else wsum + torch.tensor(1e-6, dtype=torch.float32)               # :486
    gsim = g[None] * weights[:, None] / den                         # :501
    if mutant == "gw_fp32":
        o = _seq_sum(sim * weights[:, None]) / den
        gw = torch.stack([_seq_sum(g * (sim[v] - o) / den) for v in range(S)])
    else:
        o = _seq_sum(sim.double() * weights.double()[:, None]) / den.double()                           # :494-495
        gw = torch.stack([_seq_sum(g.double() * (sim[v].double() - o) / den.double()) for v in range(S)]).float()   # :502, :508
    if mutant == "gw_shift":
        gw = torch.roll(gw, 1, 0)                                   # view v reads view v - 1
    return gsim, gw


def view_aggregate_bwd_interval(sim, weights, g):
    """gsim = (g w) / den: two roundings and the carried dden: |gsim| (2u + dden / den) (0 where g w = 0: pinned).
    gw_v = sum_d g_d (s_vd - o_d) / den with o = acc / den: everything in double except den itself (fp32, relative error e <= dden /
    den): o moves by o e, the quotient by e, so gw moves by e (|gw| + sum_d |g_d o_d| / den); one rounding at the end:
    half = (dden / den) (|gw| + sum_d |g_d o_d| / den) + u |gw| + D 2^-50 sum_d |g_d| (|s_vd| + |o_d|) / den."""
    sd, wd, gd = d64(sim), d64(weights), d64(g)
    D = sd.shape[1]
    den, dden = _den_terms(wd)
    e = dden / den
    gsim = gd[None] * wd[:, None] / den
    o = (sd * wd[:, None]).sum(0) / den
    gw = (gd[None] * (sd - o[None])).sum(1) / den
    go = (gd * o).abs().sum(0) / den
    dbl = D * 8 * DBL * (gd.abs()[None] * (sd.abs() + o.abs()[None])).sum(1) / den
    return (Interval(gsim, gsim.abs() * (2 * U + e) * SLACK),
            Interval(gw, (e * (gw.abs() + go[None]) + U * gw.abs() + dbl) * SLACK))


# ==============================================================================================================================
# convex upsampling x2
# ==============================================================================================================================
def _shuffle(q, h, w):
    """[4 (ij = 2 i + j), h, w] -> [2h, 2w]: output pixel (2y + i, 2x + j)."""
    return q.view(2, 2, h, w).permute(2, 0, 3, 1).reshape(2 * h, 2 * w)


def _unshuffle(up, h, w):
    return up.view(h, 2, w, 2).permute(1, 3, 0, 2).reshape(4, h, w)


def _neighbours(inv, h, w, clamp=False):
    """[9, 1, h, w]: nb_k = inv at (y + k / 3 - 1, x + k % 3 - 1), 0 outside the map (``clamp``: the mutant that clamps instead)."""
    x = inv.reshape(1, 1, h, w)
    if clamp:
        x = F.pad(x, (1, 1, 1, 1), mode="replicate")
        return F.unfold(x, 3).view(9, 1, h, w)
    return F.unfold(x, 3, padding=1).view(9, 1, h, w)


def _mask_taps(mask, h, w, mutant=None):
    """[36, h, w] -> [9 (k), 4 (ij), h, w]: channel k * 4 + ij ("mask_layout": the mutant that reads ij * 9 + k)."""
    return mask.view(4, 9, h, w).permute(1, 0, 2, 3) if mutant == "mask_layout" else mask.view(9, 4, h, w)


def _gather(contrib, h, w, mutant=None):
    """ginv[y][x] = sum_k contrib[k][y - (k / 3 - 1)][x - (k % 3 - 1)], k ascending, absent outside the map (adding the padding's 0
    is exact).  "gather_skip8": the mutant that loses tap 8 on the last row."""
    pad = F.pad(contrib, (1, 1, 1, 1))
    acc = torch.zeros(h, w, dtype=contrib.dtype)
    for k in range(9):
        dy, dx = k // 3 - 1, k % 3 - 1
        term = pad[k, 1 - dy:1 - dy + h, 1 - dx:1 - dx + w]
        if mutant == "gather_skip8" and k == 8:
            term = term.clone()
            term[h - 1] = 0
        acc = acc + term
    return acc


def convex_up_emulate(inv, mask, mutant=None):
    """convex_upsample2x_kernel's ``out_inv`` restated: inv [h,w], mask [36,h,w] -> [2h,2w].  Mutants: "mask_layout", "clamp_nb"."""
    h, w = inv.shape[-2:]
    nb = _neighbours(inv, h, w, mutant == "clamp_nb")
    m = _mask_taps(mask, h, w, mutant)
    e = torch.exp(m - m.max(0, keepdim=True).values)                # volume_ops.hip:540
    wk = e / _seq_sum(e)                                            # :541, :545
    return _shuffle(_seq_sum(wk * nb), h, w)                        # :545-546


def convex_up_interval(inv, mask):
    """up = sum_k m_k nb_k with m_k = expf(v_k - max) / sum: weight k is off by rho_k m_k (softmax_weights, nine terms); the nine
    products round once each and the nine additions at most eight times (0 + first): 9u sum m_k |nb_k|.
    dup = sum_k rho_k m_k |nb_k| + 9u sum_k m_k |nb_k| (+ 2^-126).  A tap outside the map is 0: its product is exactly 0."""
    h, w = inv.shape[-2:]
    nb = _neighbours(d64(inv), h, w)
    s, rho = softmax_weights(_mask_taps(d64(mask), h, w))
    mid = (s * nb).sum(0)
    half = ((rho * s * nb.abs()).sum(0) + 9 * U * (s * nb.abs()).sum(0)) * SLACK
    half = torch.where(half > 0, half + TINY, half)
    return Interval(_shuffle(mid, h, w), _shuffle(half, h, w))


def convex_up_bwd_emulate(inv, mask, gup, mutant=None):
    """convex_upsample2x_bwd_kernel + convex_upsample2x_gather_kernel restated -> (gmask [36,h,w], ginv [h,w]).  Mutants:
    "mask_layout", "clamp_nb", "gather_skip8"."""
    h, w = inv.shape[-2:]
    nb = _neighbours(inv, h, w, mutant == "clamp_nb")
    m = _mask_taps(mask, h, w, mutant)
    e = torch.exp(m - m.max(0, keepdim=True).values)                # :540
    wk = e / _seq_sum(e)                                            # :543
    up = _seq_sum(wk * nb)                                          # :543
    g = _unshuffle(gup, h, w)[None]                                 # :544
    gmask = g * wk * (nb - up[None])                                # :547
    contrib = _seq_sum((g * wk).transpose(0, 1))                    # :548: gn[k] += g m[k], ij ascending -> [9,h,w]
    if mutant == "mask_layout":
        gmask = gmask.permute(1, 0, 2, 3)
    return gmask.reshape(36, h, w), _gather(contrib, h, w, mutant)


def convex_up_bwd_interval(inv, mask, gup):
    """gmask_k = (g m_k) (nb_k - up) (:547): m_k carries rho_k m_k, up carries dup (convex_up_interval), the difference rounds (u of
    itself) and the two products round: |g| (m_k dup + (rho_k + 3u) m_k |nb_k - up|) + 2^-126.
    ginv: contrib_k = sum_ij g m_k (:548: four products, three roundings of the sum) and the gather's nine-term sum (eight roundings,
    :564): sum over the in-map taps of |g| m_k (rho_k + 4u + 8u).  Every contributing gup = 0 -> every term is 0: pinned."""
    h, w = inv.shape[-2:]
    nb = _neighbours(d64(inv), h, w)
    s, rho = softmax_weights(_mask_taps(d64(mask), h, w))
    up = (s * nb).sum(0)
    dup = ((rho * s * nb.abs()).sum(0) + 9 * U * (s * nb.abs()).sum(0)) * SLACK + TINY
    g = _unshuffle(d64(gup), h, w)[None]
    gmask = g * s * (nb - up[None])
    hmask = g.abs() * (s * dup[None] + (rho + 3 * U) * s * (nb - up[None]).abs()) * SLACK
    hmask = torch.where(hmask > 0, hmask + TINY, hmask)
    contrib = (g * s).sum(1)
    hcontrib = (g.abs() * s * (rho + 12 * U)).sum(1) * SLACK
    ginv, hinv = _gather(contrib, h, w), _gather(hcontrib, h, w)
    hinv = torch.where(hinv > 0, hinv + TINY, hinv)
    return Interval(gmask.reshape(36, h, w), hmask.reshape(36, h, w)), Interval(ginv, hinv)


# ==============================================================================================================================
# pointwise_kernel
# ==============================================================================================================================
PW_OPS = ("act_bwd_relu", "act_bwd_sigmoid", "act_bwd_tanh", "tanh", "relu", "sigmoid", "mul", "mul_bwd", "gru", "gru_bwd",
          "inv_to_depth", "inv_to_depth_bwd", "scale_ch")         # EFFI_PW_* 0..12 in order


def _f32(v):
    return torch.tensor(float(np.float32(v)), dtype=torch.float32)


def _rn_product(a, b):
    """RN(a b) of fp32 a, b as float64: the float64 product of two fp32 values is exact (48 bits), one rounding to fp32."""
    return (d64(a) * d64(b)).float().double()


def _disp_fp32(lo, hi):
    """(min_disp, max_disp - min_disp) as the kernel forms them (train_ops.hip:395-396, common.hpp:133-134): IEEE fp32 divisions."""
    lo32, hi32, one = np.float32(lo), np.float32(hi), np.float32(1.0)
    a = one / (one / lo32)
    return a, one / (one / hi32) - a


def inv_to_depth_terms(inv, lo, hi):
    """(s, ds, clamped) of s = min_disp + (max_disp - min_disp) inv in float64 terms: min_disp = 1 / (1 / lo) (2u lo), max_disp likewise,
    their difference b (u more): db = 2u (lo + hi) + u |b|; the product u |b inv|, the sum u |s|.  ``clamped``: s <= 1e-4f.  Where
    inv = 0 the product and the sum are exact and s IS the fp32 min_disp, two IEEE divisions that numpy reproduces: decided on that
    value; elsewhere on the float64 s, which the caller asserts to be further than ds from the threshold."""
    lo_, hi_ = float(np.float32(lo)), float(np.float32(hi))
    iv = d64(inv)
    b = hi_ - lo_
    db = (2 * U * (lo_ + hi_) + U * abs(b)) * SLACK
    s = lo_ + b * iv
    ds = (2 * U * lo_ + db * iv.abs() + U * (b * iv).abs() + U * s.abs()) * SLACK
    a32, _ = _disp_fp32(lo, hi)
    clamped = torch.where(iv == 0, torch.full_like(iv, float(a32)) <= THR, s <= THR)
    return s, ds, clamped, b, db


def pw_emulate(op, a, b=None, c=None, d=None, s0=0.0, s1=0.0, inner=1, C=1, mutant=None):
    """pointwise_kernel restated -> list of outputs.  Mutants: "sigmoid_plus" (y (1 + y)), "inner_off" (inner + 1), "clamp_ge"."""
    one = torch.tensor(1.0, dtype=torch.float32)
    if op == "act_bwd_relu":
        return [torch.where(b > 0, a, torch.zeros_like(a))]         # :378
    if op == "act_bwd_sigmoid":
        return [a * (b * ((one + b) if mutant == "sigmoid_plus" else (one - b)))]   # :379
    if op == "act_bwd_tanh":
        return [a * (one - b * b)]                                  # :380
    if op == "tanh":
        return [torch.tanh(a)]
    if op == "relu":
        return [a.clamp_min(0.0)]
    if op == "sigmoid":
        return [one / (one + torch.exp(-a))]                        # common.hpp:100
    if op == "mul":
        return [a * b]
    if op == "mul_bwd":
        return [a * c, a * b]                                       # :385
    if op == "gru":
        return [(one - a) * b + a * c]                              # :386
    if op == "gru_bwd":
        return [a * (d - c), a * (one - b), a * b]                  # :389-391
    if op in ("inv_to_depth", "inv_to_depth_bwd"):
        md, bb = _disp_fp32(s0, s1)
        md, bb, thr = torch.tensor(float(md)), torch.tensor(float(bb)), torch.tensor(THR, dtype=torch.float32)
        if op == "inv_to_depth":
            return [one / torch.maximum(md + bb * a, thr)]          # common.hpp:135-137
        s = md + bb * b                                             # :397
        live = (s >= thr) if mutant == "clamp_ge" else (s > thr)
        return [torch.where(live, -a * bb / (s * s), torch.zeros_like(a))]         # :398
    if op == "scale_ch":
        k = inner + 1 if mutant == "inner_off" else inner
        return [a * b[(torch.arange(a.numel()) // k) % C].view(a.shape)]           # :400
    raise KeyError(op)


def pw_interval(op, a, b=None, c=None, d=None, s0=0.0, s1=0.0, inner=1, C=1):
    """-> list of Intervals, one per output of ``pointwise_kernel`` (csrc/train_ops.hip:375-404).  Pinned: the ReLU and its backward (a
    select), every plain product (RN(a b)), g (1 - z) of the GRU backward (1 - z is exact in float64 for an fp32 z and rounds once,
    then a plain product), the clamped side of inv_to_depth (RN(1 / 1e-4f)) and of its backward (0)."""
    pin = lambda v: Interval(v, torch.zeros_like(v))                # noqa: E731
    if op == "act_bwd_relu":
        return [pin(torch.where(d64(b) > 0, d64(a), torch.zeros_like(d64(a))))]
    if op == "act_bwd_sigmoid":                                     # g (y (1 - y)): three roundings
        v = d64(a) * (d64(b) * (1.0 - d64(b)))
        return [Interval(v, 3 * U * v.abs() * SLACK)]
    if op == "act_bwd_tanh":                                        # RN(y y): u y^2; 1 - .: u |1 - y^2|; the product: u
        dd = 1.0 - d64(b) ** 2
        return [Interval(d64(a) * dd, U * d64(a).abs() * (d64(b) ** 2 + 2 * dd.abs()) * SLACK)]
    if op in ("tanh", "sigmoid"):
        return [act_interval(d64(a), torch.zeros_like(d64(a)), op, "exact")]
    if op == "relu":
        return [pin(d64(a).clamp_min(0.0))]
    if op == "mul":
        return [pin(_rn_product(a, b))]
    if op == "mul_bwd":
        return [pin(_rn_product(a, c)), pin(_rn_product(a, b))]
    if op == "gru":                                                 # 1 - z (u), (1 - z) h (u), z q (u), the sum (u)
        z, h, q = d64(a), d64(b), d64(c)
        p1, p2 = (1.0 - z) * h, z * q
        return [Interval(p1 + p2, (2 * U * p1.abs() + U * p2.abs() + U * (p1 + p2).abs()) * SLACK)]
    if op == "gru_bwd":
        g, z, h, q = d64(a), d64(b), d64(c), d64(d)
        v0 = g * (q - h)                                            # the difference and the product round
        omz = (1.0 - z).float()                                     # exact in float64 (fp32 z, |z| >= 2^-29 or 0), one rounding
        assert bool(((z == 0) | (z.abs() >= 2.0 ** -29)).all())
        return [Interval(v0, 2 * U * v0.abs() * SLACK), pin(_rn_product(a, omz)), pin(_rn_product(a, b))]
    if op == "inv_to_depth":
        s, ds, clamped, _, _ = inv_to_depth_terms(a, s0, s1)
        top = float(np.float32(1.0) / THR32)                        # 1.0f / 1e-4f
        sl = torch.where(clamped, torch.ones_like(s), s)
        mid = torch.where(clamped, torch.full_like(s, top), 1.0 / sl)
        half = torch.where(clamped, torch.zeros_like(s), (ds / sl ** 2 + U / sl) * SLACK)                 # 1 / s: ds / s^2, the quotient u
        return [Interval(mid, half)]
    if op == "inv_to_depth_bwd":                                    # ((-g) b) / (s s): three roundings, b and s carried (s twice)
        s, ds, clamped, bb, db = inv_to_depth_terms(b, s0, s1)
        sl = torch.where(clamped, torch.ones_like(s), s)
        mid = torch.where(clamped, torch.zeros_like(s), -d64(a) * bb / sl ** 2)
        half = torch.where(clamped, torch.zeros_like(s), mid.abs() * (3 * U + db / abs(bb) + 2 * ds / sl) * SLACK)
        return [Interval(mid, half)]
    if op == "scale_ch":
        f = b[(torch.arange(a.numel()) // inner) % C].view(a.shape)
        return [pin(_rn_product(a, f))]
    raise KeyError(op)


# ==============================================================================================================================
# the cases (shared by tests/test_pixel_bound_host.py and tests/test_gpu_pixel_bounds.py)
# ==============================================================================================================================
BN_FORCED = [(s, k) for s in ((3, 5, 7, 11), (3, 4, 5, 6, 7), (3, 5, 9, 11), (3, 3, 13, 17)) for k in (1, 7, 64)]
# (shape, reduce_chunk or None = the default, kind)
BN_CASES = ([(s, k, "plain") for s, k in BN_FORCED]
            + [((2, 3, 1, 2), None, "plain"), ((1, 1, 8, 10, 12), None, "plain"), ((2, 4, 40, 52), None, "plain"),
               ((2, 4, 16, 20), None, "offset"), ((3, 5, 7, 11), 7, "planted")])


def bn_inputs(shape, kind, seed):
    """As test_gpu_train_scale._bn_inputs.  "offset": every mean at 10^3 sigma.  "planted": channel 0's bias is -100, so with ReLU
    every y of that channel is exactly 0 (and its gradients are pinned to 0)."""
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    bs = (1, C) + (1,) * (len(shape) - 2)
    sig = 0.5 + 1.5 * torch.rand(C, generator=g)
    mu = 1e3 * sig if kind == "offset" else torch.randn(C, generator=g)
    x = torch.randn(shape, generator=g) * sig.view(bs) + mu.view(bs)
    gy = torch.randn(shape, generator=g) + 0.3 * torch.randn(C, generator=g).view(bs)
    par = {"weight": 0.5 + torch.rand(C, generator=g), "bias": torch.randn(C, generator=g) * 0.2,
           "running_mean": torch.randn(C, generator=g) * 0.1, "running_var": 0.5 + torch.rand(C, generator=g)}
    if kind == "planted":
        par["bias"][0] = -100.0
    return x, gy, par


SAM_CASES = ([(D, hw, hk, "randn") for D in (1, 2, 8, 47, 48) for hw in ((1, 1), (5, 7), (16, 17)) for hk in ("plane", "pixel")]
             + [(8, (5, 7), "pixel", "underflow")])


def sam_inputs(D, hw, hyp_kind, logit_kind, seed, B=2):
    """logits [B,D,h,w] = 2 randn, hypotheses [B,D] (425..935 mm, another range for sample 1) or [B,D,h,w] that differ per pixel,
    g [B,h,w].  "underflow": per pixel one logit 80 and one 16 below the maximum (probabilities ~1e-35 and ~1e-7)."""
    h, w = hw
    g = torch.Generator().manual_seed(seed)
    logits = 2.0 * torch.randn(B, D, h, w, generator=g)
    if logit_kind == "underflow":
        top = logits.max(1).values
        idx = torch.randint(0, D, (B, 1, h, w), generator=g)
        logits.scatter_(1, idx, (top - 80.0).unsqueeze(1))
        logits.scatter_(1, (idx + 1) % D, (top - 16.0).unsqueeze(1))
    ends = [(425.0, 935.0), (510.0, 800.0)]
    hyp = torch.stack([1.0 / torch.linspace(1.0 / ends[b % 2][1], 1.0 / ends[b % 2][0], D) if D > 1 else torch.tensor([680.0 + 40 * b])
                       for b in range(B)])
    if hyp_kind == "pixel":
        hyp = hyp.view(B, D, 1, 1) * (1.0 + 0.02 * torch.rand(B, D, h, w, generator=g))
    return logits, hyp.contiguous(), torch.randn(B, h, w, generator=g)


VA_CASES = ([(S, D, hw, "rand") for S in (1, 2, 12) for D in (1, 8) for hw in ((1, 1), (9, 11), (16, 17))]
            + [(3, 8, (9, 11), "tiny"), (3, 8, (9, 11), "zero")])


def va_inputs(S, D, hw, kind, seed, B=2):
    """sim [B,S,D,h,w] randn (views nearly alike plus noise), weights [B,S,h,w]: rand; "tiny": all in [0, 2e-6]; "zero": view 1's weight
    exactly 0; g [B,D,h,w]."""
    h, w = hw
    g = torch.Generator().manual_seed(seed)
    sim = torch.randn(B, 1, D, h, w, generator=g) + 0.3 * torch.randn(B, S, D, h, w, generator=g)
    wts = torch.rand(B, S, h, w, generator=g)
    if kind == "tiny":
        wts = wts * 2e-6
    if kind == "zero":
        wts[:, 1] = 0.0
    return sim.contiguous(), wts, torch.randn(B, D, h, w, generator=g)


CU_CASES = ([(hw, "randn", "dense") for hw in ((1, 1), (1, 9), (9, 1), (2, 2), (16, 17), (21, 28))]
            + [((16, 17), "dominant", "dense"), ((16, 17), "randn", "corners")])


def cu_inputs(hw, mask_kind, gup_kind, seed, B=2):
    """inv [B,1,h,w] in (0, 1), mask [B,36,h,w] randn ("dominant": one tap per (pixel, sub-pixel) at +30), gup [B,2h,2w] dense or
    non-zero in the four corner output pixels only."""
    h, w = hw
    g = torch.Generator().manual_seed(seed)
    inv = torch.rand(B, 1, h, w, generator=g)
    mask = torch.randn(B, 36, h, w, generator=g)
    if mask_kind == "dominant":
        k = torch.randint(0, 9, (B, 1, 4, h, w), generator=g)
        mask = mask.view(B, 9, 4, h, w).scatter(1, k, 30.0).view(B, 36, h, w).contiguous()
    gup = torch.randn(B, 2 * h, 2 * w, generator=g)
    if gup_kind == "corners":
        keep = torch.zeros(2 * h, 2 * w)
        keep[0, 0] = keep[0, -1] = keep[-1, 0] = keep[-1, -1] = 1.0
        gup = gup * keep
    return inv, mask, gup


PW_NS = (1, 255, 256, 257, 1000)
PW_RANGE = (1.0 / 935.0, 1.0 / 425.0)
PW_SCALE = [(inner, C) for inner in (1, 7) for C in (1, 5)]


def clamp_edge_lo():
    """An fp32 ``lo`` whose min_disp = 1 / (1 / lo) is exactly 1e-4f: with inv = 0 the kernel's s sits ON the clamp's threshold."""
    lo = THR32
    for _ in range(64):
        for cand in (lo, np.nextafter(lo, np.float32(0))):
            if _disp_fp32(cand, PW_RANGE[1])[0] == THR32:
                return float(cand)
        lo = np.nextafter(lo, np.float32(1))
    raise AssertionError("no fp32 lo round-trips to 1e-4f")


def pw_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(n, generator=g)                         # noqa: E731
    t_ = dict(g=r(), x=r(), x2=r(), h=r(), q=r(), z=torch.sigmoid(r()), y_sig=torch.sigmoid(r()), y_tanh=torch.tanh(r()),
              y_relu=r().clamp_min(0.0), inv=r())
    return t_


def pw_calls(t_, n):
    """Every EFFI_PW_* op as (name, op, kwargs of ops.pointwise / pw_emulate / pw_interval, number of outputs)."""
    lo, hi = PW_RANGE
    calls = [("act_bwd_relu", dict(a=t_["g"], b=t_["y_relu"]), 1), ("act_bwd_sigmoid", dict(a=t_["g"], b=t_["y_sig"]), 1),
             ("act_bwd_tanh", dict(a=t_["g"], b=t_["y_tanh"]), 1), ("tanh", dict(a=t_["x"]), 1), ("relu", dict(a=t_["x"]), 1),
             ("sigmoid", dict(a=t_["x"]), 1), ("mul", dict(a=t_["x"], b=t_["x2"]), 1),
             ("mul_bwd", dict(a=t_["g"], b=t_["x"], c=t_["x2"]), 2), ("gru", dict(a=t_["z"], b=t_["h"], c=t_["q"]), 1),
             ("gru_bwd", dict(a=t_["g"], b=t_["z"], c=t_["h"], d=t_["q"]), 3),
             ("inv_to_depth", dict(a=t_["inv"], s0=lo, s1=hi), 1), ("inv_to_depth_bwd", dict(a=t_["g"], b=t_["inv"], s0=lo, s1=hi), 1)]
    for inner, C in PW_SCALE:
        f = torch.linspace(0.5, 2.5, C) if C > 1 else torch.tensor([1.7])
        calls.append(("scale_ch", dict(a=t_["x"], b=f * 1.0000001, inner=inner, C=C), 1))
    return calls
