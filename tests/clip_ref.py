"""Reference of the global gradient norm, the clip coefficient and the clipped AdamW step (csrc/optim.hip: gradnorm_partial_kernel,
gradnorm_finish_kernel, the CLIP instantiations of the AdamW kernels) -- the helper of tests/test_grad_clip_host.py and
tests/test_gpu_grad_clip.py, on top of tests/optim_ref.py.

  exact norm       math.sqrt(math.fsum(x * x)) over all gradient elements as doubles: the products are exact (24-bit by 24-bit
                   significands), fsum is exactly rounded, so this is the true norm to within 2 roundings of a double.
  admissible norms the fp32 values within one fp32 ulp of it.  The kernel adds exact squares in double: relative error at most
                   N 2^-53 on the sum, half of that on the root -- for any N a test can hold, orders of magnitude below 2^-24.  The
                   only freedom left is the final rounding to fp32; anything further off is a bug.
  coefficient      the three fp32 operations of the header comment, evaluated with numpy fp32 scalars (IEEE, one rounding each):
                   den = norm + 1e-6f;  coef = fl32(max_norm) / den;  coef = 1 if coef > 1 else coef  (NaN stays NaN).
  gradient seen    g' = fl32(g * coef): one IEEE product, so it is KNOWN exactly and ``optim_ref.adamw_step_ref(p, g', m, v, ...)``
  by the update    bounds every element of the clipped step.

The chain a test walks: the norm the kernel returned must be admissible; the coefficient it returned must be ``coef_ref`` of that
returned norm, bitwise; the element intervals are those of that coefficient.  Nothing is compared with the code under test.

``adamw_step_ref_g`` is ``optim_ref.adamw_step_ref`` for a gradient that is itself only known to within a bound -- what torch's
``clip_grad_norm_`` leaves in ``p.grad``, whose norm carries torch's own fp32 summation error.
"""
import math

import numpy as np
import torch

import optim_ref as R

SIZES = (1, 3, 2047, 2048, 2049, 6149, 0)       # the chunk of csrc/optim.hip is 2048 elements; 6149 = 3 chunks + 5, odd tail
MAX_NORMS = (1.0, 0.37, 1e4)


def exact_norm(grads):
    """grads: fp32 tensors (any device).  -> the 2-norm over all their elements as a double."""
    sq = []
    for g in grads:
        x = g.detach().cpu().reshape(-1).double().numpy()
        sq.extend((x * x).tolist())                                         # exact: fp32 values squared in double
    return math.sqrt(math.fsum(sq))


def admissible_norms(exact):
    """The fp32 values within one fp32 ulp of the double ``exact`` (as a set of numpy fp32 scalars' bit patterns -> values)."""
    with np.errstate(over="ignore"):
        r = np.float32(exact)
    if not np.isfinite(r):
        return [r]
    ulp = float(np.spacing(np.abs(r))) if r != 0 else 2.0 ** -149
    cands = {float(r), float(np.nextafter(r, np.float32(np.inf))), float(np.nextafter(r, np.float32(-np.inf)))}
    return [np.float32(c) for c in sorted(cands) if abs(c - exact) <= ulp and c >= 0]


def is_admissible(norm, exact):
    n = np.float32(norm)
    return any(n.tobytes() == a.tobytes() or (np.isnan(n) and np.isnan(a)) for a in admissible_norms(exact))


def coef_ref(norm, max_norm):
    """The coefficient of an fp32 ``norm`` (the three operations, numpy fp32)."""
    with np.errstate(all="ignore"):
        den = np.float32(norm) + np.float32(1e-6)
        coef = np.float32(max_norm) / den
        return np.float32(1.0) if coef > np.float32(1.0) else np.float32(coef)


def same_bits(a, b):
    """fp32 equality by bit pattern, with every NaN equal to every NaN."""
    a, b = np.float32(a), np.float32(b)
    return bool(np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


def scaled(g, coef):
    """g' = fl32(g * coef) as an fp32 CPU tensor: the gradient the clipped update works with."""
    with np.errstate(all="ignore"):
        return torch.from_numpy(g.detach().cpu().numpy().astype(np.float32) * np.float32(coef))


def clipped_step_ref(p, g, m, v, coef, step_new, lr, **kw):
    """``optim_ref.adamw_step_ref`` on g' = fl32(g * coef)."""
    return R.adamw_step_ref(p, scaled(g, coef), m, v, step_new, lr, **kw)


def adamw_step_ref_g(p, g_val, g_err, m, v, step_new, lr, beta1=R.BETAS[0], beta2=R.BETAS[1], eps=R.ADAM_EPS, wd=0.0, scalars="double"):
    """The walk of ``optim_ref`` with the gradient given as float64 values ``g_val`` and a bound ``g_err`` on |computed g - g_val|
    (arrays shaped like p); gradual underflow is charged as with ``normal_only=False``."""
    f64 = lambda x: R.B(x.detach().cpu().double().numpy())                  # noqa: E731
    R.UNDERFLOW = 2.0 ** -149
    try:
        P, M, V = f64(p), f64(m), f64(v)
        G = R.B(np.asarray(g_val, np.float64).reshape(P.val.shape), np.asarray(g_err, np.float64).reshape(P.val.shape))
        dec, w1, b2, w2, a, c2, e = R._scalars(step_new, float(lr), beta1, beta2, eps, wd, scalars)
        pd = R.mul(P, dec)
        m1 = R.add(M, R.mul(R.sub(G, M), w1))
        v1 = R.add(R.mul(V, b2), R.mul(R.mul(w2, G), G))
        den = R.add(R.div(R.sqrt(v1), c2), e)
        p1 = R.sub(pd, R.div(R.mul(a, m1), den))
        return {"p": (p1.val, p1.err), "exp_avg": (m1.val, m1.err), "exp_avg_sq": (v1.val, v1.err)}
    finally:
        R.UNDERFLOW = 0.0


def torch_clip_gradient_interval(g, exact, max_norm, torch_norm):
    """What ``clip_grad_norm_`` leaves in p.grad, as (values, bound): g * c with c = min(1, max_norm / (exact + 1e-6)) in double, and
    |g c| times torch's own relative norm error (measured against the exact norm) plus three fp32 roundings (its fp32 sum of norm and
    1e-6, its division, its product), plus one subnormal spacing."""
    rel = abs(float(torch_norm) - exact) / exact
    c = min(1.0, max_norm / (exact + 1e-6))
    val = g.detach().cpu().double().numpy() * c
    return val, np.abs(val) * (rel + 3 * R.EPS32 + 2.0 ** -50) + 2.0 ** -149, rel
