"""Float64 restatement of ONE AdamW step (torch.optim.AdamW, amsgrad=False, maximize=False) with an absolute error bound for every
element of p', exp_avg' and exp_avg_sq' -- the reference of tests/test_optim_host.py and tests/test_gpu_optim.py.

The bound is a running error analysis in the style of DESIGN.md section 2.6, walked along the operation order that the header
comment of csrc/optim.hip documents:

    scalars:  dec = 1 - lr wd,  w1 = 1 - beta1,  b2 = beta2,  w2 = 1 - beta2,  a = lr / bc1,  c2 = sqrt(bc2),  e = eps
              with bc_k = 1 - beta_k^t, t the NEW step
    element:  pd = p dec;   d = g - m;  t1 = d w1;  m' = m + t1;   t2 = v b2;  t3 = w2 g;  t4 = t3 g;  v' = t2 + t4;
              s = sqrt(v');  q = s / c2;  den = q + e;   n = a m';  u = n / den;  p' = pd - u

Every quantity is a pair (value, err): value is the float64 evaluation from the exact fp32 inputs and the exact (double) scalars,
err bounds |computed fp32 quantity - value|.  An operation first propagates the errors of its operands through the exact operation
(sum of the errors for + and -, |a| eb + |b| ea + ea eb for a product, (ea + |a / b| eb) / (|b| - eb) for a quotient,
ea / (sqrt(a) + sqrt(a - ea)) for a square root) and then adds the rounding of its own fp32 result, 2^-24 (|value| + err): that
holds through the cancellations of g - m and pd - u too, because it is charged on the result, whatever the operands were.  The
float64 evaluation's own rounding is charged the same way with 2^-52 per operation.  fp32 division and square root are correctly
rounded on both sides (IEEE on the CPU; hipcc's default on the GPU, which csrc/optim.hip keeps).  Nothing is left to a share of
outliers or to a tensor's peak: every element has its own interval.

Scalars.  ``scalars="double"`` is the kernel's form and that of torch's non-capturable step: each scalar formed in double and
rounded once to fp32 (2^-24 |scalar|).  Two scalars get one rounding more, because the cases include ``lr`` given as an fp32
tensor and torch then forms them in fp32 0-dim arithmetic: a = lr / fl32(bc1) rounds its divisor first (2 x 2^-24), and
1 - fl32(lr fl32(wd)) carries 2 x 2^-24 lr wd besides its own rounding.  The bound admits the worse of the two forms for both, so
one interval serves the kernel and torch on the CPU.  A scalar that is exact in fp32 in every form (dec = 1 when lr wd = 0, a = 0
when lr = 0) has no error.
``scalars="fp32"`` is for torch's CAPTURABLE multi-tensor step on the device only (never for the kernel under test): it forms the
bias corrections from the fp32 step tensor in fp32, bc_k = 1 - pow(fl32(beta_k), t), and 1 - 0.999 cancels -- at t = 1 the relative
error of bc2 is about 1000 x 2^-24.  Its scalars are walked as torch forms them: beta rounded to fp32, t multiplications' worth of
that rounding in the power, 16 ulp for powf itself (the accuracy the OpenCL C specification asks of pow, which the device library
is written to), the subtraction, lr / bc1 as reciprocal(bc1 / lr), sqrt(bc2).

Inputs (``make_inputs``): |g| in {0} u [1e-12, 1e3], m and v as such gradients leave them (|m| in {0} u [1e-12, 1e3], v in
{0} u [1e-24, 1e6], both zero for a fresh state), |p| in {0} u [1e-6, 10].  With these no intermediate of the list above is
subnormal (``adamw_step_ref`` asserts it): subnormals are excluded because the flush-to-zero settings of CPU and GPU are not part of
this feature.
"""
import itertools

import numpy as np
import torch

EPS32 = 2.0 ** -24
EPS = EPS32 + 2.0 ** -52                        # rounding of an fp32 result + of the float64 evaluation of the same operation
TINY32 = 2.0 ** -126                            # smallest normal fp32

STEPS = (0, 1, 1000)                            # old step: 0 -> 1 (fresh state), 1 -> 2, 1000 -> 1001 (beta1^t underflows bc1 to 1 in fp32, bc2 < 1)
WDS = (0.0, 1e-3)                               # 1e-3: the reference's --wd default
LRS = ("float", "tensor", "zero")               # 2e-4 as a Python float, 2e-4 as an fp32 tensor, 0
LR, BETAS, ADAM_EPS = 2e-4, (0.9, 0.999), 1e-8
CASES = tuple(itertools.product(STEPS, WDS, LRS))


def lr_value(kind):
    """The exact learning rate of a case as a double: a tensor lr IS fl32(2e-4)."""
    return {"float": LR, "tensor": float(np.float32(LR)), "zero": 0.0}[kind]


def lr_arg(kind, device="cpu"):
    return torch.tensor(LR, dtype=torch.float32, device=device) if kind == "tensor" else lr_value(kind)


class B:
    """value (float64 array) with a bound on |computed - value|"""

    def __init__(self, val, err=0.0):
        self.val = np.asarray(val, dtype=np.float64)
        self.err = np.broadcast_to(np.asarray(err, dtype=np.float64), self.val.shape) if np.ndim(err) == 0 else np.asarray(err, np.float64)


UNDERFLOW = 0.0                                 # absolute rounding term per operation: see adamw_step_ref(normal_only=False)


def _rounded(val, err):
    return B(val, err + EPS * (np.abs(val) + err) + UNDERFLOW)


def add(a, b):
    return _rounded(a.val + b.val, a.err + b.err)


def sub(a, b):
    return _rounded(a.val - b.val, a.err + b.err)


def mul(a, b):
    return _rounded(a.val * b.val, np.abs(a.val) * b.err + np.abs(b.val) * a.err + a.err * b.err)


def div(a, b):
    lo = np.abs(b.val) - b.err
    assert np.all(lo > 0), "divisor interval reaches zero"
    q = a.val / b.val
    return _rounded(q, (a.err + np.abs(q) * b.err) / lo)


def sqrt(a):
    assert np.all(a.val >= 0)
    s = np.sqrt(a.val)
    den = s + np.sqrt(np.maximum(a.val - a.err, 0.0))
    err = np.where(den > 0, a.err / np.where(den > 0, den, 1.0), np.sqrt(a.err))
    return _rounded(s, err)


def _scalars(step_new, lr, beta1, beta2, eps, wd, scalars):
    t = float(step_new)
    one = lambda x, k=1: B(x, (k * EPS32 + 2.0 ** -50) * abs(x))          # noqa: E731  k fp32 roundings + the double arithmetic behind x
    dec_v = 1.0 - lr * wd
    dec = B(dec_v, 0.0 if lr * wd == 0.0 else (EPS32 + 2.0 ** -50) * abs(dec_v) + 2 * EPS32 * lr * wd)
    w1, b2, w2, e = one(1.0 - beta1), one(beta2), one(1.0 - beta2), one(eps)
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    if scalars == "double":
        a = B(0.0) if lr == 0.0 else one(lr / bc1, 2)
        c2 = one(np.sqrt(bc2))
    elif scalars == "fp32":
        def bc32(beta):
            pw = beta ** t
            rel = np.expm1(t * np.log1p(EPS32)) + 32 * EPS32                # fl32(beta)^t, then powf within 16 ulp
            return sub(B(1.0), B(pw, pw * rel * (1 + EPS32)))
        c2 = sqrt(bc32(beta2))
        a = B(0.0) if lr == 0.0 else div(B(1.0), div(bc32(beta1), B(lr, EPS32 * lr)))
    else:
        raise ValueError(scalars)
    return dec, w1, b2, w2, a, c2, e


def adamw_step_ref(p, g, m, v, step_new, lr, beta1=BETAS[0], beta2=BETAS[1], eps=ADAM_EPS, wd=0.0, scalars="double", normal_only=True):
    """p, g, m, v: fp32 tensors (any device) BEFORE the step; step_new: the incremented counter; lr: the exact rate as a double
    (``lr_value``).  -> {"p": (value, err), "exp_avg": (value, err), "exp_avg_sq": (value, err)}, float64 arrays shaped like p.
    ``normal_only`` (the drawn inputs): asserts that no intermediate is subnormal.  ``normal_only=False`` is for gradients a real
    model produced, whose squares may underflow: both sides then compute with gradual underflow (IEEE; the default of the CPU and
    of hipcc for this GPU), where a result below 2^-126 is rounded to a multiple of 2^-149 -- every operation is charged that
    spacing as an absolute term besides its relative one."""
    global UNDERFLOW
    UNDERFLOW = 0.0 if normal_only else 2.0 ** -149
    try:
        return _walk(p, g, m, v, step_new, lr, beta1, beta2, eps, wd, scalars, normal_only)
    finally:
        UNDERFLOW = 0.0


def _walk(p, g, m, v, step_new, lr, beta1, beta2, eps, wd, scalars, normal_only):
    f64 = lambda x: B(x.detach().cpu().double().numpy())                    # noqa: E731
    P, G, M, V = f64(p), f64(g), f64(m), f64(v)
    dec, w1, b2, w2, a, c2, e = _scalars(step_new, float(lr), beta1, beta2, eps, wd, scalars)
    pd = mul(P, dec)
    d = sub(G, M)
    t1 = mul(d, w1)
    m1 = add(M, t1)
    t2 = mul(V, b2)
    t3 = mul(w2, G)
    t4 = mul(t3, G)
    v1 = add(t2, t4)
    s = sqrt(v1)
    q = div(s, c2)
    den = add(q, e)
    n = mul(a, m1)
    u = div(n, den)
    p1 = sub(pd, u)
    for name, x in (("pd", pd), ("d", d), ("t1", t1), ("m1", m1), ("t2", t2), ("t3", t3), ("t4", t4), ("v1", v1), ("s", s), ("q", q),
                    ("den", den), ("n", n), ("u", u), ("p1", p1)):
        av = np.abs(x.val)
        assert not normal_only or np.all((av == 0) | (av >= 4 * TINY32)), f"intermediate {name} comes within reach of the subnormal range: choose other inputs"
    return {"p": (p1.val, p1.err), "exp_avg": (m1.val, m1.err), "exp_avg_sq": (v1.val, v1.err)}


def _signed_log_uniform(gen, n, lo, hi, p_zero):
    mag = torch.exp(torch.empty(n, dtype=torch.float64).uniform_(float(np.log(lo)), float(np.log(hi)), generator=gen))
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    x = (mag * sign).float()
    x[torch.rand(n, generator=gen) < p_zero] = 0.0
    return x


def make_inputs(numel, seed, fresh):
    """-> (p, g, m, v) fp32 CPU tensors of ``numel`` elements in the ranges of the module docstring; ``fresh``: m = v = 0."""
    gen = torch.Generator().manual_seed(seed)
    p = _signed_log_uniform(gen, numel, 1e-6, 10.0, 0.05)
    g = _signed_log_uniform(gen, numel, 1e-12, 1e3, 0.1)
    if fresh:
        return p, g, torch.zeros(numel), torch.zeros(numel)
    m = _signed_log_uniform(gen, numel, 1e-12, 1e3, 0.05)
    v = _signed_log_uniform(gen, numel, 1e-12, 1e3, 0.05).square()
    v = torch.where((v > 0) & (v < 1e-24), torch.full_like(v, 1e-24), v)
    return p, g, m, v


def outside(got, ref):
    """Number of elements of the fp32 tensor ``got`` outside [value - err, value + err], and the worst |got - value| / err."""
    val, err = ref
    dist = np.abs(got.detach().cpu().double().numpy().reshape(val.shape) - val)
    bad = dist > err
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, dist / np.where(err > 0, err, 1.0), np.where(dist > 0, np.inf, 0.0))
    return int(bad.sum()), float(ratio.max()) if ratio.size else 0.0
