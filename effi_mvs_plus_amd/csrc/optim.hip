// The optimizer step of the reference's train_sample (train.py:263, optimizer.step(), on the AdamW built at train.py:441): decoupled
// weight-decay AdamW (torch.optim.AdamW, amsgrad=False, maximize=False) over up to AW_MAX_T parameter tensors per call.  torch's
// capturable AdamW is a chain of _foreach_* operators, each cut into several launches; here one call is two launches whatever the
// number of tensors: the step counters, then every element of every tensor.
//
// Tables travel BY VALUE (as the loss of metrics.hip): the entry packs the caller's host arrays into the kernel argument, so there
// is no device-side table, no copy and no pinned buffer; a captured launch holds the pointers in its node and a replay needs nothing
// from the host.  The grid is one workgroup per chunk of AW_CHUNK elements of ONE tensor; the argument carries the running sum of
// chunks per tensor and a workgroup finds its tensor by bisecting it.  A tensor without elements takes no chunk.
//
// Step counter: `step` is a 0-dim fp32 device tensor per parameter, as in torch's capturable AdamW, which increments it FIRST and
// uses the new value.  adamw_step_kernel (one thread per tensor) increments the n counters; stream order makes adamw_update_kernel,
// launched after it, read the new value in every workgroup.  No workgroup of the update kernel writes a counter.
//
// Arithmetic.  Scalars, once per workgroup, formed in double and rounded ONCE to fp32 (t = the new step as double, lr = the value
// argument or (double)*lr_dev when lr_dev is given -- a scheduler fills that tensor between replays):
//     bc1 = 1 - beta1^t,  bc2 = 1 - beta2^t                      (double)
//     dec = fl32(1 - lr * wd)     w1 = fl32(1 - beta1)     b2 = fl32(beta2)     w2 = fl32(1 - beta2)
//     a   = fl32(lr / bc1)        c2 = fl32(sqrt(bc2))     e  = fl32(eps)
// Per element, fp32, one rounding per operation in exactly this order (the library is built with -ffp-contract=off: nothing is
// fused; hipcc's default gives correctly rounded fp32 division and square root, and that default is kept: no fast-math flag, no
// reciprocal intrinsics here):
//     pd = p * dec
//     d  = g - m;          t1 = d * w1;        m' = m + t1
//     t2 = v * b2;         t3 = w2 * g;        t4 = t3 * g;        v' = t2 + t4
//     s  = sqrt(v');       q  = s / c2;        den = q + e
//     n  = a * m';         u  = n / den;       p' = pd - u
// tests/optim_ref.py walks this list to bound every element.
//
// Memory: 128-bit accesses where all four pointers of a tensor are 16-byte aligned (a chunk starts a multiple of AW_CHUNK elements
// into its tensor, so the tensor's alignment is the chunk's), scalar accesses for the last numel % 4 elements, and for the whole
// tensor otherwise -- weight gradients are slices of arena blocks and a user's tensor may be a view at an odd offset, so alignment
// is a per-tensor run-time fact.  Writes stay inside [ptr, ptr + numel) of p, exp_avg, exp_avg_sq and the one element of step;
// g is only read.
//
// Global gradient norm, clipping and the non-finite guard (torch.nn.utils.clip_grad_norm_ between backward() and step(), and the
// skipped step of a gradient scaler, inside the step).  gradnorm_partial_kernel: the same chunking over up to GN_MAX_T gradients per
// call, one workgroup per chunk; per element sq = (double)g * (double)g, which is EXACT (a 24-bit by 24-bit product fits in 53
// bits); a thread adds its elements in a fixed order in double, the 64 lanes of a wave are folded by a fixed shuffle tree, the four
// waves through LDS, and thread 0 writes partial[blockIdx.x] as a double.  No atomics: the order of every addition is a function of
// the layout alone, so two runs agree bitwise; every slot is written on every call, so the workspace is never zeroed.
// gradnorm_finish_kernel (one workgroup) adds the n_partial doubles -- a strided pass per thread, then the same tree -- and then, in
// this order:
//     norm  = (float)sqrt(total)                 (double sqrt, one rounding to fp32)
//     den   = norm + 1e-6f                       (fp32)
//     coef  = (float)max_norm / den              (fp32, correctly rounded)
//     coef  = coef > 1.0f ? 1.0f : coef          (NaN stays NaN)
//     finite = isfinite(norm)
// and writes clip[0] = norm, clip[1] = coef, clip[2] = finite ? 1 : 0, clip[3] = 0; a given `skipped` counter (int64) is incremented
// when !finite.  The sum itself cannot overflow in double (2^31 chunks of 2048 squares below 2^256), so "non-finite" is an inf or a
// NaN among the gradients -- or a norm above FLT_MAX, which rounds to inf in fp32 and counts as non-finite as well.
// The clipped step (CLIP = true instantiations): a workgroup reads clip[1] and clip[2] once, next to its scalars; with `skip` set and
// clip[2] == 0 it returns before it writes anything, and the step kernel increments no counter; otherwise each element uses
// g' = g * coef (one fp32 rounding) in the list above.  coef == 1.0f gives g' == g bitwise: a step that does not clip is the
// unclipped step.
#include "common.hpp"

#include <climits>
#include <cstdint>

namespace {

constexpr int AW_THREADS = 256;
constexpr int AW_CHUNK = 2048;                  // elements per workgroup: two 128-bit accesses per thread and array
constexpr int AW_MAX_T = 64;                    // tensors per call: 56 bytes each in the argument

struct AdamWArgs {              // by-value kernel argument
    float* p[AW_MAX_T];
    const float* g[AW_MAX_T];
    float* m[AW_MAX_T];
    float* v[AW_MAX_T];
    float* step[AW_MAX_T];
    long numel[AW_MAX_T];
    int chunk_end[AW_MAX_T];    // chunks of tensors 0 .. i (running sum): tensor i owns chunks [chunk_end[i - 1], chunk_end[i])
    double lr, beta1, beta2, eps, wd;
    const float* lr_dev;
    int n;
    const float* clip;          // the clipped entry only: the four floats gradnorm_finish_kernel wrote
    int skip;                   // the clipped entry only: leave everything as it is when clip[2] == 0
};
static_assert(sizeof(AdamWArgs) <= 3584, "kernel arguments: HIP allows 4 KB; keep a margin for the hidden ones");
static_assert(AW_CHUNK % 4 == 0 && AW_CHUNK % AW_THREADS == 0, "a chunk starts 16-byte aligned in an aligned tensor");

// CLIP = false is the unclipped entry's kernel: a.clip and a.skip are not looked at
template <bool CLIP>
__global__ __launch_bounds__(64) void adamw_step_kernel(AdamWArgs a) {
    if constexpr (CLIP) {
        if (a.skip && a.clip[2] == 0.0f) return;
    }
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < a.n) a.step[i][0] += 1.0f;
}

struct AdamWScalars {
    float dec, w1, b2, w2, a, c2, e;
};

__device__ __forceinline__ void adamw_element(const AdamWScalars& k, float& p, float g, float& m, float& v) {
    const float pd = p * k.dec;
    const float d = g - m;
    const float t1 = d * k.w1;
    const float m1 = m + t1;
    const float t2 = v * k.b2;
    const float t3 = k.w2 * g;
    const float t4 = t3 * g;
    const float v1 = t2 + t4;
    const float s = sqrtf(v1);
    const float q = s / k.c2;
    const float den = q + k.e;
    const float n = k.a * m1;
    const float u = n / den;
    p = pd - u;
    m = m1;
    v = v1;
}

template <bool CLIP>
__global__ __launch_bounds__(AW_THREADS) void adamw_update_kernel(AdamWArgs a) {
    __shared__ AdamWScalars ks;
    __shared__ float kclip[2];                  // CLIP: coefficient, finite flag
    const int c = blockIdx.x;
    int lo = 0, hi = a.n - 1;                   // first tensor whose running sum exceeds c (uniform)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.chunk_end[mid] > c) hi = mid;
        else lo = mid + 1;
    }
    const int t = lo;
    const long numel = a.numel[t];
    const long i0 = (long)(c - (t ? a.chunk_end[t - 1] : 0)) * AW_CHUNK;
    if (i0 >= numel) return;                    // cannot happen for a table aw_pack built; keeps a wrong one inside its tensors
    const int len = (int)(numel - i0 < AW_CHUNK ? numel - i0 : AW_CHUNK);
    if (threadIdx.x == 0) {
        const double st = (double)a.step[t][0];
        const double lr = a.lr_dev ? (double)a.lr_dev[0] : a.lr;
        const double bc1 = 1.0 - pow(a.beta1, st), bc2 = 1.0 - pow(a.beta2, st);
        ks.dec = (float)(1.0 - lr * a.wd);
        ks.w1 = (float)(1.0 - a.beta1);
        ks.b2 = (float)a.beta2;
        ks.w2 = (float)(1.0 - a.beta2);
        ks.a = (float)(lr / bc1);
        ks.c2 = (float)sqrt(bc2);
        ks.e = (float)a.eps;
        if constexpr (CLIP) kclip[0] = a.clip[1], kclip[1] = a.clip[2];
    }
    __syncthreads();
    const AdamWScalars k = ks;
    float coef = 1.0f;
    if constexpr (CLIP) {
        if (a.skip && kclip[1] == 0.0f) return;     // uniform: nothing of this chunk is written
        coef = kclip[0];
    }
    float* __restrict__ p = a.p[t] + i0;
    const float* __restrict__ g = a.g[t] + i0;
    float* __restrict__ m = a.m[t] + i0;
    float* __restrict__ v = a.v[t] + i0;
    const bool aligned = (((uintptr_t)a.p[t] | (uintptr_t)a.g[t] | (uintptr_t)a.m[t] | (uintptr_t)a.v[t]) & 15) == 0;
    int done = 0;
    if (aligned) {
        const int n4 = len >> 2;
        for (int j = threadIdx.x; j < n4; j += AW_THREADS) {
            float4 pv = reinterpret_cast<const float4*>(p)[j];
            float4 gv = reinterpret_cast<const float4*>(g)[j];
            float4 mv = reinterpret_cast<const float4*>(m)[j];
            float4 vv = reinterpret_cast<const float4*>(v)[j];
            if constexpr (CLIP) gv.x = gv.x * coef, gv.y = gv.y * coef, gv.z = gv.z * coef, gv.w = gv.w * coef;
            adamw_element(k, pv.x, gv.x, mv.x, vv.x);
            adamw_element(k, pv.y, gv.y, mv.y, vv.y);
            adamw_element(k, pv.z, gv.z, mv.z, vv.z);
            adamw_element(k, pv.w, gv.w, mv.w, vv.w);
            reinterpret_cast<float4*>(p)[j] = pv;
            reinterpret_cast<float4*>(m)[j] = mv;
            reinterpret_cast<float4*>(v)[j] = vv;
        }
        done = n4 << 2;
    }
    for (int j = done + threadIdx.x; j < len; j += AW_THREADS) {
        float pj = p[j], mj = m[j], vj = v[j], gj = g[j];
        if constexpr (CLIP) gj = gj * coef;
        adamw_element(k, pj, gj, mj, vj);
        p[j] = pj;
        m[j] = mj;
        v[j] = vj;
    }
}

// Checks the arguments and packs the table; *chunks = workgroups of the update launch (0: every tensor is empty)
int aw_pack(float* const* p, const float* const* g, float* const* exp_avg, float* const* exp_avg_sq, float* const* step,
            const long* numel, int n, double lr, const float* lr_dev, double beta1, double beta2, double eps, double weight_decay,
            AdamWArgs* out, int* chunks) {
    if (!p || !g || !exp_avg || !exp_avg_sq || !step || !numel || n < 1 || n > AW_MAX_T) return EFFI_ERR_BADARG;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) return EFFI_ERR_BADARG;
    AdamWArgs a = {};
    long total = 0;
    for (int i = 0; i < n; ++i) {
        if (!p[i] || !g[i] || !exp_avg[i] || !exp_avg_sq[i] || !step[i] || numel[i] < 0) return EFFI_ERR_BADARG;
        total += numel[i] / AW_CHUNK + (numel[i] % AW_CHUNK != 0);
        if (total > INT_MAX) return EFFI_ERR_BADARG;            // the grid's x extent
        a.p[i] = p[i], a.g[i] = g[i], a.m[i] = exp_avg[i], a.v[i] = exp_avg_sq[i], a.step[i] = step[i];
        a.numel[i] = numel[i];
        a.chunk_end[i] = (int)total;
    }
    a.lr = lr, a.beta1 = beta1, a.beta2 = beta2, a.eps = eps, a.wd = weight_decay;
    a.lr_dev = lr_dev;
    a.n = n;
    *out = a;
    *chunks = (int)total;
    return EFFI_OK;
}

// ---- global gradient norm ----
constexpr int GN_MAX_T = 128;                   // gradients per call: 20 bytes each in the argument

struct GradNormArgs {           // by-value kernel argument
    const float* g[GN_MAX_T];
    long numel[GN_MAX_T];
    int chunk_end[GN_MAX_T];    // running sum of chunks, as AdamWArgs::chunk_end
    double* partial;            // one double per chunk of this call
    int n;
};
static_assert(sizeof(GradNormArgs) <= 3584, "kernel arguments: HIP allows 4 KB; keep a margin for the hidden ones");

// sum over the workgroup in a fixed order: lanes by a shuffle tree, waves through LDS; the result is valid in thread 0
__device__ __forceinline__ double gn_block_sum(double acc, double* ws) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (ws[0] + ws[1]) + (ws[2] + ws[3]);
}
static_assert(AW_THREADS == 256, "gn_block_sum folds four waves");

__device__ __forceinline__ double gn_sq(float g) { return (double)g * (double)g; }

__global__ __launch_bounds__(AW_THREADS) void gradnorm_partial_kernel(GradNormArgs a) {
    __shared__ double ws[AW_THREADS / 64];
    const int c = blockIdx.x;
    int lo = 0, hi = a.n - 1;                   // first tensor whose running sum exceeds c (uniform)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.chunk_end[mid] > c) hi = mid;
        else lo = mid + 1;
    }
    const int t = lo;
    const long numel = a.numel[t];
    const long i0 = (long)(c - (t ? a.chunk_end[t - 1] : 0)) * AW_CHUNK;
    // (i0 >= numel cannot happen for a table gn_pack built; a wrong one reads nothing and still writes its slot)
    const int len = i0 >= numel ? 0 : (int)(numel - i0 < AW_CHUNK ? numel - i0 : AW_CHUNK);
    const float* __restrict__ g = a.g[t] + i0;
    double acc = 0.0;
    int done = 0;
    if (((uintptr_t)a.g[t] & 15) == 0) {
        const int n4 = len >> 2;
        for (int j = threadIdx.x; j < n4; j += AW_THREADS) {
            const float4 gv = reinterpret_cast<const float4*>(g)[j];
            acc += gn_sq(gv.x);
            acc += gn_sq(gv.y);
            acc += gn_sq(gv.z);
            acc += gn_sq(gv.w);
        }
        done = n4 << 2;
    }
    for (int j = done + threadIdx.x; j < len; j += AW_THREADS) acc += gn_sq(g[j]);
    const double total = gn_block_sum(acc, ws);
    if (threadIdx.x == 0) a.partial[c] = total;
}

__global__ __launch_bounds__(AW_THREADS) void gradnorm_finish_kernel(const double* __restrict__ partial, long n_partial, float max_norm,
                                                                     float* __restrict__ clip, long long* __restrict__ skipped) {
    __shared__ double ws[AW_THREADS / 64];
    double acc = 0.0;
    for (long j = threadIdx.x; j < n_partial; j += AW_THREADS) acc += partial[j];
    const double total = gn_block_sum(acc, ws);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(total);
        const float den = norm + 1e-6f;
        float coef = max_norm / den;
        coef = coef > 1.0f ? 1.0f : coef;
        const bool finite = isfinite(norm);
        clip[0] = norm, clip[1] = coef, clip[2] = finite ? 1.0f : 0.0f, clip[3] = 0.0f;
        if (skipped && !finite) skipped[0] += 1;
    }
}

// chunks of n tensors, or -1: a null array, n < 0, a negative size, more than INT_MAX chunks
long gn_chunks(const long* numel, int n) {
    if (n < 0 || (n > 0 && !numel)) return -1;
    long total = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0) return -1;
        total += numel[i] / AW_CHUNK + (numel[i] % AW_CHUNK != 0);
        if (total > INT_MAX) return -1;
    }
    return total;
}

int gn_pack(const float* const* g, const long* numel, int n, double* partial, GradNormArgs* out, int* chunks) {
    if (!g || !numel || n < 1 || n > GN_MAX_T) return EFFI_ERR_BADARG;
    GradNormArgs a = {};
    long total = 0;
    for (int i = 0; i < n; ++i) {
        if (!g[i] || numel[i] < 0) return EFFI_ERR_BADARG;
        total += numel[i] / AW_CHUNK + (numel[i] % AW_CHUNK != 0);
        if (total > INT_MAX) return EFFI_ERR_BADARG;            // the grid's x extent
        a.g[i] = g[i];
        a.numel[i] = numel[i];
        a.chunk_end[i] = (int)total;
    }
    if (total > 0 && !partial) return EFFI_ERR_BADARG;
    a.partial = partial;
    a.n = n;
    *out = a;
    *chunks = (int)total;
    return EFFI_OK;
}

}  // namespace

extern "C" int effi_gradnorm_max_tensors(void) { return GN_MAX_T; }

extern "C" long effi_gradnorm_chunks(const long* numel, int n) { return gn_chunks(numel, n); }

extern "C" int effi_gradnorm_partial_f32(const float* const* g, const long* numel, int n, double* partial, effi_stream_t stream) {
    GradNormArgs a;
    int chunks = 0;
    const int rc = gn_pack(g, numel, n, partial, &a, &chunks);
    if (rc != EFFI_OK) return rc;
    if (chunks > 0) hipLaunchKernelGGL(gradnorm_partial_kernel, dim3(chunks), dim3(AW_THREADS), 0, effi_s(stream), a);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_gradnorm_finish_f32(const double* partial, long n_partial, double max_norm, float* clip, long long* skipped,
                                        effi_stream_t stream) {
    if (!clip || n_partial < 0 || (n_partial > 0 && !partial) || !(max_norm >= 0.0)) return EFFI_ERR_BADARG;
    hipLaunchKernelGGL(gradnorm_finish_kernel, dim3(1), dim3(AW_THREADS), 0, effi_s(stream), partial, n_partial, (float)max_norm, clip,
                       skipped);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_adamw_multi_clip_f32(float* const* p, const float* const* g, float* const* exp_avg, float* const* exp_avg_sq,
                                         float* const* step, const long* numel, int n, double lr, const float* lr_dev, double beta1,
                                         double beta2, double eps, double weight_decay, const float* clip, int skip_nonfinite,
                                         effi_stream_t stream) {
    if (!clip) return EFFI_ERR_BADARG;
    AdamWArgs a;
    int chunks = 0;
    const int rc = aw_pack(p, g, exp_avg, exp_avg_sq, step, numel, n, lr, lr_dev, beta1, beta2, eps, weight_decay, &a, &chunks);
    if (rc != EFFI_OK) return rc;
    a.clip = clip;
    a.skip = skip_nonfinite != 0;
    hipStream_t st = effi_s(stream);
    hipLaunchKernelGGL(adamw_step_kernel<true>, dim3(effi_cdiv(n, 64)), dim3(64), 0, st, a);
    if (chunks > 0) hipLaunchKernelGGL(adamw_update_kernel<true>, dim3(chunks), dim3(AW_THREADS), 0, st, a);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_adamw_max_tensors(void) { return AW_MAX_T; }

extern "C" int effi_adamw_multi_f32(float* const* p, const float* const* g, float* const* exp_avg, float* const* exp_avg_sq,
                                    float* const* step, const long* numel, int n, double lr, const float* lr_dev, double beta1,
                                    double beta2, double eps, double weight_decay, effi_stream_t stream) {
    AdamWArgs a;
    int chunks = 0;
    const int rc = aw_pack(p, g, exp_avg, exp_avg_sq, step, numel, n, lr, lr_dev, beta1, beta2, eps, weight_decay, &a, &chunks);
    if (rc != EFFI_OK) return rc;
    hipStream_t st = effi_s(stream);
    hipLaunchKernelGGL(adamw_step_kernel<false>, dim3(effi_cdiv(n, 64)), dim3(64), 0, st, a);
    if (chunks > 0) hipLaunchKernelGGL(adamw_update_kernel<false>, dim3(chunks), dim3(AW_THREADS), 0, st, a);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}
