// The scalar side of the reference's train.py: the training loss (models/module.py:526-552, mvs_loss) and the depth metrics of
// train_sample / test_sample_depth (utils.py:139-160, Thres_metrics / AbsDepthError_metrics; train.py:266-271,322-337).  The reference
// selects the valid pixels by boolean indexing (a data-dependent shape and a host sync per call) and reads every scalar back; here
// the valid pixels are SELECTED in registers (never multiplied by the mask: an Inf / NaN estimate at a masked pixel is dropped, as
// the indexing drops it), every scalar stays on the device, and nothing reads the host, so all of it can be captured into a graph.
//
// No atomics: a workgroup reduces MT_CHUNK elements -- fp64 sums, integer counts, __shfl_xor across the
// wave, LDS across the waves, as channel_sum_kernel (train_ops.hip) does -- and writes one row of 8-byte slots to caller-owned
// scratch; a one-workgroup finishing launch adds the rows in ascending order and forms the scalars.  The order of every addition is
// fixed by the shape alone, so results are bitwise repeatable.
//
// Per-pixel arithmetic is fp32 and rounds as the reference's separate torch ops do (the library is built with -ffp-contract=off):
// d = est - gt, z = |d|, smooth-L1 with beta = 1 as ATen writes it: z < 1 ? (0.5f * z) * z : z - 0.5f.
#include "common.hpp"

namespace {

constexpr int MT_THREADS = 256, MT_WAVES = MT_THREADS / 64;
constexpr int MT_CHUNK = 2048;                  // elements per workgroup: 8 per thread (the reduce_chunk of the training reductions)
constexpr int MT_MAX_OUT = 16, MT_MAX_T = 8, MT_MAX_R = 8;
constexpr long MT_MAX_N = 1L << 40;

struct LossArgs {               // by-value kernel argument: the K outputs of one launch
    const float* est[MT_MAX_OUT];
    const float* gt[MT_MAX_OUT];
    const void* mask[MT_MAX_OUT];
    long n[MT_MAX_OUT];         // elements of output i, batch included
    int row0[MT_MAX_OUT];       // first scratch row of output i
    int blocks[MT_MAX_OUT];     // workgroups (= scratch rows) of output i
};

struct LossBwdArgs {
    const float* est[MT_MAX_OUT];
    const float* gt[MT_MAX_OUT];
    const void* mask[MT_MAX_OUT];
    float* grad[MT_MAX_OUT];
    long n[MT_MAX_OUT];
    double w[MT_MAX_OUT];
};

struct LossWeights {
    double w[MT_MAX_OUT];
};

struct MetricArgs {             // thresholds and bands by value (utils.py:146,157 compare in the tensors' fp32)
    float thres[MT_MAX_T];
    float lo[MT_MAX_R], hi[MT_MAX_R];
    int T, R;
};

template <bool U8>
__device__ __forceinline__ bool mt_valid(const void* __restrict__ mask, long i) {
    if (U8) return static_cast<const unsigned char*>(mask)[i] != 0;
    return static_cast<const float*>(mask)[i] > 0.5f;
}

// workgroup sums; the result is valid in thread 0.  `red` holds MT_WAVES entries per call site
__device__ __forceinline__ double mt_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}

__device__ __forceinline__ long long mt_block_count(int v, int* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long s = 0;
    if (threadIdx.x == 0) s = (long long)red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return s;
}
static_assert(MT_WAVES == 4, "mt_block_sum / mt_block_count add four waves");

// scratch row of workgroup (blockIdx.x, output blockIdx.y): [count (int64), sum (fp64)]
template <bool U8>
__global__ __launch_bounds__(MT_THREADS) void mvs_loss_partial_kernel(LossArgs a, long long* __restrict__ scratch) {
    __shared__ double red_s[MT_WAVES];
    __shared__ int red_c[MT_WAVES];
    const int o = blockIdx.y;
    if ((int)blockIdx.x >= a.blocks[o]) return;                 // uniform per workgroup
    const float* __restrict__ est = a.est[o];
    const float* __restrict__ gt = a.gt[o];
    const void* __restrict__ mask = a.mask[o];
    const long i0 = (long)blockIdx.x * MT_CHUNK, i1 = min(a.n[o], i0 + MT_CHUNK);
    double s = 0.0;
    int c = 0;
    for (long i = i0 + threadIdx.x; i < i1; i += MT_THREADS) {
        if (!mt_valid<U8>(mask, i)) continue;
        const float d = est[i] - gt[i], z = fabsf(d);
        const float t = z < 1.0f ? (0.5f * z) * z : z - 0.5f;
        s += (double)t;
        c += 1;
    }
    const double bs = mt_block_sum(s, red_s);
    const long long bc = mt_block_count(c, red_c);
    if (threadIdx.x == 0) {
        long long* row = scratch + 2L * (a.row0[o] + (long)blockIdx.x);
        row[0] = bc;
        reinterpret_cast<double*>(row)[1] = bs;
    }
}

// one workgroup: thread i < K adds the rows of output i in ascending order, l[i] = fl32(sum / count) (0 / 0 = NaN: the reference's
// mean of an empty selection); thread 0 then forms total = fl32(sum_i w_i * l[i]) in fp64, ascending i
__global__ __launch_bounds__(64) void mvs_loss_finish_kernel(LossArgs a, LossWeights lw, int K, const long long* __restrict__ scratch,
                                                             float* __restrict__ l, long long* __restrict__ count,
                                                             float* __restrict__ total) {
    __shared__ float ls[MT_MAX_OUT];
    const int i = threadIdx.x;
    if (i < K) {
        const long long* row = scratch + 2L * a.row0[i];
        double s = 0.0;
        long long c = 0;
        for (int j = 0; j < a.blocks[i]; ++j) {
            c += row[2L * j];
            s += reinterpret_cast<const double*>(row)[2L * j + 1];
        }
        const float li = (float)(s / (double)c);
        ls[i] = li;
        l[i] = li;
        count[i] = c;
    }
    __syncthreads();
    if (i == 0) {
        double t = 0.0;
        for (int k = 0; k < K; ++k) t += lw.w[k] * (double)ls[k];
        *total = (float)t;
    }
}

// grad_i[p] = s_i * c(d_p) at the valid pixels, exactly 0 elsewhere.  s_i = fl32(g * w_i / count_i); c(d) as ATen's smooth-L1
// backward with beta = 1 (d < -1: -1, d > 1: 1, else d -- so d = +-1 gives +-1 and a NaN d stays NaN)
template <bool U8>
__global__ __launch_bounds__(MT_THREADS) void mvs_loss_bwd_kernel(LossBwdArgs a, const long long* __restrict__ count,
                                                                  const float* __restrict__ grad_total) {
    const int o = blockIdx.y;
    const long n = a.n[o];
    const long i0 = (long)blockIdx.x * MT_CHUNK, i1 = min(n, i0 + MT_CHUNK);
    if (i0 >= n) return;
    const float* __restrict__ est = a.est[o];
    const float* __restrict__ gt = a.gt[o];
    const void* __restrict__ mask = a.mask[o];
    float* __restrict__ grad = a.grad[o];
    const float s = (float)((double)grad_total[0] * a.w[o] / (double)count[o]);
    for (long i = i0 + threadIdx.x; i < i1; i += MT_THREADS) {
        float g = 0.0f;
        if (mt_valid<U8>(mask, i)) {
            const float d = est[i] - gt[i];
            g = s * (d < -1.0f ? -1.0f : (d > 1.0f ? 1.0f : d));
        }
        grad[i] = g;
    }
}

// scratch row of workgroup (blockIdx.x, image blockIdx.y), 2 + T + 2 R slots of 8 bytes:
// [n_valid, n_over[T], n_band[R]] (int64) then [sum_abs, sum_band[R]] (fp64)
template <bool U8>
__global__ __launch_bounds__(MT_THREADS) void depth_metrics_partial_kernel(const float* __restrict__ est, const float* __restrict__ gt,
                                                                           const void* __restrict__ mask, long n, MetricArgs m,
                                                                           long long* __restrict__ scratch) {
    __shared__ double red_s[MT_WAVES];
    __shared__ int red_c[MT_WAVES];
    const long base = (long)blockIdx.y * n;
    const long i0 = (long)blockIdx.x * MT_CHUNK, i1 = min(n, i0 + MT_CHUNK);
    int n_valid = 0, n_over[MT_MAX_T], n_band[MT_MAX_R];
    double sum_abs = 0.0, sum_band[MT_MAX_R];
#pragma unroll
    for (int t = 0; t < MT_MAX_T; ++t) n_over[t] = 0;
#pragma unroll
    for (int r = 0; r < MT_MAX_R; ++r) { n_band[r] = 0; sum_band[r] = 0.0; }
    for (long i = i0 + threadIdx.x; i < i1; i += MT_THREADS) {
        if (!mt_valid<U8>(mask, base + i)) continue;
        const float e = fabsf(est[base + i] - gt[base + i]);
        n_valid += 1;
        sum_abs += (double)e;
#pragma unroll
        for (int t = 0; t < MT_MAX_T; ++t)
            if (t < m.T && e > m.thres[t]) n_over[t] += 1;
#pragma unroll
        for (int r = 0; r < MT_MAX_R; ++r)
            if (r < m.R && e >= m.lo[r] && e <= m.hi[r]) { n_band[r] += 1; sum_band[r] += (double)e; }
    }
    const int row_len = 2 + m.T + 2 * m.R;
    long long* row = scratch + ((long)blockIdx.y * gridDim.x + blockIdx.x) * row_len;
    double* rowd = reinterpret_cast<double*>(row) + 1 + m.T + m.R;
    long long v = mt_block_count(n_valid, red_c);
    if (threadIdx.x == 0) row[0] = v;
    const double sa = mt_block_sum(sum_abs, red_s);
    if (threadIdx.x == 0) rowd[0] = sa;
#pragma unroll
    for (int t = 0; t < MT_MAX_T; ++t) {
        if (t < m.T) {                                          // uniform
            v = mt_block_count(n_over[t], red_c);
            if (threadIdx.x == 0) row[1 + t] = v;
        }
    }
#pragma unroll
    for (int r = 0; r < MT_MAX_R; ++r) {
        if (r < m.R) {
            v = mt_block_count(n_band[r], red_c);
            const double sb = mt_block_sum(sum_band[r], red_s);
            if (threadIdx.x == 0) { row[1 + m.T + r] = v; rowd[1 + r] = sb; }
        }
    }
}

// one workgroup.  First the raw table: counts [B][1 + T + R] and sums [B][1 + R], each the sum of the image's rows in ascending
// order.  Then scalar k of [abs_mean, thres_0.., band_0..]: per image fl32(sum_abs / n_valid), fl32(n_over / n_valid) (0 / 0 = NaN,
// utils.py:147,160) or fl32(sum_band / n_band) (0 for an empty band, utils.py:158-159); the B values are averaged in fp64 in
// ascending order and rounded once (utils.py:134).  acc (optional, fp64) += the scalar vector.
__global__ __launch_bounds__(MT_THREADS) void depth_metrics_finish_kernel(const long long* __restrict__ scratch, int B, int blocks, int T, int R,
                                                                          long long* counts, double* sums,     // written, then re-read
                                                                          float* __restrict__ scalars, double* __restrict__ acc) {
    const int nc = 1 + T + R, ns = 1 + R, row_len = nc + ns;
    for (int e = threadIdx.x; e < B * row_len; e += MT_THREADS) {
        const int b = e / row_len, k = e - b * row_len;
        const long long* p = scratch + (long)b * blocks * row_len + k;
        if (k < nc) {
            long long c = 0;
            for (int j = 0; j < blocks; ++j) c += p[(long)j * row_len];
            counts[(long)b * nc + k] = c;
        } else {
            double s = 0.0;
            for (int j = 0; j < blocks; ++j) s += reinterpret_cast<const double*>(p)[(long)j * row_len];
            sums[(long)b * ns + (k - nc)] = s;
        }
    }
    __threadfence();
    __syncthreads();
    const int k = threadIdx.x;
    if (k < nc) {
        double mean = 0.0;
        for (int b = 0; b < B; ++b) {
            const long long* c = counts + (long)b * nc;
            const double* s = sums + (long)b * ns;
            float v;
            if (k == 0) v = (float)(s[0] / (double)c[0]);
            else if (k <= T) v = (float)((double)c[k] / (double)c[0]);
            else v = c[k] > 0 ? (float)(s[k - T] / (double)c[k]) : 0.0f;
            mean += (double)v;
        }
        const float out = (float)(mean / (double)B);
        scalars[k] = out;
        if (acc) acc[k] += (double)out;
    }
}

int mt_blocks(long n) { return (n < 1 || n >= MT_MAX_N) ? 0 : effi_cdiv(n, MT_CHUNK); }

}  // namespace

extern "C" int effi_metrics_blocks(long n) { return mt_blocks(n); }

extern "C" long effi_metrics_scratch_bytes(long blocks, int n_thres, int n_bands) {
    if (blocks < 1 || blocks >= (1L << 31) || n_thres < 0 || n_thres > MT_MAX_T || n_bands < 0 || n_bands > MT_MAX_R) return 0;
    return blocks * (2 + n_thres + 2 * n_bands) * 8;
}

extern "C" int effi_mvs_loss_f32(const float* const* est, const float* const* gt, const void* const* mask, const long* n, int K,
                                 int mask_u8, const double* w, float* l, long long* count, float* total, void* scratch,
                                 effi_stream_t stream) {
    if (!est || !gt || !mask || !n || !w || !l || !count || !total || !scratch || K < 1 || K > MT_MAX_OUT) return EFFI_ERR_BADARG;
    LossArgs a = {};
    LossWeights lw = {};
    int rows = 0, widest = 0;
    for (int i = 0; i < K; ++i) {
        const int b = mt_blocks(n[i]);
        if (!est[i] || !gt[i] || !mask[i] || b == 0 || b > (1 << 24)) return EFFI_ERR_BADARG;
        a.est[i] = est[i], a.gt[i] = gt[i], a.mask[i] = mask[i], a.n[i] = n[i], a.row0[i] = rows, a.blocks[i] = b;
        lw.w[i] = w[i];
        rows += b;
        widest = b > widest ? b : widest;
    }
    hipStream_t st = effi_s(stream);
    long long* sc = static_cast<long long*>(scratch);
    if (mask_u8) hipLaunchKernelGGL(mvs_loss_partial_kernel<true>, dim3(widest, K), dim3(MT_THREADS), 0, st, a, sc);
    else hipLaunchKernelGGL(mvs_loss_partial_kernel<false>, dim3(widest, K), dim3(MT_THREADS), 0, st, a, sc);
    hipLaunchKernelGGL(mvs_loss_finish_kernel, dim3(1), dim3(64), 0, st, a, lw, K, sc, l, count, total);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_mvs_loss_bwd_f32(const float* const* est, const float* const* gt, const void* const* mask, const long* n, int K,
                                     int mask_u8, const double* w, const long long* count, const float* grad_total, float* const* grad,
                                     effi_stream_t stream) {
    if (!est || !gt || !mask || !n || !w || !count || !grad_total || !grad || K < 1 || K > MT_MAX_OUT) return EFFI_ERR_BADARG;
    LossBwdArgs a = {};
    int widest = 0;
    for (int i = 0; i < K; ++i) {
        const int b = mt_blocks(n[i]);
        if (!est[i] || !gt[i] || !mask[i] || !grad[i] || b == 0 || b > (1 << 24)) return EFFI_ERR_BADARG;
        a.est[i] = est[i], a.gt[i] = gt[i], a.mask[i] = mask[i], a.grad[i] = grad[i], a.n[i] = n[i], a.w[i] = w[i];
        widest = b > widest ? b : widest;
    }
    hipStream_t st = effi_s(stream);
    if (mask_u8) hipLaunchKernelGGL(mvs_loss_bwd_kernel<true>, dim3(widest, K), dim3(MT_THREADS), 0, st, a, count, grad_total);
    else hipLaunchKernelGGL(mvs_loss_bwd_kernel<false>, dim3(widest, K), dim3(MT_THREADS), 0, st, a, count, grad_total);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_depth_metrics_f32(const float* est, const float* gt, const void* mask, int B, long n, int mask_u8,
                                      const float* thres, int n_thres, const float* band_lo, const float* band_hi, int n_bands,
                                      long long* counts, double* sums, float* scalars, double* acc, void* scratch,
                                      effi_stream_t stream) {
    const int blocks = mt_blocks(n);
    if (!est || !gt || !mask || !counts || !sums || !scalars || !scratch || B < 1 || B > 65535 || blocks == 0) return EFFI_ERR_BADARG;
    if (n_thres < 0 || n_thres > MT_MAX_T || n_bands < 0 || n_bands > MT_MAX_R) return EFFI_ERR_BADARG;
    if ((n_thres > 0 && !thres) || (n_bands > 0 && (!band_lo || !band_hi)) || (long)B * blocks >= (1L << 31)) return EFFI_ERR_BADARG;
    MetricArgs m = {};
    m.T = n_thres, m.R = n_bands;
    for (int t = 0; t < n_thres; ++t) m.thres[t] = thres[t];
    for (int r = 0; r < n_bands; ++r) m.lo[r] = band_lo[r], m.hi[r] = band_hi[r];
    hipStream_t st = effi_s(stream);
    long long* sc = static_cast<long long*>(scratch);
    if (mask_u8) hipLaunchKernelGGL(depth_metrics_partial_kernel<true>, dim3(blocks, B), dim3(MT_THREADS), 0, st, est, gt, mask, n, m, sc);
    else hipLaunchKernelGGL(depth_metrics_partial_kernel<false>, dim3(blocks, B), dim3(MT_THREADS), 0, st, est, gt, mask, n, m, sc);
    hipLaunchKernelGGL(depth_metrics_finish_kernel, dim3(1), dim3(MT_THREADS), 0, st, sc, B, blocks, n_thres, n_bands, counts, sums, scalars,
                       acc);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}
