// Gipuma / fusibile depth-map fusion (reference: misc/gipuma.py:160-236 -- probability_filter, then the external CUDA program
// `fusibile` run with normal_thresh = 360, so without its normal test).  PARITY WITH THE EXTERNAL BINARY UNPINNED: neither its source
// nor its output is available to this project; the method is the consistency fusion of Galliani et al. 2015 as DESIGN.md section 7.10
// specifies it, and tests/gipuma_ref.py is its float64 restatement.
// Unlike the three filters of fusion.hip this one is ORDER DEPENDENT: a fused point consumes the source pixels that supported it (a
// byte per view and pixel in `used`), so the reference views of a scan are fused one launch after the other and each launch sees the
// flags of the earlier ones.  Inside a launch for reference view r a thread reads used[r] at its own pixel only and writes used[s]
// for s != r only (the entry refuses r among its own sources), apart from its own pixel of used[r]; two threads that claim the same
// source pixel both store the byte 1.  The result therefore does not depend on scheduling.
// One thread per reference pixel; the body is gip_thread (gipuma_pixel.hpp), which the host check runs as it stands.  The view slots
// (camera matrices, f * b) are addressed with the wave-uniform source index.
#include "common.hpp"
#include "gipuma_pixel.hpp"

namespace {

// mats [n_src + 1][GIP_STRIDE]: slot 0 = the reference view, slot 1 + s = source s
__global__ void gipuma_prepare_kernel(const float* __restrict__ cams, int ref, const int* __restrict__ sources, int n_src,
                                      float* __restrict__ mats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_src) return;
    const int v = i == 0 ? ref : sources[i - 1];
    gip_prepare_slot(cams + (long)v * 32, cams + (long)ref * 32, mats + (long)i * GIP_STRIDE);
}

__global__ __launch_bounds__(GIP_THREADS) void gipuma_view_kernel(GipView a) { gip_thread(a, blockIdx.x, threadIdx.x); }

// gipuma.py:177,188: depth_map[~(prob_map > prob_threshold)] = 0
__global__ __launch_bounds__(256) void gipuma_prob_kernel(const float* __restrict__ depth, const float* __restrict__ conf, long n, float thr,
                                                          float* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = conf[i] > thr ? depth[i] : 0.0f;
}

}  // namespace

extern "C" int effi_fusion_gipuma_prob_f32(const float* depth, const float* conf, long n, float prob_threshold, float* out,
                                           effi_stream_t stream) {
    if (!depth || !conf || !out || n < 1 || n >= (1L << 31) * 256) return EFFI_ERR_BADARG;
    hipStream_t st = effi_s(stream);
    hipLaunchKernelGGL(gipuma_prob_kernel, dim3(effi_cdiv(n, 256)), dim3(256), 0, st, depth, conf, n, prob_threshold, out);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_fusion_gipuma_view_f32(const float* depths, const float* cams, const float* images, int n_views, int ref,
                                           const int* sources_host, const int* sources, int n_src, int h, int w, float disp_threshold,
                                           int num_consistent, float depth_min, float depth_max, float* mats_scratch, unsigned char* used,
                                           float* out_points, float* out_colour, unsigned char* out_mask, unsigned char* out_count,
                                           effi_stream_t stream) {
    if (!depths || !cams || !sources_host || !sources || !mats_scratch || !used || !out_points || !out_mask || !out_count) return EFFI_ERR_BADARG;
    if ((images == nullptr) != (out_colour == nullptr)) return EFFI_ERR_BADARG;
    if (n_views < 1 || ref < 0 || ref >= n_views || n_src < 1 || n_src > GIP_MAX_SRC || h < 1 || w < 1) return EFFI_ERR_BADARG;
    if ((long)n_views * h * w >= (1L << 31)) return EFFI_ERR_BADARG;
    if (!(disp_threshold == disp_threshold) || !(depth_min == depth_min) || !(depth_max == depth_max)) return EFFI_ERR_BADARG;
    for (int s = 0; s < n_src; ++s)
        if (sources_host[s] < 0 || sources_host[s] >= n_views || sources_host[s] == ref) return EFFI_ERR_BADARG;
    hipStream_t st = effi_s(stream);
    hipLaunchKernelGGL(gipuma_prepare_kernel, dim3(effi_cdiv(n_src + 1, 64)), dim3(64), 0, st, cams, ref, sources, n_src, mats_scratch);
    EFFI_LAUNCH_CHECK();
    const GipView a{depths, images, sources, mats_scratch, ref, n_src, h, w, disp_threshold, num_consistent, depth_min, depth_max,
                    used, out_points, out_colour, out_mask, out_count};
    hipLaunchKernelGGL(gipuma_view_kernel, dim3(effi_cdiv((long)h * w, GIP_THREADS)), dim3(GIP_THREADS), 0, st, a);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}
