// Scope row n4, training half (input pipeline of train.py): what the two training datasets compute on the host with numpy / cv2
// per sample, as two launches for a whole sample batch.
//   datasets/dtu_yao.py:70-74, :186    read_img (/ 255.) of every view, np.stack(...).transpose([0, 3, 1, 2])
//   datasets/dtu_yao.py:93-125         mask > 10 and the depth map -> their cv2.resize(INTER_NEAREST) pyramids /2, /4, /8
//   datasets/blend.py:97-101, :222     the same images
//   datasets/blend.py:208-220          the depth pyramid and, per level, mask = (depth >= depth_min) & (depth <= depth_max)
// Both kernels only move data: 3 B read + 12 B written per image pixel; ~5 B read + ~10.6 B written per ground-truth pixel.
// No LDS, every store behind a bounds test.
#include "common.hpp"
#include "train_input_index.hpp"

namespace {

typedef unsigned effi_u32x2 __attribute__((ext_vector_type(2)));
struct __attribute__((aligned(4))) EffiRgb4 { unsigned d[3]; };     // four interleaved 8-bit RGB pixels

// imgs [V][hw][3] uint8 -> out [V][3][hw] fp32 = x / 255 (an IEEE division: np.float32(x) / 255 bit for bit, as
// image_prepare_kernel at dst == src).  A thread owns four consecutive pixels of one view (blockIdx.y).  VEC (hw % 4 == 0 and
// aligned bases): the 12 interleaved bytes are one 3-dword load, each plane gets one 16-byte store -- a wave reads 768 contiguous
// bytes and writes three 1-KB runs.  Otherwise: byte loads and scalar stores, each pixel tested.
template <bool VEC>
__global__ __launch_bounds__(128) void images_prepare_batch_kernel(const unsigned char* __restrict__ imgs, long hw,
                                                                   float* __restrict__ out) {
    const long p0 = effi_images_first_pixel(blockIdx.x, threadIdx.x);
    if (p0 >= hw) return;
    const unsigned char* src = imgs + effi_images_src_byte(blockIdx.y, hw, p0);
    float* dst = out + effi_images_dst_elem(blockIdx.y, hw, p0);
    if (VEC) {                                          // p0 + 3 < hw: hw is a multiple of 4
        const EffiRgb4 q = *reinterpret_cast<const EffiRgb4*>(src);
        effi_f32x4_t v[3];
#pragma unroll
        for (int e = 0; e < 12; ++e) v[e % 3][e / 3] = (float)((q.d[e >> 2] >> (8 * (e & 3))) & 0xffu) / 255.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<effi_f32x4_t*>(dst + c * hw) = v[c];
    } else {
        for (int i = 0; i < 4 && p0 + i < hw; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c * hw + i] = (float)src[3 * i + c] / 255.0f;
    }
}

struct EffiPyramidOut {         // by-value kernel argument: stage1 .. stage4 of the depth and of the mask
    float* depth[4];
    float* mask[4];
};

// depth [B][h][w] (+ mask_u8 [B][h][w], or range [B][2]) -> the four-level pyramid of both.  h and w are multiples of 8, so
// cv2.resize(INTER_NEAREST) to (w / f, h / f) reads source (f y, f x) (sx = min(floor(x * 1 / (dst / src)), src - 1) with an exact
// power-of-two ratio).  A thread owns 8 consecutive pixels of one stage-4 row of one sample (blockIdx.y); octets are numbered
// row-major, so a wave covers 512 consecutive pixels.  It writes stage 4 always (2 x 16 B per map), stage 3 when its row is even
// (16 B), stage 2 when y % 4 == 0 (8 B), stage 1 when y % 8 == 0 (4 B) -- every output element has exactly one writer.
// DTU (mask_u8 != null): mask = byte > thresh, sampled at the depth's source addresses.  BlendedMVS: mask = dmin <= d <= dmax on
// the level's own depth value in fp32 (NaN -> 0).
__global__ __launch_bounds__(64) void gt_pyramid_kernel(const float* __restrict__ depth, const unsigned char* __restrict__ mask_u8,
                                                        int thresh, const float* __restrict__ range, int h, int w,
                                                        EffiPyramidOut out) {
    const long n_oct = (long)h * (w >> 3);
    const long o = (long)blockIdx.x * 64 + threadIdx.x;
    if (o >= n_oct) return;
    const long b = blockIdx.y;
    const EffiPyramidIndex ix = effi_pyramid_index(o, b, h, w);
    const int y = ix.y;
    const long src = ix.src, o3 = ix.o3, o2 = ix.o2, o1 = ix.o1;
    const effi_f32x4_t d0 = *reinterpret_cast<const effi_f32x4_t*>(depth + src);
    const effi_f32x4_t d1 = *reinterpret_cast<const effi_f32x4_t*>(depth + src + 4);
    float d[8], m[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) { d[i] = d0[i]; d[4 + i] = d1[i]; }
    if (mask_u8) {
        const effi_u32x2 q = *reinterpret_cast<const effi_u32x2*>(mask_u8 + src);
#pragma unroll
        for (int i = 0; i < 8; ++i) m[i] = (int)((q[i >> 2] >> (8 * (i & 3))) & 0xffu) > thresh ? 1.0f : 0.0f;
    } else {
        const float lo = range[2 * b], hi = range[2 * b + 1];
#pragma unroll
        for (int i = 0; i < 8; ++i) m[i] = (d[i] >= lo && d[i] <= hi) ? 1.0f : 0.0f;
    }
    // stage 4: the copy
    *reinterpret_cast<effi_f32x4_t*>(out.depth[3] + src) = d0;
    *reinterpret_cast<effi_f32x4_t*>(out.depth[3] + src + 4) = d1;
    *reinterpret_cast<effi_f32x4_t*>(out.mask[3] + src) = effi_f32x4_t{m[0], m[1], m[2], m[3]};
    *reinterpret_cast<effi_f32x4_t*>(out.mask[3] + src + 4) = effi_f32x4_t{m[4], m[5], m[6], m[7]};
    if (y & 1) return;
    // stage 3 [h/2][w/2]: source columns x0, x0 + 2, x0 + 4, x0 + 6
    *reinterpret_cast<effi_f32x4_t*>(out.depth[2] + o3) = effi_f32x4_t{d[0], d[2], d[4], d[6]};
    *reinterpret_cast<effi_f32x4_t*>(out.mask[2] + o3) = effi_f32x4_t{m[0], m[2], m[4], m[6]};
    if (y & 3) return;
    // stage 2 [h/4][w/4]: source columns x0, x0 + 4
    *reinterpret_cast<effi_f32x2_t*>(out.depth[1] + o2) = effi_f32x2_t{d[0], d[4]};
    *reinterpret_cast<effi_f32x2_t*>(out.mask[1] + o2) = effi_f32x2_t{m[0], m[4]};
    if (y & 7) return;
    // stage 1 [h/8][w/8]: source column x0
    out.depth[0][o1] = d[0];
    out.mask[0][o1] = m[0];
}

inline bool effi_aligned(const void* p, unsigned long a) { return (reinterpret_cast<unsigned long>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int effi_images_prepare_batch_u8_f32(const unsigned char* imgs_vhwc, int n_views, int h, int w, float* out_vchw,
                                                effi_stream_t stream) {
    if (!imgs_vhwc || !out_vchw || n_views < 1 || h < 1 || w < 1) return EFFI_ERR_BADARG;
    if (n_views > 65535) return EFFI_ERR_UNSUPPORTED;
    const long hw = (long)h * w;
    const dim3 grid(effi_cdiv(effi_cdiv(hw, 4), 128), n_views);
    hipStream_t st = effi_s(stream);
    if (hw % 4 == 0 && effi_aligned(imgs_vhwc, 4) && effi_aligned(out_vchw, 16))
        hipLaunchKernelGGL(images_prepare_batch_kernel<true>, grid, dim3(128), 0, st, imgs_vhwc, hw, out_vchw);
    else
        hipLaunchKernelGGL(images_prepare_batch_kernel<false>, grid, dim3(128), 0, st, imgs_vhwc, hw, out_vchw);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_gt_pyramid_f32(const float* depth, const unsigned char* mask_u8, int thresh, const float* range, int n_smp,
                                   int h, int w, float* const* depth_out, float* const* mask_out, effi_stream_t stream) {
    if (!depth || !depth_out || !mask_out || n_smp < 1 || h < 1 || w < 1) return EFFI_ERR_BADARG;
    if ((mask_u8 != nullptr) == (range != nullptr)) return EFFI_ERR_BADARG;           // exactly one source of the mask
    if (h % 8 != 0 || w % 8 != 0 || n_smp > 65535) return EFFI_ERR_UNSUPPORTED;       // cv2's rounding is pinned for these only
    EffiPyramidOut out;
    for (int k = 0; k < 4; ++k) {
        out.depth[k] = depth_out[k];
        out.mask[k] = mask_out[k];
        if (!out.depth[k] || !out.mask[k]) return EFFI_ERR_BADARG;
        if (!effi_aligned(out.depth[k], 16) || !effi_aligned(out.mask[k], 16)) return EFFI_ERR_UNSUPPORTED;
    }
    if (!effi_aligned(depth, 16) || (mask_u8 && !effi_aligned(mask_u8, 8)) || (range && !effi_aligned(range, 4)))
        return EFFI_ERR_UNSUPPORTED;
    const dim3 grid(effi_cdiv((long)h * (w >> 3), 64), n_smp);
    hipLaunchKernelGGL(gt_pyramid_kernel, grid, dim3(64), 0, effi_s(stream), depth, mask_u8, thresh, range, h, w, out);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}
