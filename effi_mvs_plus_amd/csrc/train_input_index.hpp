// Address arithmetic of the training-input kernels (train_input.hip), host-callable so that train_input_host_check.cpp can run
// every thread's indices against exactly sized arrays under the sanitizers.
#pragma once
#include <hip/hip_runtime.h>

// gt_pyramid_kernel: thread o (row-major octet number inside a sample) of sample b -> its stage-4 row y, first column x0, the
// element offsets of its source / stage-4 octet and of its stage-3 quad, stage-2 pair and stage-1 element.  Rows with y & 1,
// y & 3, y & 7 set do not write the coarser stages.  h and w are multiples of 8.
struct EffiPyramidIndex {
    int y, x0;
    long src, o3, o2, o1;
};
__host__ __device__ inline EffiPyramidIndex effi_pyramid_index(long o, long b, int h, int w) {
    const int wo = w >> 3;                              // octets per row
    const long hw = (long)h * w;
    EffiPyramidIndex r;
    r.y = (int)(o / wo);
    r.x0 = ((int)(o - (long)r.y * wo)) << 3;
    r.src = b * hw + (long)r.y * w + r.x0;
    r.o3 = b * (hw >> 2) + (long)(r.y >> 1) * (w >> 1) + (r.x0 >> 1);
    r.o2 = b * (hw >> 4) + (long)(r.y >> 2) * (w >> 2) + (r.x0 >> 2);
    r.o1 = b * (hw >> 6) + (long)(r.y >> 3) * (w >> 3) + (r.x0 >> 3);
    return r;
}

// images_prepare_batch_kernel: first pixel of thread t of workgroup bx (4 pixels per thread, 128 threads), the byte offset of its
// source pixels and the element offset of its first output (plane c adds c * hw) in view v.
__host__ __device__ inline long effi_images_first_pixel(long bx, int t) { return 4 * (bx * 128 + t); }
__host__ __device__ inline long effi_images_src_byte(long v, long hw, long p0) { return (v * hw + p0) * 3; }
__host__ __device__ inline long effi_images_dst_elem(long v, long hw, long p0) { return v * 3 * hw + p0; }
