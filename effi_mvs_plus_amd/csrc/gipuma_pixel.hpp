// The per-pixel body of the Gipuma / fusibile depth-map fusion (gipuma.hip), host-callable so that
// gipuma_host_check.cpp runs every thread of the grid -- the same index arithmetic and the same decisions -- against exactly sized
// host arrays under the sanitizers.  The one store of this kernel whose address depends on DATA is used[s][q] (q = the rounded
// projection of the pixel's point into source view s): gip_project is the only place that forms q, and it compares the rounded
// coordinates with the image size as FLOATS (NaN fails every comparison) before anything is converted to an integer.
#pragma once
#include <hip/hip_runtime.h>

constexpr int GIP_MAX_SRC = 64;        // sources per reference view: the consistent set is a 64-bit mask
constexpr int GIP_THREADS = 256;
// per view slot (slot 0 = the reference view, slot 1 + s = its s-th source): K[9] Kinv[9] R[9] t[3] fb, one pad
constexpr int GIP_STRIDE = 32;
constexpr int GIP_K = 0, GIP_KI = 9, GIP_R = 18, GIP_T = 27, GIP_FB = 30;

struct GipP3 { float x, y, z; };

// One slot from the view's camera [2][4][4] (extrinsic, intrinsic in the top-left 3x3) and the reference view's: the 3x3 inverse by
// the adjugate in double, rounded; fb = K_ref[0][0] * |C_ref - C_view| formed in double and rounded once (C = -R^T t).
__host__ __device__ inline void gip_prepare_slot(const float* cam, const float* ref_cam, float* m) {
    double K[9], c[3], cr[3];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) K[r * 3 + k] = (double)cam[16 + r * 4 + k];
    const double a00 = K[4] * K[8] - K[5] * K[7], a01 = K[5] * K[6] - K[3] * K[8], a02 = K[3] * K[7] - K[4] * K[6];
    const double det = K[0] * a00 + K[1] * a01 + K[2] * a02;
    const double adj[9] = {a00, K[2] * K[7] - K[1] * K[8], K[1] * K[5] - K[2] * K[4],
                           a01, K[0] * K[8] - K[2] * K[6], K[2] * K[3] - K[0] * K[5],
                           a02, K[1] * K[6] - K[0] * K[7], K[0] * K[4] - K[1] * K[3]};
    for (int i = 0; i < 9; ++i) {
        m[GIP_K + i] = (float)K[i];
        m[GIP_KI + i] = (float)(adj[i] / det);
    }
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) m[GIP_R + r * 3 + k] = cam[r * 4 + k];
        m[GIP_T + r] = cam[r * 4 + 3];
    }
    for (int k = 0; k < 3; ++k) {
        c[k] = -((double)cam[k] * (double)cam[3] + (double)cam[4 + k] * (double)cam[7] + (double)cam[8 + k] * (double)cam[11]);
        cr[k] = -((double)ref_cam[k] * (double)ref_cam[3] + (double)ref_cam[4 + k] * (double)ref_cam[7] +
                  (double)ref_cam[8 + k] * (double)ref_cam[11]);
    }
    const double dx = cr[0] - c[0], dy = cr[1] - c[1], dz = cr[2] - c[2];
    m[GIP_FB] = (float)((double)ref_cam[16] * sqrt(dx * dx + dy * dy + dz * dz));
    m[GIP_FB + 1] = 0.0f;
}

__host__ __device__ inline bool gip_ok(float d, float depth_min, float depth_max) { return d >= depth_min && d <= depth_max; }   // NaN fails

// X = R^T (d K^-1 (x, y, 1)^T - t) of the integer pixel (x, y) of the slot's view
__host__ __device__ inline GipP3 gip_backproject(const float* m, float x, float y, float d) {
    const float *Ki = m + GIP_KI, *R = m + GIP_R, *t = m + GIP_T;
    const float rx = Ki[0] * x + Ki[1] * y + Ki[2], ry = Ki[3] * x + Ki[4] * y + Ki[5], rz = Ki[6] * x + Ki[7] * y + Ki[8];
    const float cx = d * rx - t[0], cy = d * ry - t[1], cz = d * rz - t[2];
    return {R[0] * cx + R[3] * cy + R[6] * cz, R[1] * cx + R[4] * cy + R[7] * cz, R[2] * cx + R[5] * cy + R[8] * cz};
}

// Y = R_s X + t_s, z = Y_z, q = floor((K_s Y)_xy / (K_s Y)_z + 0.5) -> the element offset of q in an [h][w] map, or -1 when z is not
// positive or q is outside the image (or not a number); qx, qy: the rounded coordinates as floats
__host__ __device__ inline int gip_project(const float* m, GipP3 X, int h, int w, float& z, float& qx, float& qy) {
    const float *K = m + GIP_K, *R = m + GIP_R, *t = m + GIP_T;
    const float yx = R[0] * X.x + R[1] * X.y + R[2] * X.z + t[0], yy = R[3] * X.x + R[4] * X.y + R[5] * X.z + t[1];
    const float yz = R[6] * X.x + R[7] * X.y + R[8] * X.z + t[2];
    const float kx = K[0] * yx + K[1] * yy + K[2] * yz, ky = K[3] * yx + K[4] * yy + K[5] * yz, kz = K[6] * yx + K[7] * yy + K[8] * yz;
    z = yz;
    qx = floorf(kx / kz + 0.5f);
    qy = floorf(ky / kz + 0.5f);
    if (!(yz > 0.0f)) return -1;
    if (!(qx >= 0.0f && qx < (float)w && qy >= 0.0f && qy < (float)h)) return -1;
    return (int)qy * w + (int)qx;
}

__host__ __device__ inline bool gip_consistent(float fb, float z, float ds, float disp_threshold) {
    return fabsf(fb / z - fb / ds) < disp_threshold;
}

struct GipView {
    const float* depths;            // [n_views][h][w]
    const float* images;            // [n_views][h][w][3] or null
    const int* sources;             // [n_src] view ids
    const float* mats;              // [n_src + 1][GIP_STRIDE]
    int ref, n_src, h, w;
    float disp_threshold;
    int num_consistent;
    float depth_min, depth_max;
    unsigned char* used;            // [n_views][h][w]
    float* points;                  // [3][h][w]
    float* colour;                  // [h][w][3] or null
    unsigned char *mask, *count;    // [h][w]
};

// Thread `thread` of workgroup `block`: one reference pixel.  First pass: the consistent sources as a 64-bit mask (no per-thread
// array); second pass, fused pixels only: q recomputed for the set bits, the sums in source order, the flags.
__host__ __device__ inline void gip_thread(const GipView& a, long block, int thread) {
    const long hw = (long)a.h * a.w, p = block * GIP_THREADS + thread;
    if (p >= hw) return;
    const int y = (int)(p / a.w), x = (int)(p - (long)y * a.w);
    const float d = a.depths[a.ref * hw + p];
    const bool live = gip_ok(d, a.depth_min, a.depth_max) && a.used[a.ref * hw + p] == 0;
    unsigned long long bits = 0ull;
    int n = 0;
    GipP3 X = {0.0f, 0.0f, 0.0f};
    if (live) {
        X = gip_backproject(a.mats, (float)x, (float)y, d);
        for (int s = 0; s < a.n_src; ++s) {
            const float* ms = a.mats + (long)(s + 1) * GIP_STRIDE;
            float z, qx, qy;
            const int q = gip_project(ms, X, a.h, a.w, z, qx, qy);
            if (q < 0) continue;
            const float ds = a.depths[a.sources[s] * hw + q];
            if (!gip_ok(ds, a.depth_min, a.depth_max)) continue;
            if (gip_consistent(ms[GIP_FB], z, ds, a.disp_threshold)) {
                bits |= 1ull << s;
                ++n;
            }
        }
    }
    const bool fused = live && n >= a.num_consistent;
    a.count[p] = (unsigned char)n;
    a.mask[p] = fused ? 1 : 0;
    if (!fused) return;
    GipP3 sum = X;
    float cr = 0.0f, cg = 0.0f, cb = 0.0f;
    if (a.images) {
        const float* px = a.images + (a.ref * hw + p) * 3;
        cr = px[0]; cg = px[1]; cb = px[2];
    }
    for (int s = 0; s < a.n_src; ++s) {
        if (!((bits >> s) & 1ull)) continue;
        const float* ms = a.mats + (long)(s + 1) * GIP_STRIDE;
        float z, qx, qy;
        const int q = gip_project(ms, X, a.h, a.w, z, qx, qy);          // the first pass's arithmetic: the same q, inside the image
        if (q < 0) continue;                                            // never taken; keeps the store below in bounds whatever the compiler does
        const long at = a.sources[s] * hw + q;
        const GipP3 Xs = gip_backproject(ms, qx, qy, a.depths[at]);
        sum.x = sum.x + Xs.x; sum.y = sum.y + Xs.y; sum.z = sum.z + Xs.z;
        if (a.images) {
            const float* px = a.images + at * 3;
            cr = cr + px[0]; cg = cg + px[1]; cb = cb + px[2];
        }
        a.used[at] = 1;
    }
    a.used[a.ref * hw + p] = 1;
    const float div = (float)(n + 1);
    a.points[p] = sum.x / div;
    a.points[hw + p] = sum.y / div;
    a.points[2 * hw + p] = sum.z / div;
    if (a.colour) {
        a.colour[p * 3] = cr / div;
        a.colour[p * 3 + 1] = cg / div;
        a.colour[p * 3 + 2] = cb / div;
    }
}
