// The DTU evaluation of a fused point cloud (reference: evaluations/dtu/BaseEvalMain_web.m -> PointCompareMain.m -> reducePts_haa.m,
// MaxDistCP.m), the step after effi_mvs_plus_amd/dtu_fusion.py::fuse_scan: thin the cloud to one point per `dst` neighbourhood,
// measure the capped nearest-neighbour distances cloud -> ground truth and back, and mask both sets.  MATLAB works in double, so
// every geometric decision here is made in fp64 on the fp32 coordinates converted to fp64; the squared distance is always
// (dx*dx + dy*dy) + dz*dz (the library is built with -ffp-contract=off, so no term is fused).
//
// Neighbour candidates come from a uniform grid ANCHORED AT ZERO: cell index = floor(p / cell) per axis, minus the smallest index
// of the set, keyed (x * ny + y) * nz + z.  The host sorts the points by key (plumbing), so a run of z-neighbours of one (x, y)
// column is one contiguous range of the sorted arrays and the 27 surrounding cells are nine such runs, each found by one binary
// search in the sorted keys (a dense cell table is out of reach: a DTU scene at 0.2 mm has ~10^10 cells).  Sorted points carry a
// fourth float (the reduction's rank, bit-cast; unused by the nearest-neighbour search) so that a candidate is one 16-byte load.
// No atomics: every thread owns its output element and writes it with a plain store; the per-launch "undecided left" count is a
// ballot popcount per wave combined through LDS into one int per workgroup (as fusion.hip's compaction does).
#include "common.hpp"

namespace {

constexpr int DE_THREADS = 256, DE_WAVES = DE_THREADS / 64;
constexpr unsigned char DE_UNDECIDED = 0, DE_KEPT = 1, DE_REMOVED = 2;
constexpr double DE_INDEX_LIMIT = 1073741824.0;         // |floor(p / cell)| is clamped to 2^30 (queries far outside a grid)

struct DeGrid {                 // by-value kernel argument
    double cell;
    int i0[3];                  // smallest floor(p / cell) of the gridded set, per axis
    int n[3];                   // cells per axis
};

__device__ __forceinline__ long de_cell_index(float p, double cell, int i0) {
    const double c = fmin(fmax(floor((double)p / cell), -DE_INDEX_LIMIT), DE_INDEX_LIMIT);
    return (long)c - (long)i0;
}

__device__ __forceinline__ double de_dist2(double px, double py, double pz, float qx, float qy, float qz) {
    const double dx = px - (double)qx, dy = py - (double)qy, dz = pz - (double)qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// first index whose key is >= k
__device__ __forceinline__ int de_lower_bound(const long long* __restrict__ keys, int n, long long k) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(DE_THREADS) void dtu_cell_keys_kernel(const float* __restrict__ xyz, long n, DeGrid g,
                                                                   long long* __restrict__ keys) {
    const long i = (long)blockIdx.x * DE_THREADS + threadIdx.x;
    if (i >= n) return;
    long c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)         // the clamp never acts on a point of the set the grid was sized for; it keeps the key in range
        c[a] = min(max(de_cell_index(xyz[3 * i + a], g.cell, g.i0[a]), 0L), (long)g.n[a] - 1);
    keys[i] = (c[0] * g.n[1] + c[1]) * g.n[2] + c[2];
}

// One round of reducePts_haa.m:24-30 as a fixed point over {undecided, kept, removed}: thread i (a position
// in key order) reads state_in only and writes state_out[i] only.  An undecided point is REMOVED if a neighbour (d <= dst,
// inclusive) of smaller rank is kept, KEPT if every neighbour of smaller rank is removed, and stays undecided otherwise.
__global__ __launch_bounds__(DE_THREADS) void dtu_reduce_round_kernel(const float4* __restrict__ pts, const long long* __restrict__ keys,
                                                                      int n, DeGrid g, double dst2,
                                                                      const unsigned char* __restrict__ state_in,
                                                                      unsigned char* __restrict__ state_out, int* __restrict__ undecided) {
    __shared__ int wave_n[DE_WAVES];
    const int i = blockIdx.x * DE_THREADS + threadIdx.x;
    unsigned char st = DE_REMOVED;
    if (i < n) {
        st = state_in[i];
        if (st == DE_UNDECIDED) {
            const float4 p = pts[i];
            const int rank = __float_as_int(p.w);
            const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
            const long long key = keys[i];
            const long nz = g.n[2], ny = g.n[1], nx = g.n[0];
            const long cz = key % nz, cy = (key / nz) % ny, cx = (key / nz) / ny;
            const long zlo = max(cz - 1, 0L), zhi = min(cz + 1, nz - 1);
            bool pending = false, removed = false;
            for (int r = 0; r < 9 && !removed; ++r) {
                const long x = cx + r / 3 - 1, y = cy + r % 3 - 1;
                if (x < 0 || x >= nx || y < 0 || y >= ny) continue;
                const long long base = (x * ny + y) * nz, khi = base + zhi;
                for (int j = de_lower_bound(keys, n, base + zlo); j < n && keys[j] <= khi; ++j) {
                    const float4 q = pts[j];
                    if (__float_as_int(q.w) >= rank) continue;                    // later in the order, or the point itself
                    const unsigned char sj = state_in[j];
                    if (sj == DE_REMOVED) continue;
                    if (de_dist2(px, py, pz, q.x, q.y, q.z) <= dst2) {
                        if (sj == DE_KEPT) { removed = true; break; }
                        pending = true;
                    }
                }
            }
            st = removed ? DE_REMOVED : (pending ? DE_UNDECIDED : DE_KEPT);
        }
        state_out[i] = st;
    }
    const unsigned long long b = __ballot(st == DE_UNDECIDED);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < DE_WAVES; ++w) c += wave_n[w];
        undecided[blockIdx.x] = c;
    }
}

// MaxDistCP.m:31-33 without its blocks: out[i] = min(cap^2, min_j d^2(src_i, to_j)).  Shells of cells at Chebyshev distance s around
// the query's cell, s upwards from the first shell that touches the grid.  Everything not yet visited when shell s starts lies
// >= s cells away on some axis, i.e. >= (s - 1) * cell from the query (the query is somewhere inside its own cell); the bound is
// shrunk by 2^-20 relative, which covers the rounding of the two floor(p / cell) (|p / cell| < 2^31: error < 2^-21 cell).  The search
// stops when the best squared distance (which starts at cap^2) is no larger than that bound squared, or the grid is exhausted: a
// minimum over a superset of the cells that can matter, so the value does not depend on the cell size or on the visiting order.
__global__ __launch_bounds__(DE_THREADS) void dtu_nn_capped_kernel(const float* __restrict__ src, int n_src, const float4* __restrict__ to,
                                                                   const long long* __restrict__ keys, int n_to, DeGrid g, double cap2,
                                                                   double* __restrict__ out) {
    const int i = blockIdx.x * DE_THREADS + threadIdx.x;
    if (i >= n_src) return;
    double best = cap2;
    if (n_to > 0) {
        const float fx = src[3 * (long)i], fy = src[3 * (long)i + 1], fz = src[3 * (long)i + 2];
        const double px = (double)fx, py = (double)fy, pz = (double)fz;
        const long nx = g.n[0], ny = g.n[1], nz = g.n[2];
        const long cx = de_cell_index(fx, g.cell, g.i0[0]), cy = de_cell_index(fy, g.cell, g.i0[1]), cz = de_cell_index(fz, g.cell, g.i0[2]);
        auto gap = [](long c, long n) { return c < 0 ? -c : (c > n - 1 ? c - (n - 1) : 0L); };      // shells before the grid is touched
        auto reach = [](long c, long n) { return max(c, n - 1 - c); };                             // shell of the farthest cell
        const long s0 = max(gap(cx, nx), max(gap(cy, ny), gap(cz, nz)));
        const long s1 = max(reach(cx, nx), max(reach(cy, ny), reach(cz, nz)));
        auto scan = [&](long long klo, long long khi) {
            for (int j = de_lower_bound(keys, n_to, klo); j < n_to && keys[j] <= khi; ++j) {
                const float4 q = to[j];
                best = fmin(best, de_dist2(px, py, pz, q.x, q.y, q.z));
            }
        };
        for (long s = s0; s <= s1; ++s) {
            if (s >= 1) {
                const double lb = (double)(s - 1) * g.cell * (1.0 - 0x1p-20);
                if (best <= lb * lb) break;
            }
            const long xlo = max(cx - s, 0L), xhi = min(cx + s, nx - 1), ylo = max(cy - s, 0L), yhi = min(cy + s, ny - 1);
            const long zlo = max(cz - s, 0L), zhi = min(cz + s, nz - 1);
            for (long x = xlo; x <= xhi; ++x) {
                const bool x_face = (x == cx - s) || (x == cx + s);
                for (long y = ylo; y <= yhi; ++y) {
                    const long long base = (x * ny + y) * nz;
                    if (x_face || y == cy - s || y == cy + s) {                   // the whole z column of the shell
                        if (zlo <= zhi) scan(base + zlo, base + zhi);
                    } else {                                                      // interior column: the two z faces (s >= 1 here)
                        if (cz - s >= 0 && cz - s < nz) scan(base + cz - s, base + cz - s);
                        if (cz + s >= 0 && cz + s < nz) scan(base + cz + s, base + cz + s);
                    }
                }
            }
        }
    }
    out[i] = best;
}

// PointCompareMain.m:32-40: Qv = round((Q - BB(1,:)) / Res + 1), MATLAB's round (halves away from zero = C's round()); inside iff
// every index lies in 1..size and ObsMask(Qv) is set.  obs is [X][Y][Z] row-major bytes.
__global__ __launch_bounds__(DE_THREADS) void dtu_obs_mask_kernel(const float* __restrict__ xyz, long n, double b0x, double b0y, double b0z,
                                                                  double res, const unsigned char* __restrict__ obs, int X, int Y, int Z,
                                                                  unsigned char* __restrict__ out) {
    const long i = (long)blockIdx.x * DE_THREADS + threadIdx.x;
    if (i >= n) return;
    const double vx = round(((double)xyz[3 * i] - b0x) / res + 1.0);
    const double vy = round(((double)xyz[3 * i + 1] - b0y) / res + 1.0);
    const double vz = round(((double)xyz[3 * i + 2] - b0z) / res + 1.0);
    unsigned char m = 0;
    if (vx >= 1.0 && vx <= (double)X && vy >= 1.0 && vy <= (double)Y && vz >= 1.0 && vz <= (double)Z)
        m = obs[(((long)vx - 1) * Y + ((long)vy - 1)) * Z + ((long)vz - 1)] != 0 ? 1 : 0;
    out[i] = m;
}

// PointCompareMain.m:52: P' * [q; 1] > 0, summed left to right in fp64
__global__ __launch_bounds__(DE_THREADS) void dtu_above_plane_kernel(const float* __restrict__ xyz, long n, double p0, double p1, double p2,
                                                                     double p3, unsigned char* __restrict__ out) {
    const long i = (long)blockIdx.x * DE_THREADS + threadIdx.x;
    if (i >= n) return;
    const double s = ((p0 * (double)xyz[3 * i] + p1 * (double)xyz[3 * i + 1]) + p2 * (double)xyz[3 * i + 2]) + p3;
    out[i] = s > 0.0 ? 1 : 0;
}

bool de_grid(double cell, int i0x, int i0y, int i0z, int nx, int ny, int nz, DeGrid* g) {
    if (!(cell > 0.0) || !(cell < 1e300) || nx < 1 || ny < 1 || nz < 1) return false;
    if (nx > (1 << 21) || ny > (1 << 21) || nz > (1 << 20)) return false;                  // the key stays below 2^62
    const int lim = 1 << 30;
    if (i0x < -lim || i0x > lim || i0y < -lim || i0y > lim || i0z < -lim || i0z > lim) return false;
    *g = DeGrid{cell, {i0x, i0y, i0z}, {nx, ny, nz}};
    return true;
}

}  // namespace

extern "C" int effi_dtu_cell_keys_f32(const float* xyz, long n, double cell, int i0x, int i0y, int i0z, int nx, int ny, int nz,
                                      long long* keys, effi_stream_t stream) {
    DeGrid g;
    if (!xyz || !keys || n < 1 || n >= (1L << 31) || !de_grid(cell, i0x, i0y, i0z, nx, ny, nz, &g)) return EFFI_ERR_BADARG;
    hipStream_t st = effi_s(stream);
    hipLaunchKernelGGL(dtu_cell_keys_kernel, dim3(effi_cdiv(n, DE_THREADS)), dim3(DE_THREADS), 0, st, xyz, n, g, keys);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_dtu_reduce_blocks(long n) {
    if (n < 1 || n >= (1L << 31)) return 0;
    return effi_cdiv(n, DE_THREADS);
}

extern "C" int effi_dtu_reduce_round_f32(const float* pts4, const long long* keys, long n, int nx, int ny, int nz, double dst,
                                         const unsigned char* state_in, unsigned char* state_out, int* block_undecided,
                                         effi_stream_t stream) {
    DeGrid g;
    if (!pts4 || !keys || !state_in || !state_out || !block_undecided || state_in == state_out) return EFFI_ERR_BADARG;
    if (n < 1 || n >= (1L << 31) || !(dst >= 0.0) || !(dst < 1e150) || !de_grid(1.0, 0, 0, 0, nx, ny, nz, &g)) return EFFI_ERR_BADARG;
    hipStream_t st = effi_s(stream);
    hipLaunchKernelGGL(dtu_reduce_round_kernel, dim3(effi_cdiv(n, DE_THREADS)), dim3(DE_THREADS), 0, st,
                       reinterpret_cast<const float4*>(pts4), keys, (int)n, g, dst * dst, state_in, state_out, block_undecided);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_dtu_nn_capped_f32(const float* src, long n_src, const float* to4, const long long* keys, long n_to, double cell,
                                      int i0x, int i0y, int i0z, int nx, int ny, int nz, double cap, double* out_d2,
                                      effi_stream_t stream) {
    DeGrid g = DeGrid{1.0, {0, 0, 0}, {1, 1, 1}};
    if (!src || !out_d2 || n_src < 1 || n_src >= (1L << 31) || n_to < 0 || n_to >= (1L << 31)) return EFFI_ERR_BADARG;
    if (!(cap >= 0.0) || !(cap < 1e150)) return EFFI_ERR_BADARG;
    if (n_to > 0 && (!to4 || !keys || !de_grid(cell, i0x, i0y, i0z, nx, ny, nz, &g))) return EFFI_ERR_BADARG;
    hipStream_t st = effi_s(stream);
    hipLaunchKernelGGL(dtu_nn_capped_kernel, dim3(effi_cdiv(n_src, DE_THREADS)), dim3(DE_THREADS), 0, st, src, (int)n_src,
                       reinterpret_cast<const float4*>(to4), keys, (int)n_to, g, cap * cap, out_d2);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_dtu_obs_mask_f32(const float* xyz, long n, double bb0x, double bb0y, double bb0z, double res,
                                     const unsigned char* obs_mask, int size_x, int size_y, int size_z, unsigned char* out,
                                     effi_stream_t stream) {
    if (!xyz || !obs_mask || !out || n < 1 || n >= (1L << 31) || size_x < 1 || size_y < 1 || size_z < 1 || !(res > 0.0)) return EFFI_ERR_BADARG;
    if ((long)size_x * size_y * size_z >= (1L << 40)) return EFFI_ERR_BADARG;
    hipStream_t st = effi_s(stream);
    hipLaunchKernelGGL(dtu_obs_mask_kernel, dim3(effi_cdiv(n, DE_THREADS)), dim3(DE_THREADS), 0, st, xyz, n, bb0x, bb0y, bb0z, res, obs_mask,
                       size_x, size_y, size_z, out);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}

extern "C" int effi_dtu_above_plane_f32(const float* xyz, long n, double p0, double p1, double p2, double p3, unsigned char* out,
                                        effi_stream_t stream) {
    if (!xyz || !out || n < 1 || n >= (1L << 31)) return EFFI_ERR_BADARG;
    hipStream_t st = effi_s(stream);
    hipLaunchKernelGGL(dtu_above_plane_kernel, dim3(effi_cdiv(n, DE_THREADS)), dim3(DE_THREADS), 0, st, xyz, n, p0, p1, p2, p3, out);
    EFFI_LAUNCH_CHECK();
    return EFFI_OK;
}
