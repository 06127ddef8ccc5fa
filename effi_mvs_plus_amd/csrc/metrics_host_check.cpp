// Stand-alone host check of the argument packing of csrc/metrics.hip (make -C effi_mvs_plus_amd/csrc host-check): the three entries
// are called with every refused argument and with full-size valid ones (K = 16 outputs, 8 thresholds, 8 bands) under
// -fsanitize=address,undefined.  NOTHING here reaches a GPU, with or without one in the machine: metrics.hip is included below
// with its launch path stubbed (hipLaunchKernelGGL expands to nothing, the error queries answer hipSuccess), and the program is
// compiled for the host only.  That is what makes the made-up device addresses safe: the host code copies them into the by-value
// kernel arguments and never reads through them, and no kernel ever sees them.  What is checked is that packing the caller's
// host arrays stays inside them and that every refused argument is refused before the (stubbed) launch.
#include <hip/hip_runtime.h>

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(...) ((void)0)
#define hipPeekAtLastError() hipSuccess
#define hipGetLastError() hipSuccess
#include "metrics.hip"

#include <cstdio>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

int main() {
    auto fake = [](long i) { return reinterpret_cast<void*>(0x100000 + 0x1000 * i); };
    EXPECT(effi_metrics_blocks(0) == 0 && effi_metrics_blocks(1) == 1 && effi_metrics_blocks(2048) == 1 && effi_metrics_blocks(2049) == 2);
    EXPECT(effi_metrics_blocks(1L << 40) == 0);
    EXPECT(effi_metrics_scratch_bytes(10, 0, 0) == 160 && effi_metrics_scratch_bytes(3, 5, 6) == 3 * 19 * 8);
    EXPECT(effi_metrics_scratch_bytes(0, 0, 0) == 0 && effi_metrics_scratch_bytes(1, 9, 0) == 0 && effi_metrics_scratch_bytes(1, 0, 9) == 0);

    for (int K : {1, 13, 16}) {
        // exactly K entries per host array: a read past the end is a heap overflow under the sanitizer
        std::vector<const float*> est(K), gt(K);
        std::vector<const void*> mask(K);
        std::vector<float*> grad(K);
        std::vector<long> n(K);
        std::vector<double> w(K);
        for (int i = 0; i < K; ++i) {
            est[i] = static_cast<const float*>(fake(4 * i)), gt[i] = static_cast<const float*>(fake(4 * i + 1));
            mask[i] = fake(4 * i + 2), grad[i] = static_cast<float*>(fake(4 * i + 3));
            n[i] = 35 + 40000L * i, w[i] = 1.0 / (1 + i);
        }
        float* l = static_cast<float*>(fake(100));
        long long* count = static_cast<long long*>(fake(101));
        for (int u8 = 0; u8 < 2; ++u8) {
            int rc = effi_mvs_loss_f32(est.data(), gt.data(), mask.data(), n.data(), K, u8, w.data(), l, count, l + K, fake(102), nullptr);
            EXPECT(rc == EFFI_OK);
            rc = effi_mvs_loss_bwd_f32(est.data(), gt.data(), mask.data(), n.data(), K, u8, w.data(), count, l + K, grad.data(), nullptr);
            EXPECT(rc == EFFI_OK);
        }
        EXPECT(effi_mvs_loss_f32(est.data(), gt.data(), mask.data(), n.data(), 0, 0, w.data(), l, count, l, fake(102), nullptr) == EFFI_ERR_BADARG);
        EXPECT(effi_mvs_loss_f32(est.data(), gt.data(), mask.data(), n.data(), 17, 0, w.data(), l, count, l, fake(102), nullptr) == EFFI_ERR_BADARG);
        EXPECT(effi_mvs_loss_f32(est.data(), gt.data(), mask.data(), n.data(), K, 0, w.data(), l, count, l, nullptr, nullptr) == EFFI_ERR_BADARG);
        EXPECT(effi_mvs_loss_f32(nullptr, gt.data(), mask.data(), n.data(), K, 0, w.data(), l, count, l, fake(102), nullptr) == EFFI_ERR_BADARG);
        n[K - 1] = 0;
        EXPECT(effi_mvs_loss_f32(est.data(), gt.data(), mask.data(), n.data(), K, 0, w.data(), l, count, l, fake(102), nullptr) == EFFI_ERR_BADARG);
        EXPECT(effi_mvs_loss_bwd_f32(est.data(), gt.data(), mask.data(), n.data(), K, 0, w.data(), count, l, grad.data(), nullptr) == EFFI_ERR_BADARG);
        n[K - 1] = 7;
        mask[0] = nullptr;
        EXPECT(effi_mvs_loss_f32(est.data(), gt.data(), mask.data(), n.data(), K, 0, w.data(), l, count, l, fake(102), nullptr) == EFFI_ERR_BADARG);
        mask[0] = fake(2);
        grad[K - 1] = nullptr;
        EXPECT(effi_mvs_loss_bwd_f32(est.data(), gt.data(), mask.data(), n.data(), K, 0, w.data(), count, l, grad.data(), nullptr) == EFFI_ERR_BADARG);
        EXPECT(effi_mvs_loss_bwd_f32(est.data(), gt.data(), mask.data(), n.data(), K, 0, w.data(), count, nullptr, grad.data(), nullptr) == EFFI_ERR_BADARG);
    }

    const float* est = static_cast<const float*>(fake(0));
    const float* gt = static_cast<const float*>(fake(1));
    long long* counts = static_cast<long long*>(fake(3));
    double* sums = static_cast<double*>(fake(4));
    float* scalars = static_cast<float*>(fake(5));
    for (int T : {0, 3, 8})
        for (int R : {0, 6, 8}) {
            std::vector<float> thr(T), lo(R), hi(R);
            for (int t = 0; t < T; ++t) thr[t] = 0.5f * t;
            for (int r = 0; r < R; ++r) lo[r] = 2.0f * r, hi[r] = 2.0f * r + 2.0f;
            int rc = effi_depth_metrics_f32(est, gt, fake(2), 2, 327680, T & 1, T ? thr.data() : nullptr, T, R ? lo.data() : nullptr,
                                            R ? hi.data() : nullptr, R, counts, sums, scalars, R ? sums : nullptr, fake(6), nullptr);
            EXPECT(rc == EFFI_OK);
        }
    std::vector<float> v8(8, 1.0f);
    EXPECT(effi_depth_metrics_f32(est, gt, fake(2), 1, 100, 0, v8.data(), 9, nullptr, nullptr, 0, counts, sums, scalars, nullptr, fake(6), nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_depth_metrics_f32(est, gt, fake(2), 1, 100, 0, nullptr, 0, v8.data(), v8.data(), 9, counts, sums, scalars, nullptr, fake(6), nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_depth_metrics_f32(est, gt, fake(2), 1, 100, 0, nullptr, 2, nullptr, nullptr, 0, counts, sums, scalars, nullptr, fake(6), nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_depth_metrics_f32(est, gt, fake(2), 1, 100, 0, nullptr, 0, v8.data(), nullptr, 2, counts, sums, scalars, nullptr, fake(6), nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_depth_metrics_f32(est, gt, fake(2), 0, 100, 0, nullptr, 0, nullptr, nullptr, 0, counts, sums, scalars, nullptr, fake(6), nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_depth_metrics_f32(est, gt, fake(2), 1, 0, 0, nullptr, 0, nullptr, nullptr, 0, counts, sums, scalars, nullptr, fake(6), nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_depth_metrics_f32(est, gt, nullptr, 1, 100, 0, nullptr, 0, nullptr, nullptr, 0, counts, sums, scalars, nullptr, fake(6), nullptr) == EFFI_ERR_BADARG);
    EXPECT(effi_depth_metrics_f32(est, gt, fake(2), 1, 100, 0, nullptr, 0, nullptr, nullptr, 0, counts, sums, scalars, nullptr, nullptr, nullptr) == EFFI_ERR_BADARG);
    std::printf(failures ? "metrics host check: %d FAILED\n" : "metrics host check: ok\n", failures);
    return failures ? 1 : 0;
}
