// f32_mfma_probe.hip -- measures the premise of the margin of include/batched/sparse_rx_f32_batched.h: how far the screen kernel's
// v_mfma_f32_32x32x2_f32 chain lies from the float64 dot product, in units of gamma * sum |q_i d_i| (gamma = n u / (1 - n u)).
// Stand-alone: it compiles the kernels of csrc/dense_f32_batched.hip alone and runs the screen in its matrix mode.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 -Iinclude -I<package>/csrc tools/f32_mfma_probe.hip -o f32_mfma_probe
// Prints one line per (family, dim) and the largest ratio; c of the header is max(2, 4 * that).
#define SRX_F32_BATCHED_KERNELS_ONLY
#include "dense_f32_batched.hip"

#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#define PROBE_TRY(e)                                                          \
    do {                                                                      \
        hipError_t rc_ = (e);                                                 \
        if (rc_ != hipSuccess) {                                              \
            std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(rc_));     \
            return 1;                                                         \
        }                                                                     \
    } while (0)

int main() {
    const int nq = 128, nd = 1024, dims[] = {64, 128, 256, 512, 768, 1024};
    const char *families[] = {"gaussian", "magnitude-blocks", "cancelling"};
    std::mt19937_64 rng(7);
    std::normal_distribution<float> g(0.0f, 1.0f);
    float *dq, *dd, *ds;
    PROBE_TRY(hipMalloc(&dq, nq * 1024 * 4));
    PROBE_TRY(hipMalloc(&dd, nd * 1024 * 4));
    PROBE_TRY(hipMalloc(&ds, nq * nd * 4));
    double worst = 0.0;
    for (int fam = 0; fam < 3; ++fam)
        for (int dim : dims) {
            std::vector<float> q((size_t)nq * dim), d((size_t)nd * dim), s((size_t)nq * nd);
            for (auto &x : q) x = g(rng);
            for (auto &x : d) x = g(rng);
            if (fam == 1)  // blocks of 16 columns whose magnitudes differ by up to 10^12, on both sides
                for (size_t i = 0; i < d.size(); ++i) d[i] *= std::pow(10.0f, (float)((int)((i % dim) / 16 * 7 % 13) - 6));
            if (fam == 2)  // the second half of a row undoes the first to a few ulps: the sum is tiny against sum |q_i d_i|
                for (int r = 0; r < nd; ++r)
                    for (int c = 0; c < dim / 2; ++c) d[(size_t)r * dim + dim / 2 + c] = -d[(size_t)r * dim + c] * (1.0f + 1e-6f * g(rng));
            if (fam == 2)
                for (int r = 0; r < nq; ++r)
                    for (int c = 0; c < dim / 2; ++c) q[(size_t)r * dim + dim / 2 + c] = q[(size_t)r * dim + c];
            PROBE_TRY(hipMemcpy(dq, q.data(), q.size() * 4, hipMemcpyHostToDevice));
            PROBE_TRY(hipMemcpy(dd, d.data(), d.size() * 4, hipMemcpyHostToDevice));
            FbScreenArgs a = {dd, dq, nd, 0, dim, nq, 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, ds, nd};
            hipLaunchKernelGGL(srx_f32_batched_screen_kernel<true>, dim3(nd / FB_TILE), dim3(THREADS), 0, 0, a);
            PROBE_TRY(hipGetLastError());
            PROBE_TRY(hipDeviceSynchronize());
            PROBE_TRY(hipMemcpy(s.data(), ds, s.size() * 4, hipMemcpyDeviceToHost));
            const double nu = dim * std::ldexp(1.0, -24), gamma = nu / (1.0 - nu);
            double mx = 0.0;
            for (int i = 0; i < nq; ++i)
                for (int j = 0; j < nd; ++j) {
                    double ref = 0.0, mag = 0.0;
                    for (int c = 0; c < dim; ++c) {
                        const double p = (double)q[(size_t)i * dim + c] * (double)d[(size_t)j * dim + c];
                        ref += p;
                        mag += std::fabs(p);
                    }
                    mx = std::fmax(mx, std::fabs((double)s[(size_t)i * nd + j] - ref) / (mag * gamma));
                }
            std::printf("f32_mfma_probe family=%s dim=%d max|mfma - f64| / (gamma sum|q d|) = %.6f\n", families[fam], dim, mx);
            worst = std::fmax(worst, mx);
        }
    std::printf("f32_mfma_probe largest ratio = %.6f -> c = max(2, 4 * ratio) = %.3f\n", worst, std::fmax(2.0, 4.0 * worst));
    return 0;
}
