// The full convolutions of birdnet_v30_v2l (EfficientNetV2-L's Fused-MBConv stages) on the implicit-GEMM kernels
// (launch_conv_gemm16 / launch_conv_gemm, kernels_conv.hip), 256 segments, next to the same M x K x N as a 1x1 layer on a
// materialised im2col matrix (launch_pw_gemm16 / launch_pw_gemm): us, algorithmic TFLOP/s and the fraction of the dense rate --
// 2.5 PF / 3 for split-f16 (three MFMAs per product), 157.3 TF for the f32 MFMA (MI355X_MICROARCH.md).  Then the NHWC shape the
// old direct kernel could run (3x3 24 -> 64 at 64 x 249: 54 KB of weights, inside its 64-KB LDS limit) on conv_direct_kernel and on the implicit GEMM.  Synthetic operands;
// includes kernels_conv.hip itself: the shipped code.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Wno-inline-asm -Wno-unused-result -o tools/microbench/conv_gemm.bin tools/microbench/conv_gemm.hip
//   tools/microbench/conv_gemm.bin [segments]
#include "../../birda_amd/csrc/kernels_conv.hip"
#include <cstdio>
#include <vector>

__global__ void fill_kernel(float *p, size_t n, unsigned seed) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        unsigned x = (unsigned)i * 2654435761u + seed;
        x ^= x >> 15; x *= 2246822519u; x ^= x >> 13;
        p[i] = (float)(x >> 8) * (1.0f / 16777216.0f) - 0.5f;
    }
}
static void fill(float *p, size_t n, unsigned seed) { hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, p, n, seed); }

struct Shape { int cin, cout, k, s, in_h, in_w; const char *where; };

int main(int argc, char **argv) {
    const int nseg = argc > 1 ? atoi(argv[1]) : 256;
    const double f16x3_peak = 2500.0 / 3.0, f32_peak = 157.3;   // TFLOP/s
    const Shape shapes[] = {{32, 32, 3, 1, 64, 249, "stage 1 (x4, + residual)"},
                            {32, 128, 3, 2, 64, 249, "stage 2 first"},
                            {64, 256, 3, 1, 32, 125, "stage 2 (x6)"},
                            {64, 256, 3, 2, 32, 125, "stage 3 first"},
                            {96, 384, 3, 1, 16, 63, "stage 3 (x6)"},
                            {24, 64, 3, 1, 64, 249, "an NHWC shape the old direct kernel ran"}};
    hipStream_t s; hipStreamCreate(&s);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    auto time_us = [&](auto launch) {
        for (int i = 0; i < 3; i++) launch();
        hipEventRecord(e0, s);
        const int reps = 10;
        for (int i = 0; i < reps; i++) launch();
        hipEventRecord(e1, s); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        return ms * 1e3 / reps;
    };
    printf("%d segments; fractions of %.1f TF (f16x3 = 2.5 PF / 3) and %.1f TF (f32 MFMA)\n", nseg, f16x3_peak, f32_peak);
    for (const Shape &sh : shapes) {
        bh::ConvParams p{};
        p.in_h = sh.in_h; p.in_w = sh.in_w; p.cin = sh.cin; p.cout = sh.cout; p.kh = p.kw = sh.k; p.sh = p.sw = sh.s;
        p.out_h = (sh.in_h + sh.s - 1) / sh.s; p.out_w = (sh.in_w + sh.s - 1) / sh.s;
        p.pad_t = std::max((p.out_h - 1) * sh.s + sh.k - sh.in_h, 0) / 2; p.pad_l = std::max((p.out_w - 1) * sh.s + sh.k - sh.in_w, 0) / 2;
        p.in_layout = 0; p.act = bh::ACT_SWISH;
        const int cpad = (sh.cin + 31) / 32 * 32, K = sh.k * sh.k * cpad, N = sh.cout, ldw = (N + 3) / 4 * 4;
        const size_t M = (size_t)nseg * p.out_h * p.out_w;
        const size_t nx = (size_t)nseg * sh.in_h * sh.in_w * sh.cin, nw16 = (size_t)(K / 32) * ((N + 15) / 16) * 1024;
        float *X, *Wt, *bias, *Y, *A = nullptr; void *W16;
        hipMalloc(&X, nx * 4); hipMalloc(&Wt, (size_t)K * ldw * 4); hipMalloc(&bias, N * 4); hipMalloc(&Y, M * N * 4);
        hipMalloc(&W16, nw16 * 2);
        fill(X, nx, 1); fill(Wt, (size_t)K * ldw, 2); fill(bias, N, 3); fill((float *)W16, nw16 / 2, 4);
        const bool im2col = M * (size_t)K * 4 < (size_t)6 << 30;
        if (im2col) { hipMalloc(&A, M * K * 4); fill(A, M * (size_t)K, 5); }
        hipDeviceSynchronize();
        const double flop = 2.0 * M * sh.k * sh.k * sh.cin * N;   // algorithmic: the unpadded K
        auto report = [&](const char *what, double us, double peak) {
            printf("  %-34s %9.1f us  %7.1f TFLOP/s  %.3f of peak\n", what, us, flop / (us * 1e-6) / 1e12, flop / (us * 1e-6) / 1e12 / peak);
        };
        printf("%dx%d s%d %d -> %d at %dx%d (%s): M %zu K %d N %d, %.1f GFLOP\n", sh.k, sh.k, sh.s, sh.cin, sh.cout, sh.in_h, sh.in_w,
               sh.where, M, K, N, flop / 1e9);
        const double g16 = time_us([&] { bh::launch_conv_gemm16(X, W16, bias, nullptr, Y, p, nseg, 3, 1.0f, s); });
        report("implicit GEMM f16x3", g16, f16x3_peak);
        if (im2col) {
            const double p16 = time_us([&] { bh::launch_pw_gemm16(A, W16, bias, nullptr, Y, (int)M, K, N, bh::ACT_SWISH, 3, 1.0f, s); });
            report("1x1 on im2col f16x3", p16, f16x3_peak);
            printf("  %-34s %9.2f\n", "ratio implicit / 1x1 (f16x3)", g16 / p16);
        }
        const double g32 = time_us([&] { bh::launch_conv_gemm(X, Wt, bias, nullptr, Y, p, nseg, ldw, s); });
        report("implicit GEMM f32", g32, f32_peak);
        if (im2col) {
            const double p32 = time_us([&] { bh::launch_pw_gemm(A, Wt, bias, nullptr, Y, (int)M, K, N, ldw, bh::ACT_SWISH, s); });
            report("1x1 on im2col f32", p32, f32_peak);
            printf("  %-34s %9.2f\n", "ratio implicit / 1x1 (f32)", g32 / p32);
        }
        if ((size_t)sh.k * sh.k * sh.cin * sh.cout * 4 <= 64 * 1024) {   // what the direct kernel could hold in LDS
            const double d = time_us([&] { bh::launch_conv_direct(X, Wt, bias, Y, p, nseg, s); });
            report("conv_direct_kernel (old path)", d, f32_peak);
        }
        hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) { printf("HIP error %s\n", hipGetErrorString(e)); return 1; }
        hipFree(X); hipFree(Wt); hipFree(bias); hipFree(Y); hipFree(W16);
        if (A) hipFree(A);
    }
    return 0;
}
