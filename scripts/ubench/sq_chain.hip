// Microbenchmark: nanoseconds per block of k_sqbank_fsm's serial loop (one lane per row,
// csrc/k_sqbank.hip), one wave, 16 and 64 rows of 65 536 blocks, rows whose block powers differ:
//   selects / table   the mode step as the kernel's selects, or as one 64-bit table lookup
//   8 / 16 / 32 ahead blocks of p loaded ahead of the chain
//   smoothing alone   s += alpha (p - s), the conversion and the level store, no mode step
//   no stores         the whole step, results folded into a checksum
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off sq_chain.hip -o sq_chain && ./sq_chain
// profiles/sq_chain_ubench.txt keeps a run.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

template <int V, int A, bool LUT>
__global__ void __launch_bounds__(64) chain(int C, long nb, double alpha, int timeout, float t, const double* __restrict__ p,
                                            float* __restrict__ level, unsigned char* __restrict__ status, double* out)
{
    __builtin_amdgcn_s_setprio(3);
    const int c = threadIdx.x;
    if (c >= C) return;
    const double* pr = p + (long)c * nb;
    float* lr = level + (long)c * nb;
    unsigned char* sr = status + (long)c * nb;
    double s = 0.0;
    int mode = 1, timer = 0;
    unsigned acc = 0;
    const long last = nb - 1;
    double cur[A], nxt[A];
    for (int u = 0; u < A; u++) cur[u] = pr[u];
    for (long b0 = 0; b0 + A <= nb; b0 += A) {
#pragma unroll
        for (int u = 0; u < A; u++) nxt[u] = pr[min(b0 + A + u, last)];
#pragma unroll
        for (int u = 0; u < A; u++) {
            float lv;
            s = s + alpha * (cur[u] - s);
            lv = (float)s;
            if (V != 1 && LUT) {
                const unsigned idx = 2u * (unsigned)mode + (lv > t ? 1u : 0u);
                const int next = (int)((0x11353534342100ull >> (4u * idx)) & 15u);
                const int low = mode == 5 ? 1 : 0;
                timer = mode == 4 ? timeout : timer - low;
                mode = low & (timer == 0 ? 1 : 0) ? 6 : next;
            } else if (V != 1) {
                const bool hi = lv > t;
                const int up = mode == 1 ? 2 : 3;
                const int down = mode == 1 ? 1 : (mode >= 4 ? 5 : 4);
                int next = hi ? up : down;
                timer = mode == 4 ? timeout : (mode == 5 ? timer - 1 : timer);
                next = mode == 5 && timer == 0 ? 6 : next;
                mode = mode == 6 ? 1 : next;
            }
            if (V == 3) acc += (unsigned)mode + __float_as_uint(lv);
            else { lr[b0 + u] = lv; if (V != 1) sr[b0 + u] = (unsigned char)mode; }
        }
#pragma unroll
        for (int u = 0; u < A; u++) cur[u] = nxt[u];
    }
    out[c] = s + mode + acc;
}

template <int V, int A, bool LUT>
int run(const char* name, int C, long nb, const double* p, float* level, unsigned char* status, double* out)
{
    hipEvent_t a, b;
    CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    for (int w = 0; w < 2; w++) hipLaunchKernelGGL((chain<V, A, LUT>), dim3(1), dim3(64), 0, 0, C, nb, 0.25, 4, 0.1f, p, level, status, out);
    CK(hipEventRecord(a, 0));
    for (int w = 0; w < 5; w++) hipLaunchKernelGGL((chain<V, A, LUT>), dim3(1), dim3(64), 0, 0, C, nb, 0.25, 4, 0.1f, p, level, status, out);
    CK(hipEventRecord(b, 0));
    CK(hipEventSynchronize(b));
    float ms; CK(hipEventElapsedTime(&ms, a, b));
    printf("%-28s C=%2d nb=%ld: %.3f ms per launch, %.1f ns per block\n", name, C, nb, ms / 5, ms / 5 * 1e6 / nb);
    return 0;
}

int main()
{
    const long nb = 65536;
    std::vector<double> h(64 * nb);
    for (size_t i = 0; i < h.size(); i++) h[i] = (((i % 65536) / (3 + (i / 65536) % 7)) % 5 == 0) ? 1.0 : 1e-4;
    double *p, *out; float* level; unsigned char* status;
    CK(hipMalloc(&p, h.size() * 8)); CK(hipMalloc(&out, 64 * 8)); CK(hipMalloc(&level, h.size() * 4)); CK(hipMalloc(&status, h.size()));
    CK(hipMemcpy(p, h.data(), h.size() * 8, hipMemcpyHostToDevice));
    for (int C : {16, 64}) {
        if (run<0, 8, false>("selects, 8 ahead", C, nb, p, level, status, out)) return 1;
        if (run<0, 8, true>("table, 8 ahead", C, nb, p, level, status, out)) return 1;
        if (run<0, 16, false>("selects, 16 ahead", C, nb, p, level, status, out)) return 1;
        if (run<0, 16, true>("table, 16 ahead", C, nb, p, level, status, out)) return 1;
        if (run<0, 32, false>("selects, 32 ahead", C, nb, p, level, status, out)) return 1;
        if (run<0, 32, true>("table, 32 ahead", C, nb, p, level, status, out)) return 1;
        if (run<1, 32, true>("smoothing alone, 32 ahead", C, nb, p, level, status, out)) return 1;
        if (run<3, 32, true>("table, 32 ahead, no stores", C, nb, p, level, status, out)) return 1;
    }
    return 0;
}
