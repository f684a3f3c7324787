// What the scalar kernel-argument loads at a kernel's entry cost per launch (gfx950), and what preloading the first 14 argument dwords
// into SGPRs (-mllvm -amdgpu-kernarg-preload-count=14, scopa_amd/build.py) takes off it.  A chain of dependent launches (one in-order
// stream, every launch reads what the one before it wrote) of a kernel that needs ALL its 14 or 30 argument dwords for the address of
// its one vector load, then stores: the argument block is freshly written for every launch, so its first scalar load misses.  Shapes:
// 93 x 64 threads (k_mccfr_apply_groups at 738 infosets) and 256 x 1024 (k_mccfr_traverse).  Build twice and run both on the GPU box:
//   hipcc --offload-arch=gfx950 -O3 -o kernarg_entry_plain kernarg_entry.hip
//   hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-kernarg-preload-count=14 -o kernarg_entry_preload kernarg_entry.hip
//   ./kernarg_entry_plain plain ; ./kernarg_entry_preload preload
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdint>
#include <cstdio>

constexpr uint32_t kCells = 1u << 18;   // 256 x 1024 floats; every index is masked into it

#define W4(p) uint32_t p##0, uint32_t p##1, uint32_t p##2, uint32_t p##3
#define S4(p) (p##0 + p##1 + p##2 + p##3)

// 2 + 12 = 14 argument dwords
template <int T>
__global__ void __launch_bounds__(T) k14(float *buf, W4(a), W4(b), W4(c)) {
    const uint32_t i = (blockIdx.x * T + threadIdx.x + S4(a) + S4(b) + S4(c)) & (kCells - 1);
    buf[i] = buf[i] + 1.0f;
}

// 2 + 28 = 30 argument dwords: 16 of them behind the preloaded 14
template <int T>
__global__ void __launch_bounds__(T) k30(float *buf, W4(a), W4(b), W4(c), W4(d), W4(e), W4(f), W4(g)) {
    const uint32_t i = (blockIdx.x * T + threadIdx.x + S4(a) + S4(b) + S4(c) + S4(d) + S4(e) + S4(f) + S4(g)) & (kCells - 1);
    buf[i] = buf[i] + 1.0f;
}

// the words of a launch sum to 0 mod 2^32 (the compiler cannot know): v, ~v + 1 pairs
#define Z4(v) (v), 0u - (v), (v) * 3u, 0u - (v) * 3u

template <int T, int NW> static double chain(float *d, int grid, int launches, uint32_t v) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < launches; i++) {
        const uint32_t w = v + (uint32_t)i;
        if (NW == 14) hipLaunchKernelGGL(k14<T>, dim3(grid), dim3(T), 0, 0, d, Z4(w), Z4(w + 7u), Z4(w + 11u));
        else hipLaunchKernelGGL(k30<T>, dim3(grid), dim3(T), 0, 0, d, Z4(w), Z4(w + 7u), Z4(w + 11u), Z4(w + 13u), Z4(w + 17u), Z4(w + 19u), Z4(w + 23u));
    }
    (void)hipDeviceSynchronize();
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / launches;
}

template <int T, int NW> static bool run(const char *label, float *d, int grid) {
    const int launches = 2000, warm = 200;
    (void)hipMemset(d, 0, kCells * sizeof(float));
    chain<T, NW>(d, grid, warm, 1u);
    double best = 1e30, worst = 0.0;
    for (int r = 0; r < 5; r++) {
        const double us = chain<T, NW>(d, grid, launches, 1000u * (uint32_t)r);
        best = us < best ? us : best;
        worst = us > worst ? us : worst;
    }
    float h = 0.f;
    (void)hipMemcpy(&h, d, sizeof(float), hipMemcpyDeviceToHost);
    const bool ok = h == (float)(warm + 5 * launches) && hipGetLastError() == hipSuccess;   // cell 0 was incremented by every launch
    printf("%-8s %4d x %4d threads, %2d argument dwords: %6.2f us per launch (best of 5 x %d; worst %6.2f)%s\n", label, grid, T, NW, best, launches,
           worst, ok ? "" : "  WRONG RESULT");
    return ok;
}

int main(int argc, char **argv) {
    const char *label = argc > 1 ? argv[1] : "build";
    float *d = nullptr;
    if (hipMalloc(&d, kCells * sizeof(float)) != hipSuccess) { fprintf(stderr, "no device memory\n"); return 1; }
    bool ok = true;
    ok &= run<64, 14>(label, d, 93);
    ok &= run<64, 30>(label, d, 93);
    ok &= run<1024, 14>(label, d, 256);
    ok &= run<1024, 30>(label, d, 256);
    (void)hipFree(d);
    return ok ? 0 : 1;
}
