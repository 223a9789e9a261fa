// membw — measured achievable HBM read bandwidth on THIS box (streaming
// dwordx4 reads, grid-strided, result sunk to defeat DCE). Anchors the
// roofline "achievable" figure quoted in DESIGN.md.
// Variants: U = 1, 2 or 4 independent loads in flight per lane and trip,
// plain or non-temporal, on the original 16384-block grid and on persistent
// grids of CUs x 4 and CUs x 8 blocks (the dense scan kernel's shapes).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

template <int U, bool NT>
__global__ void read_kernel(const ulonglong2 *__restrict__ p, size_t n,
                            unsigned long long *sink)
{
    unsigned long long acc = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    // whole trips: all U loads inside the buffer, issued before any is used
    for (; i + (U - 1) * stride < n; i += U * stride) {
        ulonglong2 v[U];
        #pragma unroll
        for (int u = 0; u < U; u++) {
            const ulonglong2 *q = p + i + u * stride;
            if (NT) {
                v[u].x = __builtin_nontemporal_load(&q->x);
                v[u].y = __builtin_nontemporal_load(&q->y);
            } else {
                v[u] = *q;
            }
        }
        #pragma unroll
        for (int u = 0; u < U; u++) acc ^= v[u].x ^ v[u].y;
    }
    for (; i < n; i += stride) {
        const ulonglong2 v = p[i];
        acc ^= v.x ^ v.y;
    }
    if (acc == 0xDEADBEEFCAFEF00DULL) atomicAdd(sink, acc);
}

template <int U, bool NT>
static void run(const char *name, int grid, const ulonglong2 *d, size_t n, size_t bytes,
                unsigned long long *sink, hipEvent_t e0, hipEvent_t e1)
{
    float best = 1e30f;
    for (int rep = 0; rep < 3; rep++) {
        hipEventRecord(e0);
        read_kernel<U, NT><<<dim3(grid), dim3(256)>>>(d, n, sink);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        if (ms < best) best = ms;
    }
    printf("%-4s U=%d grid=%6d: read %zu GiB in %.3f ms = %.2f TB/s (best of 3)\n",
           name, U, grid, bytes >> 30, best, bytes / (best / 1e3) / 1e12);
}

int main()
{
    const size_t bytes = 8ull << 30;               // 8 GiB
    const size_t n = bytes / 16;
    ulonglong2 *d = nullptr;
    unsigned long long *sink = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess ||
        hipMalloc(&sink, 8) != hipSuccess ||
        hipMemset(d, 0x5A, bytes) != hipSuccess) {
        fprintf(stderr, "membw: allocation failed\n");
        return 1;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
    const int cus = prop.multiProcessorCount;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    const int grids[3] = {16384, cus * 4, cus * 8};
    for (int g = 0; g < 3; g++) {
        run<1, false>("ld", grids[g], d, n, bytes, sink, e0, e1);
        run<2, false>("ld", grids[g], d, n, bytes, sink, e0, e1);
        run<4, false>("ld", grids[g], d, n, bytes, sink, e0, e1);
        run<1, true>("nt", grids[g], d, n, bytes, sink, e0, e1);
        run<2, true>("nt", grids[g], d, n, bytes, sink, e0, e1);
        run<4, true>("nt", grids[g], d, n, bytes, sink, e0, e1);
    }
    if (hipDeviceSynchronize() != hipSuccess) {
        fprintf(stderr, "membw: kernel failed\n");
        return 1;
    }
    return 0;
}
