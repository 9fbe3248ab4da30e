// TEST ONLY: the device functions of csrc/noise_spec.h behind a C entry point each, so that tests/test_gpu_noise.py can hand
// them chosen words (the production kernels only ever feed them what Philox emits).  Includes noise_spec.h and nothing else of
// the product; built by tests/noise_probe.py with the product's compiler flags.
//
// Every entry point takes host arrays, allocates, copies, launches, copies back and returns the HIP error (0 = hipSuccess).
// Kernels: one dimension, 256 threads, thread i owns elements [i N, (i + 1) N) and touches none at or beyond n_pad; the host
// pads the inputs to n_pad = a multiple of N, so every thread that passes the bounds check has N whole elements.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "noise_spec.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void k_philox(const uint32_t* __restrict__ ctr, const uint32_t k0, const uint32_t k1,
                                                     uint32_t* __restrict__ out, const size_t n) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const ccv::Philox4 r = ccv::philox4x32_10(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], k0, k1);
    out[4 * i] = r.x;
    out[4 * i + 1] = r.y;
    out[4 * i + 2] = r.z;
    out[4 * i + 3] = r.w;
}

// n_pad is a multiple of N
template <int N>
__global__ __launch_bounds__(kThreads) void k_philox_n(const uint32_t* __restrict__ ctr, const uint32_t k0, const uint32_t k1,
                                                       uint32_t* __restrict__ out, const size_t n_pad) {
    const size_t first = ((size_t)blockIdx.x * kThreads + threadIdx.x) * N;
    if (first + N > n_pad) return;
    uint32_t c0[N], c1[N], c2[N], c3[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        c0[j] = ctr[4 * (first + j)];
        c1[j] = ctr[4 * (first + j) + 1];
        c2[j] = ctr[4 * (first + j) + 2];
        c3[j] = ctr[4 * (first + j) + 3];
    }
    ccv::philox4x32_10_n<N>(c0, c1, c2, c3, k0, k1);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        out[4 * (first + j)] = c0[j];
        out[4 * (first + j) + 1] = c1[j];
        out[4 * (first + j) + 2] = c2[j];
        out[4 * (first + j) + 3] = c3[j];
    }
}

__global__ __launch_bounds__(kThreads) void k_box_muller(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                         float* __restrict__ z0, float* __restrict__ z1, const size_t n) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    float x, y;
    ccv::box_muller_f32(a[i], b[i], x, y);
    z0[i] = x;
    z1[i] = y;
}

template <int N>
__global__ __launch_bounds__(kThreads) void k_box_muller_n(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                           float* __restrict__ z0, float* __restrict__ z1, const size_t n_pad) {
    const size_t first = ((size_t)blockIdx.x * kThreads + threadIdx.x) * N;
    if (first + N > n_pad) return;
    uint32_t aa[N], bb[N];
    float x[N], y[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        aa[j] = a[first + j];
        bb[j] = b[first + j];
    }
    ccv::box_muller_f32_n<N>(aa, bb, x, y);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        z0[first + j] = x[j];
        z1[first + j] = y[j];
    }
}

__global__ __launch_bounds__(kThreads) void k_sqrt(const float* __restrict__ x, float* __restrict__ s_cr,
                                                   float* __restrict__ s_builtin, const size_t n) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    s_cr[i] = ccv::sqrt_cr_radius(x[i]);
    s_builtin[i] = __builtin_sqrtf(x[i]);
}

// device arrays of one call, freed when it returns
struct Arrays {
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    ~Arrays() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    // `bytes` of device memory, zeroed, the first `fill` of them copied from `src` (the rest is the padding)
    void* in(const void* src, const size_t fill, const size_t bytes) {
        void* p = out(bytes);
        if (err == hipSuccess && fill) err = hipMemcpy(p, src, fill, hipMemcpyHostToDevice);
        return p;
    }
    void* out(const size_t bytes) {
        void* p = nullptr;
        if (err != hipSuccess) return nullptr;
        if ((err = hipMalloc(&p, bytes ? bytes : 1)) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        err = hipMemset(p, 0, bytes ? bytes : 1);
        return p;
    }
    void back(void* dst, const void* src, const size_t bytes) {
        if (err == hipSuccess) err = hipDeviceSynchronize();
        if (err == hipSuccess && bytes) err = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    }
    void launched() {
        if (err == hipSuccess) err = hipGetLastError();
    }
};

size_t round_up(const size_t n, const size_t m) { return (n + m - 1) / m * m; }
unsigned blocks_for(const size_t threads) { return (unsigned)((threads + kThreads - 1) / kThreads); }

template <int N>
void launch_philox_n(const uint32_t* ctr, const uint32_t k0, const uint32_t k1, uint32_t* out, const size_t n_pad) {
    hipLaunchKernelGGL(k_philox_n<N>, dim3(blocks_for(n_pad / N)), dim3(kThreads), 0, 0, ctr, k0, k1, out, n_pad);
}
template <int N>
void launch_box_muller_n(const uint32_t* a, const uint32_t* b, float* z0, float* z1, const size_t n_pad) {
    hipLaunchKernelGGL(k_box_muller_n<N>, dim3(blocks_for(n_pad / N)), dim3(kThreads), 0, 0, a, b, z0, z1, n_pad);
}

}  // namespace

extern "C" {

// form 0: philox4x32_10; 3, 4, 5: philox4x32_10_n<form>, a thread taking `form` consecutive blocks.  ctr, out: [n][4]; key: [2]
int probe_philox(const int form, const size_t n, const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
    if (!(form == 0 || form == 3 || form == 4 || form == 5) || !ctr || !key || !out) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    const size_t n_pad = round_up(n, form ? (size_t)form : 1);
    Arrays d;
    const uint32_t* d_ctr = (const uint32_t*)d.in(ctr, n * 16, n_pad * 16);
    uint32_t* d_out = (uint32_t*)d.out(n_pad * 16);
    if (d.err == hipSuccess) {
        if (form == 0) hipLaunchKernelGGL(k_philox, dim3(blocks_for(n_pad)), dim3(kThreads), 0, 0, d_ctr, key[0], key[1], d_out, n_pad);
        else if (form == 3) launch_philox_n<3>(d_ctr, key[0], key[1], d_out, n_pad);
        else if (form == 4) launch_philox_n<4>(d_ctr, key[0], key[1], d_out, n_pad);
        else launch_philox_n<5>(d_ctr, key[0], key[1], d_out, n_pad);
        d.launched();
    }
    d.back(out, d_out, n * 16);
    return (int)d.err;
}

// form 0: box_muller_f32; 6, 8, 10: box_muller_f32_n<form>.  a, b, z0, z1: [n]
int probe_box_muller(const int form, const size_t n, const uint32_t* a, const uint32_t* b, float* z0, float* z1) {
    if (!(form == 0 || form == 6 || form == 8 || form == 10) || !a || !b || !z0 || !z1) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    const size_t n_pad = round_up(n, form ? (size_t)form : 1);
    Arrays d;
    const uint32_t* d_a = (const uint32_t*)d.in(a, n * 4, n_pad * 4);
    const uint32_t* d_b = (const uint32_t*)d.in(b, n * 4, n_pad * 4);
    float* d_z0 = (float*)d.out(n_pad * 4);
    float* d_z1 = (float*)d.out(n_pad * 4);
    if (d.err == hipSuccess) {
        if (form == 0) hipLaunchKernelGGL(k_box_muller, dim3(blocks_for(n_pad)), dim3(kThreads), 0, 0, d_a, d_b, d_z0, d_z1, n_pad);
        else if (form == 6) launch_box_muller_n<6>(d_a, d_b, d_z0, d_z1, n_pad);
        else if (form == 8) launch_box_muller_n<8>(d_a, d_b, d_z0, d_z1, n_pad);
        else launch_box_muller_n<10>(d_a, d_b, d_z0, d_z1, n_pad);
        d.launched();
    }
    d.back(z0, d_z0, n * 4);
    d.back(z1, d_z1, n * 4);
    return (int)d.err;
}

// s_cr: sqrt_cr_radius(x); s_builtin: __builtin_sqrtf(x) as the product's flags compile it.  x: [n], inside sqrt_cr_radius's domain
int probe_sqrt(const size_t n, const float* x, float* s_cr, float* s_builtin) {
    if (!x || !s_cr || !s_builtin) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    Arrays d;
    const float* d_x = (const float*)d.in(x, n * 4, n * 4);
    float* d_a = (float*)d.out(n * 4);
    float* d_b = (float*)d.out(n * 4);
    if (d.err == hipSuccess) {
        hipLaunchKernelGGL(k_sqrt, dim3(blocks_for(n)), dim3(kThreads), 0, 0, d_x, d_a, d_b, n);
        d.launched();
    }
    d.back(s_cr, d_a, n * 4);
    d.back(s_builtin, d_b, n * 4);
    return (int)d.err;
}

}  // extern "C"
