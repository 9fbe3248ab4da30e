// TEST ONLY: select_lowest() of csrc/mppi_select.h behind one C entry point, so that tests/test_gpu_batch_feed.py can hand it
// chosen doubles (the production kernel only ever sees what a rollout left in the cost buffer).  Includes mppi_select.h and
// nothing else of the product; built by tests/select_probe.py with the product's compiler flags.
//
// The entry point takes host arrays, allocates, copies, launches, copies back and returns the HIP error (0 = hipSuccess).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mppi_select.h"

namespace {

constexpr int kThreads = 256;   // the product's workgroup (kBlock)

// workgroup s: the n lowest of seg[s * pitch .. + k); nothing at or past column k of a segment is read
__global__ __launch_bounds__(kThreads) void k_select(const double* __restrict__ seg, const int pitch, const int k, const int n,
                                                     int32_t* __restrict__ idx_out, unsigned long long* __restrict__ key_out) {
    __shared__ ccv::SelectShared<kThreads> s;
    const size_t b = blockIdx.x;
    ccv::select_lowest<kThreads>(seg + b * (size_t)pitch, k, n, s);
    for (int j = threadIdx.x; j < n; j += kThreads) {
        idx_out[b * n + j] = s.idx[j];
        key_out[b * n + j] = s.key[j];
    }
}

}  // namespace

extern "C" {

// seg [n_seg][pitch] doubles, of which columns 0 .. k - 1 of every row take part; 1 <= n <= min(k, 1024), k <= pitch.
// idx_out [n_seg][n] int32, key_out [n_seg][n] uint64 (select_key of the selected costs), both ascending by (key, index).
int probe_select(const int n_seg, const int pitch, const int k, const int n, const double* seg, int32_t* idx_out, uint64_t* key_out) {
    if (n_seg < 1 || k < 1 || pitch < k || n < 1 || n > k || n > ccv::kSelectMax || !seg || !idx_out || !key_out) return (int)hipErrorInvalidValue;
    const size_t in_bytes = (size_t)n_seg * pitch * sizeof(double), cells = (size_t)n_seg * n;
    double* d_seg = nullptr;
    int32_t* d_idx = nullptr;
    unsigned long long* d_key = nullptr;
    hipError_t e = hipMalloc(&d_seg, in_bytes);
    if (e == hipSuccess) e = hipMalloc(&d_idx, cells * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&d_key, cells * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemcpy(d_seg, seg, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_select, dim3(n_seg), dim3(kThreads), 0, 0, d_seg, pitch, k, n, d_idx, d_key);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(idx_out, d_idx, cells * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(key_out, d_key, cells * sizeof(uint64_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_seg);
    (void)hipFree(d_idx);
    (void)hipFree(d_key);
    return (int)e;
}

}  // extern "C"
