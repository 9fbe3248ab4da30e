// TEST ONLY: top_weights() and top_order_pairs() of csrc/mppi_top_weights.h behind one C entry point, so that
// tests/test_gpu_top_candidates.py can hand them chosen doubles (the production kernel only ever sees what exp() left in the
// weight buffer).  Includes mppi_top_weights.h and nothing else of the product; built by tests/top_probe.py with the product's
// compiler flags.
//
// The entry point takes host arrays, allocates, copies, launches, copies back and returns the HIP error (0 = hipSuccess).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "mppi_top_weights.h"

namespace {

// workgroup s: the n highest of w[s * pitch .. + k), as k_top_weights runs it (one workgroup of kTopBlock per vector); nothing
// at or past column k of a vector is read
__global__ __launch_bounds__(ccv::kTopBlock) void k_top(const double* w, const int pitch, const int k, const int n, int* idx_out,
                                                        double* w_out) {
    const size_t b = blockIdx.x;
    ccv::top_weights<ccv::kTopBlock>(w + b * (size_t)pitch, k, n, idx_out + b * n, w_out + b * n);
}

}  // namespace

extern "C" {

// w [n_vec][pitch] doubles, of which columns 0 .. k - 1 of every row take part; 1 <= n <= k <= pitch.
// raw_idx [n_vec][n] int32, raw_bits [n_vec][n] uint64: what the kernel wrote, in its own layout (the weights as their bits);
// ord_idx, ord_bits: the same after top_order_pairs(), which is what ccv_mppi_read_top_candidates hands out.
int probe_top(const int n_vec, const int pitch, const int k, const int n, const double* w, int32_t* raw_idx, uint64_t* raw_bits,
              int32_t* ord_idx, uint64_t* ord_bits) {
    if (n_vec < 1 || k < 1 || pitch < k || n < 1 || n > k || !w || !raw_idx || !raw_bits || !ord_idx || !ord_bits) return (int)hipErrorInvalidValue;
    const size_t in_bytes = (size_t)n_vec * pitch * sizeof(double), cells = (size_t)n_vec * n;
    double* d_w = nullptr;
    int* d_idx = nullptr;
    double* d_sel = nullptr;
    hipError_t e = hipMalloc(&d_w, in_bytes);
    if (e == hipSuccess) e = hipMalloc(&d_idx, cells * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&d_sel, cells * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(d_w, w, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_idx, 0xFF, cells * sizeof(int));       // (a cell the kernel leaves out reads as -1 ...
    if (e == hipSuccess) e = hipMemset(d_sel, 0xFF, cells * sizeof(double));   //  ... and all ones)
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_top, dim3(n_vec), dim3(ccv::kTopBlock), 0, 0, d_w, pitch, k, n, d_idx, d_sel);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(raw_idx, d_idx, cells * sizeof(int), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(raw_bits, d_sel, cells * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(d_w);
    (void)hipFree(d_idx);
    (void)hipFree(d_sel);
    if (e != hipSuccess) return (int)e;
    static_assert(sizeof(int) == sizeof(int32_t) && sizeof(double) == sizeof(uint64_t), "the two layouts are one");
    memcpy(ord_idx, raw_idx, cells * sizeof(int32_t));
    std::vector<double> sel(n);
    for (int s = 0; s < n_vec; ++s) {
        memcpy(sel.data(), raw_bits + (size_t)s * n, n * sizeof(double));
        ccv::top_order_pairs(n, ord_idx + (size_t)s * n, sel.data());
        memcpy(ord_bits + (size_t)s * n, sel.data(), n * sizeof(double));
    }
    return 0;
}

}  // extern "C"
