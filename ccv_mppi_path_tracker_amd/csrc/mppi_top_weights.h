// "The N highest weights of one vector, in order" (DESIGN.md section 14): the device function behind k_top_weights (k_update.hip)
// and the host ordering behind ccv_mppi_read_top_candidates (capi_stage.hip); no kernel.  tests/probe/top_probe.hip hands both
// chosen doubles.
//
// The order is defined by ONE 64-bit key, top_key() below, and the sample index:
//     every NaN, of any sign or payload          -> 0xFFFFFFFFFFFFFFFF
//     anything else                              -> its bits
// on the domain  w >= +0  or  w is NaN  -- all that exp() produces -- where the unsigned order of the bits is the order of the
// numbers.  (key descending, index ascending) is then: NaN weights first, by sample index among themselves; +inf; the finite
// weights, descending; ties to the lower sample index.  No number shares the NaN key: all ones are a NaN's own bits.  (A negative
// weight, -0.0 included, is outside the domain: its sign bit would put it above +inf.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace ccv {

constexpr int kTopBlock = 1024;   // the workgroup of k_top_weights

__host__ __device__ inline unsigned long long top_key(const double w) {
    unsigned long long bits;
    __builtin_memcpy(&bits, &w, sizeof bits);
    return w != w ? ~0ull : bits;
}

// Host: the n pairs (idx[j], w[j]) that top_weights() wrote, put in order in place: key descending, sample index ascending.  The
// weights keep their bits (a NaN its payload).  The comparison is total, because no two pairs share an index.
inline void top_order_pairs(const int n, int* idx, double* w) {
    std::vector<int> order(n), idx_in(idx, idx + n);
    std::vector<double> w_in(w, w + n);
    for (int j = 0; j < n; ++j) order[j] = j;
    std::sort(order.begin(), order.end(), [&](const int a, const int b) {
        const unsigned long long ka = top_key(w_in[a]), kb = top_key(w_in[b]);
        return ka != kb ? ka > kb : idx_in[a] < idx_in[b];
    });
    for (int j = 0; j < n; ++j) {
        idx[j] = idx_in[order[j]];
        w[j] = w_in[order[j]];
    }
}

// Radix select on top_key(): eight 8-bit passes from the top find the N-th largest key T and how many samples equal to T
// belong to the answer; a last pass writes the pairs (sample index, weight) -- all samples with key > T in index order at
// [0, n_greater), then the lowest-index n_equal samples with key == T in index order behind them -- positions come from
// block-wide prefix sums in index order, so the output is the same on every run.  top_order_pairs() sorts the N pairs.
// 1 <= N <= K; every one of the workgroup's NT threads calls it (NT a multiple of 64, at least 256); nothing at or past w[K]
// is read, nothing at or past idx_out[N] / w_out[N] written.  The LDS (1176 bytes at NT = 1024) is the function's own; it has
// internal linkage so that each unit's copy lays its LDS out by itself.
template <int NT>
static __device__ __forceinline__ void top_weights(const double* w, int K, int N, int* idx_out, double* w_out) {
    static_assert(NT % 64 == 0 && NT >= 256, "whole waves, and a thread per histogram bin");
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_remaining;
    __shared__ int wsum[NT / 64][2];
    __shared__ int s_base[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) {
        s_prefix = 0ull;
        s_remaining = N;
    }
    __syncthreads();
    for (int pass = 7; pass >= 0; --pass) {
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        const unsigned long long prefix = s_prefix;
        for (int i = tid; i < K; i += NT) {
            const unsigned long long key = top_key(w[i]);
            const bool match = pass == 7 || (key >> (8 * (pass + 1))) == prefix;
            if (match) atomicAdd(&hist[(unsigned int)(key >> (8 * pass)) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            int rem = s_remaining, b = 255;
            for (; b > 0; --b) {
                if ((int)hist[b] >= rem) break;
                rem -= (int)hist[b];
            }
            s_remaining = rem;                 // how many of bin b (and, after the last pass, of key T) are still wanted
            s_prefix = (prefix << 8) | (unsigned long long)b;
        }
        __syncthreads();
    }
    const unsigned long long T = s_prefix;
    const int n_equal = s_remaining, n_greater = N - n_equal;
    if (tid == 0) s_base[0] = s_base[1] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < K; i0 += NT) {
        const int i = i0 + tid;
        const unsigned long long key = i < K ? top_key(w[i]) : 0ull;
        const int fg = (i < K && key > T) ? 1 : 0, fe = (i < K && key == T) ? 1 : 0;
        // exclusive prefix sums over the block in index order: wave ballots, then a scan of the 16 wave totals
        const unsigned long long bg = __ballot(fg), be = __ballot(fe);
        const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        const int pg = __popcll(bg & below), pe = __popcll(be & below);
        if (lane == 0) {
            wsum[wv][0] = __popcll(bg);
            wsum[wv][1] = __popcll(be);
        }
        __syncthreads();
        int og = s_base[0], oe = s_base[1];
        for (int j = 0; j < wv; ++j) {
            og += wsum[j][0];
            oe += wsum[j][1];
        }
        if (fg && og + pg < n_greater) {   // (always true: exactly n_greater keys exceed T; the test keeps the store inside [0, N))
            idx_out[og + pg] = i;
            w_out[og + pg] = w[i];
        }
        if (fe && oe + pe < n_equal) {
            idx_out[n_greater + oe + pe] = i;
            w_out[n_greater + oe + pe] = w[i];
        }
        __syncthreads();
        if (tid == 0) {
            int tg = 0, te = 0;
            for (int j = 0; j < NT / 64; ++j) {
                tg += wsum[j][0];
                te += wsum[j][1];
            }
            s_base[0] += tg;
            s_base[1] += te;
        }
        __syncthreads();
    }
}

}  // namespace ccv
