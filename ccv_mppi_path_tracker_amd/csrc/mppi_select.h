// "The N lowest costs of one segment, in order" by one workgroup: device functions only, no kernel.
// k_best_candidates (k_feed.hip) runs them once per instance of a batch; tests/probe/select_probe.hip hands them chosen doubles.
//
// The order is defined by ONE 64-bit key, select_key() below, and the sample index:
//     every NaN, of any sign or payload          -> 0xFFFFFFFFFFFFFFFF
//     -0.0                                       -> the key of +0.0
//     anything else                              -> bits ^ (sign ? ~0 : 1 << 63)
// so that unsigned key order is  -inf < ... < -0 = +0 < ... < +inf < NaN, and (key, index) ascending is the order of
// np.lexsort((arange(K), cost)): costs ascend, ties go to the lower sample index, NaN costs come last, by index among themselves.
// (No number shares the NaN key: all ones would need the bits 0x7FFF..F, which are a NaN's.)
//
// select_lowest(): radix select over the key, eight passes of eight bits from the top, the histogram in LDS, finds the N-th
// lowest key T and how many samples equal to T belong to the answer; one more pass over the segment compacts the pairs
// (key, index) with key < T, and the lowest-index ones with key == T, into LDS; a bitonic sort of those at most 1024 pairs by
// (key, index) puts them in order.  The result is a pure function of the segment's keys: positions in the compaction come
// from prefix sums in index order, and the sort's comparison is total (no two pairs are equal).  No cross-workgroup
// communication; LDS: 12 KB for the pairs, 1 KB for the histogram.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ccv {

constexpr int kSelectMax = 1024;   // CCV_MPPI_BEST_MAX: pairs one workgroup orders

__host__ __device__ inline unsigned long long select_key(const double c) {
    if (c != c) return ~0ull;
    if (c == 0.0) return 1ull << 63;   // (+0.0 and -0.0)
    unsigned long long bits;
    __builtin_memcpy(&bits, &c, sizeof bits);
    return bits ^ ((bits >> 63) ? ~0ull : 1ull << 63);
}

template <int NT>
struct SelectShared {
    unsigned long long key[kSelectMax];   // after select_lowest(): the N lowest keys, ascending
    int idx[kSelectMax];                  // ... and their sample indices
    unsigned int hist[256];
    unsigned long long prefix;
    int remaining;
    int wsum[NT / 64][2];
    int base[2];
};

// inclusive prefix sum over the 64 lanes: four row_shr steps inside every row of 16 (a lane without a source reads 0), then
// the totals of the rows before the lane's
__device__ __forceinline__ int wave_scan_inclusive(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);   // row_shr:8
    const int r0 = __builtin_amdgcn_readlane(v, 15), r1 = __builtin_amdgcn_readlane(v, 31), r2 = __builtin_amdgcn_readlane(v, 47);
    const int row = (threadIdx.x & 63) >> 4;
    return v + (row > 0 ? r0 : 0) + (row > 1 ? r1 : 0) + (row > 2 ? r2 : 0);
}

// The N lowest of seg[0 .. K) by (select_key, index), ascending, into s.key / s.idx [0 .. N).  1 <= N <= min(K, kSelectMax);
// every one of the workgroup's NT threads calls it (NT a multiple of 64, at least 64); nothing at or past seg[K] is read.
// Ends with a barrier: every thread may read the result.
template <int NT>
__device__ __forceinline__ void select_lowest(const double* __restrict__ seg, const int K, const int N, SelectShared<NT>& s) {
    static_assert(NT % 64 == 0 && NT >= 64, "whole waves");
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) {
        s.prefix = 0ull;
        s.remaining = N;
    }
    // ---- the N-th lowest key T: after pass p the top 8 (8 - p) bits of T are known, and how many samples of that prefix are wanted
    for (int pass = 7; pass >= 0; --pass) {
        for (int i = tid; i < 256; i += NT) s.hist[i] = 0u;
        __syncthreads();
        const unsigned long long prefix = s.prefix;
        for (int i = tid; i < K; i += NT) {
            const unsigned long long key = select_key(seg[i]);
            if (pass == 7 || (key >> (8 * (pass + 1))) == prefix) atomicAdd(&s.hist[(unsigned int)(key >> (8 * pass)) & 255u], 1u);
        }
        __syncthreads();
        if (wv == 0) {   // lane l: bins 4 l .. 4 l + 3; the bin in which the running count reaches `remaining`
            const int rem = s.remaining;
            int h[4];
            for (int j = 0; j < 4; ++j) h[j] = (int)s.hist[4 * lane + j];
            const int mine = h[0] + h[1] + h[2] + h[3];
            int below = wave_scan_inclusive(mine) - mine;
            for (int j = 0; j < 4; ++j) {
                if (below < rem && rem <= below + h[j]) {   // (exactly one bin of the 256: the counts of a prefix sum to >= rem)
                    s.prefix = (prefix << 8) | (unsigned long long)(4 * lane + j);
                    s.remaining = rem - below;
                }
                below += h[j];
            }
        }
        __syncthreads();
    }
    const unsigned long long T = s.prefix;
    const int n_equal = s.remaining, n_less = N - n_equal;
    if (tid == 0) s.base[0] = s.base[1] = 0;
    __syncthreads();
    // ---- compaction, NT samples at a time in index order: key < T at [0, n_less), the first n_equal of key == T behind them
    for (int i0 = 0; i0 < K; i0 += NT) {
        const int i = i0 + tid;
        const unsigned long long key = i < K ? select_key(seg[i]) : ~0ull;
        const int fl = (i < K && key < T) ? 1 : 0, fe = (i < K && key == T) ? 1 : 0;
        const unsigned long long bl = __ballot(fl), be = __ballot(fe);
        const unsigned long long lower = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        const int pl = __popcll(bl & lower), pe = __popcll(be & lower);
        if (lane == 0) {
            s.wsum[wv][0] = __popcll(bl);
            s.wsum[wv][1] = __popcll(be);
        }
        __syncthreads();
        int ol = s.base[0], oe = s.base[1];
        for (int j = 0; j < wv; ++j) {
            ol += s.wsum[j][0];
            oe += s.wsum[j][1];
        }
        if (fl && ol + pl < n_less) {   // (always true: there are exactly n_less keys below T; the test keeps the store inside s)
            s.key[ol + pl] = key;
            s.idx[ol + pl] = i;
        }
        if (fe && oe + pe < n_equal) {
            s.key[n_less + oe + pe] = key;
            s.idx[n_less + oe + pe] = i;
        }
        __syncthreads();
        if (tid == 0) {
            int tl = 0, te = 0;
            for (int j = 0; j < NT / 64; ++j) {
                tl += s.wsum[j][0];
                te += s.wsum[j][1];
            }
            s.base[0] += tl;
            s.base[1] += te;
        }
        __syncthreads();
    }
    // ---- bitonic sort of the N pairs by (key, index), padded to a power of two with pairs that sort behind every sample's
    int P = 1;
    while (P < N) P <<= 1;
    for (int i = N + tid; i < P; i += NT) {
        s.key[i] = ~0ull;
        s.idx[i] = 0x7FFFFFFF;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P / 2; t += NT) {
                const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;   // (bit j of a is clear)
                const unsigned long long ka = s.key[a], kb = s.key[b];
                const int ia = s.idx[a], ib = s.idx[b];
                const bool greater = ka > kb || (ka == kb && ia > ib);
                if (greater == ((a & k) == 0)) {
                    s.key[a] = kb;
                    s.key[b] = ka;
                    s.idx[a] = ib;
                    s.idx[b] = ia;
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace ccv
