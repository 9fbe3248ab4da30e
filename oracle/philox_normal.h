// TEST INFRASTRUCTURE ONLY (see oracle/README.md).  Independent CPU restatement
// of the repo's OWN counter-based noise spec (DESIGN.md "Noise spec"): Philox4x32-10
// (Salmon et al., SC'11 -- published algorithm, Random123 known-answer vectors are
// checked in tests/test_oracle.py and tests/test_noise_reference.py, and on the
// device in tests/test_gpu_noise.py) followed by an exactly-specified fp32
// polynomial Box-Muller (held to the exact transform by tests/noise_reference.py).  This is NOT part of the reference (the reference draws
// from std::mt19937, src/diff_drive_mppi.cpp:83-90); it exists so the GPU
// sampler can be checked bit-for-bit on the CPU.  Written separately from
// ccv_mppi_path_tracker_amd/csrc/noise_spec.h on purpose: two implementations,
// one spec.
#pragma once
#include <cmath>
#include <cstdint>

namespace orc_noise {

struct U4 { uint32_t w[4]; };

inline U4 philox4x32_10(U4 ctr, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = 0xD2511F53ull * (uint64_t)ctr.w[0];
        const uint64_t p1 = 0xCD9E8D57ull * (uint64_t)ctr.w[2];
        U4 nx;
        nx.w[0] = (uint32_t)(p1 >> 32) ^ ctr.w[1] ^ k0;
        nx.w[1] = (uint32_t)p1;
        nx.w[2] = (uint32_t)(p0 >> 32) ^ ctr.w[3] ^ k1;
        nx.w[3] = (uint32_t)p0;
        ctr = nx;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return ctr;
}

// fp32 coefficient tables (tools/fit_normal_polys.py).  Same literals as the product header.
static const float kQ[9] = {0x1.715476p+0f, -0x1.715476p-1f, 0x1.ec73e0p-2f, -0x1.715946p-2f, 0x1.26cfb8p-2f,
                            -0x1.e9df04p-3f, 0x1.ba9caap-3f, -0x1.a548fcp-3f, 0x1.f702acp-4f};
static const float kS[4] = {-0x1.555556p-3f, 0x1.11110ep-7f, -0x1.a013a2p-13f, 0x1.6dbc3ep-19f};
static const float kC[4] = {-0x1.000000p-1f, 0x1.55554cp-5f, -0x1.6c0df8p-10f, 0x1.9a6a98p-16f};

// The argument of the radius' square root, -2 ln u1 in fp32, u1 = max(a,1) * 2^-32 (normal_pair's first half; the noise tests
// hand it to the device's square root on its own)
inline float radius_arg(uint32_t a) {
    uint32_t a1 = a ? a : 1u;
    int lz = __builtin_clz(a1);
    uint32_t m = a1 << lz;                           // u1 = m * 2^(-32-lz), top bit of m set
    // mantissa folded to [sqrt(.5), sqrt(2)): t = mantissa - 1 taken straight from the integer so that it keeps
    // full relative precision when u1 -> 1 (0xB504F333 = floor(sqrt(2) * 2^31))
    int eb = m > 0xB504F333u ? 1 : 0;
    float t = eb ? -((float)(uint32_t)(0u - m) * 0x1p-32f) : (float)(m - 0x80000000u) * 0x1p-31f;
    float L0 = (float)(1 + lz - eb);
    float q = kQ[8];
    for (int i = 7; i >= 0; --i) q = fmaf(q, t, kQ[i]);
    float L = fmaf(-t, q, L0);                      // -log2(u1)
    return L * 0x1.62e430p+0f;                      // * 2 ln 2
}

// Two words -> two standard normals (fp32 resolution).  Every step is an IEEE-754
// basic operation (or an integer op), so the result is bit-reproducible.
inline void normal_pair(uint32_t a, uint32_t b, float* z0, float* z1) {
    // radius: r = sqrt(-2 ln u1), u1 = max(a,1) * 2^-32
    float r = sqrtf(radius_arg(a));
    // angle: quadrant from the two top bits, centred remainder in [-pi/4, pi/4)
    uint32_t quad = b >> 30;
    int32_t f = (int32_t)(b & 0x3FFFFFFFu) - (1 << 29);
    float al = (float)f * 0x1.921fb6p-30f;          // (pi/2) * 2^-30
    float w = al * al;
    float s = kS[3], c = kC[3];
    for (int i = 2; i >= 0; --i) { s = fmaf(s, w, kS[i]); c = fmaf(c, w, kC[i]); }
    float sn = fmaf(al * w, s, al);
    float cs = fmaf(w, c, 1.0f);
    float cq, sq;
    switch (quad) {
        case 0: cq = cs;  sq = sn;  break;
        case 1: cq = -sn; sq = cs;  break;
        case 2: cq = -cs; sq = -sn; break;
        default: cq = sn; sq = -cs; break;
    }
    *z0 = r * cq;
    *z1 = r * sq;
}

// normal number n (= t*u_dim + d) of global sample k in iteration `iter` under `seed`
inline float normal_at(uint64_t seed, uint64_t iter, uint32_t k, uint32_t n) {
    U4 ctr;
    ctr.w[0] = k; ctr.w[1] = n >> 2; ctr.w[2] = (uint32_t)iter; ctr.w[3] = (uint32_t)(iter >> 32);
    U4 o = philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
    float z0, z1;
    if ((n & 2u) == 0) normal_pair(o.w[0], o.w[1], &z0, &z1);
    else               normal_pair(o.w[2], o.w[3], &z0, &z1);
    return (n & 1u) ? z1 : z0;
}

}  // namespace orc_noise
