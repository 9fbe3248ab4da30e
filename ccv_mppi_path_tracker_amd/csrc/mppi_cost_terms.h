// The cost terms of a batch handle's instance beyond the path: disc obstacles, moving discs, the occupancy grid -- their LDS
// layouts, staging and the per-block terms the rollout kernels of every family call.
#pragma once
#include "mppi_device_util.h"
#include "mppi_kernels.h"

namespace ccv {

// ---- per-instance disc obstacles of a batch handle (OBST kernels) -----------------------------
// The power of a point p with respect to disc j, |p - o_j|^2 - r_j^2, is |p|^2 + a_j px + b_j py + c_j in pose-relative
// coordinates -- the window distance's form with c_j = |o_j - x0|^2 - r_j^2 -- so the deepest penetration over the discs is
// a second minimum of the same kind over a second, short coefficient list.
struct ObstLds {
    double2 ab[kMaxObst];
    double c[kMaxObst];
};
// the instance's obstacle fields, from the row of the parameter table its record's head points at (A.frame: batch_view);
// wave-uniform, read through the constant address space
struct ObstRow {
    const double* xyr;
    double w;
    int n;
};
__device__ __forceinline__ ObstRow obst_row(const RolloutArgs& A) {
    typedef const BatchHead __attribute__((address_space(4))) * ConstHead;
    typedef const BatchParams __attribute__((address_space(4))) * ConstParams;
    const auto& P = *(ConstParams)(const void*)((ConstHead)(const void*)A.frame)->params;
    const int n = P.n_obst;
    return ObstRow{P.obst, P.w_obs, n < 0 ? 0 : (n > kMaxObst ? kMaxObst : n)};
}
// staging, once per workgroup: thread j = 0 .. kMaxObst-1 writes disc j's coefficients relative to the pose the kernel holds,
// or the padding a = b = 0, c = +inf (never the minimum) past the instance's count
__device__ __forceinline__ void obst_stage(const RolloutArgs& A, ObstLds& ob, const int j) {
    const ObstRow o = obst_row(A);
    double a = 0.0, b = 0.0, c = INFINITY;
    if (j < o.n) {
        const double ox = o.xyr[3 * j], oy = o.xyr[3 * j + 1], r = o.xyr[3 * j + 2];
        const double dx = ox - A.x0[0], dy = oy - A.x0[1];
        a = -2.0 * dx;
        b = -2.0 * dy;
        c = fma(dx, dx, dy * dy) - r * r;
    }
    ob.ab[j] = make_double2(a, b);
    ob.c[j] = c;
}
// cost += w_obs * max(max_j(r_j^2 - |p - o_j|^2), 0) for states i < nv of the NV held in registers (p relative to the pose).
// m: registers for the running minima (the window loop's, dead by now).  Four discs per iteration over the padded list; a NaN
// position gives s = NaN and v_max_f64(-NaN, 0) = 0.
template <int NV, int NM, bool MASK = false>   // MASK: only the first nv of the NV states count (the plain kernel's blocks)
__device__ __forceinline__ void obst_term(const RolloutArgs& A, const ObstLds& ob, const double (&px)[NM], const double (&py)[NM],
                                          double (&m)[NM], double& cost, const int nv = NV) {
    const ObstRow o = obst_row(A);
    const int n4 = (o.n + 3) & ~3;
    if (n4 == 0) return;
#pragma unroll
    for (int i = 0; i < NV; ++i) m[i] = INFINITY;
    if constexpr (MASK) {
        // the plain kernel: one disc per iteration, as window_min -- four at a time cost it 21 registers and a wave per SIMD
#pragma unroll 1
        for (int j = 0; j < n4; ++j) {
            const double2 ab = ob.ab[j];
            const double c = ob.c[j];
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const double t = fma(ab.x, px[i], fma(ab.y, py[i], c));
                asm("v_min_f64 %0, %1, %2" : "=v"(m[i]) : "v"(m[i]), "v"(t));
            }
        }
    } else {
        for (int j = 0; j < n4; j += 4) {
            double2 ab[4];
            double c[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                ab[jj] = ob.ab[j + jj];
                c[jj] = ob.c[j + jj];
            }
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const double f0 = fma(ab[0].x, px[i], fma(ab[0].y, py[i], c[0]));
                const double f1 = fma(ab[1].x, px[i], fma(ab[1].y, py[i], c[1]));
                const double f2 = fma(ab[2].x, px[i], fma(ab[2].y, py[i], c[2]));
                const double f3 = fma(ab[3].x, px[i], fma(ab[3].y, py[i], c[3]));
                const double t = fmin(fmin(f0, f1), fmin(f2, f3));
                asm("v_min_f64 %0, %1, %2" : "=v"(m[i]) : "v"(m[i]), "v"(t));   // (two quiet operands: pc_consume)
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const double s = m[i] + fma(px[i], px[i], py[i] * py[i]);
        double g;
        asm("v_max_f64 %0, -%1, 0" : "=v"(g) : "v"(s));
        if (!MASK || i < nv) cost = fma(o.w, g, cost);
    }
}

// ---- moving discs (MOVING kernels, on OBST) -----------------------------------------------------
// Disc j has a constant velocity v_j over the horizon: state k (k dynamics steps after the pose) is charged against the disc at
// o_j + v_j tau_k, tau_k = k dt.  The power of the point stays linear in (px, py); its coefficients become polynomials in tau:
//   a_j(tau) = a_j - 2 vx_j tau,  b_j(tau) = b_j - 2 vy_j tau,  c_j(tau) = c_j + 2 (d_j . v_j) tau + |v_j|^2 tau^2.
// Seven doubles per disc are staged once per workgroup; the coefficients of a (disc, state) pair are formed per lane, 4 FMA,
// from tau_k held wave-uniform.
struct ObstMovLds {
    double2 ab[kMaxObst];    // a, b
    double2 vab[kMaxObst];   // -2 vx, -2 vy
    double c[kMaxObst], c1[kMaxObst], c2[kMaxObst];   // c, 2 (d . v), |v|^2
};
__device__ __forceinline__ const double* obst_velocity_rows(const RolloutArgs& A) {
    typedef const BatchHead __attribute__((address_space(4))) * ConstHead;
    typedef const BatchParams __attribute__((address_space(4))) * ConstParams;
    return (*(ConstParams)(const void*)((ConstHead)(const void*)A.frame)->params).obst_v;
}
// staging: obst_stage's a, b, c, and the velocity's four coefficients; the padding has zero velocity
__device__ __forceinline__ void obst_stage_moving(const RolloutArgs& A, ObstMovLds& ob, const int j) {
    const ObstRow o = obst_row(A);
    const double* vrows = obst_velocity_rows(A);
    double a = 0.0, b = 0.0, c = INFINITY, va = 0.0, vb = 0.0, c1 = 0.0, c2 = 0.0;
    if (j < o.n) {
        const double ox = o.xyr[3 * j], oy = o.xyr[3 * j + 1], r = o.xyr[3 * j + 2];
        const double vx = vrows[2 * j], vy = vrows[2 * j + 1];
        const double dx = ox - A.x0[0], dy = oy - A.x0[1];
        a = -2.0 * dx;
        b = -2.0 * dy;
        c = fma(dx, dx, dy * dy) - r * r;
        va = -2.0 * vx;
        vb = -2.0 * vy;
        c1 = 2.0 * fma(dx, vx, dy * vy);
        c2 = fma(vx, vx, vy * vy);
    }
    ob.ab[j] = make_double2(a, b);
    ob.vab[j] = make_double2(va, vb);
    ob.c[j] = c;
    ob.c1[j] = c1;
    ob.c2[j] = c2;
}
// the staging a kernel of rung FORM does: thread j = 0 .. kMaxObst-1 of the workgroup's staging threads writes disc j into the one
// of the two arrays the kernel has declared -- Moving and up: ObstMovLds; Obst: ObstLds; below Obst: nothing.  (The range test
// stays with the caller, in the caller's own form: made in here, it compiled to other instructions in every kernel.)
template <BatchForm FORM>
__device__ __forceinline__ void obst_stage_form(const RolloutArgs& A, ObstLds* ob, ObstMovLds* obm, const int j) {
    if constexpr (FORM >= BatchForm::Moving) obst_stage_moving(A, *obm, j);
    else if constexpr (FORM >= BatchForm::Obst) obst_stage(A, *ob, j);
}
// obst_term with the discs where they are at each state's own time: state i of the NV held in registers is global step
// k0 + i (k0: the block's first step, wave-uniform), tau = double(k0 + i) * dt, one rounding.  One disc per iteration over the
// instance's own count; per (disc, state): at = fma(va, tau, a), bt = fma(vb, tau, b), ct = fma(fma(c2, tau, c1), tau, c),
// f = fma(at, px, fma(bt, py, ct)).  The rest is obst_term's.  With v = 0 every at, bt, ct is a, b, c exactly (tau finite).
template <int NV, int NM, bool MASK = false>
__device__ __forceinline__ void obst_term_moving(const RolloutArgs& A, const ObstMovLds& ob, const double (&px)[NM], const double (&py)[NM],
                                                 double (&m)[NM], double& cost, const int k0, const int nv = NV) {
    const ObstRow o = obst_row(A);
    if (o.n == 0) return;
    double tau[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        tau[i] = uniform_f64((double)(k0 + i) * A.dt);
        if constexpr (!MASK) m[i] = INFINITY;
    }
    if constexpr (MASK) {
        // the plain kernel: state by state, one running minimum alive at a time -- the same pairs, hence the same minima; with
        // all eight alive beside a disc's seven coefficients it needed 139 registers and lost a wave per SIMD
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            double mi = INFINITY;
#pragma unroll 1
            for (int j = 0; j < o.n; ++j) {
                const double2 ab = ob.ab[j], vab = ob.vab[j];
                const double c = ob.c[j], c1 = ob.c1[j], c2 = ob.c2[j];
                const double at = fma(vab.x, tau[i], ab.x);
                const double bt = fma(vab.y, tau[i], ab.y);
                const double ct = fma(fma(c2, tau[i], c1), tau[i], c);
                const double t = fma(at, px[i], fma(bt, py[i], ct));
                asm("v_min_f64 %0, %1, %2" : "=v"(mi) : "v"(mi), "v"(t));
            }
            const double s = mi + fma(px[i], px[i], py[i] * py[i]);
            double g;
            asm("v_max_f64 %0, -%1, 0" : "=v"(g) : "v"(s));
            if (i < nv) cost = fma(o.w, g, cost);
        }
    } else {
        // the cooperative kernels: disc by disc, all NV running minima alive, every state counted
#pragma unroll 1
        for (int j = 0; j < o.n; ++j) {
            const double2 ab = ob.ab[j], vab = ob.vab[j];
            const double c = ob.c[j], c1 = ob.c1[j], c2 = ob.c2[j];
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const double at = fma(vab.x, tau[i], ab.x);
                const double bt = fma(vab.y, tau[i], ab.y);
                const double ct = fma(fma(c2, tau[i], c1), tau[i], c);
                const double t = fma(at, px[i], fma(bt, py[i], ct));
                asm("v_min_f64 %0, %1, %2" : "=v"(m[i]) : "v"(m[i]), "v"(t));
            }
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const double s = m[i] + fma(px[i], px[i], py[i] * py[i]);
            double g;
            asm("v_max_f64 %0, -%1, 0" : "=v"(g) : "v"(s));
            cost = fma(o.w, g, cost);
        }
    }
}

// ---- occupancy grid (GRID kernels, on MOVING) ------------------------------------------------------
// State (x, y) AS STORED (absolute, the doubles of ccv_mppi_batch_read_candidates) reads one cell:
//   fx = (x - origin_x) * inv, fy = (y - origin_y) * inv      (one subtraction, one multiplication each, no FMA)
//   in = fx >= 0 && fx < nx && fy >= 0 && fy < ny             (fp64 compares: false for NaN, so a NaN state reads `outside`)
//   v  = in ? cells[(int)fy * nx + (int)fx] : outside
// G = the fp64 sum of (double)v over the states the path term covers, in state order from 0.0; cost = fma(w, G, cost) is the
// LAST thing added to a sample's cost.  The row is read wave-uniformly through the constant address space (as obst_row).
typedef const GridRow __attribute__((address_space(4))) * ConstGridRow;
__device__ __forceinline__ ConstGridRow grid_row(const RolloutArgs& A) {
    typedef const BatchHead __attribute__((address_space(4))) * ConstHead;
    typedef const BatchParams __attribute__((address_space(4))) * ConstParams;
    return (ConstGridRow)(const void*)(*(ConstParams)(const void*)((ConstHead)(const void*)A.frame)->params).grid;
}
// the gather of one state: ONE unconditional load whose address is the cell's, or that of the row's own `outside` field when the
// state is in no cell -- so a block's gathers are in flight together with no branch between them, and nothing but the loaded
// float is alive until it is summed (held beside the gathers, eight `in` masks cost the four-wave kernels sixteen scalar
// registers, which they spill into vector lanes)
struct GridTap {
    float v;
};
__device__ __forceinline__ GridTap grid_tap(const ConstGridRow g, const double x, const double y) {
    typedef const float __attribute__((address_space(1))) * GlobalF32;
    const double fx = (x - g->origin_x) * g->inv;
    const double fy = (y - g->origin_y) * g->inv;
    const int nx = g->nx;
    const bool in = fx >= 0.0 && fx < (double)nx && fy >= 0.0 && fy < (double)g->ny;
    const int ix = (int)(in ? fx : 0.0), iy = (int)(in ? fy : 0.0);   // (in: 0 <= fx < 32 768 -- truncation is exact)
    const uint64_t cell = (uint64_t)(uintptr_t)g->cells + (uint64_t)(uint32_t)(iy * nx + ix) * 4u;   // (nx ny <= 2^26)
    const uint64_t outside = (uint64_t)(uintptr_t)(const void*)g + offsetof(GridRow, outside);
    return GridTap{*(GlobalF32)(uintptr_t)(in ? cell : outside)};
}
__device__ __forceinline__ double grid_value(const GridTap& t) { return (double)t.v; }
// the per-lane accumulator of a wave that meets every state of its sample (null row: the instance has no map).  slot: the sum
// lives in LDS instead of in G (the plain kernel)
struct GridAcc {
    ConstGridRow row;
    double G;
    int nstates;   // states that reach the path cost
    double* slot;
};
// states t0 .. t0+NV-1 held in registers: all gathers first (grid_issue), then the sum in state order (grid_sum); states at or
// past nstates do not count
template <int NV>
__device__ __forceinline__ void grid_issue(const GridAcc& ga, const double (&xv)[NV], const double (&yv)[NV], GridTap (&tap)[NV]) {
    if (!ga.row) return;
#pragma unroll
    for (int i = 0; i < NV; ++i) tap[i] = grid_tap(ga.row, xv[i], yv[i]);
}
template <int NV>
__device__ __forceinline__ void grid_sum(GridAcc& ga, const GridTap (&tap)[NV], const int t0) {
    if (!ga.row) return;
    double G = ga.slot ? *ga.slot : ga.G;
#pragma unroll
    for (int i = 0; i < NV; ++i)
        if (t0 + i < ga.nstates) G += grid_value(tap[i]);
    if (ga.slot) *ga.slot = G;
    else ga.G = G;
}
__device__ __forceinline__ double grid_total(const GridAcc& ga) { return ga.slot ? *ga.slot : ga.G; }

}  // namespace ccv
