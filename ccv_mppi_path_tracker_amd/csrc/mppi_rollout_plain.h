// k_rollout_cost and k_sample: the plain family -- one sample per lane, one lane does everything for its sample, OCML sincos
// and true divisions (unbounded headings, any dt; CCV_MPPI_KERNEL=v1), and the stand-alone sampler of the stage-wise ABI.
#pragma once
#include "mppi_cost_terms.h"
#include "mppi_device_util.h"
#include "mppi_epilogue.h"
#include "mppi_kernels.h"
#include "noise_spec.h"

namespace ccv {

// min over the H window points of (a_j*px + b_j*py + c_j) for NV trajectory points held in registers.
// 2 FMA + 1 MIN per (point, window point): the O(K*H^2) core (calc_MinDistance, dd:183-192).
template <int NV, bool LDSWIN>
__device__ __forceinline__ void window_min(const double (&px)[kTU], const double (&py)[kTU], double (&m)[kTU], int H,
                                           const Window& W, const double2* s_ab, const double* s_c) {
#pragma unroll 2
    for (int j = 0; j < H; ++j) {
        double a, b, c;
        if constexpr (LDSWIN) {
            const double2 ab = s_ab[j];
            a = ab.x;
            b = ab.y;
            c = s_c[j];
        } else {
            a = W.a[j];
            b = W.b[j];
            c = W.c[j];
        }
        static_for<NV>([&](auto I) {
            constexpr int i = decltype(I)::value;
            m[i] = fmin(m[i], fma(a, px[i], fma(b, py[i], c)));
        });
    }
}

// BATCH: grid (workgroups per instance, B), instance = blockIdx.y (batch_view); VARIED: with per-instance parameters;
// OBST (on VARIED): with the instance's disc obstacles (obst_term); MOVING (on OBST): the discs move (obst_term_moving);
// GRID (on MOVING): the instance's occupancy grid, read in the state loop where x and y are stored (grid_tap)
template <int MODEL, int SRC, bool LDSWIN, BatchForm FORM = BatchForm::Single>
__global__ __launch_bounds__(kBlock) void k_rollout_cost(const RolloutArgs Ak, const Window W) {
    constexpr bool BATCH = FORM >= BatchForm::Batch, VARIED = FORM >= BatchForm::Varied, OBST = FORM >= BatchForm::Obst,
                   MOVING = FORM >= BatchForm::Moving, GRID = FORM >= BatchForm::Grid;
    static_assert(!BATCH || (LDSWIN && SRC == SRC_PHILOX), "the batch runs the fused iteration with the LDS window");
    constexpr int UD = udim_of(MODEL);
    __shared__ double2 s_ab[LDSWIN ? kMaxH : 1];
    __shared__ double s_c[LDSWIN ? kMaxH : 1];
    const RolloutArgs A = BATCH ? batch_view<VARIED>(Ak, (int)blockIdx.y) : Ak;
    const int H = A.H;
    ObstLds* obst_lds = nullptr;
    ObstMovLds* obst_mov = nullptr;
    if constexpr (MOVING) {
        __shared__ ObstMovLds s_obst_mov;
        obst_mov = &s_obst_mov;
    } else if constexpr (OBST) {
        __shared__ ObstLds s_obst;
        obst_lds = &s_obst;
    }
    if constexpr (BATCH) {
        const double* win = reinterpret_cast<const double*>(A.frame) + kBatchHeadDoubles;
        for (int j = threadIdx.x; j < H; j += kBlock) {
            s_ab[j] = make_double2(win[j], win[H + j]);
            s_c[j] = win[2 * H + j];
        }
        if (threadIdx.x < kMaxObst) obst_stage_form<FORM>(A, obst_lds, obst_mov, (int)threadIdx.x);
        __syncthreads();
    } else if constexpr (LDSWIN) {
        for (int j = threadIdx.x; j < H; j += kBlock) {
            s_ab[j] = make_double2(W.a[j], W.b[j]);
            s_c[j] = W.c[j];
        }
        __syncthreads();
    }
    const int k = blockIdx.x * kBlock + threadIdx.x + (BATCH ? (int)blockIdx.y * ((Ak.K + 63) & ~63) : 0);
    const bool live = k < A.K;
    const int kk = live ? k : A.K - 1;
    const size_t pitch = (size_t)A.pitch;
    const double dt = A.dt;
    const uint32_t kg = (uint32_t)(A.k_offset + kk);

    double x = A.x0[0], y = A.x0[1], yaw = A.x0[2];
    double roll = A.x0[3], pitchang = A.x0[4];
    double cost = 0.0;
    if constexpr (MODEL == CCV_MPPI_FULL_BODY) {
        // fb:408 -- identical for every sample
        cost += A.w_yaw * (yaw - A.yaw_ref0) * (yaw - A.yaw_ref0);
    }
    // full-body carry from step t-1 (the ZMP term of index t-1 needs controls t-1 and t, fb:468-486)
    double p_v = 0.0, p_rv = 0.0, p_sdir = 0.0, p_cdir = 1.0, p_c2 = 0.0, p_c3 = 0.0, p_ac = 0.0;
    const double fb_mgz = A.fb_mass * A.fb_gz;    // (mass*gravity_).z
    const double fb_den = A.fb_mass * A.fb_gz;    // mass*(gravity_-accel).dot(z); accel.z == 0 (fb:475,601)

    GridAcc grid_acc{};
    if constexpr (GRID) {
        // the lane's running sum lives in LDS (2 KB): in two registers it took the diff-drive and steering forms from 127 to 131
        // and a workgroup per CU away; for the same reason every gather is summed at once -- this is the fallback family
        __shared__ double s_grid[kBlock];
        s_grid[threadIdx.x] = 0.0;
        grid_acc = GridAcc{grid_row(A), 0.0, MODEL == CCV_MPPI_FULL_BODY ? H - 2 : H, &s_grid[threadIdx.x]};
    }
    for (int t0 = 0; t0 < H; t0 += kTU) {
        double px[kTU], py[kTU];
        float zq[4] = {0.f, 0.f, 0.f, 0.f};
        static_for<kTU>([&](auto TT) {
            constexpr int tt = decltype(TT)::value;
            const int t = t0 + tt;
            px[tt] = x - A.x0[0];
            py[tt] = y - A.x0[1];
            if constexpr (GRID) {
                if (grid_acc.row && t < grid_acc.nstates) *grid_acc.slot += grid_value(grid_tap(grid_acc.row, x, y));
            }
            if (t < H) {
                if (A.store_xy && live) {
                    A.xs[(size_t)t * pitch + k] = x;
                    A.ys[(size_t)t * pitch + k] = y;
                }
                if (t < H - 1) {
                    double u[UD];
                    static_for<UD>([&](auto D) {
                        constexpr int d = decltype(D)::value;
                        constexpr int nloc = tt * UD + d;
                        const size_t row = (size_t)(t * UD + d);
                        if constexpr (SRC == SRC_PHILOX) {
                            if constexpr ((nloc & 3) == 0) {
                                const Philox4 r = philox4x32_10(kg, (uint32_t)((t0 * UD + nloc) >> 2), A.iter_lo,
                                                                A.iter_hi, A.seed_lo, A.seed_hi);
                                box_muller_f32(r.x, r.y, zq[0], zq[1]);
                                box_muller_f32(r.z, r.w, zq[2], zq[3]);
                            }
                            // libstdc++ normal_distribution: ret * stddev + mean (dd:96-97), then clamp (dd:98-99)
                            double v = (double)zq[nloc & 3] * A.sigma + A.nominal[row];
                            v = clampd(v, A.umin[d], A.umax[d]);
                            if constexpr (MODEL == CCV_MPPI_FULL_BODY && d == 2) {
                                if (A.steer_off) v = 0.0;  // fb:517
                            }
                            u[d] = v;
                            if (A.store_u && live) A.u[row * pitch + k] = v;
                        } else {
                            u[d] = A.u[row * pitch + kk];
                        }
                    });
                    // ---- cost terms that do not need the window ----
                    if (A.do_cost) {
                        if constexpr (MODEL != CCV_MPPI_FULL_BODY) {
                            cost += A.w_v * ((u[0] - A.v_ref) * (u[0] - A.v_ref));  // dd:204-206
                        } else {
                            if (t < H - 2) {  // fb:409
                                cost += A.w_v * (u[0] - A.v_ref) * (u[0] - A.v_ref);          // fb:413
                                if (u[0] < 0.0) cost += A.w_back * u[0] * u[0];               // fb:420
                            }
                            if (t >= 1) {  // finish index t-1 <= H-3: ZMP (fb:468-485, 597-603) and roll-rate terms
                                const double drive_accel = (u[0] - p_v) / dt;                  // fb:469
                                const double ay = drive_accel * p_sdir + p_ac * p_cdir;        // fb:473
                                const double hgdot_x = (A.fb_Ixx * u[3] - A.fb_Ixx * p_rv) / dt;  // fb:479-481
                                const double mo_x = (p_c2 * fb_mgz + p_c3 * (A.fb_mass * ay)) - hgdot_x;  // fb:600
                                const double zmp_y = mo_x / fb_den;                            // fb:601
                                cost += A.w_zmp * zmp_y * zmp_y;                               // fb:416
                                cost += A.w_rollv * (u[3] - p_rv) * (u[3] - p_rv);             // fb:418
                            }
                        }
                    }
                    // ---- dynamics: explicit Euler (dd:104-109, sd:120-125, fb:445-452) ----
                    double hd = yaw;
                    if constexpr (MODEL != CCV_MPPI_DIFF_DRIVE) hd = yaw + u[2];
                    double sn, cs;
                    sincos(hd, &sn, &cs);
                    if constexpr (MODEL == CCV_MPPI_FULL_BODY) {
                        if (A.do_cost) {
                            double sd_, cd_, sr_, cr_;
                            sincos(u[2], &sd_, &cd_);
                            sincos(roll, &sr_, &cr_);
                            p_sdir = sd_;
                            p_cdir = cd_;
                            p_c2 = -A.fb_L * sr_;                      // CoM.y (fb:482)
                            p_c3 = A.fb_L * cos(pitchang) * cr_;       // CoM.z
                            p_ac = u[0] * u[1];                        // fb:471
                            p_v = u[0];
                            p_rv = u[3];
                        }
                    }
                    x = x + u[0] * cs * dt;
                    y = y + u[0] * sn * dt;
                    yaw = yaw + u[1] * dt;
                    if constexpr (MODEL == CCV_MPPI_FULL_BODY) {
                        roll = roll + u[3] * dt;
                        pitchang = pitchang + u[4] * dt;
                    }
                } else {
                    if constexpr (MODEL != CCV_MPPI_FULL_BODY) {
                        // t == H-1: the reference reads control index H-1, one past the end (dd:199,204); defined
                        // semantics: that element is 0.0
                        if (A.do_cost) cost += A.w_v * ((0.0 - A.v_ref) * (0.0 - A.v_ref));
                    }
                }
            }
        });
        if (A.do_cost) {
            // states that reach the path cost: all H for dd/sd (dd:199), the first H-2 for fb (fb:409)
            const int nstates = (MODEL == CCV_MPPI_FULL_BODY) ? H - 2 : H;
            const int nv = min(kTU, nstates - t0);
            if (nv > 0) {
                double m[kTU];
#pragma unroll
                for (int i = 0; i < kTU; ++i) m[i] = INFINITY;
                switch (nv) {
                    case 8: window_min<8, LDSWIN>(px, py, m, H, W, s_ab, s_c); break;
                    case 7: window_min<7, LDSWIN>(px, py, m, H, W, s_ab, s_c); break;
                    case 6: window_min<6, LDSWIN>(px, py, m, H, W, s_ab, s_c); break;
                    case 5: window_min<5, LDSWIN>(px, py, m, H, W, s_ab, s_c); break;
                    case 4: window_min<4, LDSWIN>(px, py, m, H, W, s_ab, s_c); break;
                    case 3: window_min<3, LDSWIN>(px, py, m, H, W, s_ab, s_c); break;
                    case 2: window_min<2, LDSWIN>(px, py, m, H, W, s_ab, s_c); break;
                    default: window_min<1, LDSWIN>(px, py, m, H, W, s_ab, s_c); break;
                }
#pragma unroll
                for (int i = 0; i < kTU; ++i) {
                    if (i < nv) {
                        // d^2 = |p|^2 + min_j(...), gate d <= 100 (dd:185), cost += path_weight*d*d (dd:206)
                        double d2 = m[i] + fma(px[i], px[i], py[i] * py[i]);
                        d2 = d2 < 1.0e4 ? fmax(d2, 0.0) : 1.0e4;   // NaN -> gate value, as `distance < min_distance` (dd:189) is false for NaN
                        cost += A.w_path * d2;
                    }
                }
                if constexpr (MOVING) obst_term_moving<kTU, kTU, true>(A, *obst_mov, px, py, m, cost, t0, nv);
                else if constexpr (OBST) obst_term<kTU, kTU, true>(A, *obst_lds, px, py, m, cost, nv);
            }
        }
    }
    if constexpr (GRID) {
        if (grid_acc.row) {
            cost = fma(grid_acc.row->w, grid_total(grid_acc), cost);   // the last term (section 10h)
        }
    }
    if (A.do_cost && live) {
        A.cost[k] = cost;
        A.w[k] = pc_weight<false>(A, cost, live);
    }
}

// stand-alone sampling(): one thread per (sample, Philox call) -> 4 consecutive rows of u.
template <int MODEL>
__global__ __launch_bounds__(kBlock) void k_sample(const RolloutArgs A) {
    constexpr int UD = udim_of(MODEL);
    const int k = blockIdx.x * kBlock + threadIdx.x;
    const int call = blockIdx.y;
    if (k >= A.K) return;
    const int ntot = (A.H - 1) * UD;
    const Philox4 r = philox4x32_10((uint32_t)(A.k_offset + k), (uint32_t)call, A.iter_lo, A.iter_hi, A.seed_lo, A.seed_hi);
    float z[4];
    box_muller_f32(r.x, r.y, z[0], z[1]);
    box_muller_f32(r.z, r.w, z[2], z[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = call * 4 + i;
        if (n < ntot) {
            const int d = n % UD;
            double v = (double)z[i] * A.sigma + A.nominal[n];
            v = clampd(v, A.umin[d], A.umax[d]);
            if (MODEL == CCV_MPPI_FULL_BODY && d == 2 && A.steer_off) v = 0.0;
            A.u[(size_t)n * A.pitch + k] = v;
        }
    }
}

}  // namespace ccv
