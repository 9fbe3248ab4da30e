// How the waves of a workgroup and of a SIMD take turns: wave priorities and the LDS hand-offs (sequence numbers, the
// LDS-only barrier) of the cooperative rollout kernels.
#pragma once
#include "mppi_kernels.h"

namespace ccv {

// Wave arbitration on a SIMD is by priority, then age: with every workgroup at priority 0 the workgroup dispatched first
// to a CU runs almost unimpeded and the last one gets the left-over issue slots -- measured at K = 65 536, four
// workgroups per CU: 26 / 33 / 41 / 45 us for the same work, and the kernel ends with the slowest.  Alternating which
// half of a CU's workgroups is favoured, once per time block, evens them out (28 / 33 / 39 / 40 us; kernel -4 us).
// rank = position of the workgroup in its CU's dispatch order (workgroups go round-robin over the CUs).
__device__ __forceinline__ void pc_set_priority(const int p) {   // (s_setprio takes an immediate)
    switch (p) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
    }
}
// prio_rotate 1: two levels, alternating halves (two- and three-wave kernels); 2: four levels, level = (rank + s) mod 4 (the
// four-wave kernel, mppi_rollout_r4.h: its waves call this with s = time block + role)
__device__ __forceinline__ void pc_rotate_priority(const RolloutArgs& A, const int s) {
    if (!A.prio_rotate) return;
    const int rank = (int)blockIdx.x / A.cu_count;
    if (A.prio_rotate == 1) {
        if ((rank ^ s) & 1) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
    } else {
        pc_set_priority((rank + s) & 3);
    }
}

// four-wave kernel: the level from the workgroup's dispatch rank, the time block and the wave's role.
//   prio_rotate >= 16: (rank + level[role] + b) mod 4 with level[] = the four base-4 digits of prio_rotate - 16 (digit 0: noise
//   wave, 1: dynamics, 2: distance, 3: store) -- the default, with one table per model (ccv_mppi_capi.hip: r4_prio_levels);
//   2: level[role] = role, i.e. (rank + role + b); 5: (role - rank - b); 3, 4: the other two sign combinations (CCV_MPPI_PRIO).
// What matters, measured at C2 on one box (gpurun_out/r3bn, r3bj): no priorities 36.6 us; the prologue's rank priorities only
// 35.3; rank only, constant 34.5; (rank + role) 34.5; (rank + b) 32.4; (rank + role + b) 31.7; (rank + role - b) 32.9 -- the
// rotation with the time block is worth 3 us, its direction 1, the role term 0.7.  And WHICH role sits on which level another
// 0.7 us at C2 and 2 us at C3 (all 24 assignments, gpurun_out/r3br): diff drive noise 3 / dynamics 2 / distance 1 / store 0
// 31.9 us against 32.6 for 0 / 1 / 2 / 3, steering 2 / 3 / 1 / 0 39.7 against 41.7 (and 42.1 with diff drive's) -- the roles'
// blocks differ in length between the models, and the best interleaving with them.
__device__ __forceinline__ void r4_rotate_priority(const RolloutArgs& A, const int b, const int role) {
    if (!A.prio_rotate) return;
    const int rank = (int)blockIdx.x / A.cu_count;
    if (A.prio_rotate >= 16) {
        pc_set_priority((rank + (((A.prio_rotate - 16) >> (2 * role)) & 3) + b) & 3);
        return;
    }
    switch (A.prio_rotate) {
        case 2: pc_set_priority((rank + role + b) & 3); break;
        case 3: pc_set_priority((rank + role - b) & 3); break;
        case 4: pc_set_priority((role - rank + b) & 3); break;
        default: pc_set_priority((role - rank - b) & 3); break;
    }
}

// LDS sequence numbers for hand-offs without a barrier (mppi_rollout_r3.h, mppi_rollout_r4.h): written by one wave, polled by another.  The
// LDS operations of a wave execute in order, so a number written after the data (or after the loads have returned) needs
// no fence -- and must not get one: a release at workgroup scope would also wait for the wave's global stores.  Relaxed
// workgroup-scope atomics compile to plain ds_write_b32 / ds_read_b32; the empty asm statements keep the compiler from
// moving other memory accesses across them.
__device__ __forceinline__ void pc_publish(int* flag, const int value) {
    asm volatile("" ::: "memory");
    __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    asm volatile("" ::: "memory");
}
__device__ __forceinline__ void pc_wait_for(int* flag, const int value) {
    asm volatile("" ::: "memory");
    while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) < value)
        __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
}

// Workgroup barrier for the block hand-off.  The two waves exchange data through LDS only, so the barrier waits for LDS
// (lgkmcnt) and not, as __syncthreads() does, for the acknowledgement of every control / state store still in flight.
__device__ __forceinline__ void pc_barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace ccv
