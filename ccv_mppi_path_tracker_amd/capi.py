"""ctypes binding of libccv_mppi_hip.so -- exactly the symbols include/ccv_mppi.h and
include/ccv_mppi_host.h declare (SIGNATURES) and those of include/ccv_mppi_fleet.h (FLEET_SIGNATURES), include/ccv_mppi_sense.h (SENSE_SIGNATURES) include/ccv_mppi_plan.h (PLAN_SIGNATURES), include/ccv_mppi_follow.h (FOLLOW_SIGNATURES) and include/ccv_mppi_plan_cost.h (PLAN_COST_SIGNATURES).  No torch types cross this boundary; there is no CPU fallback:
if the library is missing it is built with hipcc, and if that fails the import raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

MAX_UDIM = 5
MAX_HORIZON = 128
ABI_VERSION = 1

OK = 0
ERR_INVALID_ARG = -1
ERR_NO_DEVICE = -2
ERR_HIP = -3
ERR_STATE = -4
ERR_ALLOC = -5
ERR_TIMEOUT = -6

DIFF_DRIVE, STEERING_DIFF_DRIVE, FULL_BODY = 0, 1, 2
FLAG_ROLL_OFF, FLAG_STEER_OFF, FLAG_MIN_SHIFT, FLAG_NO_STATE_STORE = 0x1, 0x2, 0x4, 0x8
BATCH_MAX_SAMPLES = 1 << 29
BATCH_KERNEL_PLAIN, BATCH_KERNEL_ONE_WAVE, BATCH_KERNEL_FOUR_WAVE, BATCH_KERNEL_WIDE = 0, 1, 4, 16
BATCH_KERNEL_VARIED = 32
BATCH_KERNEL_SHIFT = 64
BATCH_KERNEL_OBST = 128
BATCH_KERNEL_MOVING = 256
BATCH_KERNEL_GRID = 512
MAX_OBSTACLES = 32
INFLATE_MAX_RADIUS = 64
OCC_PATCH_MAX_CELLS = 1 << 20
OCC_PATCH_SLOTS = 4
SCAN_MAX_REACH = 4096
SCAN_RAY_BYTES, SCAN_ENTRY_BYTES = 9, 128   # of a staging slot (OCC_PATCH_MAX_CELLS bytes) per ray, and per entry that has rays
SENSE_MAX_BEAMS = 4096
SENSE_BEAM_BYTES, SENSE_ENTRY_BYTES = 8, 112   # of a staging slot per beam of ccv_mppi_batch_resident_sense_enqueue, and per entry
PLAN_MAX_FIELD, PLAN_MAX_POSES = 81920, 16384
PLAN_OK, PLAN_TRUNCATED, PLAN_NO_START, PLAN_START_BLOCKED, PLAN_GOAL_BLOCKED, PLAN_UNREACHABLE, PLAN_NOT_CONVERGED = 1, 2, 3, 4, 5, 6, 7
BEST_MAX = 1024
BATCH_TRACE_ROWS = 1024


class Config(C.Structure):
    """struct ccv_mppi_config"""
    _fields_ = [
        ("abi_version", C.c_int32), ("model", C.c_int32), ("num_samples", C.c_int32), ("horizon", C.c_int32),
        ("sample_offset", C.c_int32), ("device", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
        ("control_noise", C.c_double), ("lam", C.c_double), ("v_ref", C.c_double),
        ("u_min", C.c_double * MAX_UDIM), ("u_max", C.c_double * MAX_UDIM),
        ("path_weight", C.c_double), ("v_weight", C.c_double), ("zmp_weight", C.c_double),
        ("roll_v_weight", C.c_double), ("back_weight", C.c_double), ("yaw_weight", C.c_double),
    ]


class Stats(C.Structure):
    """struct ccv_mppi_stats"""
    _fields_ = [
        ("sum_w", C.c_double), ("min_cost", C.c_double), ("max_cost", C.c_double),
        ("n_zero_weight", C.c_int64), ("nonfinite", C.c_int32), ("reserved", C.c_int32),
        ("device_us", C.c_float), ("rollout_us", C.c_float),
    ]


class Grid(C.Structure):
    """struct ccv_mppi_grid"""
    _fields_ = [
        ("origin_x", C.c_double), ("origin_y", C.c_double), ("resolution", C.c_double),
        ("outside", C.c_float), ("nx", C.c_int32), ("ny", C.c_int32), ("cells", C.POINTER(C.c_float)),
    ]


class Occupancy(C.Structure):
    """struct ccv_mppi_occupancy"""
    _fields_ = [
        ("origin_x", C.c_double), ("origin_y", C.c_double), ("resolution", C.c_double),
        ("outside", C.c_float), ("nx", C.c_int32), ("ny", C.c_int32), ("threshold", C.c_int32), ("cells", C.POINTER(C.c_uint8)),
    ]


class Inflation(C.Structure):
    """struct ccv_mppi_inflation"""
    _fields_ = [("radius", C.c_int32), ("free_value", C.c_float), ("profile", C.POINTER(C.c_float))]


_dp = C.POINTER(C.c_double)
_H = C.c_void_p

# name -> (restype, argtypes): every symbol of the two public headers
SIGNATURES = {
    "ccv_mppi_create": (C.c_int, [C.POINTER(Config), C.POINTER(_H)]),
    "ccv_mppi_destroy": (C.c_int, [_H]),
    "ccv_mppi_set_stream": (C.c_int, [_H, C.c_void_p]),
    "ccv_mppi_last_error": (C.c_char_p, [_H]),
    "ccv_mppi_version": (C.c_char_p, []),
    "ccv_mppi_udim": (C.c_int, [C.c_int]),
    "ccv_mppi_set_nominal": (C.c_int, [_H, _dp]),
    "ccv_mppi_get_nominal": (C.c_int, [_H, _dp]),
    "ccv_mppi_iterate": (C.c_int, [_H, _dp, C.c_double, _dp, _dp, C.c_double, C.c_uint64, C.c_uint64, _dp,
                                   C.POINTER(Stats)]),
    "ccv_mppi_iterate_enqueue": (C.c_int, [_H, _dp, C.c_double, _dp, _dp, C.c_double, C.c_uint64, C.c_uint64]),
    "ccv_mppi_synchronize": (C.c_int, [_H]),
    "ccv_mppi_sample": (C.c_int, [_H, C.c_uint64, C.c_uint64]),
    "ccv_mppi_inject_controls": (C.c_int, [_H, _dp]),
    "ccv_mppi_rollout": (C.c_int, [_H, _dp, C.c_double]),
    "ccv_mppi_weights": (C.c_int, [_H, _dp, _dp, C.c_double]),
    "ccv_mppi_update": (C.c_int, [_H, _dp, C.POINTER(Stats)]),
    "ccv_mppi_read_candidates": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, _dp]),
    "ccv_mppi_read_top_candidates": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32), _dp, _dp]),
    "ccv_mppi_read_costs": (C.c_int, [_H, C.c_int32, C.c_int32, _dp]),
    "ccv_mppi_read_weights": (C.c_int, [_H, C.c_int32, C.c_int32, _dp]),
    "ccv_mppi_read_controls": (C.c_int, [_H, C.c_int32, C.c_int32, _dp]),
    "ccv_mppi_partials_size": (C.c_int, [_H]),
    "ccv_mppi_iterate_partials_enqueue": (C.c_int, [_H, _dp, C.c_double, _dp, _dp, C.c_double, C.c_uint64,
                                                    C.c_uint64, C.c_void_p]),
    "ccv_mppi_apply_partials_enqueue": (C.c_int, [_H, C.c_void_p]),
    "ccv_mppi_exchange_handle_bytes": (C.c_int, []),
    "ccv_mppi_exchange_create": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p]),
    "ccv_mppi_exchange_connect": (C.c_int, [_H, C.c_void_p]),
    "ccv_mppi_exchange_info": (C.c_int, [_H, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ccv_mppi_iterate_exchange_enqueue": (C.c_int, [_H, _dp, C.c_double, _dp, _dp, C.c_double, C.c_uint64, C.c_uint64]),
    "ccv_mppi_resident_set_path": (C.c_int, [_H, _dp, _dp, C.c_int32, C.c_double]),
    "ccv_mppi_resident_set_pose": (C.c_int, [_H, _dp]),
    "ccv_mppi_resident_step_enqueue": (C.c_int, [_H, C.c_double, C.c_uint64, C.c_uint64, C.c_int32]),
    "ccv_mppi_resident_step_partials_enqueue": (C.c_int, [_H, C.c_double, C.c_uint64, C.c_uint64, C.c_int32, C.c_void_p]),
    "ccv_mppi_resident_step_exchange_enqueue": (C.c_int, [_H, C.c_double, C.c_uint64, C.c_uint64, C.c_int32]),
    "ccv_mppi_resident_read": (C.c_int, [_H, _dp, C.POINTER(C.c_int32), _dp, _dp, _dp, C.POINTER(C.c_int64)]),
    "ccv_mppi_resident_read_trace": (C.c_int, [_H, C.c_int32, _dp, C.POINTER(C.c_int32)]),
    "ccv_mppi_timing_enable": (C.c_int, [_H, C.c_int32]),
    "ccv_mppi_timing_read": (C.c_int, [_H, _dp, _dp, C.POINTER(C.c_int64), C.c_int32]),
    "ccv_mppi_batch_create": (C.c_int, [C.POINTER(Config), C.c_int32, C.POINTER(_H)]),
    "ccv_mppi_batch_destroy": (C.c_int, [_H]),
    "ccv_mppi_batch_set_stream": (C.c_int, [_H, C.c_void_p]),
    "ccv_mppi_batch_synchronize": (C.c_int, [_H]),
    "ccv_mppi_batch_last_error": (C.c_char_p, [_H]),
    "ccv_mppi_batch_size": (C.c_int, [_H]),
    "ccv_mppi_batch_last_kernel": (C.c_int, [_H]),
    "ccv_mppi_batch_set_nominal": (C.c_int, [_H, _dp]),
    "ccv_mppi_batch_get_nominal": (C.c_int, [_H, _dp]),
    "ccv_mppi_batch_set_params": (C.c_int, [_H, C.POINTER(Config)]),
    "ccv_mppi_batch_get_params": (C.c_int, [_H, C.POINTER(Config)]),
    "ccv_mppi_batch_set_min_shift": (C.c_int, [_H, C.c_int32]),
    "ccv_mppi_batch_get_min_shift": (C.c_int, [_H]),
    "ccv_mppi_batch_set_obstacles": (C.c_int, [_H, _dp, C.POINTER(C.c_int32), C.c_int32, _dp]),
    "ccv_mppi_batch_get_obstacles": (C.c_int, [_H, _dp, C.POINTER(C.c_int32), C.c_int32, _dp]),
    "ccv_mppi_batch_set_obstacle_velocities": (C.c_int, [_H, _dp, C.c_int32]),
    "ccv_mppi_batch_get_obstacle_velocities": (C.c_int, [_H, _dp, C.c_int32]),
    "ccv_mppi_batch_set_fleet_prediction": (C.c_int, [_H, C.c_int32]),
    "ccv_mppi_batch_get_fleet_prediction": (C.c_int, [_H]),
    "ccv_mppi_batch_read_fleet_velocities": (C.c_int, [_H, _dp]),
    "ccv_mppi_batch_set_grids": (C.c_int, [_H, C.POINTER(Grid), C.c_int32, C.POINTER(C.c_int32), _dp]),
    "ccv_mppi_batch_get_grids": (C.c_int, [_H, C.POINTER(Grid), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp]),
    "ccv_mppi_batch_read_grid_cells": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_float)]),
    "ccv_mppi_batch_set_occupancy": (C.c_int, [_H, C.POINTER(Occupancy), C.POINTER(Inflation), C.c_int32, C.POINTER(C.c_int32), _dp]),
    "ccv_mppi_batch_update_occupancy_enqueue": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]),
    "ccv_mppi_batch_roll_occupancy_enqueue": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                        C.POINTER(C.c_uint8), C.c_int32]),
    "ccv_mppi_batch_scan_occupancy_enqueue": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                        C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_int32, C.c_int32]),
    "ccv_mppi_batch_get_occupancy": (C.c_int, [_H, C.POINTER(Occupancy), C.POINTER(Inflation), C.c_int32, C.POINTER(C.c_int32)]),
    "ccv_mppi_batch_read_occupancy": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_uint8)]),
    "ccv_mppi_batch_set_world": (C.c_int, [_H, C.POINTER(Occupancy), C.POINTER(C.c_int32), C.c_int32]),
    "ccv_mppi_batch_get_world": (C.c_int, [_H, C.POINTER(Occupancy), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]),
    "ccv_mppi_batch_read_world": (C.c_int, [_H, C.POINTER(C.c_uint8)]),
    "ccv_mppi_batch_update_world_enqueue": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]),
    "ccv_mppi_batch_iterate": (C.c_int, [_H, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_uint64), C.c_uint64, _dp,
                                         C.POINTER(Stats)]),
    "ccv_mppi_batch_iterate_enqueue": (C.c_int, [_H, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_uint64), C.c_uint64]),
    "ccv_mppi_batch_read_costs": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, _dp]),
    "ccv_mppi_batch_read_weights": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, _dp]),
    "ccv_mppi_batch_read_candidates": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp]),
    "ccv_mppi_batch_read_best_candidates": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32), _dp, _dp]),
    "ccv_mppi_batch_read_optimal_paths": (C.c_int, [_H, _dp]),
    "ccv_mppi_batch_timing_enable": (C.c_int, [_H, C.c_int32]),
    "ccv_mppi_batch_timing_read": (C.c_int, [_H, _dp, _dp, C.POINTER(C.c_int64), C.c_int32]),
    "ccv_mppi_batch_resident_set_paths": (C.c_int, [_H, _dp, _dp, C.POINTER(C.c_int32), _dp]),
    "ccv_mppi_batch_resident_set_poses": (C.c_int, [_H, _dp, C.POINTER(C.c_uint64)]),
    "ccv_mppi_batch_resident_step_enqueue": (C.c_int, [_H, C.c_double, C.c_uint64, C.c_int32]),
    "ccv_mppi_batch_resident_read": (C.c_int, [_H, _dp, C.POINTER(C.c_int32), _dp, _dp, _dp, C.POINTER(C.c_int64)]),
    "ccv_mppi_batch_resident_read_trace": (C.c_int, [_H, C.c_int32, C.c_int32, _dp, C.POINTER(C.c_int32)]),
    # include/ccv_mppi_host.h
    "ccv_mppi_calc_ref_path": (C.c_int, [_dp, _dp, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                         C.c_double, C.c_int32, _dp, _dp, _dp]),
    "ccv_mppi_path_cosine": (C.c_int, [_dp, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_double, _dp, _dp,
                                       C.c_int32]),
    "ccv_mppi_path_dkan": (C.c_int, [C.c_double, _dp, _dp, C.c_int32]),
    "ccv_mppi_plant_step": (C.c_int, [C.c_int32, _dp, _dp, C.c_double]),
    # include/ccv_mppi_node.hpp (extern "C" part): the ROS-free mirror of the reference controller classes
    "ccv_mppi_node_create": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), _dp, C.c_int, C.c_int, C.POINTER(_H)]),
    "ccv_mppi_node_destroy": (C.c_int, [_H]),
    "ccv_mppi_node_set_path": (C.c_int, [_H, _dp, _dp, C.c_int]),
    "ccv_mppi_node_set_state": (C.c_int, [_H, _dp]),
    "ccv_mppi_node_set_seed": (C.c_int, [_H, C.c_uint64]),
    "ccv_mppi_node_set_fused": (C.c_int, [_H, C.c_int]),
    "ccv_mppi_node_set_device_prologue": (C.c_int, [_H, C.c_int]),
    "ccv_mppi_node_run_once": (C.c_int, [_H, C.c_double, _dp]),
    "ccv_mppi_node_get_optimal": (C.c_int, [_H, _dp]),
    "ccv_mppi_node_get_ref_path": (C.c_int, [_H, _dp]),
    "ccv_mppi_node_get_optimal_path": (C.c_int, [_H, _dp]),
    "ccv_mppi_node_fb_imu": (C.c_int, [_H, _dp, _dp, _dp, _dp]),
    "ccv_mppi_node_fb_wrench": (C.c_int, [_H, C.c_int, _dp, _dp]),
    "ccv_mppi_node_fb_pose": (C.c_int, [_H, C.c_double, C.c_double, C.c_double]),
    "ccv_mppi_node_fb_update_state": (C.c_int, [_H, C.c_double]),
    "ccv_mppi_node_fb_read": (C.c_int, [_H, _dp]),
    "ccv_mppi_fb_estimator_create": (C.c_int, [C.POINTER(_H)]),
    "ccv_mppi_fb_estimator_destroy": (C.c_int, [_H]),
    "ccv_mppi_fb_estimator_imu": (C.c_int, [_H, _dp, _dp, _dp, _dp]),
    "ccv_mppi_fb_estimator_wrench": (C.c_int, [_H, C.c_int, _dp, _dp]),
    "ccv_mppi_fb_estimator_update": (C.c_int, [_H, C.c_double, C.c_double, C.c_double, C.c_double]),
    "ccv_mppi_fb_estimator_read": (C.c_int, [_H, _dp]),
}
# include/ccv_mppi_fleet.h: the fleet term of the resident loop, a table of its own like its header
FLEET_SIGNATURES = {
    "ccv_mppi_batch_resident_set_fleet": (C.c_int, [_H, _dp, C.c_double, C.c_int32, _dp]),
    "ccv_mppi_batch_resident_get_fleet": (C.c_int, [_H, _dp, C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "ccv_mppi_batch_resident_read_fleet": (C.c_int, [_H, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp]),
}

# include/ccv_mppi_sense.h: the simulated range sensor of the resident loop, a table of its own like its header
SENSE_SIGNATURES = {
    "ccv_mppi_batch_resident_sense_enqueue": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32]),
    "ccv_mppi_batch_resident_read_sense": (C.c_int, [_H, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
}

# include/ccv_mppi_plan.h: paths planned on the device for the resident loop, a table of its own like its header
_i32p = C.POINTER(C.c_int32)
PLAN_SIGNATURES = {
    "ccv_mppi_batch_resident_set_plan": (C.c_int, [_H, _i32p, C.c_int32]),
    "ccv_mppi_batch_resident_get_plan": (C.c_int, [_H, _i32p, _i32p]),
    "ccv_mppi_batch_resident_plan_enqueue": (C.c_int, [_H, C.c_int32, _i32p, _i32p, C.c_float, C.c_int32]),
    "ccv_mppi_batch_resident_read_plan": (C.c_int, [_H, _i32p, _i32p, _i32p, _i32p, _i32p]),
    "ccv_mppi_batch_resident_read_plan_field": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_uint16)]),
    "ccv_mppi_batch_resident_read_path": (C.c_int, [_H, C.c_int32, C.c_int32, _dp, _dp, _i32p]),
}

# include/ccv_mppi_follow.h: costmaps that follow their robots in the resident loop, a table of its own like its header
FOLLOW_SIGNATURES = {
    "ccv_mppi_batch_resident_set_follow": (C.c_int, [_H, C.c_int32]),
    "ccv_mppi_batch_resident_get_follow": (C.c_int, [_H, _i32p]),
    "ccv_mppi_batch_resident_follow_enqueue": (C.c_int, [_H, C.c_int32, _i32p, C.c_int32, C.c_int32, C.c_int32]),
    "ccv_mppi_batch_resident_read_follow": (C.c_int, [_H, _i32p, _i32p, C.POINTER(C.c_int64), _dp]),
    "ccv_mppi_batch_resident_plan_goals_enqueue": (C.c_int, [_H, C.c_int32, _i32p, _dp, C.c_float, C.c_int32]),
}
FOLLOW_MOVED, FOLLOW_HELD, FOLLOW_NO_POSE, FOLLOW_LIMIT = 1, 2, 3, 4

# include/ccv_mppi_plan_cost.h: traversal weights of the paths planned on the device, a table of its own like its header
PLAN_COST_SIGNATURES = {
    "ccv_mppi_batch_resident_set_plan_penalty": (C.c_int, [_H, C.c_float, C.c_int32]),
    "ccv_mppi_batch_resident_get_plan_penalty": (C.c_int, [_H, C.POINTER(C.c_float), _i32p]),
}
PLAN_MAX_PENALTY = 15

_lib = None


def load():
    """dlopen the in-tree library (building it first if it is missing or stale)."""
    global _lib
    if _lib is None:
        path = os.environ.get("CCV_MPPI_LIB") or _build.build()   # CCV_MPPI_LIB: experiment builds only
        if not os.path.exists(path):
            raise ImportError("libccv_mppi_hip.so is missing and could not be built; there is no CPU fallback")
        lib = C.CDLL(path)
        for name, (res, args) in list(SIGNATURES.items()) + list(FLEET_SIGNATURES.items()) + list(SENSE_SIGNATURES.items()) + list(PLAN_SIGNATURES.items()) + list(FOLLOW_SIGNATURES.items()) + list(PLAN_COST_SIGNATURES.items()):
            fn = getattr(lib, name)  # AttributeError = the .so does not export what the header declares
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def dptr(a):
    return a.ctypes.data_as(_dp)


def as_f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError("expected shape %s, got %s" % (shape, a.shape))
    return a
