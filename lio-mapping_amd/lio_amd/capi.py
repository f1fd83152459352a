"""ctypes view of include/lio_c.h.

`load_hip()` opens the product (liblio_hip.so next to csrc/) and raises if it is missing: there is no
CPU fallback.  Tests additionally open the oracle with `LioLib(path_to_liblio_oracle)`; product code
never does.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.environ.get("LIO_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "csrc", "liblio_hip.so")   # LIO_HIP_LIB: A/B builds of the product

c_double_p = C.POINTER(C.c_double)
c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)
c_uint16_p = C.POINTER(C.c_uint16)


class TransformF(C.Structure):
    _fields_ = [("q", C.c_float * 4), ("p", C.c_float * 3)]

    @staticmethod
    def make(q_xyzw, p):
        t = TransformF()
        for i in range(4):
            t.q[i] = float(q_xyzw[i])
        for i in range(3):
            t.p[i] = float(p[i])
        return t

    def to_np(self):
        return np.array(list(self.q), dtype=np.float32), np.array(list(self.p), dtype=np.float32)


class PPConfig(C.Structure):
    _fields_ = [
        ("scan_period", C.c_double),
        ("num_scan_subregions", C.c_int),
        ("num_curvature_regions", C.c_int),
        ("surf_curv_th", C.c_float),
        ("max_corner_sharp", C.c_int),
        ("max_corner_less_sharp", C.c_int),
        ("max_surf_flat", C.c_int),
        ("less_flat_filter_size", C.c_float),
        ("infer_start_ori", C.c_int),
        ("rad_diff", C.c_double),
    ]


class MapConfig(C.Structure):
    _fields_ = [
        ("corner_filter_size", C.c_float),
        ("surf_filter_size", C.c_float),
        ("min_match_sq_dis", C.c_float),
        ("min_plane_dis", C.c_float),
        ("num_max_iterations", C.c_int),
        ("map_builder", C.c_int),
        ("enable_4d", C.c_int),
        ("skip_count", C.c_int),
    ]


class EstConfig(C.Structure):
    _fields_ = [
        ("window_size", C.c_int),
        ("opt_window_size", C.c_int),
        ("corner_filter_size", C.c_float),
        ("surf_filter_size", C.c_float),
        ("min_match_sq_dis", C.c_float),
        ("min_plane_dis", C.c_float),
        ("transform_lb", TransformF),
        ("opt_extrinsic", C.c_int),
        ("imu_factor", C.c_int),
        ("point_distance_factor", C.c_int),
        ("prior_factor", C.c_int),
        ("marginalization_factor", C.c_int),
        ("enable_deskew", C.c_int),
        ("cutoff_deskew", C.c_int),
        ("keep_features", C.c_int),
        ("acc_n", C.c_double),
        ("gyr_n", C.c_double),
        ("acc_w", C.c_double),
        ("gyr_w", C.c_double),
        ("g_norm", C.c_double),
        ("max_num_iterations", C.c_int),
        ("max_solver_time", C.c_double),
        ("extrinsic_stage", C.c_int),
        ("init_window_factor", C.c_int),
        ("device_solve", C.c_int),
        ("inline_marg", C.c_int),
        ("stream_sync", C.c_int),
        ("resident_moments", C.c_int),
    ]


class SolveReport(C.Structure):
    _fields_ = [
        ("iterations", C.c_int),
        ("successful_steps", C.c_int),
        ("termination", C.c_int),
        ("n_lidar_residuals", C.c_int),
        ("n_local_map", C.c_int),
        ("laser_odom_iterations", C.c_int),
        ("turn_off", C.c_int),
        ("convergence_flag", C.c_int),
        ("marginalized", C.c_int),
        ("cost_pim_before", C.c_double),
        ("cost_ppp_before", C.c_double),
        ("cost_marg_before", C.c_double),
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("cost_trace", C.c_double * 32),
        ("ms_build_map", C.c_double),
        ("ms_features", C.c_double),
        ("ms_prepare", C.c_double),
        ("ms_opt", C.c_double),
        ("ms_marg", C.c_double),
        ("ms_total", C.c_double),
        ("laser_odom_kz", C.c_int),
    ]

    def as_dict(self):
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = list(v) if name == "cost_trace" else v
        return d


# every symbol include/lio_c.h declares (checked by tests/test_abi.py against the header text)
_SIGS = {
    "lio_backend": (C.c_char_p, []),
    "lio_pp_default_config": (None, [C.POINTER(PPConfig)]),
    "lio_pp_create": (C.c_void_p, [C.c_float, C.c_float, C.c_int, C.POINTER(PPConfig)]),
    "lio_pp_destroy": (None, [C.c_void_p]),
    "lio_pp_process": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t]),
    "lio_pp_process_rings": (C.c_int, [C.c_void_p, c_float_p, c_uint16_p, C.c_size_t]),
    "lio_bench_voxel_grid": (C.c_int, [c_float_p, C.c_size_t, C.c_float, C.c_int, c_double_p, C.POINTER(C.c_size_t)]),
    "lio_pp_process_async": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t]),
    "lio_pp_process_batch": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(c_float_p), C.POINTER(C.c_size_t), C.c_int]),
    "lio_pp_process_batch_device": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int]),
    "lio_pp_process_rings_batch": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(c_float_p), C.POINTER(c_uint16_p), C.POINTER(C.c_size_t), C.c_int]),
    "lio_pp_wait": (C.c_int, [C.c_void_p]),
    "lio_pp_start_ori": (C.c_float, [C.c_void_p]),
    "lio_pp_count": (C.c_size_t, [C.c_void_p, C.c_int]),
    "lio_pp_get_cloud": (C.c_int, [C.c_void_p, C.c_int, c_float_p]),
    "lio_pp_get_indices": (C.c_int, [C.c_void_p, C.c_int, c_int32_p, c_int32_p]),
    "lio_pp_get_ring_offsets": (C.c_int, [C.c_void_p, c_int32_p]),
    "lio_pp_get_curvature": (C.c_int, [C.c_void_p, c_float_p, c_int32_p]),
    "lio_odom_create": (C.c_void_p, [C.c_float, C.c_int, C.c_int, C.c_int]),
    "lio_odom_destroy": (None, [C.c_void_p]),
    "lio_odom_process": (C.c_int, [C.c_void_p] + [c_float_p, C.c_size_t] * 4 + [C.POINTER(TransformF), C.POINTER(TransformF), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lio_odom_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "lio_odom_get_last_cloud": (C.c_size_t, [C.c_void_p, C.c_int, c_float_p]),
    "lio_odom_get_iteration_trace": (C.c_int, [C.c_void_p, C.POINTER(TransformF), C.c_int, C.POINTER(C.c_int)]),
    "lio_map_get_degeneracy": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "lio_kf_batch_get_degeneracy": (C.c_int, [C.c_void_p, c_int32_p]),
    "lio_imu_estimate_extrinsic_rotation": (C.c_int, [C.c_size_t, C.POINTER(TransformF), C.POINTER(C.c_void_p), C.POINTER(TransformF)]),
    "lio_imu_initialization": (C.c_int, [C.c_size_t, C.POINTER(TransformF), C.POINTER(C.c_void_p), C.POINTER(TransformF), c_double_p, c_double_p, c_double_p, c_double_p]),
    "lio_map_default_config": (None, [C.POINTER(MapConfig)]),
    "lio_map_create": (C.c_void_p, [C.POINTER(MapConfig)]),
    "lio_map_destroy": (None, [C.c_void_p]),
    "lio_map_process": (C.c_int, [C.c_void_p] + [c_float_p, C.c_size_t] * 2 + [C.POINTER(TransformF), C.POINTER(TransformF), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lio_map_set_init_flag": (C.c_int, [C.c_void_p, C.c_int]),
    "lio_map_set_transform_tobe_mapped": (C.c_int, [C.c_void_p, C.POINTER(TransformF)]),
    "lio_map_get_transform_tobe_mapped": (C.c_int, [C.c_void_p, C.POINTER(TransformF)]),
    "lio_map_update_map_database": (C.c_int, [C.c_void_p] + [c_float_p, C.c_size_t] * 2 + [C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(TransformF), C.POINTER(C.c_int)]),
    "lio_map_get_cloud": (C.c_size_t, [C.c_void_p, C.c_int, c_float_p]),
    "lio_map_get_cube": (C.c_size_t, [C.c_void_p, C.c_int, C.c_uint32, c_float_p]),
    "lio_map_get_cube_state": (C.c_size_t, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "lio_map_get_score_point_coeff": (C.c_size_t, [C.c_void_p, c_float_p, c_float_p, c_float_p]),
    "lio_kf_batch_create": (C.c_void_p, [C.POINTER(MapConfig)]),
    "lio_kf_batch_destroy": (None, [C.c_void_p]),
    "lio_kf_batch_add_map": (C.c_int, [C.c_void_p] + [c_float_p, C.c_size_t] * 2),
    "lio_kf_batch_add_keyframe": (C.c_int, [C.c_void_p, C.c_int] + [c_float_p, C.c_size_t] * 2 + [C.POINTER(TransformF)]),
    "lio_kf_batch_clear_keyframes": (C.c_int, [C.c_void_p]),
    "lio_kf_batch_refine": (C.c_int, [C.c_void_p, C.POINTER(TransformF), c_int32_p, c_int32_p, c_double_p]),
    "lio_kf_batch_size": (C.c_size_t, [C.c_void_p]),
    "lio_compact_encode": (C.c_size_t, [C.POINTER(TransformF)] + [c_float_p, C.c_size_t] * 3 + [c_float_p]),
    "lio_compact_decode": (C.c_int, [c_float_p, C.c_size_t, C.POINTER(TransformF)] + [C.POINTER(C.c_size_t)] * 3),
    "lio_voxel_grid": (C.c_int, [c_float_p, C.c_size_t, C.c_float, c_float_p, C.POINTER(C.c_size_t)]),
    "lio_knn": (C.c_int, [c_float_p, C.c_size_t, c_float_p, C.c_size_t, C.c_int, C.c_float, c_int32_p, c_float_p]),
    "lio_calculate_features": (
        C.c_int,
        [c_float_p, C.c_size_t, c_float_p, C.c_size_t, C.POINTER(TransformF), C.c_float, C.c_float, c_uint8_p, c_float_p, c_float_p],
    ),
    "lio_pim_create": (C.c_void_p, [c_double_p] * 4 + [C.c_double] * 5),
    "lio_pim_destroy": (None, [C.c_void_p]),
    "lio_pim_push_back": (C.c_int, [C.c_void_p, C.c_double, c_double_p, c_double_p]),
    "lio_pim_repropagate": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "lio_pim_get": (C.c_int, [C.c_void_p] + [c_double_p] * 6),
    "lio_pim_evaluate": (C.c_int, [C.c_void_p] + [c_double_p] * 5),
    "lio_factor_imu": (C.c_int, [C.c_void_p] + [c_double_p] * 9),
    "lio_factor_pivot_point_plane": (C.c_int, [c_double_p] * 9),
    "lio_factor_prior": (C.c_int, [c_double_p] * 5),
    "lio_pose_plus": (C.c_int, [c_double_p] * 3),
    "lio_est_default_config": (None, [C.POINTER(EstConfig)]),
    "lio_est_create": (C.c_void_p, [C.POINTER(EstConfig)]),
    "lio_est_destroy": (None, [C.c_void_p]),
    "lio_est_process_imu": (C.c_int, [C.c_void_p, C.c_double, c_double_p, c_double_p, C.c_double]),
    "lio_est_process_imu_batch": (C.c_int, [C.c_void_p, C.c_size_t, c_double_p, c_double_p, c_double_p, c_double_p]),
    "lio_est_process_laser_odom": (
        C.c_int,
        [C.c_void_p, C.POINTER(TransformF), c_float_p, C.c_size_t, c_float_p, C.c_size_t, C.c_double, C.POINTER(SolveReport)],
    ),
    "lio_est_process_compact": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, C.c_double, C.POINTER(TransformF), C.POINTER(SolveReport)]),
    "lio_est_get_stage": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int)] * 4 + [c_double_p, c_double_p]),
    "lio_est_push_frame": (C.c_int, [C.c_void_p, C.POINTER(TransformF), c_float_p, C.c_size_t, c_float_p, C.c_size_t, C.c_double]),
    "lio_est_solve_optimization": (C.c_int, [C.c_void_p, C.POINTER(SolveReport)]),
    "lio_est_slide_window": (C.c_int, [C.c_void_p]),
    "lio_est_sync": (C.c_int, [C.c_void_p]),
    "lio_est_set_window": (C.c_int, [C.c_void_p, C.c_int] + [c_double_p] * 6),
    "lio_est_get_window": (C.c_int, [C.c_void_p, C.c_int] + [c_double_p] * 5 + [C.POINTER(TransformF)]),
    "lio_est_set_surf_stack": (C.c_int, [C.c_void_p, C.c_int, c_float_p, C.c_size_t]),
    "lio_est_get_surf_stack": (C.c_size_t, [C.c_void_p, C.c_int, c_float_p]),
    "lio_est_set_preintegration": (C.c_int, [C.c_void_p, C.c_int] + [c_double_p] * 7 + [C.c_size_t]),
    "lio_est_begin_frame": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "lio_est_build_local_map": (C.c_int, [C.c_void_p]),
    "lio_est_get_local_map": (C.c_size_t, [C.c_void_p, c_float_p]),
    "lio_est_get_features": (C.c_size_t, [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p]),
    "lio_est_get_laser_odom_transform": (C.c_int, [C.c_void_p, C.POINTER(TransformF)]),
    "lio_est_get_prior": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p, C.POINTER(C.c_int)]),
    "lio_est_get_prior_factor": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p, C.POINTER(C.c_int)]),
    "lio_est_set_prior_factor": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, C.c_int]),
    "lio_est_set_extrinsic": (C.c_int, [C.c_void_p, C.POINTER(TransformF)]),
    "lio_dense_spd_solve": (C.c_int, [c_double_p, c_double_p, C.c_int, c_double_p]),
    "lio_marginalize_schur": (C.c_int, [c_double_p, c_double_p, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p]),
    "lio_est_snapshot": (C.c_int, [C.c_void_p]),
    "lio_est_restore": (C.c_int, [C.c_void_p]),
    "lio_est_solve_restored": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(SolveReport)]),
    "lio_pp_get_ring_intensity": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "lio_pp_check_config": (C.c_int, [C.c_float, C.c_float, C.c_int, C.POINTER(PPConfig)]),
    "lio_est_copy_snapshot": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lio_est_batch_create": (C.c_void_p, [C.POINTER(C.c_void_p), C.c_int]),
    "lio_est_batch_destroy": (None, [C.c_void_p]),
    "lio_est_batch_size": (C.c_int, [C.c_void_p]),
    "lio_est_batch_solve": (C.c_int, [C.c_void_p, C.POINTER(SolveReport)]),
    "lio_est_batch_solve_restored": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(SolveReport)]),
    "lio_est_batch_sync": (C.c_int, [C.c_void_p]),
    "lio_est_batch_get_clock": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "lio_est_batch_stage_digest": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong)]),
    "lio_est_batch_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "lio_seg_sort_pairs": (C.c_int, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int,
                           C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "lio_est_set_factor_sharding": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "lio_rccl_unique_id": (C.c_int, [C.c_char_p]),
    "lio_rccl_init": (C.c_void_p, [C.c_char_p, C.c_int, C.c_int]),
    "lio_rccl_destroy": (None, [C.c_void_p]),
    "lio_rccl_rank": (C.c_int, [C.c_void_p]),
    "lio_rccl_world": (C.c_int, [C.c_void_p]),
    "lio_est_set_factor_sharding_rccl": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lio_kf_batch_refine_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_float_p, c_double_p]),
    "lio_rccl_bench_all_reduce": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p]),
    "lio_est_bench_batched_moments": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p]),
    "lio_est_enable_kernel_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "lio_est_get_kernel_timing": (C.c_int, [C.c_void_p, C.c_char_p, c_double_p, c_double_p]),
}
# include/lio_test_hooks.h: test hooks kept apart from the ABI of lio_c.h
_TEST_SIGS = {
    "lio_est_eval_lidar_moments": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p, C.POINTER(C.c_int)]),
    "lio_est_force_moments_per_lane": (C.c_int, [C.c_void_p, C.c_int]),
    "lio_est_batch_get_moments": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p]),
    "lio_est_set_max_num_iterations": (C.c_int, [C.c_void_p, C.c_int]),
    "lio_est_batch_get_linearization": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), c_double_p, c_double_p, c_double_p]),
    "lio_knn_walk": (C.c_int, [c_float_p, C.c_size_t, c_float_p, C.c_size_t, C.c_float, C.c_int, c_int32_p, c_float_p, c_float_p]),
    "lio_fit_five": (C.c_int, [C.c_int, c_float_p, c_float_p, c_float_p, C.c_size_t, C.POINTER(TransformF), c_float_p, C.c_float, C.c_float,
                               c_uint8_p, c_float_p, c_float_p, c_float_p]),
    "lio_odom_correspondences": (C.c_int, [c_float_p, C.c_size_t, c_float_p, C.c_size_t, c_float_p, C.c_size_t, c_float_p, C.c_size_t,
                                           C.POINTER(TransformF), C.c_float, C.c_int, c_int32_p, c_int32_p, c_float_p]),
    "lio_gn_rows_map": (C.c_int, [C.c_int, c_float_p, C.c_size_t, c_uint8_p, c_float_p, C.POINTER(TransformF), c_uint8_p, c_float_p, c_int32_p,
                                  c_double_p]),
    "lio_gn_rows_odom": (C.c_int, [c_float_p, C.c_size_t, c_float_p, C.c_size_t, c_float_p, C.c_size_t, c_float_p, C.c_size_t, c_int32_p, c_int32_p,
                                   C.POINTER(TransformF), C.c_float, C.c_int, C.c_int, c_uint8_p, c_float_p, c_int32_p, c_double_p]),
    "lio_gn_fold": (C.c_int, [c_double_p, C.c_int, C.c_int, c_double_p]),
    "lio_gn_step": (C.c_int, [C.c_int, c_double_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "lio_gn_round": (C.c_int, [c_float_p, C.c_size_t, c_float_p, C.c_size_t, C.POINTER(TransformF), C.c_float, C.c_float, C.c_int, c_int32_p,
                               c_double_p, C.c_void_p]),
}
# lio_gn_state of include/lio_test_hooks.h as a numpy record: 13 words
GN_STATE = np.dtype([("T", np.float32, 8), ("converged", np.int32), ("iters", np.int32), ("degenerate", np.int32), ("kz", np.int32),
                     ("nsel", np.int32)])
# include/lio_ext.h: the product's entry points beyond the shared ABI (the map refresh and the surround map).  Attached to the HIP
# library only: the oracle does not implement them, and loading it must keep working
_EXT_SIGS = {
    "lio_est_map": (C.c_void_p, [C.c_void_p]),
    "lio_est_set_map_refresh": (C.c_int, [C.c_void_p, C.c_int]),
    "lio_est_refresh_map": (C.c_int, [C.c_void_p]),
    "lio_map_get_surround": (C.c_size_t, [C.c_void_p, C.c_float, c_float_p]),
    "lio_est_get_last_map_refresh": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(TransformF), C.POINTER(C.c_int), C.POINTER(C.c_uint32),
                                               C.POINTER(C.c_int), C.POINTER(C.c_size_t), c_float_p, C.POINTER(C.c_size_t), c_float_p]),
}
# include/lio_est_wide.h: seven optimised frames on the device loop (the product only, attached like _EXT_SIGS)
_EST_WIDE_SIGS = {
    "lio_est_set_device_solve_limit": (C.c_int, [C.c_void_p, C.c_int]),
    "lio_est_get_device_solve_limit": (C.c_int, [C.c_void_p]),
}
# include/lio_full_cloud.h: the full-resolution sweep on the device (the product only, attached like _EXT_SIGS)
_FULL_SIGS = {
    "lio_odom_full_to_end": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, c_float_p]),
    "lio_map_set_full_cloud": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t]),
    "lio_map_get_full_cloud": (C.c_size_t, [C.c_void_p, c_float_p]),
    "lio_est_set_full_cloud": (C.c_int, [C.c_void_p, C.c_int]),
    "lio_est_get_full_stack": (C.c_size_t, [C.c_void_p, C.c_int, c_float_p, C.POINTER(C.c_int)]),
    "lio_est_get_registered_full": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(TransformF), C.POINTER(C.c_size_t), c_float_p]),
    "lio_est_get_full_transform_es": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(TransformF)]),
    "lio_deskew_to_end": (C.c_int, [c_float_p, C.c_size_t, C.POINTER(TransformF), C.c_float, C.c_int, c_float_p]),
}
FULL_MAP_FRAME, FULL_SENSOR_RAW, FULL_SENSOR_END = 1, 2, 3   # LIO_FULL_* of include/lio_full_cloud.h
# include/lio_odom_batch.h: the scan-to-scan odometry of many sensors through one launch chain (the product only, attached like _EXT_SIGS)
_c_float_pp, _c_size_p = C.POINTER(c_float_p), C.POINTER(C.c_size_t)
_ODOM_BATCH_SIGS = {
    "lio_odom_process_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, _c_float_pp, _c_size_p, _c_float_pp, _c_size_p, _c_float_pp, _c_size_p,
                                         _c_float_pp, _c_size_p, C.POINTER(TransformF), C.POINTER(TransformF), c_int32_p, c_int32_p]),
}
ODOM_BATCH_MAX_SENSORS = 1024   # LIO_ODOM_BATCH_MAX_SENSORS
# include/lio_frontend_batch.h: the batched odometry fed from the feature extraction on the device (the product only, attached like _EXT_SIGS)
_FRONTEND_SIGS = {
    "lio_odom_process_batch_from_pp": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.POINTER(TransformF), C.POINTER(TransformF),
                                                 c_int32_p, c_int32_p]),
}
# include/lio_map_batch.h: the scan-to-map step of many sensors through one launch chain (the product only, attached like _EXT_SIGS)
_MAP_BATCH_SIGS = {
    "lio_map_process_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, _c_float_pp, _c_size_p, _c_float_pp, _c_size_p, C.POINTER(TransformF),
                                        C.POINTER(TransformF), c_int32_p, c_int32_p]),
}
MAP_BATCH_MAX_SENSORS = 1024   # LIO_MAP_BATCH_MAX_SENSORS
# include/lio_map_from_odom.h: the batched scan-to-map step fed from the odometry on the device (the product only, attached like _MAP_BATCH_SIGS)
_MAP_FROM_ODOM_SIGS = {
    "lio_map_process_batch_from_odom": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.POINTER(TransformF),
                                                  c_int32_p, c_int32_p]),
}
# include/lio_est_push_batch.h: PushFrame / SlideWindow / ProcessLaserOdom of the windows of a batch through one launch chain (the product
# only; attached where the library has them, so that a build from before them still loads as an A/B tool's --parent-lib)
class EstFrame(C.Structure):
    _fields_ = [("transform_in", TransformF), ("surf_xyzi", c_float_p), ("n_surf", C.c_size_t), ("corner_xyzi", c_float_p), ("n_corner", C.c_size_t),
                ("stamp", C.c_double)]


_EST_PUSH_SIGS = {
    "lio_est_batch_push_frames": (C.c_int, [C.c_void_p, C.POINTER(EstFrame)]),
    "lio_est_batch_slide_windows": (C.c_int, [C.c_void_p]),
    "lio_est_batch_process_laser_odom": (C.c_int, [C.c_void_p, C.POINTER(EstFrame), C.POINTER(SolveReport)]),
    "lio_est_batch_push_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
}
PUSH_STATS = ("chain", "redone", "as_is", "host_waits", "sort_passes")   # lio_est_batch_push_stats [0 .. 4]
# include/lio_est_from_odom.h: the windows of a batch fed from the odometry handles on the device (the product only, attached like _EST_PUSH_SIGS)
_EST_FROM_ODOM_SIGS = {
    "lio_est_batch_push_frames_from_odom": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(TransformF), c_double_p]),
    "lio_est_batch_process_compact_from_odom": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_double_p, C.POINTER(TransformF),
                                                          C.POINTER(SolveReport)]),
    "lio_est_batch_from_odom_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
}
FROM_ODOM_STATS = ("device_sources", "as_is_copies", "full_clouds", "uploads")   # lio_est_batch_from_odom_stats [0 .. 3]
# include/lio_vox_sort.h: the voxel filter's sort on caller-given keys and the counters of the paths it took (the product only, attached like _EXT_SIGS)
_c_uint32_p = C.POINTER(C.c_uint32)
_VOX_SORT_SIGS = {
    "lio_vox_sort_pairs": (C.c_int, [_c_uint32_p, C.c_size_t, _c_uint32_p, _c_uint32_p, C.POINTER(C.c_int)]),
    "lio_vox_sort_stats": (C.c_int, [C.POINTER(C.c_uint64)]),
}
VOX_SORT_SAMPLE, VOX_SORT_SINGLE, VOX_SORT_LIBRARY = 0, 1, 2   # LIO_VOX_SORT_* paths
VOX_SORT_SINGLE_MAX, VOX_SORT_BUCKET_CAP, VOX_SORT_MEAN_BUCKET, VOX_SORT_OVERSAMPLE = 4096, 4096, 384, 8   # the sizing rule of the header


# include/lio_seg_bounds.h: the bounds pass the sensor chains share, on caller-given clouds (the product only, attached like _VOX_SORT_SIGS)
class SegBoundsOut(C.Structure):
    _fields_ = [("mn", C.c_float * 3), ("mx", C.c_float * 3), ("minb", C.c_int32 * 3), ("divb", C.c_int32 * 3), ("overflow", C.c_int32),
                ("n_valid", C.c_int32)]


_SEG_BOUNDS_SIGS = {
    "lio_seg_bounds": (C.c_int, [_c_float_pp, _c_size_p, C.c_int, C.c_float, C.POINTER(SegBoundsOut)]),
}


def _dp(a):
    return None if a is None else a.ctypes.data_as(c_double_p)


def _fp(a):
    return None if a is None else a.ctypes.data_as(c_float_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class LioError(RuntimeError):
    pass


def _chk(rc, what):
    if rc != 0:
        raise LioError(f"{what} failed with code {rc}")


class LioLib:
    def __init__(self, path):
        if not os.path.exists(path):
            raise LioError(f"{path} is missing — build it first (python -c 'import __graft_entry__ as g; g.build()')")
        self.path = path
        self.dll = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(self.dll, name)
            fn.restype = res
            fn.argtypes = args
        # the test hooks (include/lio_test_hooks.h): a library built before a hook existed still loads, and only a call to the
        # missing hook fails (AttributeError); tests/test_abi.py holds both libraries to the whole header
        self.missing = []
        for name, (res, args) in _TEST_SIGS.items():
            fn = getattr(self.dll, name, None)
            if fn is None:
                self.missing.append(name)
                continue
            fn.restype = res
            fn.argtypes = args
        self.backend = self.dll.lio_backend().decode()
        self.has_ext = self.backend.startswith("hip")
        if self.has_ext:
            for name, (res, args) in (list(_EXT_SIGS.items()) + list(_FULL_SIGS.items()) + list(_ODOM_BATCH_SIGS.items()) + list(_FRONTEND_SIGS.items())
                                      + list(_MAP_BATCH_SIGS.items()) + list(_MAP_FROM_ODOM_SIGS.items())):
                fn = getattr(self.dll, name)
                fn.restype = res
                fn.argtypes = args
            # a build from before the sample sort still loads (the A/B tools take one as --parent-lib); only a call to these fails there
            for name, (res, args) in list(_VOX_SORT_SIGS.items()) + (list(_SEG_BOUNDS_SIGS.items()) + list(_EST_PUSH_SIGS.items())
                                                                             + list(_EST_FROM_ODOM_SIGS.items()) + list(_EST_WIDE_SIGS.items())):
                fn = getattr(self.dll, name, None)
                if fn is not None:
                    fn.restype = res
                    fn.argtypes = args

    def deskew_to_end(self, xyzi, T_es: TransformF, time_factor=10.0, keep_intensity=False):
        """lio_deskew_to_end (include/lio_full_cloud.h, test hook): the estimator's TransformToEnd, Estimator.cc:62-103."""
        c = _f32(xyzi).reshape(-1, 4)
        out = np.zeros_like(c)
        _chk(self.dll.lio_deskew_to_end(_fp(c), c.shape[0], C.byref(T_es), time_factor, 1 if keep_intensity else 0, _fp(out)), "lio_deskew_to_end")
        return out

    # ---- ImuInitializer (host math)
    @staticmethod
    def _laser_frames(transforms, pims):
        n = len(transforms)
        T = (TransformF * n)(*[TransformF.make(q, p) for q, p in transforms])
        P = (C.c_void_p * n)(*[(p.h if p is not None else None) for p in pims])
        return n, T, P

    def imu_estimate_extrinsic_rotation(self, transforms, pims, T_lb):
        """ImuInitializer::EstimateExtrinsicRotation -> (accepted, q_lb xyzw)."""
        n, T, P = self._laser_frames(transforms, pims)
        lb = TransformF.make(*T_lb)
        rc = self.dll.lio_imu_estimate_extrinsic_rotation(n, T, P, C.byref(lb))
        if rc < 0:
            raise LioError(f"lio_imu_estimate_extrinsic_rotation -> {rc}")
        return bool(rc), lb.to_np()[0]

    def imu_initialization(self, transforms, pims, T_lb, Bgs=None):
        """ImuInitializer::Initialization -> dict(ok, Vs, Bgs, g, R_WI); re-propagates the pims."""
        n, T, P = self._laser_frames(transforms, pims)
        lb = TransformF.make(*T_lb)
        Vs = np.zeros((n, 3))
        bgs = np.zeros((n, 3)) if Bgs is None else _f64(Bgs).reshape(n, 3).copy()
        g, R = np.zeros(3), np.zeros((3, 3))
        rc = self.dll.lio_imu_initialization(n, T, P, C.byref(lb), _dp(Vs), _dp(bgs), _dp(g), _dp(R))
        if rc < 0:
            raise LioError(f"lio_imu_initialization -> {rc}")
        return dict(ok=bool(rc), Vs=Vs, Bgs=bgs, g=g, R_WI=R)

    # ---- stateless blocks
    def dense_spd_solve(self, A, b):
        A, b = _f64(A), _f64(b)
        n = b.shape[0]
        assert A.shape == (n, n)
        x = np.zeros(n)
        _chk(self.dll.lio_dense_spd_solve(_dp(A), _dp(b), n, _dp(x)), "lio_dense_spd_solve")
        return x

    def marginalize_schur(self, A, b, m):
        """-> (lin_jac n x n, lin_res n, evals n) of MarginalizationInfo::Marginalize's dense tail (MarginalizationFactor.cc:271-302)."""
        A, b = _f64(A), _f64(b)
        n = b.shape[0] - m
        assert A.shape == (m + n, m + n)
        J, r, s = np.zeros((n, n)), np.zeros(n), np.zeros(n)
        _chk(self.dll.lio_marginalize_schur(_dp(A), _dp(b), m, n, _dp(J), _dp(r), _dp(s)), "lio_marginalize_schur")
        return J, r, s

    def bench_voxel_grid(self, xyzi, leaf, reps=10):
        """device time of one VoxelGrid of a resident cloud (HIP events over `reps` runs) -> (ms, output points)"""
        xyzi = _f32(xyzi).reshape(-1, 4)
        ms, n_out = C.c_double(0), C.c_size_t(0)
        _chk(self.dll.lio_bench_voxel_grid(_fp(xyzi), xyzi.shape[0], float(leaf), int(reps), C.byref(ms), C.byref(n_out)), "lio_bench_voxel_grid")
        return ms.value, int(n_out.value)

    def seg_sort_pairs(self, keys, values, seg_off, seg_n, bits, passes):
        """stable radix sort of (key, value) pairs inside segments (lio_seg_sort_pairs); values None: the elements' positions"""
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        vals = None if values is None else np.ascontiguousarray(values, dtype=np.uint32)
        so, sn = np.ascontiguousarray(seg_off, dtype=np.int32), np.ascontiguousarray(seg_n, dtype=np.int32)
        ko, vo = np.zeros_like(keys), np.zeros_like(keys)
        u32 = C.POINTER(C.c_uint32)
        _chk(self.dll.lio_seg_sort_pairs(keys.ctypes.data_as(u32), vals.ctypes.data_as(u32) if vals is not None else None, keys.shape[0],
                                         so.ctypes.data_as(c_int32_p), sn.ctypes.data_as(c_int32_p), so.shape[0], int(bits), int(passes),
                                         ko.ctypes.data_as(u32), vo.ctypes.data_as(u32)), "lio_seg_sort_pairs")
        return ko, vo

    def vox_sort_pairs(self, keys):
        """lio_vox_sort_pairs (include/lio_vox_sort.h): the voxel filter's sort of (key, position) -> (sorted keys, their positions, LIO_VOX_SORT_* path)"""
        k = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
        ko, vo, path = np.zeros_like(k), np.zeros_like(k), C.c_int(-1)
        _chk(self.dll.lio_vox_sort_pairs(k.ctypes.data_as(_c_uint32_p), k.size, ko.ctypes.data_as(_c_uint32_p), vo.ctypes.data_as(_c_uint32_p),
                                         C.byref(path)), "lio_vox_sort_pairs")
        return ko, vo, path.value

    def vox_sort_stats(self):
        """lio_vox_sort_stats: lio_voxel_grid runs of this thread by the sort that gave their result (sample, direct, library)"""
        out = (C.c_uint64 * 3)()
        _chk(self.dll.lio_vox_sort_stats(out), "lio_vox_sort_stats")
        return tuple(int(v) for v in out)

    def seg_bounds(self, clouds, inv_leaf):
        """lio_seg_bounds (include/lio_seg_bounds.h): one bounds pass over all `clouds` -> per cloud dict(mn, mx, minb, divb, overflow, n_valid)"""
        cs = [_f32(c).reshape(-1, 4) for c in clouds]
        ptrs = (c_float_p * len(cs))(*[_fp(c) if c.shape[0] else None for c in cs])
        ns = (C.c_size_t * len(cs))(*[c.shape[0] for c in cs])
        out = (SegBoundsOut * len(cs))()
        _chk(self.dll.lio_seg_bounds(ptrs, ns, len(cs), float(inv_leaf), out), "lio_seg_bounds")
        return [dict(mn=np.array(o.mn, np.float32), mx=np.array(o.mx, np.float32), minb=np.array(o.minb, np.int32), divb=np.array(o.divb, np.int32),
                     overflow=int(o.overflow), n_valid=int(o.n_valid)) for o in out]

    def voxel_grid(self, xyzi, leaf):
        xyzi = _f32(xyzi).reshape(-1, 4)
        out = np.zeros_like(xyzi)
        n = C.c_size_t(0)
        _chk(self.dll.lio_voxel_grid(_fp(xyzi), xyzi.shape[0], leaf, _fp(out), C.byref(n)), "lio_voxel_grid")
        return out[: n.value].copy()

    def knn(self, map_xyzi, query_xyzi, k, radius_sq=0.0):
        m_ = _f32(map_xyzi).reshape(-1, 4)
        q_ = _f32(query_xyzi).reshape(-1, 4)
        idx = np.zeros((q_.shape[0], k), dtype=np.int32)
        sqd = np.zeros((q_.shape[0], k), dtype=np.float32)
        _chk(
            self.dll.lio_knn(_fp(m_), m_.shape[0], _fp(q_), q_.shape[0], k, radius_sq, idx.ctypes.data_as(c_int32_p), _fp(sqd)), "lio_knn"
        )
        return idx, sqd

    def knn_walk(self, map_xyzi, query_xyzi, cell, lanes_per_query):
        """the product's five-nearest walk on its own (include/lio_test_hooks.h: lio_knn_walk), no radius cut ->
        (idx (m, 5) int32, -1 = missing; sqd (m, 5) fp32, +inf = missing; nbr_xyz (m, 5, 3) the points the plane fit would load)"""
        m_ = _f32(map_xyzi).reshape(-1, 4)
        q_ = _f32(query_xyzi).reshape(-1, 4)
        idx = np.zeros((q_.shape[0], 5), dtype=np.int32)
        sqd = np.zeros((q_.shape[0], 5), dtype=np.float32)
        nbr = np.zeros((q_.shape[0], 5, 3), dtype=np.float32)
        _chk(self.dll.lio_knn_walk(_fp(m_), m_.shape[0], _fp(q_), q_.shape[0], float(cell), int(lanes_per_query),
                                   idx.ctypes.data_as(c_int32_p), _fp(sqd), _fp(nbr)), "lio_knn_walk")
        return idx, sqd, nbr

    def fit_five(self, form, nbr_xyz, fifth_sqd, stack_xyzi, T: TransformF, fixed_pz=(0.0, 0.0, 0.0), min_match_sq_dis=1.0, min_plane_dis=0.2):
        """the plane fit (form 0 estimator, 1 PointMapping, 2 MapBuilder) or the line fit (form 3) on caller-given neighbours
        (include/lio_test_hooks.h: lio_fit_five) -> (valid (m,) uint8, coeff (m, 4), score (m,), abs_coeff (m, 4)), zeros where invalid"""
        s_ = _f32(stack_xyzi).reshape(-1, 4)
        m = s_.shape[0]
        n_ = _f32(nbr_xyz).reshape(m, 5, 3)
        f_ = _f32(fifth_sqd).reshape(m)
        pz = _f32(fixed_pz).reshape(3)
        valid = np.zeros(m, dtype=np.uint8)
        coeff = np.zeros((m, 4), dtype=np.float32)
        score = np.zeros(m, dtype=np.float32)
        abs_coeff = np.zeros((m, 4), dtype=np.float32)
        _chk(self.dll.lio_fit_five(int(form), _fp(n_), _fp(f_), _fp(s_), m, C.byref(T), _fp(pz), float(min_match_sq_dis), float(min_plane_dis),
                                   valid.ctypes.data_as(c_uint8_p), _fp(coeff), _fp(score), _fp(abs_coeff)), "lio_fit_five")
        return valid, coeff, score, abs_coeff

    def odom_correspondences(self, sharp, flat, last_corner, last_surf, T_es: TransformF, scan_period=0.1, no_deskew=False):
        """the scan-to-scan correspondence search on its own (include/lio_test_hooks.h: lio_odom_correspondences) ->
        (corner_idx (n_sharp, 2) int32, surf_idx (n_flat, 3) int32, -1 = missing; sel (n_sharp + n_flat, 3) fp32, sharp first)"""
        cl = [_f32(c).reshape(-1, 4) for c in (sharp, flat, last_corner, last_surf)]
        nc, ns = cl[0].shape[0], cl[1].shape[0]
        corner_idx = np.zeros((nc, 2), dtype=np.int32)
        surf_idx = np.zeros((ns, 3), dtype=np.int32)
        sel = np.zeros((nc + ns, 3), dtype=np.float32)
        args = []
        for c in cl:
            args += [_fp(c), c.shape[0]]
        _chk(self.dll.lio_odom_correspondences(*args, C.byref(T_es), float(scan_period), 1 if no_deskew else 0,
                                               corner_idx.ctypes.data_as(c_int32_p), surf_idx.ctypes.data_as(c_int32_p), _fp(sel)),
             "lio_odom_correspondences")
        return corner_idx, surf_idx, sel

    def gn_rows_map(self, form, stack_xyzi, valid, coeff, T: TransformF):
        """the rows of the scan-to-map family and the partials of one production rows launch (include/lio_test_hooks.h: lio_gn_rows_map) ->
        (ok (m,) uint8, rows (m, 7) fp32 = a0 .. a5, b, partials (nb, 28) fp64)"""
        s_ = _f32(stack_xyzi).reshape(-1, 4)
        m = s_.shape[0]
        v_ = np.ascontiguousarray(valid, dtype=np.uint8).reshape(m)
        c_ = _f32(coeff).reshape(m, 4)
        ok = np.zeros(m, dtype=np.uint8)
        rows = np.zeros((m, 7), dtype=np.float32)
        nb = np.zeros(1, dtype=np.int32)
        partials = np.zeros((256, 28), dtype=np.float64)
        _chk(self.dll.lio_gn_rows_map(int(form), _fp(s_), m, v_.ctypes.data_as(c_uint8_p), _fp(c_), C.byref(T), ok.ctypes.data_as(c_uint8_p),
                                      _fp(rows), nb.ctypes.data_as(c_int32_p), partials.ctypes.data_as(c_double_p)), "lio_gn_rows_map")
        return ok, rows, partials[: int(nb[0])].copy()

    def gn_rows_odom(self, sharp, flat, last_corner, last_surf, corner_idx, surf_idx, T_es: TransformF, iter, scan_period=0.1, no_deskew=False):
        """the rows of the scan-to-scan loop and the partials of one production rows launch, on given correspondences
        (include/lio_test_hooks.h: lio_gn_rows_odom) -> (ok (nq,) uint8, rows (nq, 7) fp32, partials (nb, 28) fp64), sharp first"""
        cl = [_f32(c).reshape(-1, 4) for c in (sharp, flat, last_corner, last_surf)]
        nc, ns = cl[0].shape[0], cl[1].shape[0]
        ci = np.ascontiguousarray(corner_idx, dtype=np.int32).reshape(nc, 2)
        si = np.ascontiguousarray(surf_idx, dtype=np.int32).reshape(ns, 3)
        ok = np.zeros(nc + ns, dtype=np.uint8)
        rows = np.zeros((nc + ns, 7), dtype=np.float32)
        nb = np.zeros(1, dtype=np.int32)
        partials = np.zeros((64, 28), dtype=np.float64)
        args = []
        for c in cl:
            args += [_fp(c), c.shape[0]]
        _chk(self.dll.lio_gn_rows_odom(*args, ci.ctypes.data_as(c_int32_p), si.ctypes.data_as(c_int32_p), C.byref(T_es), float(scan_period),
                                       1 if no_deskew else 0, int(iter), ok.ctypes.data_as(c_uint8_p), _fp(rows), nb.ctypes.data_as(c_int32_p),
                                       partials.ctypes.data_as(c_double_p)), "lio_gn_rows_odom")
        return ok, rows, partials[: int(nb[0])].copy()

    def gn_fold(self, partials, wide):
        """the fixed-order fold of (nblocks, 28) partials (include/lio_test_hooks.h: lio_gn_fold) -> sums (28,) fp64"""
        p_ = np.ascontiguousarray(partials, dtype=np.float64).reshape(-1, 28)
        sums = np.zeros(28, dtype=np.float64)
        _chk(self.dll.lio_gn_fold(p_.ctypes.data_as(c_double_p), p_.shape[0], int(wide), sums.ctypes.data_as(c_double_p)), "lio_gn_fold")
        return sums

    def gn_step(self, family, sums, state_in, iter, min_rows=0, left_update=0):
        """the serial 6x6 step behind the sums (include/lio_test_hooks.h: lio_gn_step); state_in / the result: records of GN_STATE"""
        s_ = np.ascontiguousarray(sums, dtype=np.float64).reshape(28)
        si = np.array(state_in, dtype=GN_STATE).reshape(1)
        so = np.zeros(1, dtype=GN_STATE)
        _chk(self.dll.lio_gn_step(int(family), s_.ctypes.data_as(c_double_p), si.ctypes.data, int(iter), int(min_rows), int(left_update),
                                  so.ctypes.data), "lio_gn_step")
        return so[0]

    def gn_round(self, map_xyzi, stack_xyzi, T: TransformF, lanes_per_query, min_match_sq_dis=1.0, min_plane_dis=0.2):
        """round 0 of the newest-frame loop through the production launch pair (include/lio_test_hooks.h: lio_gn_round) ->
        (partials (nb, 28) fp64, state: a record of GN_STATE)"""
        m_ = _f32(map_xyzi).reshape(-1, 4)
        s_ = _f32(stack_xyzi).reshape(-1, 4)
        m = s_.shape[0]
        nb = np.zeros(1, dtype=np.int32)
        partials = np.zeros((max(1, -(-m * int(lanes_per_query) // 256)), 28), dtype=np.float64)
        so = np.zeros(1, dtype=GN_STATE)
        _chk(self.dll.lio_gn_round(_fp(m_), m_.shape[0], _fp(s_), m, C.byref(T), float(min_match_sq_dis), float(min_plane_dis),
                                   int(lanes_per_query), nb.ctypes.data_as(c_int32_p), partials.ctypes.data_as(c_double_p), so.ctypes.data),
             "lio_gn_round")
        return partials[: int(nb[0])].copy(), so[0]

    def calculate_features(self, map_xyzi, stack_xyzi, T: TransformF, min_match_sq_dis=1.0, min_plane_dis=0.2):
        m_ = _f32(map_xyzi).reshape(-1, 4)
        s_ = _f32(stack_xyzi).reshape(-1, 4)
        valid = np.zeros(s_.shape[0], dtype=np.uint8)
        coeff = np.zeros((s_.shape[0], 4), dtype=np.float32)
        score = np.zeros(s_.shape[0], dtype=np.float32)
        _chk(
            self.dll.lio_calculate_features(
                _fp(m_), m_.shape[0], _fp(s_), s_.shape[0], C.byref(T), min_match_sq_dis, min_plane_dis, valid.ctypes.data_as(c_uint8_p), _fp(coeff), _fp(score)
            ),
            "lio_calculate_features",
        )
        return valid, coeff, score

    # ---- /compact_data codec
    def compact_encode(self, T: TransformF, corner, surf, full):
        cl = [_f32(c).reshape(-1, 4) for c in (corner, surf, full)]
        out = np.zeros((3 + sum(c.shape[0] for c in cl), 4), dtype=np.float32)
        args = []
        for c in cl:
            args += [_fp(c), c.shape[0]]
        n = self.dll.lio_compact_encode(C.byref(T), *args, _fp(out))
        assert n == out.shape[0]
        return out

    def compact_decode(self, data):
        data = _f32(data).reshape(-1, 4)
        T = TransformF()
        nc, ns, nf = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        rc = self.dll.lio_compact_decode(_fp(data), data.shape[0], C.byref(T), C.byref(nc), C.byref(ns), C.byref(nf))
        if rc != 0:
            raise LioError(f"lio_compact_decode failed with code {rc}")
        a, b = 3 + nc.value, 3 + nc.value + ns.value
        return T.to_np(), data[3:a], data[a:b], data[b:]

    # ---- factors
    def factor_ppp(self, point, coeff, pose_p, pose_i, pose_ex, jac=True):
        res = np.zeros(1)
        js = [np.zeros(7) for _ in range(3)] if jac else [None] * 3
        _chk(
            self.dll.lio_factor_pivot_point_plane(
                _dp(_f64(point)), _dp(_f64(coeff)), _dp(_f64(pose_p)), _dp(_f64(pose_i)), _dp(_f64(pose_ex)), _dp(res), *[_dp(j) for j in js]
            ),
            "lio_factor_pivot_point_plane",
        )
        return res[0], js

    def factor_prior(self, pos0, rot0, pose, jac=True):
        res = np.zeros(6)
        J = np.zeros((6, 7)) if jac else None
        _chk(self.dll.lio_factor_prior(_dp(_f64(pos0)), _dp(_f64(rot0)), _dp(_f64(pose)), _dp(res), _dp(J)), "lio_factor_prior")
        return res, J

    def pose_plus(self, pose, delta):
        out = np.zeros(7)
        _chk(self.dll.lio_pose_plus(_dp(_f64(pose)), _dp(_f64(delta)), _dp(out)), "lio_pose_plus")
        return out

    def default_est_config(self) -> EstConfig:
        c = EstConfig()
        self.dll.lio_est_default_config(C.byref(c))
        return c


class Pim:
    def __init__(self, lib: LioLib, acc0, gyr0, ba, bg, acc_n=0.1, gyr_n=0.01, acc_w=0.0002, gyr_w=2.0e-5, g_norm=9.805):
        self.lib = lib
        self.h = lib.dll.lio_pim_create(_dp(_f64(acc0)), _dp(_f64(gyr0)), _dp(_f64(ba)), _dp(_f64(bg)), acc_n, gyr_n, acc_w, gyr_w, g_norm)
        if not self.h:
            raise LioError("lio_pim_create failed")

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.dll.lio_pim_destroy(self.h)
            self.h = None

    def push_back(self, dt, acc, gyr):
        _chk(self.lib.dll.lio_pim_push_back(self.h, dt, _dp(_f64(acc)), _dp(_f64(gyr))), "lio_pim_push_back")

    def repropagate(self, ba, bg):
        _chk(self.lib.dll.lio_pim_repropagate(self.h, _dp(_f64(ba)), _dp(_f64(bg))), "lio_pim_repropagate")

    def get(self):
        sum_dt = np.zeros(1)
        dp, dq, dv = np.zeros(3), np.zeros(4), np.zeros(3)
        jac, cov = np.zeros((15, 15)), np.zeros((15, 15))
        _chk(self.lib.dll.lio_pim_get(self.h, _dp(sum_dt), _dp(dp), _dp(dq), _dp(dv), _dp(jac), _dp(cov)), "lio_pim_get")
        return dict(sum_dt=sum_dt[0], dp=dp, dq=dq, dv=dv, jac=jac, cov=cov)

    def evaluate(self, pose_i, sb_i, pose_j, sb_j):
        res = np.zeros(15)
        _chk(self.lib.dll.lio_pim_evaluate(self.h, _dp(_f64(pose_i)), _dp(_f64(sb_i)), _dp(_f64(pose_j)), _dp(_f64(sb_j)), _dp(res)), "lio_pim_evaluate")
        return res

    def factor(self, pose_i, sb_i, pose_j, sb_j, jac=True):
        res = np.zeros(15)
        js = [np.zeros((15, 7)), np.zeros((15, 9)), np.zeros((15, 7)), np.zeros((15, 9))] if jac else [None] * 4
        _chk(
            self.lib.dll.lio_factor_imu(self.h, _dp(_f64(pose_i)), _dp(_f64(sb_i)), _dp(_f64(pose_j)), _dp(_f64(sb_j)), _dp(res), *[_dp(j) for j in js]),
            "lio_factor_imu",
        )
        return res, js


class PointProcessor:
    RINGS, SHARP, LESS_SHARP, FLAT, LESS_FLAT = range(5)

    def __init__(self, lib: LioLib, lower, upper, rings, cfg: PPConfig | None = None):
        self.lib = lib
        self.rings = rings
        self.h = lib.dll.lio_pp_create(lower, upper, rings, C.byref(cfg) if cfg is not None else None)
        if not self.h:
            raise LioError("lio_pp_create failed")

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.dll.lio_pp_destroy(self.h)
            self.h = None

    def process_async(self, xyzi):
        """enqueue a sweep and return; `wait()` (or any accessor) blocks until it is done.  Keeps `xyzi` alive meanwhile."""
        self._pending = _f32(xyzi).reshape(-1, 4)
        _chk(self.lib.dll.lio_pp_process_async(self.h, _fp(self._pending), self._pending.shape[0]), "lio_pp_process_async")

    def wait(self):
        _chk(self.lib.dll.lio_pp_wait(self.h), "lio_pp_wait")
        self._pending = None

    @staticmethod
    def process_batch(processors, sweeps):
        """lio_pp_process_batch: one sweep per handle, all enqueued before the first is waited for."""
        assert len(processors) == len(sweeps)
        B = len(processors)
        if B == 0:
            return
        arrs = [_f32(x).reshape(-1, 4) for x in sweeps]
        hs = (C.c_void_p * B)(*[p.h for p in processors])
        ptrs = (c_float_p * B)(*[_fp(a) for a in arrs])
        ns = (C.c_size_t * B)(*[a.shape[0] for a in arrs])
        _chk(processors[0].lib.dll.lio_pp_process_batch(hs, ptrs, ns, B), "lio_pp_process_batch")

    @staticmethod
    def process_rings_batch(processors, sweeps, rings):
        """lio_pp_process_rings_batch: the PointIR overload (a ring per point) for B sweeps in one call."""
        B = len(processors)
        assert B == len(sweeps) == len(rings)
        if B == 0:
            return
        arrs = [_f32(x).reshape(-1, 4) for x in sweeps]
        rgs = [np.ascontiguousarray(r, dtype=np.uint16) for r in rings]
        hs = (C.c_void_p * B)(*[p.h for p in processors])
        ptrs = (c_float_p * B)(*[_fp(a) for a in arrs])
        rptrs = (c_uint16_p * B)(*[r.ctypes.data_as(c_uint16_p) for r in rgs])
        ns = (C.c_size_t * B)(*[a.shape[0] for a in arrs])
        _chk(processors[0].lib.dll.lio_pp_process_rings_batch(hs, ptrs, rptrs, ns, B), "lio_pp_process_rings_batch")

    @staticmethod
    def process_batch_device(processors, device_ptrs, counts):
        """lio_pp_process_batch_device: the sweeps are already in device memory (device_ptrs[k]: address of counts[k] x 4 floats)."""
        B = len(processors)
        assert B == len(device_ptrs) == len(counts)
        if B == 0:
            return
        hs = (C.c_void_p * B)(*[p.h for p in processors])
        ptrs = (C.c_void_p * B)(*[int(a) for a in device_ptrs])
        ns = (C.c_size_t * B)(*[int(c) for c in counts])
        _chk(processors[0].lib.dll.lio_pp_process_batch_device(hs, ptrs, ns, B), "lio_pp_process_batch_device")

    def process(self, xyzi, ring=None):
        """ring (uint16 per point) selects the PointIR overload of PointToRing (uneven sensors, PointProcessor.cc:428-536)."""
        xyzi = _f32(xyzi).reshape(-1, 4)
        if ring is None:
            _chk(self.lib.dll.lio_pp_process(self.h, _fp(xyzi), xyzi.shape[0]), "lio_pp_process")
            return
        ring = np.ascontiguousarray(ring, dtype=np.uint16)
        assert ring.shape[0] == xyzi.shape[0]
        _chk(self.lib.dll.lio_pp_process_rings(self.h, _fp(xyzi), ring.ctypes.data_as(c_uint16_p), xyzi.shape[0]), "lio_pp_process_rings")

    def start_ori(self):
        """start_ori_ of the last process call (after infer_start_ori's filter when that is enabled)."""
        return float(self.lib.dll.lio_pp_start_ori(self.h))

    def cloud(self, which):
        n = self.lib.dll.lio_pp_count(self.h, which)
        out = np.zeros((n, 4), dtype=np.float32)
        if n:
            _chk(self.lib.dll.lio_pp_get_cloud(self.h, which, _fp(out)), "lio_pp_get_cloud")
        return out

    def indices(self, which):
        n = self.lib.dll.lio_pp_count(self.h, which)
        ring = np.zeros(n, dtype=np.int32)
        idx = np.zeros(n, dtype=np.int32)
        if n:
            _chk(self.lib.dll.lio_pp_get_indices(self.h, which, ring.ctypes.data_as(c_int32_p), idx.ctypes.data_as(c_int32_p)), "lio_pp_get_indices")
        return ring, idx

    def ring_offsets(self):
        out = np.zeros(self.rings + 1, dtype=np.int32)
        _chk(self.lib.dll.lio_pp_get_ring_offsets(self.h, out.ctypes.data_as(c_int32_p)), "lio_pp_get_ring_offsets")
        return out

    def ring_intensity(self):
        """intensity channel of the reference's intensity_scans, ring order: int(input intensity) + rel_time"""
        out = np.zeros(int(self.lib.dll.lio_pp_count(self.h, self.RINGS)), np.float32)
        _chk(self.lib.dll.lio_pp_get_ring_intensity(self.h, _fp(out)), "lio_pp_get_ring_intensity")
        return out

    def curvature(self):
        n = self.lib.dll.lio_pp_count(self.h, 0)
        curv = np.zeros(n, dtype=np.float32)
        mask = np.zeros(n, dtype=np.int32)
        _chk(self.lib.dll.lio_pp_get_curvature(self.h, _fp(curv), mask.ctypes.data_as(c_int32_p)), "lio_pp_get_curvature")
        return curv, mask


class PointMapping:
    """PointMapping (scan-to-map + cube map) — reference src/point_processor/PointMapping.cc."""

    CORNER_STACK_DS, SURF_STACK_DS, CORNER_FROM_MAP, SURF_FROM_MAP = 0, 1, 2, 3

    def __init__(self, lib: LioLib, **overrides):
        self.lib = lib
        cfg = MapConfig()
        lib.dll.lio_map_default_config(C.byref(cfg))
        for k, v in overrides.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        self.h = lib.dll.lio_map_create(C.byref(cfg))
        if not self.h:
            raise LioError("lio_map_create failed")

    @classmethod
    def borrowed(cls, lib: LioLib, handle, owner):
        """The lio_map of an estimator (lio_est_map): owned by `owner`, which this object keeps alive; never destroyed here."""
        m = cls.__new__(cls)
        m.lib, m.cfg, m.h, m.owner = lib, None, handle, owner
        return m

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "owner", None) is None:
            self.lib.dll.lio_map_destroy(self.h)
        self.h = None

    def surround(self, leaf=0.6):
        """lio_map_get_surround (include/lio_ext.h): the down-sampled 5 x 5 x 5 surround map, PointMapping.cc:1223-1234."""
        n = self.lib.dll.lio_map_get_surround(self.h, leaf, None)
        out = np.zeros((n, 4), dtype=np.float32)
        if n:
            m = self.lib.dll.lio_map_get_surround(self.h, leaf, _fp(out))
            assert m == n
        return out

    def set_full_cloud(self, xyzi):
        """lio_map_set_full_cloud (include/lio_full_cloud.h): full_cloud_, PointMapping.cc:212-224; an empty cloud clears it."""
        c = _f32(xyzi).reshape(-1, 4)
        _chk(self.lib.dll.lio_map_set_full_cloud(self.h, _fp(c), c.shape[0]), "lio_map_set_full_cloud")

    def full_cloud(self):
        """lio_map_get_full_cloud: full_cloud_ as it is now (/cloud_registered after a process with the init flag off)."""
        n = self.lib.dll.lio_map_get_full_cloud(self.h, None)
        out = np.zeros((n, 4), dtype=np.float32)
        if n:
            m = self.lib.dll.lio_map_get_full_cloud(self.h, _fp(out))
            assert m == n
        return out

    def process(self, corner_last, surf_last, T_sum):
        c, s = _f32(corner_last).reshape(-1, 4), _f32(surf_last).reshape(-1, 4)
        Ts = TransformF.make(*T_sum)
        Ta = TransformF()
        it, ns = C.c_int(0), C.c_int(0)
        _chk(self.lib.dll.lio_map_process(self.h, _fp(c), c.shape[0], _fp(s), s.shape[0], C.byref(Ts), C.byref(Ta), C.byref(it), C.byref(ns)),
             "lio_map_process")
        kz = C.c_int(0)
        deg = self.lib.dll.lio_map_get_degeneracy(self.h, C.byref(kz))
        return dict(T_aft=Ta.to_np(), iterations=it.value, num_selected=ns.value, degenerate=int(deg), kz=kz.value)

    @staticmethod
    def process_batch(handles, inputs):
        """lio_map_process_batch (include/lio_map_batch.h): one sweep of every PointMapping of `handles` with the rounds of all of them in
        one launch chain; inputs[k] = (corner_last, surf_last, T_sum) of sensor k.  -> list of the dicts process() returns."""
        n = len(handles)
        if n < 1 or len(inputs) != n:
            raise LioError("process_batch: one (corner_last, surf_last, T_sum) per handle, at least one handle")
        lib = handles[0].lib
        cl = [[_f32(c).reshape(-1, 4) for c in inp[:2]] for inp in inputs]   # (kept alive until the call returns)
        H = (C.c_void_p * n)(*[h.h for h in handles])
        args = []
        for w in range(2):
            args += [(c_float_p * n)(*[_fp(cl[k][w]) for k in range(n)]), (C.c_size_t * n)(*[cl[k][w].shape[0] for k in range(n)])]
        Ts = (TransformF * n)(*[TransformF.make(*inp[2]) for inp in inputs])
        Ta = (TransformF * n)()
        it, ns = np.zeros(n, np.int32), np.zeros(n, np.int32)
        _chk(lib.dll.lio_map_process_batch(H, n, *args, Ts, Ta, it.ctypes.data_as(c_int32_p), ns.ctypes.data_as(c_int32_p)), "lio_map_process_batch")
        out = []
        for k, h in enumerate(handles):
            kz = C.c_int(0)
            deg = lib.dll.lio_map_get_degeneracy(h.h, C.byref(kz))
            out.append(dict(T_aft=Ta[k].to_np(), iterations=int(it[k]), num_selected=int(ns[k]), degenerate=int(deg), kz=kz.value))
        return out

    @staticmethod
    def process_batch_from_odom(handles, odoms, processors_or_none=None):
        """lio_map_process_batch_from_odom (include/lio_map_from_odom.h): process_batch with the clouds and T_sum of handles[k] taken from
        the PointOdometry odoms[k] on the device, and its full cloud from the PointProcessor processors_or_none[k] (None, or a None entry:
        the handle's full cloud stays as it is).  -> list of the dicts process() returns."""
        n = len(handles)
        if n < 1 or len(odoms) != n or (processors_or_none is not None and len(processors_or_none) != n):
            raise LioError("process_batch_from_odom: one odometry (and one processor or None) per handle, at least one handle")
        lib = handles[0].lib
        H = (C.c_void_p * n)(*[h.h for h in handles])
        O = (C.c_void_p * n)(*[o.h for o in odoms])
        P = None if processors_or_none is None else (C.c_void_p * n)(*[None if p is None else p.h for p in processors_or_none])
        Ta = (TransformF * n)()
        it, ns = np.zeros(n, np.int32), np.zeros(n, np.int32)
        _chk(lib.dll.lio_map_process_batch_from_odom(H, O, P, n, Ta, it.ctypes.data_as(c_int32_p), ns.ctypes.data_as(c_int32_p)),
             "lio_map_process_batch_from_odom")
        out = []
        for k, h in enumerate(handles):
            kz = C.c_int(0)
            deg = lib.dll.lio_map_get_degeneracy(h.h, C.byref(kz))
            out.append(dict(T_aft=Ta[k].to_np(), iterations=int(it[k]), num_selected=int(ns[k]), degenerate=int(deg), kz=kz.value))
        return out

    def set_init_flag(self, on):
        _chk(self.lib.dll.lio_map_set_init_flag(self.h, 1 if on else 0), "lio_map_set_init_flag")

    def set_transform_tobe_mapped(self, q_xyzw, p):
        T = TransformF.make(q_xyzw, p)
        _chk(self.lib.dll.lio_map_set_transform_tobe_mapped(self.h, C.byref(T)), "lio_map_set_transform_tobe_mapped")

    def transform_tobe_mapped(self):
        T = TransformF()
        _chk(self.lib.dll.lio_map_get_transform_tobe_mapped(self.h, C.byref(T)), "lio_map_get_transform_tobe_mapped")
        return T.to_np()

    def update_map_database(self, corner_ds, surf_ds, valid_idx, T, cube_center):
        c, s = _f32(corner_ds).reshape(-1, 4), _f32(surf_ds).reshape(-1, 4)
        v = np.ascontiguousarray(valid_idx, dtype=np.uint32)
        Tt = TransformF.make(*T)
        cen = (C.c_int * 3)(*[int(x) for x in cube_center])
        _chk(self.lib.dll.lio_map_update_map_database(self.h, _fp(c), c.shape[0], _fp(s), s.shape[0], v.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                      v.shape[0], C.byref(Tt), cen), "lio_map_update_map_database")

    def cloud(self, which):
        n = self.lib.dll.lio_map_get_cloud(self.h, which, None)
        out = np.zeros((n, 4), dtype=np.float32)
        if n:
            self.lib.dll.lio_map_get_cloud(self.h, which, _fp(out))
        return out

    def cube(self, cls, cube_idx):
        n = self.lib.dll.lio_map_get_cube(self.h, cls, int(cube_idx), None)
        out = np.zeros((n, 4), dtype=np.float32)
        if n:
            self.lib.dll.lio_map_get_cube(self.h, cls, int(cube_idx), _fp(out))
        return out

    def cube_state(self):
        cen = (C.c_int * 3)()
        valid = np.zeros(125, dtype=np.uint32)
        n = self.lib.dll.lio_map_get_cube_state(self.h, cen, valid.ctypes.data_as(C.POINTER(C.c_uint32)))
        return list(cen), valid[:n].copy()

    def score_point_coeff(self):
        n = self.lib.dll.lio_map_get_score_point_coeff(self.h, None, None, None)
        score = np.zeros(n, dtype=np.float32)
        point = np.zeros((n, 4), dtype=np.float32)
        coeff = np.zeros((n, 4), dtype=np.float32)
        if n:
            self.lib.dll.lio_map_get_score_point_coeff(self.h, _fp(score), _fp(point), _fp(coeff))
        return score, point, coeff


class Rccl:
    """In-library RCCL communicator (one per process / GPU): `Rccl.unique_id(lib)` on rank 0, the bytes sent to every rank by
    any side channel, then `Rccl(lib, id_bytes, rank, world)` on the device the process drives."""

    @staticmethod
    def unique_id(lib: LioLib) -> bytes:
        buf = C.create_string_buffer(128)
        _chk(lib.dll.lio_rccl_unique_id(buf), "lio_rccl_unique_id")
        return bytes(buf.raw)

    def __init__(self, lib: LioLib, id_bytes: bytes, rank: int, world: int):
        assert len(id_bytes) == 128
        self.lib = lib
        self.h = lib.dll.lio_rccl_init(C.create_string_buffer(id_bytes, 128), int(rank), int(world))
        if not self.h:
            raise LioError("lio_rccl_init failed")
        self.rank, self.world = int(rank), int(world)

    def world_seen_by_rccl(self) -> int:
        """lio_rccl_world: what the communicator itself reports (bench.py prints it next to n_gpus)."""
        return int(self.lib.dll.lio_rccl_world(self.h))

    def bench_all_reduce(self, count: int, reps: int = 200) -> float:
        """collective: mean microseconds per in-place SUM all-reduce of `count` doubles (HIP events, this rank)."""
        us = C.c_double(0)
        _chk(self.lib.dll.lio_rccl_bench_all_reduce(self.h, int(count), int(reps), C.byref(us)), "lio_rccl_bench_all_reduce")
        return us.value

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.dll.lio_rccl_destroy(self.h)
            self.h = None


class KeyframeBatch:
    """Batched keyframe refinement (BASELINE.json configs[4]): one OptimizeMap / OptimizeTransformTobeMapped loop per
    keyframe (MapBuilder.cc:624-1014 / PointMapping.cc:325-753), all keyframes of the handle advanced together."""

    def __init__(self, lib: LioLib, **overrides):
        self.lib = lib
        cfg = MapConfig()
        lib.dll.lio_map_default_config(C.byref(cfg))
        for k, v in overrides.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        self.h = lib.dll.lio_kf_batch_create(C.byref(cfg))
        if not self.h:
            raise LioError("lio_kf_batch_create failed")

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.dll.lio_kf_batch_destroy(self.h)
            self.h = None

    def add_map(self, corner_map, surf_map):
        c, s = _f32(corner_map).reshape(-1, 4), _f32(surf_map).reshape(-1, 4)
        idx = self.lib.dll.lio_kf_batch_add_map(self.h, _fp(c), c.shape[0], _fp(s), s.shape[0])
        if idx < 0:
            _chk(idx, "lio_kf_batch_add_map")
        return idx

    def add_keyframe(self, map_index, corner_stack, surf_stack, T_init):
        c, s = _f32(corner_stack).reshape(-1, 4), _f32(surf_stack).reshape(-1, 4)
        T = TransformF.make(*T_init)
        idx = self.lib.dll.lio_kf_batch_add_keyframe(self.h, int(map_index), _fp(c), c.shape[0], _fp(s), s.shape[0], C.byref(T))
        if idx < 0:
            _chk(idx, "lio_kf_batch_add_keyframe")
        return idx

    def clear_keyframes(self):
        _chk(self.lib.dll.lio_kf_batch_clear_keyframes(self.h), "lio_kf_batch_clear_keyframes")

    def __len__(self):
        return int(self.lib.dll.lio_kf_batch_size(self.h))

    def refine_gather(self, comm: "Rccl", slots_per_rank: int):
        """refine() + all-gather of every rank's results inside the library (ncclAllGather from the device pose buffer).
        -> (world, slots_per_rank, 9) float32: q xyzw, p, iterations, rows; rows beyond a rank's keyframe count are zero."""
        out = np.zeros((comm.world, int(slots_per_rank), 9), dtype=np.float32)
        ms = C.c_double(0)
        _chk(self.lib.dll.lio_kf_batch_refine_gather(self.h, comm.h, int(slots_per_rank), _fp(out), C.byref(ms)), "lio_kf_batch_refine_gather")
        self.last_device_ms = ms.value
        return out

    def refine(self):
        """-> dict(q (n,4) xyzw, p (n,3), iterations (n,), rows (n,), device_ms)"""
        n = len(self)
        T = (TransformF * max(n, 1))()
        it = np.zeros(max(n, 1), dtype=np.int32)
        rows = np.zeros(max(n, 1), dtype=np.int32)
        ms = C.c_double(0)
        _chk(self.lib.dll.lio_kf_batch_refine(self.h, T, it.ctypes.data_as(c_int32_p), rows.ctypes.data_as(c_int32_p), C.byref(ms)),
             "lio_kf_batch_refine")
        arr = np.frombuffer(T, dtype=np.float32).reshape(-1, 7)[:n]
        kz = np.zeros(max(n, 1), dtype=np.int32)
        _chk(self.lib.dll.lio_kf_batch_get_degeneracy(self.h, kz.ctypes.data_as(c_int32_p)), "lio_kf_batch_get_degeneracy")
        return dict(q=arr[:, :4].copy(), p=arr[:, 4:7].copy(), iterations=it[:n], rows=rows[:n], kz=kz[:n], device_ms=ms.value)


class PointOdometry:
    def __init__(self, lib: LioLib, scan_period=0.1, io_ratio=2, max_iter=25, no_deskew=False):
        self.lib = lib
        self.h = lib.dll.lio_odom_create(scan_period, io_ratio, max_iter, 1 if no_deskew else 0)
        if not self.h:
            raise LioError("lio_odom_create failed")

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.dll.lio_odom_destroy(self.h)
            self.h = None

    def process(self, sharp, less_sharp, flat, less_flat):
        cl = [_f32(c).reshape(-1, 4) for c in (sharp, less_sharp, flat, less_flat)]
        Ts, Te = TransformF(), TransformF()
        it, ns = C.c_int(0), C.c_int(0)
        args = []
        for c in cl:
            args += [_fp(c), c.shape[0]]
        _chk(self.lib.dll.lio_odom_process(self.h, *args, C.byref(Ts), C.byref(Te), C.byref(it), C.byref(ns)), "lio_odom_process")
        cap = max(it.value, 1)
        tr = (TransformF * cap)()
        kz = C.c_int(0)
        n = self.lib.dll.lio_odom_get_iteration_trace(self.h, tr, cap, C.byref(kz))
        if n < 0:
            raise LioError(f"lio_odom_get_iteration_trace -> {n}")
        trace = np.frombuffer(tr, dtype=np.float32).reshape(-1, 7)[:n].copy()   # rows: q xyzw, p
        return dict(T_sum=Ts.to_np(), T_es=Te.to_np(), iterations=it.value, num_selected=ns.value, trace=trace, kz=kz.value)

    @staticmethod
    def process_batch(handles, clouds):
        """lio_odom_process_batch (include/lio_odom_batch.h): one sweep of every PointOdometry of `handles` through one launch chain;
        clouds[k] = (sharp, less_sharp, flat, less_flat) of sensor k.  -> list of the dicts process() returns, without trace and kz
        (ask iteration_trace() of the handle)."""
        n = len(handles)
        if n < 1 or len(clouds) != n:
            raise LioError("process_batch: one set of four clouds per handle, at least one handle")
        lib = handles[0].lib
        cl = [[_f32(c).reshape(-1, 4) for c in four] for four in clouds]   # (kept alive until the call returns)
        H = (C.c_void_p * n)(*[h.h for h in handles])
        args = []
        for w in range(4):
            args += [(c_float_p * n)(*[_fp(cl[k][w]) for k in range(n)]), (C.c_size_t * n)(*[cl[k][w].shape[0] for k in range(n)])]
        Ts, Te = (TransformF * n)(), (TransformF * n)()
        it, ns = np.zeros(n, np.int32), np.zeros(n, np.int32)
        _chk(lib.dll.lio_odom_process_batch(H, n, *args, Ts, Te, it.ctypes.data_as(c_int32_p), ns.ctypes.data_as(c_int32_p)), "lio_odom_process_batch")
        return [dict(T_sum=Ts[k].to_np(), T_es=Te[k].to_np(), iterations=int(it[k]), num_selected=int(ns[k])) for k in range(n)]

    @staticmethod
    def process_batch_from_pp(handles, processors):
        """lio_odom_process_batch_from_pp (include/lio_frontend_batch.h): process_batch with the four clouds of handles[k] taken on the
        device from the last sweep of the PointProcessor processors[k] (one processor may feed several handles).  -> what process_batch
        returns."""
        n = len(handles)
        if n < 1 or len(processors) != n:
            raise LioError("process_batch_from_pp: one processor per handle, at least one handle")
        lib = handles[0].lib
        H = (C.c_void_p * n)(*[h.h for h in handles])
        P = (C.c_void_p * n)(*[p.h for p in processors])
        Ts, Te = (TransformF * n)(), (TransformF * n)()
        it, ns = np.zeros(n, np.int32), np.zeros(n, np.int32)
        _chk(lib.dll.lio_odom_process_batch_from_pp(H, P, n, Ts, Te, it.ctypes.data_as(c_int32_p), ns.ctypes.data_as(c_int32_p)),
             "lio_odom_process_batch_from_pp")
        return [dict(T_sum=Ts[k].to_np(), T_es=Te[k].to_np(), iterations=int(it[k]), num_selected=int(ns[k])) for k in range(n)]

    def iteration_trace(self):
        """lio_odom_get_iteration_trace: transform_es_ after every iteration of the last step (rows: q xyzw, p) and kz."""
        n = self.lib.dll.lio_odom_get_iteration_trace(self.h, None, 0, None)
        if n < 0:
            raise LioError(f"lio_odom_get_iteration_trace -> {n}")
        tr = (TransformF * max(n, 1))()
        kz = C.c_int(0)
        n = self.lib.dll.lio_odom_get_iteration_trace(self.h, tr, max(n, 1), C.byref(kz))
        return np.frombuffer(tr, dtype=np.float32).reshape(-1, 7)[:n].copy(), kz.value

    def enable(self, on):
        _chk(self.lib.dll.lio_odom_enable(self.h, 1 if on else 0), "lio_odom_enable")

    def full_to_end(self, xyzi):
        """lio_odom_full_to_end (include/lio_full_cloud.h): TransformToEnd(full_cloud_), PointOdometry.cc:261-292 at :725-730."""
        c = _f32(xyzi).reshape(-1, 4)
        out = np.zeros_like(c)
        _chk(self.lib.dll.lio_odom_full_to_end(self.h, _fp(c), c.shape[0], _fp(out)), "lio_odom_full_to_end")
        return out

    def last_cloud(self, which):
        n = self.lib.dll.lio_odom_get_last_cloud(self.h, which, None)
        out = np.zeros((n, 4), dtype=np.float32)
        if n:
            self.lib.dll.lio_odom_get_last_cloud(self.h, which, _fp(out))
        return out


class Estimator:
    def __init__(self, lib: LioLib, cfg: EstConfig):
        self.lib = lib
        self.cfg = cfg
        self.W = cfg.window_size
        self.h = lib.dll.lio_est_create(C.byref(cfg))
        if not self.h:
            raise LioError("lio_est_create failed")

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.dll.lio_est_destroy(self.h)
            self.h = None

    def process_imu(self, dt, acc, gyr, stamp):
        _chk(self.lib.dll.lio_est_process_imu(self.h, dt, _dp(_f64(acc)), _dp(_f64(gyr)), stamp), "lio_est_process_imu")

    def process_imu_batch(self, dt, acc, gyr, stamp):
        """All IMU samples of one laser interval in one call (the loop of Estimator::ProcessEstimation)."""
        dt, stamp = _f64(dt).reshape(-1), _f64(stamp).reshape(-1)
        acc, gyr = _f64(acc).reshape(-1, 3), _f64(gyr).reshape(-1, 3)
        assert acc.shape[0] == gyr.shape[0] == dt.shape[0] == stamp.shape[0]
        _chk(self.lib.dll.lio_est_process_imu_batch(self.h, dt.shape[0], _dp(dt), _dp(acc), _dp(gyr), _dp(stamp)), "lio_est_process_imu_batch")

    def process_laser_odom(self, T: TransformF, surf, corner, stamp):
        surf = _f32(surf).reshape(-1, 4)
        corner = _f32(corner).reshape(-1, 4)
        rep = SolveReport()
        _chk(
            self.lib.dll.lio_est_process_laser_odom(self.h, C.byref(T), _fp(surf), surf.shape[0], _fp(corner), corner.shape[0], stamp, C.byref(rep)),
            "lio_est_process_laser_odom",
        )
        return rep

    def process_compact(self, compact, stamp):
        """Estimator::ProcessCompactData -> (transform_to_init (q, p), SolveReport)."""
        data = _f32(compact).reshape(-1, 4)
        rep = SolveReport()
        T = TransformF()
        _chk(self.lib.dll.lio_est_process_compact(self.h, _fp(data), data.shape[0], stamp, C.byref(T), C.byref(rep)), "lio_est_process_compact")
        return T.to_np(), rep

    EVENTS = ("skipped", "filling", "init_failed", "initialised", "solved")

    def stage(self):
        st, cb, ex, ev = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        R, g = np.zeros((3, 3)), np.zeros(3)
        _chk(self.lib.dll.lio_est_get_stage(self.h, C.byref(st), C.byref(cb), C.byref(ex), C.byref(ev), _dp(R), _dp(g)), "lio_est_get_stage")
        return dict(inited=bool(st.value), cir_buf_count=cb.value, extrinsic_stage=ex.value, event=self.EVENTS[ev.value], R_WI=R, g_vec=g)

    def push_frame(self, T: TransformF, surf, corner, stamp):
        surf = _f32(surf).reshape(-1, 4)
        corner = _f32(corner).reshape(-1, 4)
        _chk(self.lib.dll.lio_est_push_frame(self.h, C.byref(T), _fp(surf), surf.shape[0], _fp(corner), corner.shape[0], stamp), "lio_est_push_frame")

    def solve(self):
        rep = SolveReport()
        _chk(self.lib.dll.lio_est_solve_optimization(self.h, C.byref(rep)), "lio_est_solve_optimization")
        return rep

    def slide(self):
        _chk(self.lib.dll.lio_est_slide_window(self.h), "lio_est_slide_window")

    # ---- include/lio_ext.h (the product only)
    def map(self):
        """The estimator's PointMapping base as a PointMapping object (borrowed: it lives as long as this estimator)."""
        h = self.lib.dll.lio_est_map(self.h)
        if not h:
            raise LioError("lio_est_map failed")
        return PointMapping.borrowed(self.lib, h, self)

    def set_map_refresh(self, on):
        _chk(self.lib.dll.lio_est_set_map_refresh(self.h, 1 if on else 0), "lio_est_set_map_refresh")

    # ---- include/lio_est_wide.h (the product only)
    def set_device_solve_limit(self, max_opt_window):
        """the largest optimisation window of this handle the device loop takes: 6 (default) or 7"""
        _chk(self.lib.dll.lio_est_set_device_solve_limit(self.h, int(max_opt_window)), f"lio_est_set_device_solve_limit({max_opt_window})")

    def device_solve_limit(self):
        rc = self.lib.dll.lio_est_get_device_solve_limit(self.h)
        if rc < 0:
            raise LioError(f"lio_est_get_device_solve_limit failed with code {rc}")
        return int(rc)

    def refresh_map(self):
        """Estimator.cc:703-708 after a solve, before the slide -> 1 the map was updated, 0 masked / ring not full."""
        rc = self.lib.dll.lio_est_refresh_map(self.h)
        if rc < 0:
            raise LioError(f"lio_est_refresh_map failed with code {rc}")
        return rc

    def last_map_refresh(self):
        """The arguments of the last refresh_map (test hook) or None before the first one."""
        ap, nv = C.c_int(0), C.c_int(0)
        T = TransformF()
        cen = (C.c_int * 3)()
        valid = np.zeros(125, dtype=np.uint32)
        nc, ns = C.c_size_t(0), C.c_size_t(0)
        vp = valid.ctypes.data_as(C.POINTER(C.c_uint32))
        fn = self.lib.dll.lio_est_get_last_map_refresh
        rc = fn(self.h, C.byref(ap), C.byref(T), cen, vp, C.byref(nv), C.byref(nc), None, C.byref(ns), None)
        if rc != 0:
            return None
        corner, surf = np.zeros((nc.value, 4), np.float32), np.zeros((ns.value, 4), np.float32)
        _chk(fn(self.h, None, None, None, None, None, None, _fp(corner) if nc.value else None, None, _fp(surf) if ns.value else None),
             "lio_est_get_last_map_refresh")
        return dict(applied=ap.value, T=T.to_np(), cube_center=list(cen), valid_idx=valid[:nv.value].copy(), corner=corner, surf=surf)

    # ---- include/lio_full_cloud.h (the product only)
    def set_full_cloud(self, on):
        _chk(self.lib.dll.lio_est_set_full_cloud(self.h, 1 if on else 0), "lio_est_set_full_cloud")

    def full_stack(self, frame):
        """lio_est_get_full_stack -> (points, LIO_FULL_* state) of window frame `frame`, or (empty, None) for a frame without an entry."""
        st = C.c_int(0)
        n = self.lib.dll.lio_est_get_full_stack(self.h, frame, None, C.byref(st))
        out = np.zeros((n, 4), dtype=np.float32)
        if n:
            m = self.lib.dll.lio_est_get_full_stack(self.h, frame, _fp(out), None)
            assert m == n
        return out, (st.value or None)

    def full_transform_es(self, frame):
        """The transform_es_ kept with the entry (test hook) as (q xyzw, p)."""
        T = TransformF()
        _chk(self.lib.dll.lio_est_get_full_transform_es(self.h, frame, C.byref(T)), "lio_est_get_full_transform_es")
        return T.to_np()

    def registered_full(self, frame):
        """lio_est_get_registered_full -> ((q xyzw, p) lidar pose of the frame, its corrected full cloud mapped into the world)."""
        T, n = TransformF(), C.c_size_t(0)
        _chk(self.lib.dll.lio_est_get_registered_full(self.h, frame, C.byref(T), C.byref(n), None), "lio_est_get_registered_full")
        out = np.zeros((n.value, 4), dtype=np.float32)
        if n.value:
            _chk(self.lib.dll.lio_est_get_registered_full(self.h, frame, None, None, _fp(out)), "lio_est_get_registered_full")
        return T.to_np(), out

    def sync(self):
        """Wait for the handle's deferred work (the marginalization worker of the product)."""
        _chk(self.lib.dll.lio_est_sync(self.h), "lio_est_sync")

    def set_window(self, Ps, Rs, Vs, Bas, Bgs, g_vec):
        n = self.W + 1
        Ps, Rs, Vs, Bas, Bgs = (_f64(a) for a in (Ps, Rs, Vs, Bas, Bgs))
        assert Ps.shape == (n, 3) and Rs.shape == (n, 3, 3)
        _chk(self.lib.dll.lio_est_set_window(self.h, n, _dp(Ps), _dp(Rs), _dp(Vs), _dp(Bas), _dp(Bgs), _dp(_f64(g_vec))), "lio_est_set_window")

    def get_window(self):
        n = self.W + 1
        Ps, Rs, Vs, Bas, Bgs = np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
        T = TransformF()
        _chk(self.lib.dll.lio_est_get_window(self.h, n, _dp(Ps), _dp(Rs), _dp(Vs), _dp(Bas), _dp(Bgs), C.byref(T)), "lio_est_get_window")
        q, p = T.to_np()
        return dict(Ps=Ps, Rs=Rs, Vs=Vs, Bas=Bas, Bgs=Bgs, q_lb=q, t_lb=p)

    def set_surf_stack(self, frame, xyzi):
        xyzi = _f32(xyzi).reshape(-1, 4)
        _chk(self.lib.dll.lio_est_set_surf_stack(self.h, frame, _fp(xyzi), xyzi.shape[0]), "lio_est_set_surf_stack")

    def get_surf_stack(self, frame):
        n = self.lib.dll.lio_est_get_surf_stack(self.h, frame, None)
        out = np.zeros((n, 4), dtype=np.float32)
        if n:
            self.lib.dll.lio_est_get_surf_stack(self.h, frame, _fp(out))
        return out

    def set_preintegration(self, frame, acc0, gyr0, ba, bg, dt, acc, gyr):
        dt, acc, gyr = _f64(dt), _f64(acc), _f64(gyr)
        _chk(
            self.lib.dll.lio_est_set_preintegration(
                self.h, frame, _dp(_f64(acc0)), _dp(_f64(gyr0)), _dp(_f64(ba)), _dp(_f64(bg)), _dp(dt), _dp(acc), _dp(gyr), dt.shape[0]
            ),
            "lio_est_set_preintegration",
        )

    def begin_frame(self, acc_last, gyr_last):
        _chk(self.lib.dll.lio_est_begin_frame(self.h, _dp(_f64(acc_last)), _dp(_f64(gyr_last))), "lio_est_begin_frame")

    def build_local_map(self):
        _chk(self.lib.dll.lio_est_build_local_map(self.h), "lio_est_build_local_map")

    def local_map(self):
        n = self.lib.dll.lio_est_get_local_map(self.h, None)
        out = np.zeros((n, 4), dtype=np.float32)
        if n:
            self.lib.dll.lio_est_get_local_map(self.h, _fp(out))
        return out

    def features(self, frame):
        n = self.lib.dll.lio_est_get_features(self.h, frame, None, None, None)
        pt, co, sc = np.zeros((n, 3)), np.zeros((n, 4)), np.zeros(n)
        if n:
            self.lib.dll.lio_est_get_features(self.h, frame, _dp(pt), _dp(co), _dp(sc))
        return pt, co, sc

    def eval_lidar_moments(self, Rt):
        """Rt: (n_passes, Wo, 12) T_{pivot<-i} (R row-major, t) -> (moments (n_passes, Wo, 258): S 16x16 row-major, cost, count;
        path of the last pass: 0 MFMA launch pair, 2 resident kernel, -1 the oracle)"""
        Rt = _f64(Rt)
        n_passes, wo = Rt.shape[0], Rt.shape[1]
        out = np.zeros((n_passes, wo, 258))
        path = C.c_int(-3)
        _chk(self.lib.dll.lio_est_eval_lidar_moments(self.h, n_passes, _dp(Rt), _dp(out), C.byref(path)), "lio_est_eval_lidar_moments")
        return out, path.value

    def force_moments_per_lane(self, per_lane):
        """residuals per lane of the resident moments kernel for later solves and eval_lidar_moments: 1 / 2 / 4 / 8, 0 = chosen per window"""
        _chk(self.lib.dll.lio_est_force_moments_per_lane(self.h, int(per_lane)), "lio_est_force_moments_per_lane")

    def set_max_num_iterations(self, n):
        """test hook: max_num_iterations of the handle's later solves (0: stop behind the first linearisation)"""
        _chk(self.lib.dll.lio_est_set_max_num_iterations(self.h, int(n)), "lio_est_set_max_num_iterations")

    def laser_odom_transform(self):
        T = TransformF()
        _chk(self.lib.dll.lio_est_get_laser_odom_transform(self.h, C.byref(T)), "lio_est_get_laser_odom_transform")
        return T.to_np()

    def prior(self):
        n = self.lib.dll.lio_est_get_prior(self.h, None, None, None, None)
        if n <= 0:
            return None
        JtJ, Jtr = np.zeros((n, n)), np.zeros(n)
        ln = C.c_int(0)
        self.lib.dll.lio_est_get_prior(self.h, None, None, None, C.byref(ln))
        x0 = np.zeros(ln.value)
        self.lib.dll.lio_est_get_prior(self.h, _dp(JtJ), _dp(Jtr), _dp(x0), C.byref(ln))
        return dict(n=n, JtJ=JtJ, Jtr=Jtr, x0=x0)

    def prior_factor(self):
        """linearized_jacobians / linearized_residuals / keep_block_data of the current prior (None when there is none)."""
        n = self.lib.dll.lio_est_get_prior_factor(self.h, None, None, None, None)
        if n <= 0:
            return None
        ln = C.c_int(0)
        self.lib.dll.lio_est_get_prior_factor(self.h, None, None, None, C.byref(ln))
        J, r, x0 = np.zeros((n, n)), np.zeros(n), np.zeros(ln.value)
        self.lib.dll.lio_est_get_prior_factor(self.h, _dp(J), _dp(r), _dp(x0), C.byref(ln))
        return dict(n=n, lin_jac=J, lin_res=r, x0=x0)

    def set_prior_factor(self, pf):
        J, r, x0 = _f64(pf["lin_jac"]), _f64(pf["lin_res"]), _f64(pf["x0"])
        _chk(self.lib.dll.lio_est_set_prior_factor(self.h, int(pf["n"]), _dp(J), _dp(r), _dp(x0), x0.shape[0]), "lio_est_set_prior_factor")

    def set_extrinsic(self, q_xyzw, p):
        T = TransformF.make(q_xyzw, p)
        _chk(self.lib.dll.lio_est_set_extrinsic(self.h, C.byref(T)), "lio_est_set_extrinsic")

    def set_factor_sharding_rccl(self, comm):
        """comm: capi.Rccl or None.  The all-reduce of the per-shard moments then runs inside the library (ncclAllReduce on the
        estimator's stream)."""
        self._rccl = comm   # keep the communicator alive as long as the estimator uses it
        _chk(self.lib.dll.lio_est_set_factor_sharding_rccl(self.h, comm.h if comm is not None else None), "lio_est_set_factor_sharding_rccl")

    def set_factor_sharding(self, rank, world, allreduce_numpy):
        """`allreduce_numpy(buf: np.ndarray[float64])` must sum `buf` in place over all ranks (e.g. torch.distributed)."""
        ALLREDUCE = C.CFUNCTYPE(C.c_int, c_double_p, C.c_int, C.c_void_p)

        def _cb(ptr, count, _user):
            try:
                buf = np.ctypeslib.as_array(ptr, shape=(count,))
                allreduce_numpy(buf)
                return 0
            except Exception:  # noqa: BLE001 - must not propagate through the C frame
                return 1

        self._allreduce_cb = ALLREDUCE(_cb) if (world > 1 and allreduce_numpy is not None) else None  # keep alive
        fn = C.cast(self._allreduce_cb, C.c_void_p) if self._allreduce_cb else None
        _chk(self.lib.dll.lio_est_set_factor_sharding(self.h, rank, world, fn, None), "lio_est_set_factor_sharding")

    def bench_batched_moments(self, n_windows, reps=20):
        """One moments launch over n_windows copies of the current window's lidar factors -> (avg ms, algorithmic bytes)."""
        ms, b = np.zeros(1), np.zeros(1)
        _chk(self.lib.dll.lio_est_bench_batched_moments(self.h, int(n_windows), int(reps), _dp(ms), _dp(b)), "lio_est_bench_batched_moments")
        return float(ms[0]), float(b[0])

    def enable_kernel_timing(self, on=True):
        """on: False/0 stop, True/1 every launch, N > 1 every N-th launch of each kernel kind."""
        _chk(self.lib.dll.lio_est_enable_kernel_timing(self.h, int(on)), "lio_est_enable_kernel_timing")

    def kernel_timing(self, name):
        t, b = np.zeros(1), np.zeros(1)
        n = self.lib.dll.lio_est_get_kernel_timing(self.h, name.encode(), _dp(t), _dp(b))
        return dict(launches=int(n), total_ms=float(t[0]), algorithmic_bytes=float(b[0]))

    def snapshot(self):
        _chk(self.lib.dll.lio_est_snapshot(self.h), "lio_est_snapshot")

    def restore(self):
        _chk(self.lib.dll.lio_est_restore(self.h), "lio_est_restore")

    def copy_snapshot_of(self, src):
        """this handle's snapshot <- a copy of src's (lio_est_copy_snapshot)"""
        _chk(self.lib.dll.lio_est_copy_snapshot(self.h, src.h), "lio_est_copy_snapshot")

    def solve_restored(self, steps):
        """`steps` x (restore + SolveOptimization) inside the library -> the last solve's report"""
        rep = SolveReport()
        _chk(self.lib.dll.lio_est_solve_restored(self.h, int(steps), C.byref(rep)), "lio_est_solve_restored")
        return rep


class EstimatorBatch:
    """lio_est_batch: B estimators solved together, every stage one launch over all windows (include/lio_c.h).  The batch adopts
    the estimators; they must outlive it (this object keeps them referenced)."""

    def __init__(self, lib: LioLib, estimators):
        self.lib = lib
        self.members = list(estimators)
        arr = (C.c_void_p * len(self.members))(*[e.h for e in self.members])
        self.h = lib.dll.lio_est_batch_create(arr, len(self.members))
        if not self.h:
            raise LioError("lio_est_batch_create failed (null / duplicate / already adopted window, or no device)")

    def close(self):
        if getattr(self, "h", None):
            self.lib.dll.lio_est_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def __len__(self):
        return int(self.lib.dll.lio_est_batch_size(self.h))

    def solve(self):
        reps = (SolveReport * len(self.members))()
        _chk(self.lib.dll.lio_est_batch_solve(self.h, reps), "lio_est_batch_solve")
        return list(reps)

    def solve_restored(self, steps):
        reps = (SolveReport * len(self.members))()
        _chk(self.lib.dll.lio_est_batch_solve_restored(self.h, int(steps), reps), "lio_est_batch_solve_restored")
        return list(reps)

    def sync(self):
        _chk(self.lib.dll.lio_est_batch_sync(self.h), "lio_est_batch_sync")

    # ---- include/lio_est_push_batch.h (tests and tools)
    @staticmethod
    def frames(items):
        """items: per window (TransformF, surf, corner, stamp) -> (EstFrame array, the arrays it points into)"""
        arr = (EstFrame * max(len(items), 1))()
        keep = []
        for k, (T, surf, corner, stamp) in enumerate(items):
            s, c = _f32(surf).reshape(-1, 4), _f32(corner).reshape(-1, 4)
            keep += [s, c]
            arr[k].transform_in = T
            arr[k].surf_xyzi, arr[k].n_surf = (_fp(s) if s.shape[0] else None), s.shape[0]
            arr[k].corner_xyzi, arr[k].n_corner = (_fp(c) if c.shape[0] else None), c.shape[0]
            arr[k].stamp = stamp
        return arr, keep

    def push_frames(self, items):
        """lio_est_batch_push_frames: lio_est_push_frame of every window; items as frames() takes them, one per window"""
        assert len(items) == len(self.members)
        arr, keep = self.frames(items)
        _chk(self.lib.dll.lio_est_batch_push_frames(self.h, arr), "lio_est_batch_push_frames")

    def slide(self):
        _chk(self.lib.dll.lio_est_batch_slide_windows(self.h), "lio_est_batch_slide_windows")

    def process_laser_odom(self, items):
        """lio_est_batch_process_laser_odom -> one SolveReport per window"""
        assert len(items) == len(self.members)
        arr, keep = self.frames(items)
        reps = (SolveReport * len(self.members))()
        _chk(self.lib.dll.lio_est_batch_process_laser_odom(self.h, arr, reps), "lio_est_batch_process_laser_odom")
        return list(reps)

    def push_stats(self):
        out = (C.c_int * 8)()
        _chk(self.lib.dll.lio_est_batch_push_stats(self.h, out), "lio_est_batch_push_stats")
        return dict(zip(PUSH_STATS, [int(v) for v in out[:5]]))

    # ---- include/lio_est_from_odom.h
    def _sources(self, odoms, pps, what):
        n = len(self.members)
        if len(odoms) != n or (pps is not None and len(pps) != n):
            raise LioError(f"{what}: one odometry (and one processor or None) per window")
        O = (C.c_void_p * n)(*[o.h for o in odoms])
        P = None if pps is None else (C.c_void_p * n)(*[None if p is None else p.h for p in pps])
        return O, P

    def push_frames_from_odom(self, odoms, pps, transforms, stamps):
        """lio_est_batch_push_frames_from_odom: push_frames with window w's clouds taken from the PointOdometry odoms[w] on the device, and
        its map's full cloud from the PointProcessor pps[w] (pps None, or a None entry: the full cloud stays as it is)."""
        n = len(self.members)
        O, P = self._sources(odoms, pps, "push_frames_from_odom")
        if len(transforms) != n or len(stamps) != n:
            raise LioError("push_frames_from_odom: one transform and one stamp per window")
        T = (TransformF * n)(*transforms)
        t = _f64(stamps).reshape(-1)
        _chk(self.lib.dll.lio_est_batch_push_frames_from_odom(self.h, O, P, T, _dp(t)), "lio_est_batch_push_frames_from_odom")

    def process_compact_from_odom(self, odoms, pps, stamps):
        """lio_est_batch_process_compact_from_odom -> (transform_to_init (q, p) per window, one SolveReport per window)"""
        n = len(self.members)
        O, P = self._sources(odoms, pps, "process_compact_from_odom")
        if len(stamps) != n:
            raise LioError("process_compact_from_odom: one stamp per window")
        t = _f64(stamps).reshape(-1)
        T, reps = (TransformF * n)(), (SolveReport * n)()
        _chk(self.lib.dll.lio_est_batch_process_compact_from_odom(self.h, O, P, _dp(t), T, reps), "lio_est_batch_process_compact_from_odom")
        return [T[k].to_np() for k in range(n)], list(reps)

    def from_odom_stats(self):
        out = (C.c_int * 8)()
        _chk(self.lib.dll.lio_est_batch_from_odom_stats(self.h, out), "lio_est_batch_from_odom_stats")
        return dict(zip(FROM_ODOM_STATS, [int(v) for v in out[:4]]))

    STAGES = ("filtered_map", "knn_grid", "feature_flags", "plane_coefficients", "newest_frame_state", "solver_state", "moments", "jacobi_scaling", "scaled_hessian", "new_prior")

    def set_option(self, name, value):
        """an execution choice of the batch (lio_est_batch_set_option): results do not depend on it"""
        _chk(self.lib.dll.lio_est_batch_set_option(self.h, name.encode(), int(value)), f"lio_est_batch_set_option({name}, {value})")

    def stage_digest(self, stage):
        """one 64-bit digest per window of what stage `stage` (index into STAGES) of the last solve left on the device"""
        out = (C.c_ulonglong * len(self.members))()
        _chk(self.lib.dll.lio_est_batch_stage_digest(self.h, int(stage), out), "lio_est_batch_stage_digest")
        return np.array(list(out), dtype=np.uint64)

    def moments(self, window):
        """(moments (Wo, 258), Rt (Wo, 12)) of window `window` at the point its last batch solve accepted"""
        wo = self.members[window].cfg.opt_window_size
        out, Rt = np.zeros((wo, 258)), np.zeros((wo, 12))
        _chk(self.lib.dll.lio_est_batch_get_moments(self.h, int(window), _dp(out), _dp(Rt)), "lio_est_batch_get_moments")
        return out, Rt

    DSL_SIZES = (208, 3387 + 2 * 80 * 80 + 2 * 80, 664 + 128 * 128, 10191)   # LIO_DSL_INTS, _PROBLEM, _STATE, _AUX

    def linearization(self, window):
        """lio_est_batch_get_linearization of window `window`, unpacked by the layout of include/lio_test_hooks.h into a dict:
        the problem the device loop read, its state and the aux row of its last launch A (at `cand`)."""
        ni, npb, nst, nax = self.DSL_SIZES
        ints = np.zeros(ni, np.int32)
        pbm, st, aux = np.zeros(npb), np.zeros(nst), np.zeros(nax)
        _chk(self.lib.dll.lio_est_batch_get_linearization(self.h, int(window), ints.ctypes.data_as(C.POINTER(C.c_int32)), _dp(pbm), _dp(st), _dp(aux)),
             "lio_est_batch_get_linearization")
        names = ["Wo", "n", "ex_col", "n_prior", "have_prior", "use_ex_prior", "n_keep", "it", "successful", "termination", "need_host", "ntrace", "n_pad",
                 "started", "done", "max_iterations"]
        d = {k: int(v) for k, v in zip(names, ints[:16])}
        wo, n, npr = d["Wo"], d["n"], d["n_prior"]
        d["prior_col"] = ints[16:16 + n].copy()
        d["keep"] = ints[144:194].reshape(10, 5)[:d["n_keep"]].copy()   # kind, index, size, offset, x0 offset
        d["present"] = ints[194:194 + wo].copy()
        d["prior_x0"] = pbm[0:90].copy()
        d["ex_prior_pos"], d["ex_prior_rot"] = pbm[90:93].copy(), pbm[93:97].copy()
        pims = []
        for i in range(wo):
            o = pbm[97 + 470 * i:97 + 470 * (i + 1)]
            pims.append(dict(dp=o[0:3].copy(), dq=o[3:7].copy(), dv=o[7:10].copy(), ba=o[10:13].copy(), bg=o[13:16].copy(), g=o[16:19].copy(),
                             sum_dt=float(o[19]), jac=o[20:245].reshape(15, 15).copy(), sqrt_info=o[245:470].reshape(15, 15).copy()))
        d["pim"] = pims
        m = pbm[3387:]
        d["prior"] = dict(JtJ=m[:npr * npr].reshape(npr, npr).copy(), lin_jac=m[npr * npr:2 * npr * npr].reshape(npr, npr).copy(),
                          lin_res=m[2 * npr * npr:2 * npr * npr + npr].copy(), Jtr0=m[2 * npr * npr + npr:2 * npr * npr + 2 * npr].copy())

        def params(v):
            return dict(pose=v[0:56].reshape(8, 7)[:wo + 1].copy(), sb=v[56:128].reshape(8, 9)[:wo + 1].copy(), ex=v[128:135].copy())

        d["x"], d["cand"] = params(st[0:135]), params(st[135:270])
        d["cand_Rt"] = st[270:354].reshape(7, 12)[:wo].copy()
        d["scale"], d["g"] = st[354:354 + n].copy(), st[482:482 + n].copy()
        d["costs0"] = st[610:614].copy()
        d["trace"] = st[614:614 + d["ntrace"]].copy()
        for k, nm in enumerate(["radius", "mu", "alpha", "dogleg_norm", "model_change", "step_norm", "x_cost", "x_norm", "gmax", "n_lidar"]):
            d[nm] = float(st[654 + k])
        d["Hcur"] = st[664:664 + n * n].reshape(n, n).copy()
        d["imu_out"] = aux[0:6524].reshape(7, 932)[:wo].copy()
        d["lmap"] = aux[6524:8260].reshape(7, 248)[:wo].copy()
        d["prior_out"] = aux[8260:8260 + npr + 1].copy()
        d["exprior_out"] = aux[8341:8385].copy()
        d["cand_moments"] = aux[8385:10191].reshape(7, 258)[:wo].copy()
        return d

    def clock(self):
        out = (C.c_double * 24)()
        _chk(self.lib.dll.lio_est_batch_get_clock(self.h, out), "lio_est_batch_get_clock")
        names = ["describe", "filter", "grid_features_rounds", "pack", "solve", "finish", "fallback", "total", "n_device", "rounds",
                 "dev_filter", "dev_grid", "dev_features", "dev_rounds", "dev_loop", "dev_marg", "dev_marg_wait", "aux_ms", "moments_ms", "step_ms", "aux_launches", "moments_launches", "step_launches"]
        return dict(zip(names, [float(v) for v in out]))


def load_hip() -> LioLib:
    """The product library.  Fails loudly when it has not been built; never substitutes the oracle."""
    return LioLib(HIP_LIB_PATH)
