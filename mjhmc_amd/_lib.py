"""ctypes binding of libmjhmc_hip.so (include/mjhmc_hip.h).

There is deliberately NO CPU fallback: if the HIP library is missing or no MI355X is visible the
product path raises.  (The NumPy restatement under oracle/ is test infrastructure and is never
imported from here.)
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
KERNEL_HEADERS = os.path.join(_HERE, 'csrc')     # jump_kernel.hpp / philox.hpp / functionals.hpp: what hipRTC compiles user expressions against
LIB_PATH = os.environ.get('MJHMC_HIP_LIB') or os.path.join(_HERE, 'lib', 'libmjhmc_hip.so')

# enums of include/mjhmc_hip.h
E_ISO_GAUSS, E_DIAG_GAUSS, E_ROUGH_WELL, E_MM_GAUSS, E_FUNNEL_NEAL, E_FUNNEL_REF, E_PRODUCT_OF_T, E_SPARSE_CODE, E_USER_EXPR, E_HOST, \
    E_LINEAR_EXPR = range(11)
F64, F32, BF16 = 0, 1, 2
MODE_MJHMC, MODE_CONTROL, MODE_CTHMC = 0, 1, 2
F_X, F_V, F_EX, F_EV, F_DEDX, F_HFLF, F_CACHE, F_DWELL, F_TRANS = range(9)
ERR_NO_DEVICE = -4
ERR_NONFINITE = -5
OP_SUM, OP_MIN, OP_MAX = 0, 1, 2
COMM_ID_BYTES = 128


class IterStats(ctypes.Structure):
    _fields_ = [('l', ctypes.c_int64), ('f', ctypes.c_int64), ('r', ctypes.c_int64), ('fl', ctypes.c_int64),
                ('n_cold', ctypes.c_int64), ('E_evals', ctypes.c_int64), ('dEdX_evals', ctypes.c_int64),
                ('nonfinite', ctypes.c_int32), ('L_used', ctypes.c_int32), ('eps_used', ctypes.c_double),
                ('n_flf_run', ctypes.c_int64)]


class EngineError(RuntimeError):
    pass


class EngineValueError(EngineError, ValueError):
    """MJHMC_ERR_INVALID from an entry point whose wrapper promises ValueError for a refused argument (check_args)"""


_P = ctypes.c_void_p
_dp = ctypes.POINTER(ctypes.c_double)

# name -> (restype, argtypes): the complete export list of include/mjhmc_hip.h
PROTOTYPES = {
    'mjhmc_last_error': (ctypes.c_char_p, []),
    'mjhmc_abi_version': (ctypes.c_int, []),
    'mjhmc_ctx_create': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_P)]),
    'mjhmc_ctx_destroy': (ctypes.c_int, [_P]),
    'mjhmc_ctx_info': (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(ctypes.c_uint64)]),
    'mjhmc_energy_create': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P, ctypes.c_size_t, ctypes.POINTER(_P)]),
    'mjhmc_energy_create_expr': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, _P, ctypes.c_size_t,
                                                ctypes.c_char_p, ctypes.POINTER(_P)]),
    'mjhmc_expr_check': (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]),
    'mjhmc_energy_create_expr_coupled': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                                        ctypes.c_char_p, _P, ctypes.c_size_t, ctypes.c_char_p,
                                                        ctypes.POINTER(_P)]),
    'mjhmc_energy_create_linear': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P, _P, ctypes.c_char_p, ctypes.c_char_p, _P,
                                                  ctypes.c_size_t, _P, ctypes.c_int, ctypes.c_char_p, _P]),
    'mjhmc_linear_check': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]),
    'mjhmc_energy_create_linear_tall': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int64, _P, _P, ctypes.c_char_p, ctypes.c_char_p,
                                                       _P, ctypes.c_size_t, _P, ctypes.c_int, ctypes.c_char_p, _P]),
    'mjhmc_linear_tall_check': (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]),
    'mjhmc_energy_create_linear_wide': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int64, _P, _P, ctypes.c_char_p, ctypes.c_char_p,
                                                       _P, ctypes.c_size_t, _P, ctypes.c_int, ctypes.c_char_p, _P]),
    'mjhmc_linear_wide_check': (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]),
    'mjhmc_energy_create_linear_grouped': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int64, _P, _P, ctypes.c_int, ctypes.c_int64,
                                                          ctypes.c_char_p, ctypes.c_char_p, _P, ctypes.c_size_t, _P, ctypes.c_int,
                                                          ctypes.c_char_p, _P]),
    'mjhmc_linear_grouped_check': (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_char_p,
                                                  ctypes.c_char_p, ctypes.c_char_p]),
    'mjhmc_linear_grouped_layout': (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, _P, _P]),
    'mjhmc_expr_check_coupled': (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                                ctypes.c_char_p, ctypes.c_char_p]),
    'mjhmc_energy_destroy': (ctypes.c_int, [_P]),
    'mjhmc_eval': (ctypes.c_int, [_P, ctypes.c_int, _P, ctypes.c_int64, _P, _P]),
    'mjhmc_sampler_create': (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, _P, _P,
                                            ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(_P)]),
    'mjhmc_sampler_destroy': (ctypes.c_int, [_P]),
    'mjhmc_set_hparams': (ctypes.c_int, [_P, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                         ctypes.c_double]),
    'mjhmc_iterate': (ctypes.c_int, [_P, ctypes.c_int, _P, _P, _P, ctypes.c_int, ctypes.POINTER(IterStats),
                                     ctypes.POINTER(ctypes.c_int)]),
    'mjhmc_host_set_energy': (ctypes.c_int, [_P, _P, _P]),
    'mjhmc_traj_begin': (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int64)]),
    'mjhmc_traj_step': (ctypes.c_int, [_P, _P, ctypes.c_int, _P]),
    'mjhmc_traj_finish': (ctypes.c_int, [_P, _P, _P, _P, _P, ctypes.c_int, ctypes.POINTER(IterStats)]),
    'mjhmc_checkpoint': (ctypes.c_int, [_P]),
    'mjhmc_restore': (ctypes.c_int, [_P]),
    'mjhmc_rollback': (ctypes.c_int, [_P]),
    'mjhmc_get_tick': (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    'mjhmc_set_tick': (ctypes.c_int, [_P, ctypes.c_uint64]),
    'mjhmc_advance_tick': (ctypes.c_int, [_P, ctypes.c_int64]),
    'mjhmc_reset_flf_cache': (ctypes.c_int, [_P]),
    'mjhmc_read': (ctypes.c_int, [_P, ctypes.c_int, _P, ctypes.c_size_t]),
    'mjhmc_write': (ctypes.c_int, [_P, ctypes.c_int, _P, ctypes.c_size_t]),
    'mjhmc_ring_alloc': (ctypes.c_int, [_P, ctypes.c_int]),
    'mjhmc_ring_slot_bytes': (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    'mjhmc_mem_info': (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    'mjhmc_iterate_download': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int64, ctypes.c_int64,
                                              ctypes.POINTER(IterStats), ctypes.POINTER(ctypes.c_int)]),
    'mjhmc_ring_read_dwell': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P]),
    'mjhmc_ring_gather': (ctypes.c_int, [_P, _P, ctypes.c_int64, _P]),
    'mjhmc_ring_read': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    'mjhmc_ring_moments': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_double, _dp, _dp]),
    'mjhmc_estimator_create': (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(_P)]),
    'mjhmc_estimator_destroy': (ctypes.c_int, [_P]),
    'mjhmc_estimator_set_shift': (ctypes.c_int, [_P, _P]),
    'mjhmc_estimator_accumulate': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'mjhmc_estimator_read': (ctypes.c_int, [_P, _dp, _P, _P, _P, ctypes.POINTER(ctypes.c_int64)]),
    'mjhmc_estimator_reset': (ctypes.c_int, [_P]),
    'mjhmc_ring_copy': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int]),
    'mjhmc_chainstats_create': (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(_P)]),
    'mjhmc_chainstats_destroy': (ctypes.c_int, [_P]),
    'mjhmc_chainstats_set_shift': (ctypes.c_int, [_P, _P]),
    'mjhmc_chainstats_accumulate': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'mjhmc_chainstats_read': (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), _dp, _P, _P, _P]),
    'mjhmc_chainstats_read_chains': (ctypes.c_int, [_P, ctypes.c_int, _P, _P, _P]),
    'mjhmc_chainstats_reset': (ctypes.c_int, [_P]),
    'mjhmc_histogram_create': (ctypes.c_int, [_P, ctypes.c_int, _P, _P, ctypes.c_double, ctypes.POINTER(_P)]),
    'mjhmc_histogram_destroy': (ctypes.c_int, [_P]),
    'mjhmc_histogram_accumulate': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'mjhmc_histogram_read': (ctypes.c_int, [_P, _P, _P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)]),
    'mjhmc_histogram_reset': (ctypes.c_int, [_P]),
    'mjhmc_pairhist_create': (ctypes.c_int, [_P, ctypes.c_int, _P, ctypes.c_int, _P, _P, ctypes.c_double, ctypes.POINTER(_P)]),
    'mjhmc_pairhist_create_on': (ctypes.c_int, [_P, ctypes.c_int, _P, ctypes.c_int, _P, _P, ctypes.c_double, ctypes.POINTER(_P)]),
    'mjhmc_pairhist_destroy': (ctypes.c_int, [_P]),
    'mjhmc_pairhist_accumulate': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'mjhmc_pairhist_read': (ctypes.c_int, [_P, _P, _P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)]),
    'mjhmc_pairhist_reset': (ctypes.c_int, [_P]),
    'mjhmc_functionals_check': (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]),
    'mjhmc_functionals_create': (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_char_p, _P, ctypes.c_size_t, ctypes.c_char_p,
                                                ctypes.POINTER(_P)]),
    'mjhmc_functionals_create_energy': (ctypes.c_int, [_P, ctypes.POINTER(_P)]),
    'mjhmc_functionals_create_linear': (ctypes.c_int, [_P, ctypes.c_int, _P, _P, ctypes.c_char_p, _P, ctypes.c_size_t,
                                                       ctypes.c_char_p, ctypes.POINTER(_P)]),
    'mjhmc_projections_check': (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p]),
    'mjhmc_functionals_destroy': (ctypes.c_int, [_P]),
    'mjhmc_functionals_info': (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]),
    'mjhmc_functionals_ring_alloc': (ctypes.c_int, [_P, ctypes.c_int]),
    'mjhmc_functionals_evaluate': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'mjhmc_functionals_read': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P]),
    'mjhmc_estimator_create_on': (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(_P)]),
    'mjhmc_chainstats_create_on': (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(_P)]),
    'mjhmc_histogram_create_on': (ctypes.c_int, [_P, ctypes.c_int, _P, _P, ctypes.c_double, ctypes.POINTER(_P)]),
    'mjhmc_occupancy_create': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P, _P, ctypes.c_double, ctypes.POINTER(_P)]),
    'mjhmc_occupancy_create_on': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P, _P, ctypes.c_double, ctypes.POINTER(_P)]),
    'mjhmc_occupancy_destroy': (ctypes.c_int, [_P]),
    'mjhmc_occupancy_accumulate': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'mjhmc_occupancy_read': (ctypes.c_int, [_P, _P, _P, _P, _P, _P, ctypes.POINTER(ctypes.c_uint64), _P, _P, _P, _P,
                                            ctypes.POINTER(ctypes.c_int64)]),
    'mjhmc_occupancy_read_labels': (ctypes.c_int, [_P, ctypes.c_int, _P]),
    'mjhmc_occupancy_reset': (ctypes.c_int, [_P]),
    'mjhmc_occupancy_info': (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                            ctypes.POINTER(ctypes.c_int)]),
    'mjhmc_stein_create': (ctypes.c_int, [_P, ctypes.c_double, ctypes.POINTER(_P)]),
    'mjhmc_stein_evaluate': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int64, _P]),
    'mjhmc_stein_destroy': (ctypes.c_int, [_P]),
    'mjhmc_crossmoments_create': (ctypes.c_int, [_P, ctypes.POINTER(_P)]),
    'mjhmc_crossmoments_create_on': (ctypes.c_int, [_P, ctypes.POINTER(_P)]),
    'mjhmc_crossmoments_set_shift': (ctypes.c_int, [_P, _P]),
    'mjhmc_crossmoments_accumulate': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'mjhmc_crossmoments_read': (ctypes.c_int, [_P, _dp, _P, _P, _P, _P, _P, _P, ctypes.POINTER(ctypes.c_int64)]),
    'mjhmc_crossmoments_reset': (ctypes.c_int, [_P]),
    'mjhmc_crossmoments_info': (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    'mjhmc_crossmoments_destroy': (ctypes.c_int, [_P]),
    'mjhmc_pointwise_check': (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_char_p, ctypes.c_char_p]),
    'mjhmc_pointwise_create': (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_uint, ctypes.c_char_p, ctypes.POINTER(_P)]),
    'mjhmc_pointwise_info': (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64),
                                            ctypes.POINTER(ctypes.c_int)]),
    'mjhmc_pointwise_accumulate': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'mjhmc_pointwise_read': (ctypes.c_int, [_P, _dp, _P, _P, _P, _P, ctypes.POINTER(ctypes.c_int64)]),
    'mjhmc_pointwise_reset': (ctypes.c_int, [_P]),
    'mjhmc_pointwise_destroy': (ctypes.c_int, [_P]),
    'mjhmc_pointwise_grouped_check': (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_char_p,
                                                     ctypes.c_uint, ctypes.c_char_p]),
    'mjhmc_pointwise_create_grouped': (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_uint, ctypes.c_uint, ctypes.c_char_p,
                                                      ctypes.POINTER(_P)]),
    'mjhmc_influence_check': (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_char_p, ctypes.c_char_p]),
    'mjhmc_influence_create': (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_char_p,
                                              ctypes.POINTER(_P)]),
    'mjhmc_influence_set_shift': (ctypes.c_int, [_P, _P, _P]),
    'mjhmc_influence_info': (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64),
                                            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int),
                                            ctypes.POINTER(ctypes.c_int64)]),
    'mjhmc_influence_accumulate': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'mjhmc_influence_read': (ctypes.c_int, [_P, _dp, _P, _P, _P, _P, ctypes.POINTER(ctypes.c_int64)]),
    'mjhmc_influence_read_cross': (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int64, _P]),
    'mjhmc_influence_reset': (ctypes.c_int, [_P]),
    'mjhmc_influence_destroy': (ctypes.c_int, [_P]),
    'mjhmc_timegrid_create': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_double, ctypes.POINTER(_P)]),
    'mjhmc_timegrid_destroy': (ctypes.c_int, [_P]),
    'mjhmc_timegrid_accumulate': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'mjhmc_timegrid_progress': (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    'mjhmc_timegrid_read_clocks': (ctypes.c_int, [_P, _P, _P]),
    'mjhmc_timegrid_read': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    'mjhmc_timegrid_autocor': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    'mjhmc_timegrid_reset': (ctypes.c_int, [_P]),
    'mjhmc_leapfrog': (ctypes.c_int, [_P, ctypes.c_int, _P, _P, ctypes.c_int64, ctypes.c_double, ctypes.c_int, _P, _P, _P, _P, _P]),
    'mjhmc_ring_autocor': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    'mjhmc_autocor': (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _P]),
    'mjhmc_grid_lagcov': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P]),
    'mjhmc_ring_lagcov': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P]),
    'mjhmc_lagcov': (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _P, _P, _P]),
    'mjhmc_draw_from': (ctypes.c_int, [_P, _P, _P, ctypes.c_int64, _P, ctypes.POINTER(ctypes.c_int64)]),
    'mjhmc_min_idx': (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int64, _P]),
    'mjhmc_comm_unique_id': (ctypes.c_int, [_P]),
    'mjhmc_comm_create': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P, ctypes.POINTER(_P)]),
    'mjhmc_comm_destroy': (ctypes.c_int, [_P]),
    'mjhmc_comm_available': (ctypes.c_int, []),
    'mjhmc_comm_count': (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int)]),
    'mjhmc_comm_allreduce_i64': (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int]),
    'mjhmc_comm_allreduce_f64': (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int]),
    'mjhmc_comm_bcast': (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.c_int]),
    'mjhmc_comm_allgatherv': (ctypes.c_int, [_P, _P, _P, _P]),
    'mjhmc_comm_allgather_ring': (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    'mjhmc_comm_allgather_columns': (ctypes.c_int, [_P, _P, _P, ctypes.c_int64, _P, _P]),
    'mjhmc_last_timing': (ctypes.c_int, [_P, _dp, _dp, ctypes.POINTER(ctypes.c_int)]),
    'mjhmc_set_timing': (ctypes.c_int, [_P, ctypes.c_int]),
    'mjhmc_sync': (ctypes.c_int, [_P]),
}

# libmjhmc_hip_test.so only (csrc/Makefile: test_hooks; built with -DMJHMC_TEST_HOOKS): the SAME sources plus the
# environment A/B switches of the launch strategies, the failure-placing hook and the single-GPU gather hooks
TEST_HOOKS_PATH = os.path.join(_HERE, 'lib', 'libmjhmc_hip_test.so')
TEST_HOOK_PROTOTYPES = {
    'mjhmc_test_gather_ring_local': (ctypes.c_int, [ctypes.POINTER(_P), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    'mjhmc_test_gather_columns_local': (ctypes.c_int, [ctypes.POINTER(_P), ctypes.c_int, _P, _P, _P]),
    'mjhmc_test_ring_write_dwell': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int64, ctypes.c_double]),
    'mjhmc_test_ring_write': (ctypes.c_int, [_P, ctypes.c_int, _P]),
    'mjhmc_test_ring_fill_padding': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int]),
    'mjhmc_test_ring_fill_element_padding': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int]),
    'mjhmc_test_occupancy_part': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'mjhmc_test_timegrid_read_raw': (ctypes.c_int, [_P, ctypes.c_int, _P, ctypes.c_size_t]),
    'mjhmc_test_functionals_read_raw': (ctypes.c_int, [_P, ctypes.c_int, _P, ctypes.c_size_t]),
    'mjhmc_test_energy_observables_part': (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'mjhmc_test_device_math': (ctypes.c_int, [_P, ctypes.c_int, _P, _P, ctypes.c_int64, _P, _P]),
    'mjhmc_test_normal_pairs': (ctypes.c_int, [_P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _P]),
}

_lib = None
_hooks = None


def _attach(lib, protos):
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)          # AttributeError here == header/library mismatch
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """Load the shared library (once) and attach prototypes.  Raises EngineError when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError('libmjhmc_hip.so not found at %s -- build it with `make -C mjhmc_amd/csrc` '
                          '(or python -c "import __graft_entry__ as g; g.build()"). There is no CPU fallback.'
                          % LIB_PATH)
    _lib = _attach(ctypes.CDLL(LIB_PATH), PROTOTYPES)
    return _lib


def load_test_hooks():
    """The test build of the library (tests and measurement tools only; the product never loads it): pass it to
    engine.Context(device, lib=...)."""
    global _hooks
    if _hooks is None:
        if not os.path.exists(TEST_HOOKS_PATH):
            raise EngineError('libmjhmc_hip_test.so not found at %s -- `make -C mjhmc_amd/csrc test_hooks`' % TEST_HOOKS_PATH)
        _hooks = _attach(_attach(ctypes.CDLL(TEST_HOOKS_PATH), PROTOTYPES), TEST_HOOK_PROTOTYPES)
    return _hooks


def check(rc, lib=None):
    if rc != 0:
        msg = (lib or load()).mjhmc_last_error()
        raise EngineError('libmjhmc_hip: %s (status %d)' % (msg.decode() if msg else '?', rc))


def check_args(rc, lib=None):
    """``check``, with MJHMC_ERR_INVALID raised as a ValueError (that is an EngineError too) carrying the library's message"""
    if rc == -1:
        msg = (lib or load()).mjhmc_last_error()
        raise EngineValueError('libmjhmc_hip: %s (status %d)' % (msg.decode() if msg else '?', rc))
    check(rc, lib)


def as_f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError('expected shape %r, got %r' % (tuple(shape), a.shape))
    return a


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)
