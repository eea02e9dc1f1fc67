"""ctypes binding of libemi355x.so (the C ABI declared in include/emi355x.h).

There is no CPU fallback: if the shared library is missing, or it cannot find
a gfx950 device when a context is created, the caller gets an exception.
"""
import ctypes as C
import os

# torch ships its own libamdhip64 (same soname as /opt/rocm's).  Import torch
# first so that one HIP runtime serves both torch and libemi355x in this process.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libemi355x.so")

EMI_OK = 0
STATUS = {0: "EMI_OK", 1: "EMI_ERR_ARG", 2: "EMI_ERR_STATE", 3: "EMI_ERR_HIP",
          4: "EMI_ERR_NO_DEVICE", 5: "EMI_ERR_UNSUPPORTED", 6: "EMI_ERR_COMM"}

MODEL_POINTMASS2D, MODEL_QUADROTOR2D, MODEL_FIXEDWING12 = 0, 1, 2
MODEL_SOURCE = 100   # installed by emi_set_model_source
PATH_ELLIPSE, PATH_DISC, PATH_TRACK = 0, 1, 2
PATH_REC = 8
EVAL_NODES, EVAL_DEFECT, EVAL_ALL, EVAL_NOJAC = 1, 2, 3, 4
EVAL_KEEP_INVARIANT = 8   # the model-invariant VALS rows are in place: see emi_eval_dev in include/emi355x.h


class EmiError(RuntimeError):
    pass


class Layout(C.Structure):
    _fields_ = [("model", C.c_int), ("ns", C.c_int), ("nc", C.c_int), ("np", C.c_int),
                ("M", C.c_int), ("B", C.c_int), ("nres", C.c_int), ("nvals", C.c_int),
                ("nhess", C.c_int), ("real_bytes", C.c_int), ("px", C.c_int), ("py", C.c_int),
                ("t0", C.c_double), ("tf", C.c_double)]


class PassPlan(C.Structure):
    """emi_pass_plan_t: what the default dispatch does with a batch (include/emi355x.h, emi_plan_pass)"""
    _fields_ = [(n, C.c_int) for n in ("one_launch", "sw", "ksplit", "ring_stages", "cpart", "cx", "mfma_workgroups", "store_mode",
                                       "block_order", "tiles16", "piece", "tail", "k_tile", "column_tiles", "k_halves")]


_P = C.c_void_p
_D = C.POINTER(C.c_double)
_I = C.POINTER(C.c_int)


def _ptr_struct(name, fields):
    return type(name, (C.Structure,), {"_fields_": [(f, _P) for f in fields], "FIELDS": tuple(fields)})


# the argument groups of the emi_ipm_* calls (include/emi355x.h): device pointers in the _dev forms, host arrays in the _host forms
IpmPoint = _ptr_struct("IpmPoint", ("X", "U", "S", "E1", "E2"))
IpmDuals = _ptr_struct("IpmDuals", ("LamF", "Y", "ZL", "ZU", "VL", "VU", "W1", "W2"))
IpmStep = _ptr_struct("IpmStep", ("DZLam", "DS", "DY", "DE1", "DE2", "DZL", "DZU", "DVL", "DVU", "DW1", "DW2"))
IpmElim = _ptr_struct("IpmElim", ("Sigma", "SigT", "SigS", "RhatS", "Rt"))


class IpmBounds(C.Structure):
    _fields_ = [("zl", _P), ("zu", _P), ("nsets", C.c_int), ("cl", _D), ("cu", _D), ("cscale", _D)]


class IpmOptions(C.Structure):
    """emi_ipm_options_t: fields left at zero take solve_nlp's defaults"""
    _fields_ = [(n, C.c_double) for n in ("tol", "mu_init", "bound_push", "bound_frac", "rho_init", "acceptable_factor")] + \
               [(n, C.c_int) for n in ("max_iter", "acceptable_iter", "max_futile_escalations", "rules", "crawl_limit")] + \
               [("crawl_frac", C.c_double)]


class IpmResult(C.Structure):
    """emi_ipm_result_t: how one instance of emi_ipm_solve_shard_* ended"""
    _fields_ = [(n, C.c_int) for n in ("status", "iterations", "evaluations", "factorisations", "reflected_steps")] + \
               [(n, C.c_double) for n in ("cost", "kkt_error", "constr_viol", "emax", "mu", "rho")] + \
               [(n, C.c_int) for n in ("newton_steps", "restored_steps")]


class IpmRung(C.Structure):
    """emi_ipm_rung_t: one rung of emi_ipm_solve_ladder_*"""
    _fields_ = [("M", C.c_int), ("bd", IpmBounds), ("recs", _D), ("opt", IpmOptions), ("repair", C.c_int)]


class IpmRefine(C.Structure):
    """emi_ipm_refine_t: when an instance of emi_ipm_solve_refine_* retires"""
    _fields_ = [("ode_tol", C.c_double), ("first_check", C.c_int), ("ul", _D), ("uu", _D)]


class IpmRefineResult(C.Structure):
    """emi_ipm_refine_result_t: where and how one instance of emi_ipm_solve_refine_* retired"""
    _fields_ = [("rung", C.c_int), ("verdict", C.c_int), ("rungs_solved", C.c_int), ("err", C.c_double)]


class Start(C.Structure):
    """emi_start_t: which start emi_start_guess_* writes, and from what"""
    _fields_ = [("kind", C.c_int), ("nsets", C.c_int), ("xa", _D), ("xb", _D), ("box", _D), ("bend", C.c_double), ("clearance", C.c_double),
                ("grid", C.c_int), ("repair", C.c_int)]


class IpmRestart(C.Structure):
    """emi_ipm_restart_t: the starts of emi_ipm_solve_restart_* and who goes to the next one"""
    _fields_ = [("nstarts", C.c_int), ("starts", C.POINTER(Start)), ("patience", _I), ("retry_mask", C.c_int), ("flags", C.c_int)]


class IpmRestartResult(C.Structure):
    """emi_ipm_restart_result_t: which attempt of emi_ipm_solve_restart_* an instance's trajectory comes from, and how it ended"""
    _fields_ = [("attempt", C.c_int), ("attempts", C.c_int), ("level", C.c_int), ("refine", IpmRefineResult)]


START_LINE, START_BEND, START_PLANNED = range(3)
RESTART_DROP_FAILED = 1   # emi_ipm_restart_t.flags: a rung that fails ends the instance's climb at once
REFINE_MET, REFINE_NOT_MET, REFINE_FELL_BACK, REFINE_FAILED = range(4)
IPM_RULE_RESIDUAL = 1   # emi_ipm_options_t.rules: residual-based acceptance of the full step and the crawl rule
IPM_CONVERGED, IPM_ACCEPTABLE, IPM_MAX_ITER, IPM_LINE_SEARCH, IPM_INFEASIBLE, IPM_FACTOR, IPM_NOT_FINITE = range(7)

_PT, _DU, _ST, _EL, _BD = (C.POINTER(t) for t in (IpmPoint, IpmDuals, IpmStep, IpmElim, IpmBounds))

# every symbol include/emi355x.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "emi_abi_version": (C.c_int, []),
    "emi_status_string": (C.c_char_p, [C.c_int]),
    "emi_device_count": (C.c_int, [_I]),
    "emi_lgl": (C.c_int, [C.c_int, _D, _D, _D]),
    "emi_model_dims": (C.c_int, [C.c_int, _I, _I, _I]),
    "emi_edge_ellipse": (C.c_int, [C.c_double] * 4 + [_D]),
    "emi_track_centres": (C.c_int, [C.c_int, _D, _D, _D, C.c_int, _D, _D, _D]),
    "emi_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "emi_create_f32": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "emi_destroy": (C.c_int, [_P]),
    "emi_last_error": (C.c_char_p, [_P]),
    "emi_set_stream": (C.c_int, [_P, _P]),
    "emi_get_stream": (C.c_int, [_P, C.POINTER(_P)]),
    "emi_synchronize": (C.c_int, [_P]),
    "emi_set_mesh": (C.c_int, [_P, C.c_int, _D, _D, _D, C.c_double, C.c_double]),
    "emi_set_model": (C.c_int, [_P, C.c_int, _D, C.c_int, C.c_int]),
    "emi_set_model_source": (C.c_int, [_P, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, _I, C.c_int, _D, C.c_int, C.c_int]),
    "emi_check_model_source": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "emi_kkt_factor": (C.c_int, [_P, _D, _D, C.POINTER(C.c_ubyte), C.c_double, C.POINTER(C.c_int)]),
    "emi_kkt_factor_dev": (C.c_int, [_P, _P, _P, _P, C.c_double, C.POINTER(C.c_int)]),
    "emi_kkt_blocks_rows": (C.c_int, [_P, C.c_int, _I, _I, _I]),
    "emi_kkt_blocks_dev": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_double, _P, _P, C.c_int, _P, _P, _P, _P, _P]),
    "emi_kkt_blocks_host": (C.c_int, [_P, _D, _D, _D, _D, C.POINTER(C.c_ubyte), C.c_double, _D, _D, C.c_int, _I, _I, _D, _D, _D]),
    "emi_kkt_solve": (C.c_int, [_P, _D, C.c_int]),
    "emi_kkt_solve_dev": (C.c_int, [_P, _P, C.c_int]),
    "emi_ipm_reduce_dev": (C.c_int, [_P, _PT, _DU, _P, _P, _P, _BD, _P, _P, _P, _EL, _P]),
    "emi_ipm_expand_dev": (C.c_int, [_P, _PT, _DU, _P, _BD, _P, _EL, _P, _ST, _P]),
    "emi_ipm_trial_dev": (C.c_int, [_P, _PT, _ST, _P, _PT]),
    "emi_ipm_merit_dev": (C.c_int, [_P, _PT, _P, _P, _BD, _P, _P, C.c_int, _P]),
    "emi_ipm_accept_dev": (C.c_int, [_P, _PT, _PT, _DU, _ST, _BD, _P, _P, _P, _P]),
    "emi_ipm_error_dev": (C.c_int, [_P, _PT, _DU, _P, _P, _BD, _P, _P]),
    "emi_ipm_reduce_host": (C.c_int, [_P, _PT, _DU, _P, _P, _P, _BD, _P, _P, _P, _EL, _P]),
    "emi_ipm_expand_host": (C.c_int, [_P, _PT, _DU, _P, _BD, _P, _EL, _P, _ST, _P]),
    "emi_ipm_trial_host": (C.c_int, [_P, _PT, _ST, _P, _PT]),
    "emi_ipm_merit_host": (C.c_int, [_P, _PT, _P, _P, _BD, _P, _P, C.c_int, _P]),
    "emi_ipm_accept_host": (C.c_int, [_P, _PT, _PT, _DU, _ST, _BD, _P, _P, _P, _P]),
    "emi_ipm_error_host": (C.c_int, [_P, _PT, _DU, _P, _P, _BD, _P, _P]),
    "emi_ipm_start_dev": (C.c_int, [_P, C.c_int, _PT, _DU, _P, _BD, _P, C.c_double, C.c_double, _P, _P]),
    "emi_ipm_error_parts_dev": (C.c_int, [_P, _PT, _DU, _P, _P, _BD, _P, _P]),
    "emi_ipm_error_parts_host": (C.c_int, [_P, _PT, _DU, _P, _P, _BD, _P, _P]),
    "emi_ipm_keep_dev": (C.c_int, [_P, _PT, _DU, _PT, _DU, _P, C.c_int]),
    "emi_ipm_keep_host": (C.c_int, [_P, _PT, _DU, _PT, _DU, _P, C.c_int]),
    "emi_ipm_solve_shard_dev": (C.c_int, [_P, _P, _P, _BD, C.POINTER(IpmOptions), _P, _P, C.POINTER(IpmResult)]),
    "emi_ipm_solve_shard_host": (C.c_int, [_P, _P, _P, _BD, C.POINTER(IpmOptions), _P, _P, C.POINTER(IpmResult)]),
    "emi_prolong_matrix": (C.c_int, [C.c_int, _D, _D, C.c_int, _D, _D]),
    "emi_prolong_dev": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_int, _P]),
    "emi_repair_guess_dev": (C.c_int, [_P, _P]),
    "emi_ipm_solve_ladder_dev": (C.c_int, [_P, C.c_int, C.POINTER(IpmRung), C.c_double, C.c_double, _P, _P, _P, _P, _P, _P, C.POINTER(IpmResult)]),
    "emi_ipm_solve_ladder_host": (C.c_int, [_P, C.c_int, C.POINTER(IpmRung), C.c_double, C.c_double, _P, _P, _P, _P, _P, _P, C.POINTER(IpmResult)]),
    "emi_ode_error_operator": (C.c_int, [C.c_int, _D, _D, _D, _D, _D]),
    "emi_interp_dev": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, _P]),
    "emi_ode_error_dev": (C.c_int, [_P, _P, _P, _D, _D, _P, _P]),
    "emi_ode_error_host": (C.c_int, [_P, _P, _P, _D, _D, _P, _P]),
    "emi_ode_error_delay_operator": (C.c_int, [C.c_int, _D, _D, C.c_double, C.c_double, C.c_double, _D]),
    "emi_ode_error_total_dev": (C.c_int, [_P, _P, _P, _D, _D, _P, _P]),
    "emi_ode_error_total_host": (C.c_int, [_P, _P, _P, _D, _D, _P, _P]),
    "emi_ipm_refine_decide": (C.c_int, [C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, _I]),
    "emi_prolong_rows_dev": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P]),
    "emi_shard_move_dev": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, _I, C.POINTER(_P), _I, C.POINTER(_P), _I, C.c_int]),
    "emi_ipm_solve_refine_dev": (C.c_int, [_P, C.c_int, C.POINTER(IpmRung), C.c_double, C.c_double, C.POINTER(IpmRefine), _P, _P, C.c_int,
                                           _P, _P, _P, _P, C.POINTER(IpmResult), _D, C.POINTER(IpmRefineResult)]),
    "emi_ipm_solve_refine_host": (C.c_int, [_P, C.c_int, C.POINTER(IpmRung), C.c_double, C.c_double, C.POINTER(IpmRefine), _P, _P, C.c_int,
                                            _P, _P, _P, _P, C.POINTER(IpmResult), _D, C.POINTER(IpmRefineResult)]),
    "emi_ipm_restart_decide": (C.c_int, [C.c_int, C.c_int]),
    "emi_ipm_solve_restart_dev": (C.c_int, [_P, C.c_int, C.POINTER(IpmRung), C.c_double, C.c_double, C.POINTER(IpmRefine), C.POINTER(IpmRestart),
                                            _P, _P, C.c_int, _P, _P, _P, _P, C.POINTER(IpmResult), _D, C.POINTER(IpmRestartResult)]),
    "emi_ipm_solve_restart_host": (C.c_int, [_P, C.c_int, C.POINTER(IpmRung), C.c_double, C.c_double, C.POINTER(IpmRefine), C.POINTER(IpmRestart),
                                             _P, _P, C.c_int, _P, _P, _P, _P, C.POINTER(IpmResult), _D, C.POINTER(IpmRestartResult)]),
    "emi_plan_route": (C.c_int, [C.c_int, _D, _D, _D, C.c_double, C.c_int, C.c_int, _D, _D, _D, _I, _D, _I, _I]),
    "emi_start_guess_dev": (C.c_int, [_P, C.POINTER(Start), _P, _P]),
    "emi_start_guess_host": (C.c_int, [_P, C.POINTER(Start), _P, _P]),
    "emi_kkt_last_regularisation": (C.c_int, [_P, _D, _D]),
    "emi_kkt_factor_batch": (C.c_int, [C.c_int, C.POINTER(_P), C.POINTER(_D), C.POINTER(_D), C.POINTER(C.POINTER(C.c_ubyte)), _D, _I]),
    "emi_kkt_solve_batch": (C.c_int, [C.c_int, C.POINTER(_P), C.POINTER(_D)]),
    "emi_kkt_is_schur": (C.c_int, [_P]),
    "emi_kkt_solve_refined": (C.c_int, [_P, _D, C.c_double, C.c_int, _D, _I, _I, _I]),
    "emi_kkt_solve_refined_batch": (C.c_int, [C.c_int, C.POINTER(_P), C.POINTER(_D), _D, C.c_int, _D, _I, _I, _I]),
    "emi_kkt_lowrank": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int), _D, _D, C.POINTER(C.c_int)]),
    "emi_kkt_factor_shard_dev": (C.c_int, [_P, _P, _P, _P, _D, C.POINTER(C.c_ubyte), _I]),
    "emi_kkt_lowrank_shard_dev": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.POINTER(C.c_ubyte), _I]),
    "emi_kkt_solve_shard_dev": (C.c_int, [_P, _P, C.POINTER(C.c_ubyte)]),
    "emi_kkt_solve_refined_shard_dev": (C.c_int, [_P, _P, C.POINTER(C.c_ubyte), _D, C.c_int, _D, _I, _I, _I]),
    "emi_set_batch": (C.c_int, [_P, C.c_int]),
    "emi_set_model_params_batch": (C.c_int, [_P, _D, C.c_int, C.c_int]),
    "emi_get_model_params_batch": (C.c_int, [_P, _D, _I, _I]),
    "emi_set_path": (C.c_int, [_P, C.c_int, C.c_int, _D, C.c_int, C.c_int]),
    "emi_set_tracks": (C.c_int, [_P, C.c_int, C.c_int, _D, _D]),
    "emi_set_track_waypoints": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _I, _D, _D, _D]),
    "emi_tracks_from_waypoints_dev": (C.c_int, [_P, C.c_int, _P]),
    "emi_get_tracks": (C.c_int, [_P, _D, _D]),
    "emi_get_layout": (C.c_int, [_P, C.POINTER(Layout)]),
    "emi_jac_structure": (C.c_int, [_P, _I, _I]),
    "emi_invariant_rows": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_ubyte), _I]),
    "emi_dev_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "emi_dev_free": (C.c_int, [_P, _P]),
    "emi_h2d": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "emi_d2h": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "emi_eval_dev": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint]),
    "emi_eval_host": (C.c_int, [_P, _D, _D, _D, _D, _D, C.c_uint]),
    "emi_hess_dev": (C.c_int, [_P, _P, _P, _P, _P, C.c_double, _P]),
    "emi_hess_host": (C.c_int, [_P, _D, _D, _D, _D, C.c_double, _D]),
    "emi_lagr_grad_dev": (C.c_int, [_P, _P, _P, _P, C.c_double, _P]),
    "emi_lagr_grad_host": (C.c_int, [_P, _D, _D, _D, C.c_double, _D]),
    "emi_kkt_certificate_dev": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_double, _P, _P, C.c_int, _D, _D, _P, _P]),
    "emi_kkt_certificate_host": (C.c_int, [_P, _D, _D, _D, _D, C.c_double, _D, _D, C.c_int, _D, _D, _D, _D]),
    "emi_lagr_grad_total_dev": (C.c_int, [_P, _P, _P, _P, C.c_double, _P, _P]),
    "emi_lagr_grad_total_host": (C.c_int, [_P, _D, _D, _D, C.c_double, _D, _D]),
    "emi_kkt_certificate_total_dev": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_double, _P, _P, C.c_int, _D, _D, _P, _P, _P]),
    "emi_kkt_certificate_total_host": (C.c_int, [_P, _D, _D, _D, _D, C.c_double, _D, _D, C.c_int, _D, _D, _D, _D, _D]),
    "emi_timer_start": (C.c_int, [_P]),
    "emi_timer_stop": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "emi_profile_enable": (C.c_int, [_P, C.c_int]),
    "emi_profile_read": (C.c_int, [_P, C.POINTER(C.c_float), _I, C.POINTER(C.c_float), _I, C.POINTER(C.c_float), _I]),
    "emi_set_option": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "emi_last_path": (C.c_int, [_P, _I]),
    "emi_plan_pass": (C.c_int, [_P, C.c_int, C.POINTER(PassPlan)]),
    "emi_plan_pass_residency": (C.c_int, [_P, C.c_int, _I]),
    "emi_last_defect_kernel": (C.c_char_p, [_P]),
    "emi_debug_pass_roles": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "emi_debug_tile_order": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "emi_debug_pass_work": (C.c_int, [C.c_int] * 11 + [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]),
    "emi_debug_pass_work_uploads": (C.c_int, [_P, C.POINTER(C.c_ulonglong), _I]),
    "emi_set_delays": (C.c_int, [_P, C.c_int, C.c_int, C.c_double]),
    "emi_get_delays": (C.c_int, [_P, _I, _I, _I]),
    "emi_delay_matrix": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "emi_debug_operator_fragments": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "emi_debug_tile_order2": (C.c_int, [C.c_int] * 7 + [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "emi_comm_unique_id": (C.c_int, [_P]),
    "emi_comm_create": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "emi_comm_gather": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, _P]),
    "emi_comm_destroy": (C.c_int, [_P]),
    "emi_comm_last_error": (C.c_char_p, [_P]),
}

_lib = None


def load():
    """Load libemi355x.so (once) and type every entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EmiError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(or `make lib`) first; there is no CPU fallback")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError here = ABI mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status, ctx=None, what=""):
    if status == EMI_OK:
        return
    lib = load()
    msg = lib.emi_status_string(status).decode()
    if ctx:
        detail = lib.emi_last_error(ctx).decode()
        if detail:
            msg += ": " + detail
    raise EmiError(f"{what or 'libemi355x'}: {STATUS.get(status, status)} ({msg})")
