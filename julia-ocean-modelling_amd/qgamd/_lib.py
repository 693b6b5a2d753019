"""ctypes binding of lib/libqgmi355.so (the C-ABI declared in include/qg_mi355.h).

There is no fallback: if the HIP library is missing or fails to load, every entry point
raises.  The parity tests rely on that (a CPU fallback would void them).
"""
from __future__ import annotations

import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# QGMI355_LIB: alternative build of the same library (tuning experiments); never a fallback
LIB_PATH = os.environ.get("QGMI355_LIB") or os.path.join(PKG_DIR, "lib", "libqgmi355.so")

QG_OK = 0
QG_ERR_INVALID_ARG, QG_ERR_UNSUPPORTED, QG_ERR_HIP, QG_ERR_NOT_BOUND = -1, -2, -3, -4
QG_ERR_ALLOC, QG_ERR_RCCL, QG_ERR_NOT_CONVERGED = -5, -6, -7
QG_ENS_MAX_MEMBERS = 65535
QG_SPEC_LINES, QG_SPEC_MAX_STRIPS = 5, 64
QG_PROF_LINES = 12
QG_TRACERS_MAX, QG_TRC_LINES = 8, 6
QG_TRC_FORM_AUTO, QG_TRC_FORM_RING, QG_TRC_FORM_ONE_POINT = 0, 1, 2
QG_FLT_LINES, QG_FLOATS_MAX_PER_LAYER = 8, 1 << 26
QG_FLT_PSI, QG_FLT_ZETA = 0, 1
QG_TSTATS_MEAN, QG_TSTATS_EDDY = 0, 1
QG_TSTATS_FIELDS, QG_TSTATS_LAYER_FIELDS, QG_TSTATS_SUM_LINES = 26, 11, 12


def QG_TRC_FORM_RING_TILE(w, r):
    """The ring form with strips w columns wide (64, 128, 256) and r rows per workgroup."""
    return (int(w) << 16) | (int(r) << 4) | QG_TRC_FORM_RING


QG_XBUF_TO_NEXT, QG_XBUF_TO_PREV, QG_XBUF_FROM_PREV, QG_XBUF_FROM_NEXT = 0, 1, 2, 3
QG_SOLVER_SPECTRAL = 0
QG_F64, QG_F32 = 0, 1
QG_SOLVER_PCG = 1
QG_PRECOND_NONE = 0
QG_PRECOND_SPECTRAL = 1
QG_PRECOND_MULTIGRID = 2
QG_KEEP_ORDER_SLOT1, QG_KEEP_ORDER_SLOT1_DEFERRED = 2, 3
# qg_set_form (kernel-form selection, process-wide; 0 = automatic)
QG_FORM_TENDENCY, QG_FORM_TENDENCY_TILE, QG_FORM_ROW_SPLIT, QG_FORM_PCG_NO_CERTIFICATE = 0, 1, 2, 3
QG_TEND_AUTO, QG_TEND_RING, QG_TEND_DIRECT, QG_TEND_ONE_POINT = 0, 1, 2, 3
QG_TEND_KERNEL_RING, QG_TEND_KERNEL_PAIR, QG_TEND_KERNEL_DIRECT = 0, 1, 2
QG_SLOT_CALL_TENDENCY, QG_SLOT_CALL_SOLVE, QG_SLOT_CALL_SETTLE, QG_SLOT_CALL_CANONICALIZE = 0, 1, 2, 3
QG_SLOT_AFTER_NONE, QG_SLOT_AFTER_MOVE, QG_SLOT_AFTER_DEFER = 0, 1, 2
# qg_spectral_plan: the row families and the blocks of the solver's device memory, in order
(QG_SPEC_TWOPOINT, QG_SPEC_POW2, QG_SPEC_HALF, QG_SPEC_GEN, QG_SPEC_SPLIT, QG_SPEC_WIDE_SPLIT, QG_SPEC_WIDE_POW2,
 QG_SPEC_BLUESTEIN) = range(8)
QG_SPEC_BLOCK_NAMES = ("tw", "coef", "hot", "U", "ULS", "WLS", "UIN", "WIN", "dcpart", "rec", "grec", "EXT", "line",
                       "hline", "scal", "pinpart", "members", "tw2", "half_tmp", "perm", "bl_chirp", "bl_bhat",
                       "bl_tw", "bl_buf0", "bl_buf1")
QG_SPEC_BLOCKS = len(QG_SPEC_BLOCK_NAMES)


class QgParams(C.Structure):
    """Mirror of ``struct qg_params`` (field order and types must match the header)."""

    _fields_ = [
        ("H_1", C.c_double), ("H_2", C.c_double), ("beta", C.c_double), ("Lx", C.c_double),
        ("Ly", C.c_double), ("dt", C.c_double), ("T", C.c_double), ("U", C.c_double),
        ("M", C.c_int64), ("P", C.c_int64),
        ("dx", C.c_double), ("visc", C.c_double), ("r", C.c_double), ("R_d", C.c_double),
        ("initial_kick", C.c_double),
        ("P_fwd", C.c_double * 4),
        ("solver", C.c_int32), ("precond", C.c_int32),
        ("pcg_rtol", C.c_double),
        ("pcg_maxit", C.c_int32), ("chunk_rows", C.c_int32),
        ("dtype", C.c_int32), ("reserved0", C.c_int32),
        ("wind_tau0", C.c_double), ("wind_rho0", C.c_double),
    ]


class QgDiag(C.Structure):
    _fields_ = [("zeta_max", C.c_double * 2), ("zeta_min", C.c_double * 2), ("psi_max", C.c_double * 2),
                ("psi_min", C.c_double * 2), ("zeta_sum", C.c_double * 2), ("enstrophy", C.c_double * 2),
                ("energy", C.c_double * 2), ("interface", C.c_double), ("reserved", C.c_double)]


class QgMemberParams(C.Structure):
    """Mirror of ``struct qg_member_params`` (include/qg_mi355_sweep.h): one member's own values."""

    _fields_ = [("U", C.c_double), ("beta", C.c_double), ("r", C.c_double), ("visc", C.c_double),
                ("R_d", C.c_double), ("initial_kick", C.c_double), ("wind_tau0", C.c_double),
                ("reserved", C.c_double)]


class QgSpread(C.Structure):
    """Mirror of ``struct qg_spread`` (include/qg_mi355_stats.h): 16 doubles, 128 bytes."""

    _fields_ = [("zeta_var", C.c_double * 2), ("psi_var", C.c_double * 2), ("zeta_mean_sq", C.c_double * 2),
                ("psi_mean_sq", C.c_double * 2), ("energy_spread", C.c_double * 2),
                ("energy_mean", C.c_double * 2), ("step", C.c_double), ("nmembers", C.c_double),
                ("reserved", C.c_double * 2)]


class QgTracerParams(C.Structure):
    """Mirror of ``struct qg_tracer_params`` (include/qg_mi355_tracers.h): one tracer's layer (0 or
    1), diffusivity and imposed mean meridional gradient."""

    _fields_ = [("layer", C.c_int32), ("reserved", C.c_int32), ("kappa", C.c_double), ("gamma", C.c_double)]


class QgTendPlan(C.Structure):
    """Mirror of ``struct qg_tend_plan``: qg_tendency_plan's launch of one tendency."""

    _fields_ = [("kernel", C.c_int32), ("width", C.c_int32), ("threads", C.c_int32), ("rows", C.c_int32),
                ("chipfulls", C.c_int32), ("nx", C.c_int32), ("nyA", C.c_int32), ("nyB", C.c_int32),
                ("nz", C.c_int32), ("reserved", C.c_int32), ("blocks", C.c_int64)]


class QgSlotState(C.Structure):
    """Mirror of ``struct qg_slot_state``: what qg_slot_plan decides from."""

    _fields_ = [("heads", C.c_int32 * 3), ("keep_order", C.c_int32), ("distributed", C.c_int32),
                ("zcopy_pending", C.c_int32), ("can_defer", C.c_int32), ("reserved", C.c_int32)]


class QgSlotCall(C.Structure):
    """Mirror of ``struct qg_slot_call``: qg_slot_plan's plan of one call."""

    _fields_ = [("settle", C.c_int32), ("move", (C.c_int32 * 3) * 3), ("shift", C.c_int32 * 3),
                ("zeta_in", C.c_int32), ("psi_in", C.c_int32), ("f1_in", C.c_int32), ("f2_in", C.c_int32),
                ("zeta_out", C.c_int32), ("psi_out", C.c_int32), ("f_out", C.c_int32),
                ("fshift", C.c_int32 * 2), ("zeta_copy", C.c_int32), ("after", C.c_int32),
                ("next", QgSlotState)]


class QgSpecBlock(C.Structure):
    _fields_ = [("offset", C.c_int64), ("bytes", C.c_int64)]


class QgSpecPlan(C.Structure):
    """Mirror of ``struct qg_spec_plan``: qg_spectral_plan's plan of one direct solver."""

    _fields_ = [("family", C.c_int32), ("nrad", C.c_int32), ("rad", C.c_int32 * 16), ("L", C.c_int32),
                ("Nc", C.c_int32), ("KH", C.c_int32), ("KS", C.c_int32), ("carry_blocks", C.c_int32),
                ("carry_groups", C.c_int32), ("carry_variant", C.c_int32), ("fuse_pin", C.c_int32),
                ("npin", C.c_int32), ("row_groups", C.c_int32), ("bl_L", C.c_int32), ("bl_rows", C.c_int32),
                ("reserved", C.c_int32 * 2), ("length", C.c_int64), ("member_bytes", C.c_int64),
                ("total_bytes", C.c_int64), ("block", QgSpecBlock * QG_SPEC_BLOCKS)]


class QgStats(C.Structure):
    _fields_ = [("iters", C.c_int32 * 2), ("relres", C.c_double * 2), ("delta", C.c_double),
                ("pin", C.c_double)]


# host-transport callbacks (qg_allgather_fn, qg_sendrecv_fn)
AllgatherFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
SendrecvFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                         C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                         C.POINTER(C.c_int), C.c_void_p)

# (name, restype, argtypes) of every symbol include/qg_mi355.h and qg_mi355_ensemble.h declare
_vp, _dp, _i64, _i32 = C.c_void_p, C.c_void_p, C.c_int64, C.c_int
SIGNATURES = [
    ("qg_abi_version", C.c_int, []),
    ("qg_strerror", C.c_char_p, [C.c_int]),
    ("qg_default_params", None, [C.POINTER(QgParams)]),
    ("qg_create", C.c_int, [C.POINTER(QgParams), C.c_int, _vp, C.POINTER(_vp)]),
    ("qg_destroy", C.c_int, [_vp]),
    ("qg_bind_state", C.c_int, [_vp, _dp, _dp, _dp]),
    ("qg_initialise", C.c_int, [_vp, C.c_uint64, C.c_uint64]),
    ("qg_evolve_zeta", C.c_int, [_vp, _i64]),
    ("qg_evolve_psi", C.c_int, [_vp]),
    ("qg_step", C.c_int, [_vp, _i64]),
    ("qg_run", C.c_int, [_vp, _i64, _i64]),
    ("qg_slot", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    ("qg_set_slots", C.c_int, [_vp, C.c_int * 3]),
    ("qg_canonicalize", C.c_int, [_vp]),
    ("qg_set_keep_order", C.c_int, [_vp, C.c_int]),
    ("qg_get_stats", C.c_int, [_vp, C.POINTER(QgStats)]),
    ("qg_solver_stats", C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                  C.POINTER(C.c_double)]),
    ("qg_synchronize", C.c_int, [_vp]),
    ("qg_snapshot", C.c_int, [_vp, _vp, _vp]),
    ("qg_snapshot_wait", C.c_int, [_vp]),
    ("qg_diagnostics", C.c_int, [_vp, C.POINTER(QgDiag)]),
    ("qg_comm_unique_id", C.c_int, [C.c_char_p]),
    ("qg_comm_init", C.c_int, [_vp, C.c_int, C.c_int, C.c_char_p]),
    ("qg_comm_init_host", C.c_int, [_vp, C.c_int, C.c_int, AllgatherFn, SendrecvFn, _vp]),
    ("qg_comm_set_timeout", C.c_int, [_vp, C.c_double]),
    ("qg_set_overlap", C.c_int, [_vp, C.c_int]),
    ("qg_comm_set_halo_transport", C.c_int, [_vp, C.c_int]),
    ("qg_comm_set_gather_transport", C.c_int, [_vp, C.c_int]),
    ("qg_comm_probe", C.c_int, [_vp, C.c_int, C.POINTER(C.c_double)]),
    ("qg_set_pcg_sync", C.c_int, [_vp, C.c_int]),
    ("qg_pcg_certificate", C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_double)]),
    ("qg_comm_exchange_plan", C.c_int, [C.c_int, C.c_int, C.c_int * 2, C.c_int * 2, C.c_int * 2, C.c_int * 2]),
    ("qg_solver_create", C.c_int, [_i64, _i64, C.c_double, C.c_double * 2, C.c_int * 2,
                                   C.c_double * 4, C.c_double * 4, C.c_int, C.c_int, C.c_int, _vp,
                                   C.POINTER(_vp)]),
    ("qg_solver_solve", C.c_int, [_vp, _dp, _dp, _dp, _dp]),
    ("qg_solver_destroy", C.c_int, [_vp]),
    ("qg_set_form", C.c_int, [C.c_int, C.c_int]),
    ("qg_get_form", C.c_int, [C.c_int]),
    ("qg_tendency_plan", C.c_int, [_i64, C.c_int * 4, C.c_int, C.c_int, C.c_int, C.c_int, _i64,
                                   C.POINTER(QgTendPlan)]),
    ("qg_slot_plan", C.c_int, [C.POINTER(QgSlotState), C.c_int, _i64, C.POINTER(QgSlotCall)]),
    ("qg_spectral_plan", C.c_int, [_i64, _i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.POINTER(QgSpecPlan)]),
    ("qg_spectral_plan_permutation", C.c_int, [C.POINTER(QgSpecPlan), C.POINTER(C.c_int32)]),
    ("qg_laplace_5p", C.c_int, [_dp, _dp, _i64, _i64, C.c_double, _vp]),
    ("qg_cd", C.c_int, [_dp, _dp, _i64, _i64, C.c_double, _vp]),
    ("qg_arakawa_J", C.c_int, [_dp, _dp, _dp, _i64, _i64, C.c_double, _vp]),
    ("qg_fill_ghosts", C.c_int, [_dp, _i64, _i64, _vp]),
    # include/qg_mi355_ensemble.h
    ("qg_ens_create", C.c_int, [C.POINTER(QgParams), C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    ("qg_ens_destroy", C.c_int, [_vp]),
    ("qg_ens_members", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("qg_ens_bind_state", C.c_int, [_vp, _dp, _dp, _dp]),
    ("qg_ens_initialise", C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("qg_ens_step", C.c_int, [_vp, _i64]),
    ("qg_ens_run", C.c_int, [_vp, _i64, _i64]),
    ("qg_ens_slot", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    ("qg_ens_canonicalize", C.c_int, [_vp]),
    ("qg_ens_diagnostics", C.c_int, [_vp, C.POINTER(QgDiag)]),
    ("qg_ens_synchronize", C.c_int, [_vp]),
    # include/qg_mi355_sweep.h
    ("qg_member_params_default", C.c_int, [C.POINTER(QgParams), C.POINTER(QgMemberParams)]),
    ("qg_ens_create_sweep", C.c_int, [C.POINTER(QgParams), C.POINTER(QgMemberParams), C.c_int, C.c_int, _vp,
                                      C.POINTER(_vp)]),
    ("qg_ens_member_params", C.c_int, [_vp, C.c_int, C.POINTER(QgMemberParams)]),
    # include/qg_mi355_stats.h (records of qg_ens_run_recorded: a device pointer)
    ("qg_ens_moments", C.c_int, [_vp, C.c_int, _dp, _dp]),
    ("qg_ens_spread", C.c_int, [_vp, C.POINTER(QgSpread)]),
    ("qg_ens_run_recorded", C.c_int, [_vp, _i64, _i64, _i64, _dp, _i64, C.POINTER(_i64)]),
    # include/qg_mi355_spectra.h (outputs and records: device pointers)
    ("qg_spectra", C.c_int, [_vp, _dp]),
    ("qg_run_spectra", C.c_int, [_vp, _i64, _i64, _i64, _dp, _i64, C.POINTER(_i64)]),
    ("qg_ens_spectra", C.c_int, [_vp, _dp]),
    ("qg_ens_run_spectra", C.c_int, [_vp, _i64, _i64, _i64, _dp, _i64, C.POINTER(_i64)]),
    # include/qg_mi355_profiles.h (outputs and records: device pointers)
    ("qg_profiles", C.c_int, [_vp, _dp]),
    ("qg_run_profiles", C.c_int, [_vp, _i64, _i64, _i64, _dp, _i64, C.POINTER(_i64)]),
    ("qg_ens_profiles", C.c_int, [_vp, _dp]),
    ("qg_ens_run_profiles", C.c_int, [_vp, _i64, _i64, _i64, _dp, _i64, C.POINTER(_i64)]),
    # include/qg_mi355_spectra2d.h (the qg_iso_* are host functions; outputs and records: device pointers)
    ("qg_iso_shells", C.c_int, [_i64, _i64]),
    ("qg_iso_shell_of", C.c_int, [_i64, _i64, _i64, _i64]),
    ("qg_iso_shell_counts", C.c_int, [_i64, _i64, C.POINTER(_i64)]),
    ("qg_spectra2d", C.c_int, [_vp, _dp, _dp]),
    ("qg_run_iso_spectra", C.c_int, [_vp, _i64, _i64, _i64, _dp, _i64, C.POINTER(_i64)]),
    ("qg_ens_spectra2d", C.c_int, [_vp, _dp, _dp]),
    ("qg_ens_run_iso_spectra", C.c_int, [_vp, _i64, _i64, _i64, _dp, _i64, C.POINTER(_i64)]),
    # include/qg_mi355_tracers.h (arrays, outputs and records: device pointers)
    ("qg_tracers_create", C.c_int, [_vp, C.c_int, C.POINTER(QgTracerParams), C.POINTER(_vp)]),
    ("qg_ens_tracers_create", C.c_int, [_vp, C.c_int, C.POINTER(QgTracerParams), C.POINTER(_vp)]),
    ("qg_tracers_destroy", C.c_int, [_vp]),
    ("qg_tracers_bind", C.c_int, [_vp, _dp, _dp]),
    ("qg_tracers_reset", C.c_int, [_vp]),
    ("qg_tracers_advance", C.c_int, [_vp]),
    ("qg_tracers_step", C.c_int, [_vp, _i64]),
    ("qg_tracers_run", C.c_int, [_vp, _i64, _i64, _i64, _dp, _i64, C.POINTER(_i64)]),
    ("qg_tracers_diagnostics", C.c_int, [_vp, _dp]),
    ("qg_tracers_slot", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    ("qg_tracers_get_state", C.c_int, [_vp, C.POINTER(_i64), C.POINTER(C.c_int)]),
    ("qg_tracers_set_state", C.c_int, [_vp, _i64, C.POINTER(C.c_int)]),
    ("qg_tracers_set_form", C.c_int, [_vp, C.c_int]),
    # include/qg_mi355_floats.h (arrays, outputs and records: device pointers)
    ("qg_floats_create", C.c_int, [_vp, _i64, _i64, C.POINTER(_vp)]),
    ("qg_ens_floats_create", C.c_int, [_vp, _i64, _i64, C.POINTER(_vp)]),
    ("qg_floats_destroy", C.c_int, [_vp]),
    ("qg_floats_bind", C.c_int, [_vp, _dp, _dp, _dp]),
    ("qg_floats_reset", C.c_int, [_vp]),
    ("qg_floats_advance", C.c_int, [_vp]),
    ("qg_floats_step", C.c_int, [_vp, _i64]),
    ("qg_floats_run", C.c_int, [_vp, _i64, _i64, _i64, _dp, _dp, _i64, C.POINTER(_i64)]),
    ("qg_floats_stats", C.c_int, [_vp, _dp]),
    ("qg_floats_sample", C.c_int, [_vp, C.c_int, _dp]),
    ("qg_floats_get_state", C.c_int, [_vp, C.POINTER(_i64), C.POINTER(C.c_int)]),
    ("qg_floats_set_state", C.c_int, [_vp, _i64, C.c_int]),
    # include/qg_mi355_tstats.h (outputs and checkpoint arrays: device pointers)
    ("qg_tstats_create", C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    ("qg_ens_tstats_create", C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    ("qg_tstats_destroy", C.c_int, [_vp]),
    ("qg_tstats_reset", C.c_int, [_vp]),
    ("qg_tstats_accumulate", C.c_int, [_vp]),
    ("qg_tstats_run", C.c_int, [_vp, _i64, _i64, _i64]),
    ("qg_tstats_count", C.c_int, [_vp, C.POINTER(_i64)]),
    ("qg_tstats_field", C.c_int, [_vp, C.c_int, _dp]),
    ("qg_tstats_summary", C.c_int, [_vp, _dp]),
    ("qg_tstats_raw_doubles", C.c_int, [_vp, C.POINTER(_i64)]),
    ("qg_tstats_save", C.c_int, [_vp, _dp]),
    ("qg_tstats_load", C.c_int, [_vp, _dp, _i64]),
]

_lib = None


class QGError(RuntimeError):
    def __init__(self, fn, status):
        msg = _lib.qg_strerror(status).decode() if _lib is not None else str(status)
        super().__init__(f"{fn} failed with status {status}: {msg}")
        self.status = status


def lib():
    """Load the HIP library (raises if it is not built -- there is no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `make -C julia-ocean-modelling_amd` "
                "(or __graft_entry__.build()); the QG hot path has no CPU fallback")
        # PyTorch first: it ships its own HIP runtime, and the library must bind to that one
        # (loading ours first would bring in /opt/rocm's libamdhip64 as a second runtime)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES:
            # (an older experiment build named by QGMI355_LIB may lack newer entry points)
            if os.environ.get("QGMI355_LIB") and not hasattr(L, name):
                continue
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def check(fn, status):
    if status != QG_OK:
        raise QGError(fn, status)
    return status


def call(name, *args):
    return check(name, getattr(lib(), name)(*args))
