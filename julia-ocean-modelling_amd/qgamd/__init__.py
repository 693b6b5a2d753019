"""qgamd -- MI355X-native two-layer Phillips (baroclinic QG) hot path.

Host mirror of the reference's operator surface (src/model.jl, src/schemes/*.jl,
src/run_model_no_output.jl of JSLeadbetter/julia-ocean-modelling) over the HIP C-ABI in
include/qg_mi355.h (and the batched ensembles of include/qg_mi355_ensemble.h, qg_mi355_sweep.h, qg_mi355_stats.h, qg_mi355_spectra.h, qg_mi355_spectra2d.h, qg_mi355_profiles.h, qg_mi355_tracers.h, qg_mi355_floats.h and qg_mi355_tstats.h).  See model.py
for the mapping.
"""
from . import _lib
from ._lib import LIB_PATH, QGError, lib
from .model import *  # noqa: F401,F403
from .model import (BaroclinicModel, Ensemble, PairSolver, State, bench_model, cd, device_zeros,
                    evolve_psi_, evolve_zeta_, get_helmholtz_cholesky, get_poisson_cholesky,
                    initialise_model, J, laplace_5p, make_model, run_ensemble_no_output, run_model_no_output,
                    set_dropin_slots, sp_solve_modified_helmholtz, sp_solve_poisson, spread_dicts, sweep_members,
                    unbind,
                    update_doubly_periodic_bc_, SPECTRA_LINES, SPECTRA_STRIP_CAP, spectra_wavenumbers, ISO_LINES, iso_shells, iso_wavenumbers,
                    PROFILE_LINES, profile_dict, zonal_wind,
                    Tracers, TRACER_LINES, tracer_dicts, eddy_diffusivity,
                    Floats, FLOAT_LINES, float_dicts, float_positions,
                    TimeStats, TSTATS_FIELDS, TSTATS_SUMMARY_LINES, tstats_field_names, eke)
from .checkpoint import load_checkpoint, read_checkpoint, save_checkpoint
from .run import SnapshotWriter, create_metadata, log_model_params, run_model, update_max, update_min

__all__ = ["TimeStats", "TSTATS_FIELDS", "TSTATS_SUMMARY_LINES", "tstats_field_names", "eke", "Floats", "FLOAT_LINES", "float_dicts", "float_positions", "Tracers", "TRACER_LINES", "tracer_dicts", "eddy_diffusivity", "PROFILE_LINES", "profile_dict", "zonal_wind", "SPECTRA_LINES", "SPECTRA_STRIP_CAP", "spectra_wavenumbers", "ISO_LINES", "iso_shells", "iso_wavenumbers", "BaroclinicModel", "Ensemble", "run_ensemble_no_output", "sweep_members", "spread_dicts", "PairSolver", "State", "bench_model", "cd", "device_zeros",
           "evolve_psi_", "evolve_zeta_", "get_helmholtz_cholesky", "get_poisson_cholesky",
           "initialise_model", "J", "laplace_5p", "make_model", "run_model_no_output", "set_dropin_slots",
           "sp_solve_modified_helmholtz", "sp_solve_poisson", "unbind", "update_doubly_periodic_bc_",
           "run_model", "update_max", "update_min", "create_metadata", "log_model_params", "SnapshotWriter",
           "save_checkpoint", "load_checkpoint", "read_checkpoint", "LIB_PATH", "QGError", "lib"]
