"""Host-side mirror of the reference's operator surface for the hot path, driving the HIP
C-ABI (include/qg_mi355.h) on device arrays.

Reference surface (JSLeadbetter/julia-ocean-modelling, paths relative to its root):
  BaroclinicModel + outer constructor          src/model.jl:12-34
  ratio_term, S1_plus, S2_minus, beta_1/2, S_eig  src/model.jl:109-121
  P_matrix, P_inv_matrix                        src/model.jl:83-99
  initialise_model                              src/model.jl:37-62
  evolve_zeta!, evolve_psi!                     src/model.jl:155-199
  get_poisson_cholesky, get_helmholtz_cholesky  src/schemes/laplacian.jl:60-75
  run_model_no_output                           src/run_model_no_output.jl:3-16
  laplace_5p, cd, J, update_doubly_periodic_bc! laplacian.jl:15, model.jl:68, arakawa.jl:58,
                                                boundary_conditions.jl:2
  sp_solve_modified_helmholtz, sp_solve_poisson laplacian.jl:78-111

Device arrays are torch float64 CUDA tensors used only as memory: a Julia
(M+2, P+2, 2, 3) column-major array is a C-contiguous tensor of shape (3, 2, P+2, M+2)
(``[slot, layer, j, i]``), a Julia (M+2, P+2) matrix a (P+2, M+2) tensor.  Python names
cannot carry ``!``; the mutating functions end in ``_`` instead.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
import itertools
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import QgParams, QgStats, call

MINUTES = 60
DAY = 60 * 60 * 24
KM = 1000.0
YEAR = 60 * 60 * 24 * 365

SEED_LAYER1 = 20241008
SEED_LAYER2 = 20241009


# ---------------------------------------------------------------------------------------
# kernel-form selection (qg_set_form: process-wide, 0 = the library's choice by size)
# ---------------------------------------------------------------------------------------
def set_form(which, value):
    """Force one kernel form (``_lib.QG_FORM_*``); value 0 restores the automatic choice."""
    call("qg_set_form", int(which), int(value))


def get_form(which):
    v = _lib.lib().qg_get_form(int(which))
    if v < 0:
        raise _lib.QGError("qg_get_form", v)
    return v


@contextlib.contextmanager
def forced_form(which, value):
    """``with forced_form(QG_FORM_TENDENCY, QG_TEND_RING): ...`` -- the previous value after."""
    old = get_form(which)
    set_form(which, value)
    try:
        yield
    finally:
        set_form(which, old)


# ---------------------------------------------------------------------------------------
# parameters
# ---------------------------------------------------------------------------------------
@dataclass(frozen=True)
class BaroclinicModel:
    """``struct BaroclinicModel`` (src/model.jl:12-30).  Build with :func:`make_model`
    (the outer constructor, model.jl:33-34) or :meth:`create`."""

    H_1: float
    H_2: float
    H: float
    beta: float
    Lx: float
    Ly: float
    dt: float
    T: float
    U: float
    M: int
    P: int
    dx: float
    visc: float
    r: float
    R_d: float
    initial_kick: float

    @staticmethod
    def create(H_1, H_2, beta, Lx, Ly, dt, T, U, M, P, dx, visc, r, R_d, initial_kick):
        return make_model(H_1, H_2, beta, Lx, Ly, dt, T, U, M, P, dx, visc, r, R_d, initial_kick)


def make_model(H_1, H_2, beta, Lx, Ly, dt, T, U, M, P, dx, visc, r, R_d, initial_kick):
    """Outer constructor (model.jl:33-34): H = H_1 + H_2."""
    return BaroclinicModel(float(H_1), float(H_2), float(H_1) + float(H_2), float(beta), float(Lx),
                           float(Ly), float(dt), float(T), float(U), int(M), int(P), float(dx),
                           float(visc), float(r), float(R_d), float(initial_kick))


def bench_model(N, dt=30.0 * MINUTES, T=1.0 * DAY, P=None, Lx=4000.0 * KM):
    """Benchmark parameter set of src/benchmarking/julia_bench_parts.jl:6-18 (square cells)."""
    P = N if P is None else P
    return make_model(1.0 * KM, 2.0 * KM, 2e-11, Lx, Lx * P / N, dt, T, 0.1, N, P, Lx / N, 100.0,
                      1e-7, 40.0 * KM, 1e-6)


def ratio_term(m):  # model.jl:109-111
    return 0.5 * (m.H_1 + m.H_2) / ((m.R_d * m.R_d) * ((1 / m.H_1) + (1 / m.H_2)))


def S1_plus(m):  # model.jl:113
    return (2 * ratio_term(m)) / (m.H_1 * (m.H_1 + m.H_2))


def S2_minus(m):  # model.jl:114
    return (2 * ratio_term(m)) / (m.H_2 * (m.H_1 + m.H_2))


def beta_1(m):  # model.jl:117
    return m.beta + (S1_plus(m) * m.U)


def beta_2(m):  # model.jl:118
    return m.beta - (S2_minus(m) * m.U)


def S_eig(m):  # model.jl:121
    return -1 / (m.R_d * m.R_d)


def P_matrix(H_1, H_2):  # model.jl:83-87
    P = np.ones((2, 2))
    P[0, 1] = -H_2 / H_1
    return P


def P_inv_matrix(m):  # model.jl:90-99
    a, b = S1_plus(m), S2_minus(m)
    return (1 / (a + b)) * np.array([[b, a], [-b, b]])


def qg_params(m, solver=_lib.QG_SOLVER_SPECTRAL, P_fwd=None, chunk_rows=0, P_local=None,
              precond=_lib.QG_PRECOND_SPECTRAL, pcg_rtol=1e-12, pcg_maxit=500, dtype=_lib.QG_F64,
              wind=None):
    """wind = (tau0 [N m^-2], rho0 [kg m^-3]) switches on the double-gyre wind forcing
    extension of the upper layer (include/qg_mi355.h; not in the reference)."""
    p = QgParams()
    _lib.lib().qg_default_params(C.byref(p))
    for n in ("H_1", "H_2", "beta", "Lx", "Ly", "dt", "T", "U", "dx", "visc", "r", "R_d",
              "initial_kick"):
        setattr(p, n, float(getattr(m, n)))
    p.M = int(m.M)
    p.P = int(m.P if P_local is None else P_local)
    if P_fwd is not None:
        for k, v in enumerate(np.asarray(P_fwd, dtype=np.float64).reshape(-1)):
            p.P_fwd[k] = float(v)
    p.solver = int(solver)
    p.precond = int(precond)
    p.pcg_rtol = float(pcg_rtol)
    p.pcg_maxit = int(pcg_maxit)
    p.chunk_rows = int(chunk_rows)
    p.dtype = int(dtype)
    if wind is not None:
        p.wind_tau0, p.wind_rho0 = float(wind[0]), float(wind[1])
    return p


# ---------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _stream_ptr():
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _check_field(t, M, P):
    torch = _torch()
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise ValueError("expected a contiguous float64 CUDA tensor")
    if tuple(t.shape[-2:]) != (P + 2, M + 2):
        raise ValueError(f"field shape {tuple(t.shape)} does not match (P+2, M+2) = {(P + 2, M + 2)}")


def device_zeros(m, P_local=None, device="cuda", dtype=None):
    """zeros(M+2, P+2, 2, 3) in Julia layout -> tensor (3, 2, P+2, M+2)."""
    torch = _torch()
    P = m.P if P_local is None else P_local
    return torch.zeros((3, 2, P + 2, m.M + 2), dtype=torch.float64 if dtype is None else dtype, device=device)


class State:
    """The model state zeta, psi, f_store plus the library context that evolves it.

    Plays the role of the reference's (zeta, psi, f_store) arrays and its two CHOLMOD
    factors.  History slots rotate (no copies): :meth:`slot` maps the reference's slot
    index (1 = newest) to the physical slot, :meth:`logical` returns the reference-ordered
    view, :meth:`canonicalize` physically restores the reference order.
    """

    def __init__(self, m, solver=_lib.QG_SOLVER_SPECTRAL, P_fwd=None, chunk_rows=0,
                 device=None, rank=0, nranks=1, P_local=None, precond=_lib.QG_PRECOND_SPECTRAL,
                 pcg_rtol=1e-12, pcg_maxit=500, dtype=None, wind=None, arrays=None):
        """dtype: torch.float64 (default, the reference's arithmetic) or torch.float32 (the
        F32 state of BASELINE config 5; spectral solver only).  wind: (tau0, rho0) of the
        wind-forcing extension, or None (the reference's right-hand side).  arrays: an
        existing (zeta, psi, f_store) triple of (3, 2, P+2, M+2) device tensors to bind
        instead of allocating new ones (the caller keeps ownership)."""
        _lib.lib()  # the HIP library first: no CPU fallback, fail before touching the device
        torch = _torch()
        self.model = m
        self.P_local = m.P if P_local is None else P_local
        # device: None (current), an ordinal, "cuda:k" or a torch.device -> ordinal k.  The
        # arrays and the stream the library launches on all belong to that device.
        if device is None:
            self.device = torch.cuda.current_device()
        else:
            dev = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
            if dev.type != "cuda":
                raise ValueError(f"State needs a CUDA (HIP) device, got {dev}")
            self.device = dev.index if dev.index is not None else torch.cuda.current_device()
        self.dtype = torch.float64 if dtype is None else dtype
        if self.dtype not in (torch.float64, torch.float32):
            raise ValueError("dtype must be torch.float64 or torch.float32")
        with torch.cuda.device(self.device):
            dev = torch.device("cuda", self.device)
            if arrays is None:
                self.zeta = device_zeros(m, self.P_local, device=dev, dtype=self.dtype)
                self.psi = device_zeros(m, self.P_local, device=dev, dtype=self.dtype)
                self.f_store = device_zeros(m, self.P_local, device=dev, dtype=self.dtype)
            else:
                shape = (3, 2, self.P_local + 2, m.M + 2)
                for t in arrays:
                    if (tuple(t.shape) != shape or t.dtype != self.dtype or t.device != dev
                            or not t.is_contiguous()):
                        raise ValueError(f"bound arrays must be contiguous {self.dtype} tensors of shape "
                                         f"{shape} on {dev}")
                self.zeta, self.psi, self.f_store = arrays
            self.params = qg_params(m, solver, P_fwd, chunk_rows, self.P_local, precond, pcg_rtol, pcg_maxit,
                                    _lib.QG_F32 if self.dtype == torch.float32 else _lib.QG_F64, wind)
            self._ctx = C.c_void_p()
            call("qg_create", C.byref(self.params), int(self.device), _stream_ptr(), C.byref(self._ctx))
            call("qg_bind_state", self._ctx, _ptr(self.zeta), _ptr(self.psi), _ptr(self.f_store))
        # rank / nranks describe the slab this state holds (e.g. read back from a slab
        # checkpoint); stepping a slab of a multi-rank run needs that transport attached first
        self.rank, self.nranks = rank, nranks
        self._attached_ranks = 1

    def close(self):
        """Destroy the library context now (qg_destroy); the arrays stay with the caller."""
        ctx = getattr(self, "_ctx", None)
        if ctx and _lib._lib is not None:
            _lib._lib.qg_destroy(ctx)
            self._ctx = None

    def __del__(self):
        self.close()

    # -- multi-GPU ---------------------------------------------------------------------
    def comm_init(self, nranks, rank, uid: bytes):
        call("qg_comm_init", self._ctx, int(nranks), int(rank), C.c_char_p(uid))
        self.rank, self.nranks = rank, nranks
        self._attached_ranks = nranks

    def set_overlap(self, on=True):
        """qg_set_overlap: post each step's halo exchange on a second stream and run the
        interior rows' tendency meanwhile (multi-rank only; bit-identical results)."""
        call("qg_set_overlap", self._ctx, 1 if on else 0)

    def set_halo_transport(self, transport="rccl"):
        """qg_comm_set_halo_transport (collective, RCCL transport only): "rccl" (pack kernel +
        grouped send/recv), "peer" (copy-engine copies into the neighbours' IPC-mapped
        receive regions + arrival flags; no collective kernel beside the interior tendency) or
        "put" (the same regions, rows stored by one small kernel that also waits)."""
        modes = {"rccl": 0, "peer": 1, "put": 2}
        if transport not in modes:
            raise ValueError(f"halo transport {transport!r}: one of {sorted(modes)}")
        call("qg_comm_set_halo_transport", self._ctx, modes[transport])
        self.halo_transport = transport

    def set_gather_transport(self, transport="rccl"):
        """qg_comm_set_gather_transport (collective, RCCL transport, direct solver): "rccl"
        (ncclAllGather of the rank records) or "peer" (one kernel storing the record into every
        peer's IPC-mapped region in parallel, flags, copy-out)."""
        modes = {"rccl": 0, "peer": 1}
        if transport not in modes:
            raise ValueError(f"gather transport {transport!r}: one of {sorted(modes)}")
        call("qg_comm_set_gather_transport", self._ctx, modes[transport])
        self.gather_transport = transport

    def comm_probe(self, reps=20):
        """qg_comm_probe: event-timed halo exchange and record all-gather of one step, in
        isolation (every rank must call it): ms and bytes per collective."""
        out = (C.c_double * 4)()
        call("qg_comm_probe", self._ctx, int(reps), out)
        return {"halo_ms": out[0], "halo_bytes_sent": int(out[1]), "allgather_ms": out[2],
                "allgather_bytes_received": int(out[3]), "reps": int(reps)}

    def set_pcg_sync(self, sync=True):
        """qg_set_pcg_sync: 1 = the host checks every PCG residual (and iterates when the
        certificate fails); 0 = deferred on-device certification (default)."""
        call("qg_set_pcg_sync", self._ctx, 1 if sync else 0)

    def pcg_certificate(self):
        """qg_pcg_certificate: deferred PCG certificates so far."""
        n, f, first, worst = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        call("qg_pcg_certificate", self._ctx, C.byref(n), C.byref(f), C.byref(first), C.byref(worst))
        return {"solves": n.value, "failures": f.value, "first_failure": first.value, "worst_relres": worst.value}

    def _need_transport(self):
        if self.nranks != self._attached_ranks:
            raise RuntimeError(f"this state is slab {self.rank} of {self.nranks}: attach the {self.nranks}-rank "
                               "transport (comm_init / TorchDistTransport.attach) before stepping it")

    # -- reference operations ----------------------------------------------------------
    def initialise(self, seeds=(SEED_LAYER1, SEED_LAYER2)):
        call("qg_initialise", self._ctx, int(seeds[0]), int(seeds[1]))
        return self

    def evolve_zeta_(self, timestep):
        self._need_transport()
        call("qg_evolve_zeta", self._ctx, int(timestep))

    def evolve_psi_(self):
        self._need_transport()
        call("qg_evolve_psi", self._ctx)

    def step(self, timestep):
        self._need_transport()
        call("qg_step", self._ctx, int(timestep))

    def run(self, first_step, nsteps):
        self._need_transport()
        call("qg_run", self._ctx, int(first_step), int(nsteps))

    def synchronize(self):
        call("qg_synchronize", self._ctx)

    def stats(self):
        s = QgStats()
        call("qg_get_stats", self._ctx, C.byref(s))
        return {"delta": s.delta, "pin": s.pin, "iters": list(s.iters), "relres": list(s.relres)}

    def diagnostics(self):
        """qg_diagnostics: max / min of the newest zeta and psi per layer (the update_max /
        update_min of run_model.jl:41-53), circulation, enstrophy, kinetic energy and the
        interface term, over the global domain (multi-GPU: every rank calls it)."""
        d = _lib.QgDiag()
        call("qg_diagnostics", self._ctx, C.byref(d))
        return {f: (list(getattr(d, f)) if f != "interface" else d.interface)
                for f, _ in _lib.QgDiag._fields_ if f != "reserved"}

    # -- zonal wavenumber spectra (include/qg_mi355_spectra.h) ---------------------------
    def spectra(self):
        """qg_spectra: the zonal wavenumber spectra of the newest state as a (5, M/2+1) float64
        device tensor -- rows in the order of :data:`SPECTRA_LINES`, column k the zonal
        wavenumber :func:`spectra_wavenumbers` (M, dx)[k]; each row sums over k to the field of
        the same name of :meth:`diagnostics`.  Enqueued on the current stream, not synchronised.
        One rank, M a power of two in 8..2048."""
        torch = _torch()
        out = torch.empty((_lib.QG_SPEC_LINES, self.model.M // 2 + 1), dtype=torch.float64, device=self.zeta.device)
        with torch.cuda.device(self.device):
            call("qg_spectra", self._ctx, _ptr(out))
        return out

    def run_spectra(self, first_step, nsteps, every):
        """qg_run_spectra: :meth:`run` (stepped on the stream) that records :meth:`spectra` after
        every ``every``-th step on the device, without a host round trip.  Returns the
        (nsteps // every, 5, M/2+1) float64 device tensor of records.  Not synchronised."""
        self._need_transport()
        return _run_spectra("qg_run_spectra", self._ctx, self.device, self.zeta.device,
                            (_lib.QG_SPEC_LINES, self.model.M // 2 + 1), first_step, nsteps, every)

    # -- (kx, ky) and isotropic spectra (include/qg_mi355_spectra2d.h) --------------------
    def spectra2d(self, full=False):
        """qg_spectra2d: the isotropic spectrum of the newest state as a (5, NK) float64 device
        tensor -- rows in the order of :data:`ISO_LINES`, column n the shell of total wavenumber
        :func:`iso_wavenumbers` (M, P, dx)[0][n]; each row sums over n to the field of the same
        name of :meth:`diagnostics`.  ``full=True`` returns ``(full2d, iso)`` with the (5, P,
        M/2+1) spectrum over (ky, kx) it is folded from (the layout of an rfft2 over (y, x));
        iso is bit for bit the same either way.  Enqueued on the current stream, not
        synchronised.  One rank, M and P powers of two in 8..2048."""
        return _spectra2d("qg_spectra2d", self._ctx, self.device, self.zeta.device, (), self.model, full)

    def run_iso_spectra(self, first_step, nsteps, every):
        """qg_run_iso_spectra: :meth:`run` (stepped on the stream) that records the isotropic
        spectrum of :meth:`spectra2d` after every ``every``-th step on the device, without a host
        round trip.  Returns the (nsteps // every, 5, NK) float64 device tensor of records.  Not
        synchronised."""
        self._need_transport()
        return _run_spectra("qg_run_iso_spectra", self._ctx, self.device, self.zeta.device,
                            (_lib.QG_SPEC_LINES, iso_shells(self.model.M, self.model.P)), first_step, nsteps, every)

    # -- zonal-mean profiles per latitude (include/qg_mi355_profiles.h) -----------------
    def profiles(self):
        """qg_profiles: the per-latitude lines of the newest state as a (12, P) float64 device
        tensor -- rows in the order of :data:`PROFILE_LINES` (see there for the table), column j
        the interior row; rows 0-4 sum over j to the fields of the same name of
        :meth:`diagnostics`.  Enqueued on the current stream, not synchronised.  One rank, any
        M, P >= 3."""
        torch = _torch()
        out = torch.empty((_lib.QG_PROF_LINES, self.model.P), dtype=torch.float64, device=self.zeta.device)
        with torch.cuda.device(self.device):
            call("qg_profiles", self._ctx, _ptr(out))
        return out

    def run_profiles(self, first_step, nsteps, every):
        """qg_run_profiles: :meth:`run` (stepped on the stream) that records :meth:`profiles`
        after every ``every``-th step on the device, without a host round trip: the time-latitude
        (Hovmoeller) array.  Returns the (nsteps // every, 12, P) float64 device tensor of
        records.  Not synchronised."""
        self._need_transport()
        return _run_spectra("qg_run_profiles", self._ctx, self.device, self.zeta.device,
                            (_lib.QG_PROF_LINES, self.model.P), first_step, nsteps, every)

    # -- slot rotation -----------------------------------------------------------------
    def slot(self, which, logical):
        w = {"zeta": 0, "psi": 1, "f_store": 2}[which]
        out = C.c_int()
        call("qg_slot", self._ctx, w, int(logical), C.byref(out))
        return out.value

    def heads(self):
        return [self.slot(w, 1) for w in ("zeta", "psi", "f_store")]

    def set_heads(self, heads):
        call("qg_set_slots", self._ctx, (C.c_int * 3)(*[int(h) for h in heads]))

    def logical(self, which):
        """(3, 2, P+2, M+2) tensor in reference slot order (a gathered copy)."""
        torch = _torch()
        t = getattr(self, which)
        order = [self.slot(which, s) for s in (1, 2, 3)]
        return t[torch.tensor(order, device=t.device)]

    def current(self, which, layer):
        """Reference ``X[:, :, layer, 1]`` (layer 1-based) as a (P+2, M+2) view (multi-GPU:
        ghost rows current after synchronize())."""
        return getattr(self, which)[self.slot(which, 1), layer - 1]

    def canonicalize(self):
        call("qg_canonicalize", self._ctx)

    def set_keep_order(self, on=True, slot1_only=False, deferred=False):
        """qg_set_keep_order: every call leaves slot 1 = newest (store_new_state!'s shift, in
        place, before the new values are written), so the arrays are always in the
        reference's slot order; off (default) rotates the slots instead.  slot1_only
        (QG_KEEP_ORDER_SLOT1): slot 1 of zeta / psi and all of f_store kept so after every
        call, slots 2-3 of zeta and psi (never read by the reference) not maintained -- one
        slot copy per step instead of four.  deferred (with slot1_only,
        QG_KEEP_ORDER_SLOT1_DEFERRED): that copy rides in the next evolve_psi!'s first solver
        pass, so slot 1 of zeta is stale between evolve_zeta! and evolve_psi! (qg_slot names
        the newest; synchronize() completes the move)."""
        mode = (_lib.QG_KEEP_ORDER_SLOT1_DEFERRED if deferred else _lib.QG_KEEP_ORDER_SLOT1) if slot1_only else 1
        call("qg_set_keep_order", self._ctx, mode if on else 0)

    def to_numpy(self, which):
        """Reference-ordered numpy array of shape (M+2, P+2, 2, 3) (Julia index order).
        Synchronises first (multi-GPU: completes the lazily refreshed ghost rows)."""
        self.synchronize()
        return self.logical(which).permute(3, 2, 1, 0).contiguous().cpu().numpy()


# ---------------------------------------------------------------------------------------
# the reference's free functions
# ---------------------------------------------------------------------------------------
def initialise_model(m, seeds=(SEED_LAYER1, SEED_LAYER2), **kw):
    """initialise_model (model.jl:37-62) with seeded noise; returns the device State."""
    if not np.sign(beta_1(m)) == -np.sign(beta_2(m)):  # model.jl:38
        raise AssertionError("sign(beta_1) must equal -sign(beta_2)")
    return State(m, **kw).initialise(seeds)


_BOUND = {}
_DROPIN_SLOTS = ["all"]


def set_dropin_slots(mode):
    """Slots the reference-signature calls below maintain on arrays bound from now on:
    "all" (default: store_new_state! exactly, slots 2-3 of zeta and psi shifted too),
    "slot1" (QG_KEEP_ORDER_SLOT1: slot 1 of zeta and psi and all of f_store, the values the
    reference's loop reads, newest after every call; one slot copy per step instead of four)
    or "slot1_deferred" (QG_KEEP_ORDER_SLOT1_DEFERRED: as "slot1", the copy of the new zeta
    into slot 1 done by the next evolve_psi!'s first solver pass -- slot 1 of zeta is stale
    between evolve_zeta! and evolve_psi!, which the reference's loop never reads there)."""
    if mode not in ("all", "slot1", "slot1_deferred"):
        raise ValueError("mode must be 'all', 'slot1' or 'slot1_deferred'")
    _DROPIN_SLOTS[0] = mode


def _bound_state(m, zeta, psi, f_store):
    """The library context bound to a caller's (zeta, psi, f_store) arrays, created on first
    use and cached by their addresses (the reference-signature calls below).  The context
    keeps the reference's slot order on every call (qg_set_keep_order), as store_new_state!
    does.  A different model for the same arrays replaces the cached context."""
    key = (zeta.data_ptr(), psi.data_ptr(), f_store.data_ptr())
    st = _BOUND.get(key)
    if st is None or st.model != m:
        if st is not None:  # settle and release the old context (its failure is raised after)
            st = None
            unbind(zeta, psi, f_store)
        st = _BOUND[key] = State(m, device=zeta.device, dtype=zeta.dtype, arrays=(zeta, psi, f_store))
        st.set_keep_order(True, slot1_only=_DROPIN_SLOTS[0] != "all",
                          deferred=_DROPIN_SLOTS[0] == "slot1_deferred")
    return st


def unbind(zeta=None, psi=None, f_store=None):
    """Release the cached contexts of the reference-signature calls: the one bound to these
    arrays, or all of them (no arguments).  The contexts hold references to the arrays, so
    without this the arrays stay alive as long as the process.  Every selected context is
    released even if settling one fails (e.g. a deferred PCG certificate that failed,
    QG_ERR_NOT_CONVERGED); the first such error is raised after all of them are released."""
    if zeta is None:
        keys = list(_BOUND)
    else:
        keys = [k for k in _BOUND if k[0] == zeta.data_ptr()
                and (psi is None or k[1] == psi.data_ptr())
                and (f_store is None or k[2] == f_store.data_ptr())]
    err = None
    for k in keys:
        st = _BOUND.pop(k)
        try:
            st.synchronize()
        except Exception as e:  # noqa: BLE001 -- re-raised below, after every release
            err = err or e
        finally:
            st.close()
            del st
    if err is not None:
        raise err
    return len(keys)


def evolve_zeta_(m, *args):
    """evolve_zeta!(model, zeta, psi, timestep, f_store) (model.jl:155-158).

    Two forms: ``evolve_zeta_(m, state, timestep)`` on a :class:`State` (slots rotate, no
    copies), and the reference's own signature ``evolve_zeta_(m, zeta, psi, timestep,
    f_store)`` on (3, 2, P+2, M+2) device tensors, which leaves the arrays in the reference's
    slot order after the call (slot 1 = newest, as store_new_state! leaves them)."""
    if len(args) == 2:
        state, timestep = args
        state.evolve_zeta_(timestep)
        return
    zeta, psi, timestep, f_store = args
    st = _bound_state(m, zeta, psi, f_store)
    st.evolve_zeta_(timestep)  # (keep-order context: the arrays stay in reference order)


class SolverHandle:
    """Stands in for SparseArrays.CHOLMOD.Factor in evolve_psi!'s signature.  The state's
    context owns the actual solver (both systems are solved together on the device)."""

    def __init__(self, kind, M, P, dx, alpha):
        self.kind, self.M, self.P, self.dx, self.alpha = kind, M, P, dx, alpha


def get_poisson_cholesky(M, P, dx):  # laplacian.jl:66-75
    return SolverHandle("poisson", M, P, dx, 0.0)


def get_helmholtz_cholesky(M, P, dx, alpha):  # laplacian.jl:60-64
    return SolverHandle("helmholtz", M, P, dx, alpha)


def evolve_psi_(m, *args):
    """evolve_psi!(model, zeta, psi, poisson_cholesky, helmholtz_cholesky) (model.jl:172-199).

    ``evolve_psi_(m, state[, poisson, helmholtz])`` on a :class:`State`, or the reference's
    signature ``evolve_psi_(m, zeta, psi, poisson, helmholtz)`` on device tensors already
    bound by :func:`evolve_zeta_` (which knows their f_store)."""
    if isinstance(args[0], State):
        state, poisson, helmholtz = (tuple(args) + (None, None))[:3]
    else:
        zeta, psi, poisson, helmholtz = args
        hits = [st for k, st in _BOUND.items() if k[:2] == (zeta.data_ptr(), psi.data_ptr())]
        if len(hits) != 1:
            raise ValueError("evolve_psi_: call evolve_zeta_ on these arrays first (it binds them "
                             "with their f_store)")
        state = hits[0]
        if state.model != m:
            raise ValueError("evolve_psi_: these arrays are bound to a different model (call "
                             "evolve_zeta_ with this model first, or unbind them)")
    for h, kind in ((poisson, "poisson"), (helmholtz, "helmholtz")):
        if h is not None and (h.kind != kind or h.M != m.M or h.P != m.P or h.dx != m.dx):
            raise ValueError(f"{kind} handle does not match the model")
    if helmholtz is not None and helmholtz.alpha != S_eig(m):
        raise ValueError("helmholtz handle alpha != S_eig(model)")
    state.evolve_psi_()


def run_model_no_output(m, nsteps=None, seeds=(SEED_LAYER1, SEED_LAYER2), **kw):
    """run_model_no_output.jl:3-16: init, total_steps = floor(T/dt) steps; returns State."""
    st = initialise_model(m, seeds, **kw)
    total = int(np.floor(m.T / m.dt)) if nsteps is None else int(nsteps)
    st.run(1, total)
    return st


# ---------------------------------------------------------------------------------------
# batched ensembles (include/qg_mi355_ensemble.h)
# ---------------------------------------------------------------------------------------
def ensemble_seeds(nmembers):
    """The default seeds of an ensemble: member b gets (SEED_LAYER1 + 2b, SEED_LAYER2 + 2b), so
    member 0 is the default single run and no two layers of any members share a seed."""
    return [(SEED_LAYER1 + 2 * b, SEED_LAYER2 + 2 * b) for b in range(int(nmembers))]


MEMBER_KEYS = ("U", "beta", "r", "visc", "R_d", "initial_kick", "wind_tau0")


def sweep_members(**axes):
    """The Cartesian product of value lists as a ``members`` list for :class:`Ensemble`:
    ``sweep_members(U=[a, b], r=[c, d, e])`` is the 6 mappings {U: a, r: c}, {U: a, r: d}, ...,
    {U: b, r: e} -- row-major in the keyword order (the last keyword varies fastest)."""
    for k in axes:
        if k not in MEMBER_KEYS:
            raise ValueError(f"unknown member parameter {k!r} (one of {', '.join(MEMBER_KEYS)})")
    keys = list(axes)
    return [dict(zip(keys, vals)) for vals in itertools.product(*[list(axes[k]) for k in keys])]


class Ensemble:
    """B members of one model -- same parameters, different states -- advanced together: every
    step is the four kernel launches a :class:`State` needs for one member (qg_ens_*).

    With ``members`` (include/qg_mi355_sweep.h) each member may carry its own U, beta, r, visc,
    R_d, initial_kick and wind_tau0: member b is then bit for bit a State of
    :meth:`member_model` (b) with wind :meth:`member_wind` (b).

    ``zeta``, ``psi``, ``f_store`` are (B, 3, 2, P+2, M+2) float64 tensors (the Julia
    (M+2, P+2, 2, 3, B) arrays); member b's block is a :class:`State`'s array, and after the same
    calls holds bit for bit what a State with that member's seeds holds.  The history slots
    rotate with one set of heads for all members.  F64, spectral solver, one GPU, M a power of
    two in 8..2048, P >= 3 (QGError with QG_ERR_UNSUPPORTED otherwise)."""

    def __init__(self, m, nmembers, seeds=None, chunk_rows=0, P_fwd=None, wind=None, device=None, members=None):
        """seeds: a sequence of B (seed1, seed2) pairs to initialise with right away, or None
        (call :meth:`initialise`, or fill the tensors, before stepping).  members: a sequence of
        B mappings with keys from U, beta, r, visc, R_d, initial_kick, wind_tau0 (ValueError for
        any other); a missing key takes the model's value, wind_tau0 overrides wind[0]."""
        _lib.lib()  # the HIP library first: no CPU fallback, fail before touching the device
        torch = _torch()
        self.model = m
        self.nmembers = int(nmembers)
        self.params = qg_params(m, _lib.QG_SOLVER_SPECTRAL, P_fwd, chunk_rows, wind=wind)
        self._ens = C.c_void_p()
        mp = None
        if members is not None:
            members = list(members)
            if len(members) != self.nmembers:
                raise ValueError(f"{len(members)} member mappings for {self.nmembers} members")
            mp = (_lib.QgMemberParams * self.nmembers)()
            for b, kv in enumerate(members):
                for k in kv:
                    if k not in MEMBER_KEYS:
                        raise ValueError(f"member {b}: unknown parameter {k!r} (one of {', '.join(MEMBER_KEYS)})")
                call("qg_member_params_default", C.byref(self.params), C.byref(mp[b]))
                for k, v in kv.items():
                    setattr(mp[b], k, float(v))
        if device is None:
            self.device = torch.cuda.current_device()
        else:
            dev = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
            if dev.type != "cuda":
                raise ValueError(f"Ensemble needs a CUDA (HIP) device, got {dev}")
            self.device = dev.index if dev.index is not None else torch.cuda.current_device()
        with torch.cuda.device(self.device):
            # created first: an unsupported configuration is refused before anything is allocated
            if mp is None:
                call("qg_ens_create", C.byref(self.params), self.nmembers, int(self.device), _stream_ptr(),
                     C.byref(self._ens))
            else:
                call("qg_ens_create_sweep", C.byref(self.params), mp, self.nmembers, int(self.device),
                     _stream_ptr(), C.byref(self._ens))
            shape = (self.nmembers, 3, 2, m.P + 2, m.M + 2)
            dev = torch.device("cuda", self.device)
            self.zeta = torch.zeros(shape, dtype=torch.float64, device=dev)
            self.psi = torch.zeros(shape, dtype=torch.float64, device=dev)
            self.f_store = torch.zeros(shape, dtype=torch.float64, device=dev)
            call("qg_ens_bind_state", self._ens, _ptr(self.zeta), _ptr(self.psi), _ptr(self.f_store))
            if seeds is not None:
                self.initialise(seeds)

    def close(self):
        """Destroy the library handle now (qg_ens_destroy); the tensors stay with the caller."""
        ens = getattr(self, "_ens", None)
        if ens and _lib._lib is not None:
            _lib._lib.qg_ens_destroy(ens)
            self._ens = None

    def __del__(self):
        self.close()

    def member(self, b):
        """The (zeta, psi, f_store) views of member b, each (3, 2, P+2, M+2)."""
        return self.zeta[b], self.psi[b], self.f_store[b]

    def member_params(self, b):
        """qg_ens_member_params: member b's seven values as a dict (the model's, without ``members``)."""
        mp = _lib.QgMemberParams()
        call("qg_ens_member_params", self._ens, int(b), C.byref(mp))
        return {k: getattr(mp, k) for k in MEMBER_KEYS}

    def member_model(self, b):
        """The BaroclinicModel of member b: the ensemble's with b's values substituted."""
        v = self.member_params(b)
        v.pop("wind_tau0")
        return dataclasses.replace(self.model, **v)

    def member_wind(self, b):
        """Member b's ``wind`` argument of a :class:`State`: (tau0, rho0), or None (no wind)."""
        tau0 = self.member_params(b)["wind_tau0"]
        return (tau0, self.params.wind_rho0) if tau0 != 0 else None

    def initialise(self, seeds=None):
        """qg_ens_initialise: initialise_model per member from B (seed1, seed2) pairs (default
        :func:`ensemble_seeds`)."""
        seeds = ensemble_seeds(self.nmembers) if seeds is None else list(seeds)
        if len(seeds) != self.nmembers:
            raise ValueError(f"{len(seeds)} seed pairs for {self.nmembers} members")
        arr = C.c_uint64 * self.nmembers
        call("qg_ens_initialise", self._ens, arr(*[int(s[0]) for s in seeds]), arr(*[int(s[1]) for s in seeds]))
        return self

    def step(self, timestep):
        call("qg_ens_step", self._ens, int(timestep))

    def run(self, first_step, nsteps):
        call("qg_ens_run", self._ens, int(first_step), int(nsteps))

    def synchronize(self):
        call("qg_ens_synchronize", self._ens)

    def slot(self, which, logical):
        w = {"zeta": 0, "psi": 1, "f_store": 2}[which]
        out = C.c_int()
        call("qg_ens_slot", self._ens, w, int(logical), C.byref(out))
        return out.value

    def logical(self, which):
        """(B, 3, 2, P+2, M+2) tensor in reference slot order (a gathered copy)."""
        torch = _torch()
        t = getattr(self, which)
        order = [self.slot(which, s) for s in (1, 2, 3)]
        return t[:, torch.tensor(order, device=t.device)]

    def current(self, which, layer):
        """Reference ``X[:, :, layer, 1]`` (layer 1-based) of every member: a (B, P+2, M+2) view."""
        return getattr(self, which)[:, self.slot(which, 1), layer - 1]

    def canonicalize(self):
        call("qg_ens_canonicalize", self._ens)

    def diagnostics(self):
        """qg_ens_diagnostics: a list of B dicts shaped like :meth:`State.diagnostics`."""
        d = (_lib.QgDiag * self.nmembers)()
        call("qg_ens_diagnostics", self._ens, d)
        return [{f: (list(getattr(r, f)) if f != "interface" else r.interface)
                 for f, _ in _lib.QgDiag._fields_ if f != "reserved"} for r in d]

    # ---- statistics across the members (include/qg_mi355_stats.h) ----
    def moments(self, which, var=True):
        """qg_ens_moments: (mean, var) over the members of the newest ``which`` ("zeta" or
        "psi"), point by point, as (2, P+2, M+2) tensors (layer, row, column; ghost ring
        included); var is the unbiased variance, or None with ``var=False``.  One launch on the
        current stream, no synchronisation.  The arithmetic (Welford's recurrence in member
        order) is fixed by the header: the fields are reproducible bit for bit."""
        torch = _torch()
        w = {"zeta": 0, "psi": 1}[which]
        shape = (2, self.model.P + 2, self.model.M + 2)
        dev = self.zeta.device
        mean = torch.empty(shape, dtype=torch.float64, device=dev)
        v = torch.empty(shape, dtype=torch.float64, device=dev) if var else None
        with torch.cuda.device(self.device):
            call("qg_ens_moments", self._ens, w, _ptr(mean), _ptr(v) if var else None)
        return mean, v

    def spread(self):
        """qg_ens_spread: the domain-integrated spread record of the newest state as a dict
        (per-layer lists; ``step`` is 0).  Synchronous."""
        r = _lib.QgSpread()
        with _torch().cuda.device(self.device):
            call("qg_ens_spread", self._ens, C.byref(r))
        return spread_dicts([(C.c_double * SPREAD_LEN).from_buffer(r)])[0]

    def run_recorded(self, first_step, nsteps, every):
        """qg_ens_run_recorded: :meth:`run` that records the spread record after every
        ``every``-th step on the device, without a host round trip.  Returns the
        (nsteps // every, 16) float64 device tensor of records (rows in the field order of
        qg_spread; :func:`spread_dicts` turns rows into dicts).  Not synchronised."""
        torch = _torch()
        if int(every) < 1:
            raise ValueError(f"every = {every}: must be at least 1")
        n = max(int(nsteps), 0) // int(every)
        # (at least one row: a null pointer is refused also when no record is due)
        rec = torch.zeros((max(n, 1), SPREAD_LEN), dtype=torch.float64, device=self.zeta.device)
        got = C.c_int64()
        with torch.cuda.device(self.device):
            call("qg_ens_run_recorded", self._ens, int(first_step), int(nsteps), int(every), _ptr(rec), n,
                 C.byref(got))
        return rec[:got.value]

    # ---- zonal wavenumber spectra (include/qg_mi355_spectra.h) ----
    def spectra(self):
        """qg_ens_spectra: every member's zonal wavenumber spectra of the newest state as a
        (B, 5, M/2+1) float64 device tensor; member b's block is bit for bit
        :meth:`State.spectra` of a State holding member b's arrays.  One pair of launches for
        all members on the current stream, not synchronised."""
        torch = _torch()
        out = torch.empty((self.nmembers, _lib.QG_SPEC_LINES, self.model.M // 2 + 1), dtype=torch.float64,
                          device=self.zeta.device)
        with torch.cuda.device(self.device):
            call("qg_ens_spectra", self._ens, _ptr(out))
        return out

    def run_spectra(self, first_step, nsteps, every):
        """qg_ens_run_spectra: :meth:`run` that records :meth:`spectra` after every ``every``-th
        step on the device, without a host round trip.  Returns the (nsteps // every, B, 5, M/2+1)
        float64 device tensor of records.  Not synchronised."""
        return _run_spectra("qg_ens_run_spectra", self._ens, self.device, self.zeta.device,
                            (self.nmembers, _lib.QG_SPEC_LINES, self.model.M // 2 + 1), first_step, nsteps, every)

    # ---- (kx, ky) and isotropic spectra (include/qg_mi355_spectra2d.h) ----
    def spectra2d(self, full=False):
        """qg_ens_spectra2d: every member's isotropic spectrum of the newest state as a
        (B, 5, NK) float64 device tensor, or with ``full=True`` ``(full2d, iso)`` with the
        (B, 5, P, M/2+1) spectra over (ky, kx); member b's blocks are bit for bit
        :meth:`State.spectra2d` of a State holding member b's arrays.  Three launches per batch
        of members on the current stream, not synchronised."""
        return _spectra2d("qg_ens_spectra2d", self._ens, self.device, self.zeta.device, (self.nmembers,),
                          self.model, full)

    def run_iso_spectra(self, first_step, nsteps, every):
        """qg_ens_run_iso_spectra: :meth:`run` that records the isotropic spectra of
        :meth:`spectra2d` after every ``every``-th step on the device, without a host round trip.
        Returns the (nsteps // every, B, 5, NK) float64 device tensor of records.  Not
        synchronised."""
        return _run_spectra("qg_ens_run_iso_spectra", self._ens, self.device, self.zeta.device,
                            (self.nmembers, _lib.QG_SPEC_LINES, iso_shells(self.model.M, self.model.P)),
                            first_step, nsteps, every)

    # ---- zonal-mean profiles per latitude (include/qg_mi355_profiles.h) ----
    def profiles(self):
        """qg_ens_profiles: every member's per-latitude lines of the newest state as a
        (B, 12, P) float64 device tensor; member b's block is bit for bit :meth:`State.profiles`
        of a State holding member b's arrays.  One launch for all members on the current stream,
        not synchronised."""
        torch = _torch()
        out = torch.empty((self.nmembers, _lib.QG_PROF_LINES, self.model.P), dtype=torch.float64,
                          device=self.zeta.device)
        with torch.cuda.device(self.device):
            call("qg_ens_profiles", self._ens, _ptr(out))
        return out

    def run_profiles(self, first_step, nsteps, every):
        """qg_ens_run_profiles: :meth:`run` that records :meth:`profiles` after every
        ``every``-th step on the device, without a host round trip.  Returns the
        (nsteps // every, B, 12, P) float64 device tensor of records.  Not synchronised."""
        return _run_spectra("qg_ens_run_profiles", self._ens, self.device, self.zeta.device,
                            (self.nmembers, _lib.QG_PROF_LINES, self.model.P), first_step, nsteps, every)


class Tracers:
    """Passive tracers advected by the layer flow of a :class:`State` or an :class:`Ensemble`
    (include/qg_mi355_tracers.h): tracer k lives in layer ``layers[k]`` (0 or 1), has the
    diffusivity ``kappa[k]`` >= 0 and the imposed mean meridional gradient ``gamma[k]``,

      G_k = ((kappa_k laplace_5p(c_k) - J(dx, c_k, psi_l)) - U_l cd(c_k)) - gamma_k cd(psi_l)

    stepped by the reference's Euler / AB3 update on its own history, bit for bit the numpy
    expression on the owner's newest psi.  The owner is never changed.

    ``c`` and ``g_store`` are (3, NT, P+2, M+2) float64 tensors -- (B, 3, NT, P+2, M+2) for an
    Ensemble -- whose slots rotate: :meth:`slot` names the physical slot of logical slot 1 (the
    newest), :meth:`current` returns the newest field.  Fill slot 0 (:meth:`set`) and call
    :meth:`reset` before the first advance.  F64, one rank, M and P >= 3, no sweep ensembles
    (QGError with QG_ERR_UNSUPPORTED otherwise).  Close it before its owner."""

    def __init__(self, owner, layers, kappa=None, gamma=None):
        torch = _torch()
        layers = [int(v) for v in layers]
        nt = len(layers)
        kappa = [0.0] * nt if kappa is None else [float(v) for v in kappa]
        gamma = [0.0] * nt if gamma is None else [float(v) for v in gamma]
        if len(kappa) != nt or len(gamma) != nt:
            raise ValueError(f"{nt} layers, {len(kappa)} kappa, {len(gamma)} gamma: one of each per tracer")
        self.owner = owner
        self.ntracers = nt
        self.layers, self.kappa, self.gamma = layers, kappa, gamma
        self.device = owner.device
        self.nmembers = getattr(owner, "nmembers", None)
        m = owner.model
        tp = (_lib.QgTracerParams * max(nt, 1))()
        for k in range(nt):
            tp[k].layer, tp[k].reserved, tp[k].kappa, tp[k].gamma = layers[k], 0, kappa[k], gamma[k]
        self._trc = C.c_void_p()
        with torch.cuda.device(self.device):
            # created first: an unsupported owner is refused before anything is allocated
            if self.nmembers is None:
                call("qg_tracers_create", owner._ctx, nt, tp, C.byref(self._trc))
            else:
                call("qg_ens_tracers_create", owner._ens, nt, tp, C.byref(self._trc))
            shape = (3, nt, m.P + 2, m.M + 2)
            if self.nmembers is not None:
                shape = (self.nmembers,) + shape
            self.c = torch.zeros(shape, dtype=torch.float64, device=owner.psi.device)
            self.g_store = torch.zeros(shape, dtype=torch.float64, device=owner.psi.device)
            call("qg_tracers_bind", self._trc, _ptr(self.c), _ptr(self.g_store))

    def close(self):
        """Destroy the library handle now (qg_tracers_destroy); the tensors stay with the caller."""
        trc = getattr(self, "_trc", None)
        if trc and _lib._lib is not None:
            _lib._lib.qg_tracers_destroy(trc)
            self._trc = None

    def __del__(self):
        self.close()

    def bind(self, c, g_store):
        """qg_tracers_bind: other arrays of the same shape (the caller keeps them alive); follow
        with :meth:`reset` or :meth:`set_state`."""
        for t in (c, g_store):
            if tuple(t.shape) != tuple(self.c.shape) or t.dtype != self.c.dtype or not t.is_contiguous():
                raise ValueError(f"expected contiguous float64 tensors of shape {tuple(self.c.shape)}")
        call("qg_tracers_bind", self._trc, _ptr(c), _ptr(g_store))
        self.c, self.g_store = c, g_store

    def set(self, k, field):
        """Tracer k's initial interior: ``field`` is (P, M) -- (B, P, M) or (P, M) for every member
        of an Ensemble -- written into slot 0; :meth:`reset` then fills the ghost ring."""
        torch = _torch()
        f = torch.as_tensor(field, dtype=torch.float64, device=self.c.device)
        self.c[..., 0, int(k), 1:-1, 1:-1] = f

    def reset(self):
        """qg_tracers_reset: slot 0 of ``c`` becomes the initial tracers (ghost ring filled from
        the interior), everything else zero, age 0."""
        with _torch().cuda.device(self.device):
            call("qg_tracers_reset", self._trc)
        return self

    def advance(self):
        """qg_tracers_advance: one tracer step with the owner's newest psi; the owner is not
        touched.  Call it before the owner's step of the same timestep."""
        with _torch().cuda.device(self.device):
            call("qg_tracers_advance", self._trc)

    def step(self, timestep):
        """qg_tracers_step: :meth:`advance`, then the owner's step."""
        with _torch().cuda.device(self.device):
            call("qg_tracers_step", self._trc, int(timestep))

    def run(self, first_step, nsteps, every=None):
        """qg_tracers_run: ``nsteps`` of :meth:`step`.  With ``every=k`` the diagnostics record is
        taken on the device after every k-th step: returns the (nsteps // k, [B,] NT, 6) float64
        device tensor of records (see :data:`TRACER_LINES`).  Not synchronised."""
        torch = _torch()
        if every is None:
            with torch.cuda.device(self.device):
                call("qg_tracers_run", self._trc, int(first_step), int(nsteps), 1, None, 0, None)
            return None
        lead = () if self.nmembers is None else (self.nmembers,)
        return _run_spectra("qg_tracers_run", self._trc, self.device, self.c.device,
                            lead + (self.ntracers, _lib.QG_TRC_LINES), first_step, nsteps, every)

    def diagnostics(self):
        """qg_tracers_diagnostics: the ([B,] NT, 6) float64 device tensor of the newest tracers'
        records, columns in the order of :data:`TRACER_LINES`.  Not synchronised."""
        torch = _torch()
        lead = () if self.nmembers is None else (self.nmembers,)
        out = torch.empty(lead + (self.ntracers, _lib.QG_TRC_LINES), dtype=torch.float64, device=self.c.device)
        with torch.cuda.device(self.device):
            call("qg_tracers_diagnostics", self._trc, _ptr(out))
        return out

    def slot(self, which, logical):
        w = {"c": 0, "g_store": 1}[which]
        out = C.c_int()
        call("qg_tracers_slot", self._trc, w, int(logical), C.byref(out))
        return out.value

    def current(self, k):
        """The newest field of tracer k: a (P+2, M+2) view, (B, P+2, M+2) for an Ensemble."""
        return self.c[..., self.slot("c", 1), int(k), :, :]

    def state(self):
        """qg_tracers_get_state: ``(age, [head_c, head_g_store])`` for a checkpoint beside the
        two tensors."""
        age, heads = C.c_int64(), (C.c_int * 2)()
        call("qg_tracers_get_state", self._trc, C.byref(age), heads)
        return age.value, list(heads)

    def set_state(self, age, heads):
        """qg_tracers_set_state: resume from :meth:`state` with the tensors' contents restored."""
        call("qg_tracers_set_state", self._trc, int(age), (C.c_int * 2)(*[int(h) for h in heads]))

    def set_form(self, form):
        """qg_tracers_set_form: ``_lib.QG_TRC_FORM_*`` (0: chosen by size)."""
        call("qg_tracers_set_form", self._trc, int(form))


TRACER_LINES = ("sum", "variance", "min", "max", "flux_v", "grad2")
"""The columns of a tracer diagnostics record, interior points only, indices wrapping:
dx^2 sum c; 1/2 dx^2 sum c^2; min; max; (1/(M P)) sum v_l c with v_l = cd(psi_l); and
1/2 sum (cx^2 + cy^2) of the forward differences."""


def tracer_dicts(records):
    """Records of :meth:`Tracers.diagnostics` or :meth:`Tracers.run` -- (..., 6), any leading
    dimensions -- as a dict of (...) blocks keyed by :data:`TRACER_LINES`."""
    return {name: records[..., q] for q, name in enumerate(TRACER_LINES)}


def eddy_diffusivity(records, gamma):
    """K = -flux_v / Gamma per tracer from records (..., NT, 6) and the NT gradients: (..., NT)
    of the records' kind (infinite or nan where Gamma is 0)."""
    flux = records[..., 4]
    if isinstance(flux, np.ndarray):
        with np.errstate(divide="ignore", invalid="ignore"):
            return -flux / np.asarray(gamma, dtype=np.float64)
    torch = _torch()
    return -flux / torch.as_tensor(gamma, dtype=torch.float64, device=flux.device)


class Floats:
    """Lagrangian floats advected by the layer flow of a :class:`State` or an :class:`Ensemble`
    (include/qg_mi355_floats.h): ``n0`` floats in layer 0, then ``n1`` in layer 1, in every
    member.  A float's velocity is the bilinear interpolant of the centred-difference node
    velocities of the owner's newest psi (plus ``U`` in layer 0), stepped by the reference's
    Euler / AB3 update on its own history, bit for bit the header's contract in numpy.  The
    owner is never changed.

    ``pos`` and ``origin`` are (2, N) float64 tensors -- (B, 2, N) for an Ensemble -- holding
    xi (along x, M points) and eta in grid units, unwrapped; ``hist`` is (2, 2, N) -- (B, 2, 2,
    N) -- with the two previous (u, v) in m/s.  :meth:`seed` and :meth:`reset` before the first
    advance.  F64, one rank, M and P >= 3, no sweep ensembles (QGError with QG_ERR_UNSUPPORTED
    otherwise).  Close it before its owner."""

    def __init__(self, owner, n0, n1=0):
        torch = _torch()
        self.owner = owner
        self.n0, self.n1 = int(n0), int(n1)
        self.nfloats = self.n0 + self.n1
        self.device = owner.device
        self.nmembers = getattr(owner, "nmembers", None)
        self._flt = C.c_void_p()
        with torch.cuda.device(self.device):
            # created first: an unsupported owner or count is refused before anything is allocated
            if self.nmembers is None:
                call("qg_floats_create", owner._ctx, self.n0, self.n1, C.byref(self._flt))
            else:
                call("qg_ens_floats_create", owner._ens, self.n0, self.n1, C.byref(self._flt))
            lead = () if self.nmembers is None else (self.nmembers,)
            kw = dict(dtype=torch.float64, device=owner.psi.device)
            self.pos = torch.zeros(lead + (2, self.nfloats), **kw)
            self.origin = torch.zeros(lead + (2, self.nfloats), **kw)
            self.hist = torch.zeros(lead + (2, 2, self.nfloats), **kw)
            call("qg_floats_bind", self._flt, _ptr(self.pos), _ptr(self.origin), _ptr(self.hist))

    def close(self):
        """Destroy the library handle now (qg_floats_destroy); the tensors stay with the caller."""
        flt = getattr(self, "_flt", None)
        if flt and _lib._lib is not None:
            _lib._lib.qg_floats_destroy(flt)
            self._flt = None

    def __del__(self):
        self.close()

    def _lead(self):
        return () if self.nmembers is None else (self.nmembers,)

    def bind(self, pos, origin, hist):
        """qg_floats_bind: other arrays of the same shapes (the caller keeps them alive); follow
        with :meth:`reset` or :meth:`set_state`."""
        for t, ref in ((pos, self.pos), (origin, self.origin), (hist, self.hist)):
            if tuple(t.shape) != tuple(ref.shape) or t.dtype != ref.dtype or not t.is_contiguous():
                raise ValueError(f"expected a contiguous float64 tensor of shape {tuple(ref.shape)}")
        call("qg_floats_bind", self._flt, _ptr(pos), _ptr(origin), _ptr(hist))
        self.pos, self.origin, self.hist = pos, origin, hist

    def seed(self, xi, eta):
        """The initial positions in grid units: ``xi`` and ``eta`` are (N,) -- or (B, N) -- and
        go into ``pos``; :meth:`reset` then makes them the origin."""
        torch = _torch()
        self.pos[..., 0, :] = torch.as_tensor(xi, dtype=torch.float64, device=self.pos.device)
        self.pos[..., 1, :] = torch.as_tensor(eta, dtype=torch.float64, device=self.pos.device)
        return self

    def reset(self):
        """qg_floats_reset: origin = pos, hist = 0, head = 0, age = 0."""
        with _torch().cuda.device(self.device):
            call("qg_floats_reset", self._flt)
        return self

    def advance(self):
        """qg_floats_advance: one float step with the owner's newest psi; the owner is not
        touched.  Call it before the owner's step of the same timestep."""
        with _torch().cuda.device(self.device):
            call("qg_floats_advance", self._flt)

    def step(self, timestep):
        """qg_floats_step: :meth:`advance`, then the owner's step."""
        with _torch().cuda.device(self.device):
            call("qg_floats_step", self._flt, int(timestep))

    def run(self, first_step, nsteps, every=None, trajectories=True, stats=True):
        """qg_floats_run: ``nsteps`` of :meth:`step`.  With ``every=k``, after every k-th step the
        positions and / or the statistics record are kept on the device: returns
        ``(traj, records)`` -- (nsteps // k, [B,] 2, N) and (nsteps // k, [B,] 2, 8) float64
        device tensors, ``None`` for the one switched off.  Not synchronised."""
        torch = _torch()
        first_step, nsteps = int(first_step), int(nsteps)
        if every is None or not (trajectories or stats):
            with torch.cuda.device(self.device):
                call("qg_floats_run", self._flt, first_step, nsteps, 1, None, None, 0, None)
            return None
        every = int(every)
        if every < 1:
            raise ValueError("every must be >= 1")
        n = max(nsteps, 0) // every
        kw = dict(dtype=torch.float64, device=self.pos.device)
        # (an empty tensor has no address: one spare record keeps the pointer non-null)
        traj = torch.zeros((max(n, 1),) + self._lead() + (2, self.nfloats), **kw) if trajectories else None
        rec = torch.zeros((max(n, 1),) + self._lead() + (2, _lib.QG_FLT_LINES), **kw) if stats else None
        got = C.c_int64()
        with torch.cuda.device(self.device):
            call("qg_floats_run", self._flt, first_step, nsteps, every, None if traj is None else _ptr(traj),
                 None if rec is None else _ptr(rec), n, C.byref(got))
        return (None if traj is None else traj[:got.value], None if rec is None else rec[:got.value])

    def stats(self):
        """qg_floats_stats: the ([B,] 2, 8) float64 device tensor of the Lagrangian record, one
        row per layer, columns in the order of :data:`FLOAT_LINES`.  Not synchronised."""
        torch = _torch()
        out = torch.empty(self._lead() + (2, _lib.QG_FLT_LINES), dtype=torch.float64, device=self.pos.device)
        with torch.cuda.device(self.device):
            call("qg_floats_stats", self._flt, _ptr(out))
        return out

    def sample(self, field="psi"):
        """qg_floats_sample: the owner's newest ``"psi"`` or ``"zeta"`` of each float's own layer
        at its position (the contract's bilinear lines): ([B,] N) float64, on the device."""
        torch = _torch()
        f = {"psi": _lib.QG_FLT_PSI, "zeta": _lib.QG_FLT_ZETA}[field]
        out = torch.empty(self._lead() + (self.nfloats,), dtype=torch.float64, device=self.pos.device)
        with torch.cuda.device(self.device):
            call("qg_floats_sample", self._flt, f, _ptr(out))
        return out

    def state(self):
        """qg_floats_get_state: ``(age, head)`` for a checkpoint beside the three tensors."""
        age, head = C.c_int64(), C.c_int()
        call("qg_floats_get_state", self._flt, C.byref(age), C.byref(head))
        return age.value, head.value

    def set_state(self, age, head):
        """qg_floats_set_state: resume from :meth:`state` with the tensors' contents restored."""
        call("qg_floats_set_state", self._flt, int(age), int(head))


FLOAT_LINES = ("n", "mean_dx", "mean_dy", "var_dx", "var_dy", "cov_dxdy", "kinetic", "pair_dispersion")
"""The columns of a floats record, one row per layer, physical units: the number of floats; the
mean displacements <Dx>, <Dy> with D = (pos - origin) dx; the second moments <Dx^2>, <Dy^2>,
<Dx Dy> (about zero, not about the mean); 1/2 <u^2 + v^2> of the newest sampled velocities; and
<|r_2p - r_2p+1|^2> over the consecutive pairs of the layer's floats."""


def float_dicts(records):
    """Records of :meth:`Floats.stats` or :meth:`Floats.run` -- (..., 8), any leading dimensions
    -- as a dict of (...) blocks keyed by :data:`FLOAT_LINES`."""
    return {name: records[..., q] for q, name in enumerate(FLOAT_LINES)}


def float_positions(pos, dx, wrap=False):
    """Positions (..., 2, N) in grid units as metres: x = xi dx, y = eta dx.  ``wrap=(M, P)``
    folds them into the domain [0, M dx) x [0, P dx) first; the unwrapped ones (``wrap=False``)
    keep the turns a float has made.  numpy in, numpy out; torch in, torch out."""
    if not wrap:
        return pos * dx
    M, P = wrap
    floor = np.floor if isinstance(pos, np.ndarray) else (lambda t: t.floor())
    out = pos.copy() if isinstance(pos, np.ndarray) else pos.clone()
    for comp, n in ((0, int(M)), (1, int(P))):
        x = out[..., comp, :]
        out[..., comp, :] = x - floor(x / n) * n
    return out * dx


TSTATS_LAYER_FIELDS = ("mean_psi", "mean_zeta", "mean_u", "mean_v", "var_psi", "var_zeta", "var_u", "var_v",
                       "cov_u_v", "cov_u_zeta", "cov_v_zeta")
TSTATS_FIELDS = (tuple(f"{n}_{l}" for l in (1, 2) for n in TSTATS_LAYER_FIELDS)
                 + ("mean_tau", "mean_vb", "var_tau", "cov_vb_tau"))
"""The 26 fields of include/qg_mi355_tstats.h in index order (layers 1-based, as the reference
counts them): per layer the time means of psi, zeta, u, v, their variances, the Reynolds stress
<u'v'> and the eddy vorticity fluxes <u'zeta'>, <v'zeta'>; then tau = psi_1 - psi_2,
vb = (v_1 + v_2) / 2, var tau and the eddy heat flux <vb'tau'>.  u and v are the centred-difference
velocities of psi: the eddy flow, without the model's U."""

TSTATS_SUMMARY_LINES = ("mke_1", "mke_2", "eke_1", "eke_2", "mean_enstrophy_1", "mean_enstrophy_2",
                        "eddy_enstrophy_1", "eddy_enstrophy_2", "mean_ape", "eddy_ape", "heat_flux", "n")


def tstats_field_names():
    """The names :meth:`TimeStats.field` accepts, in the header's index order."""
    return TSTATS_FIELDS


class TimeStats:
    """Running time statistics of a :class:`State` or of every member of an :class:`Ensemble`
    (include/qg_mi355_tstats.h): time means, variances and eddy covariances as fields, accumulated
    on the device sample by sample with Welford's recurrence in float64, bit for bit the header's
    contract in numpy.  The owner is never written.

    ``level="eddy"`` keeps all 26 fields of :func:`tstats_field_names`; ``level="mean"`` only
    ``mean_psi`` and ``mean_zeta`` of both layers, at a fifth of the memory traffic.  One rank,
    M and P >= 3; F64 or F32 states, uniform or sweep ensembles.  Close it before its owner."""

    def __init__(self, owner, level="eddy"):
        torch = _torch()
        self.owner = owner
        self.level = {"mean": _lib.QG_TSTATS_MEAN, "eddy": _lib.QG_TSTATS_EDDY}[level]
        self.device = owner.device
        self.nmembers = getattr(owner, "nmembers", None)
        self._ts = C.c_void_p()
        with torch.cuda.device(self.device):
            if self.nmembers is None:
                call("qg_tstats_create", owner._ctx, self.level, C.byref(self._ts))
            else:
                call("qg_ens_tstats_create", owner._ens, self.level, C.byref(self._ts))

    def close(self):
        """Destroy the library handle and its accumulators now (qg_tstats_destroy)."""
        ts = getattr(self, "_ts", None)
        if ts and _lib._lib is not None:
            _lib._lib.qg_tstats_destroy(ts)
            self._ts = None

    def __del__(self):
        self.close()

    def _lead(self):
        return () if self.nmembers is None else (self.nmembers,)

    def _out(self, shape):
        torch = _torch()
        return torch.empty(self._lead() + shape, dtype=torch.float64, device=self.owner.psi.device)

    def reset(self):
        """qg_tstats_reset: n = 0, every accumulator +0.0."""
        with _torch().cuda.device(self.device):
            call("qg_tstats_reset", self._ts)
        return self

    def accumulate(self):
        """qg_tstats_accumulate: one sample of the owner's newest state.  Not synchronised."""
        with _torch().cuda.device(self.device):
            call("qg_tstats_accumulate", self._ts)

    def run(self, first_step, nsteps, every=1):
        """qg_tstats_run: ``nsteps`` steps of the owner, one sample after every ``every``-th."""
        with _torch().cuda.device(self.device):
            call("qg_tstats_run", self._ts, int(first_step), int(nsteps), int(every))

    @property
    def count(self):
        """qg_tstats_count: the samples since the last :meth:`reset` (or the n of :meth:`load`)."""
        n = C.c_int64()
        call("qg_tstats_count", self._ts, C.byref(n))
        return n.value

    def field(self, field):
        """qg_tstats_field: one field by name (:func:`tstats_field_names`) or index as a
        ([B,] P+2, M+2) float64 device tensor with its periodic ghost ring: a mean as stored, a
        variance or covariance as C / (n - 1) (0 for n = 1).  Not synchronised."""
        k = TSTATS_FIELDS.index(field) if isinstance(field, str) else int(field)
        m = self.owner.model
        out = self._out((m.P + 2, m.M + 2))
        with _torch().cuda.device(self.device):
            call("qg_tstats_field", self._ts, k, _ptr(out))
        return out

    def summary(self):
        """qg_tstats_summary: the ([B,] 12) record of :data:`TSTATS_SUMMARY_LINES` (eddy level)."""
        out = self._out((_lib.QG_TSTATS_SUM_LINES,))
        with _torch().cuda.device(self.device):
            call("qg_tstats_summary", self._ts, _ptr(out))
        return out

    def save(self):
        """qg_tstats_save: ``(raw, n)``, the accumulators as an opaque float64 device tensor and
        the count, for :meth:`load` of a handle of the same owner shape and level."""
        torch = _torch()
        nd = C.c_int64()
        call("qg_tstats_raw_doubles", self._ts, C.byref(nd))
        raw = torch.empty((nd.value,), dtype=torch.float64, device=self.owner.psi.device)
        with torch.cuda.device(self.device):
            call("qg_tstats_save", self._ts, _ptr(raw))
        return raw, self.count

    def load(self, raw, n):
        """qg_tstats_load: resume from :meth:`save`."""
        torch = _torch()
        nd = C.c_int64()
        call("qg_tstats_raw_doubles", self._ts, C.byref(nd))
        if raw.dtype != torch.float64 or raw.numel() != nd.value or not raw.is_contiguous() or not raw.is_cuda:
            raise ValueError(f"expected a contiguous float64 device tensor of {nd.value} elements")
        with torch.cuda.device(self.device):
            call("qg_tstats_load", self._ts, _ptr(raw), int(n))
        return self


def eke(ts):
    """The eddy kinetic energy map of a :class:`TimeStats` at the eddy level: 1/2 (var u + var v)
    per layer, a ([B,] 2, P+2, M+2) device tensor."""
    torch = _torch()
    return torch.stack([0.5 * (ts.field(f"var_u_{l}") + ts.field(f"var_v_{l}")) for l in (1, 2)], dim=-3)


PROFILE_LINES = ("energy_1", "energy_2", "enstrophy_1", "enstrophy_2", "interface", "psi_mean_1", "psi_mean_2",
                 "zeta_mean_1", "zeta_mean_2", "vort_flux_1", "vort_flux_2", "heat_flux")
"""The rows of a profiles record (layers 1-based, as the reference counts them), each a function
of the interior row j.  Interior i = 0..M-1, i -+ 1 and j + 1 wrap; px = psi_l(i+1,j) - psi_l(i,j),
py = psi_l(i,j+1) - psi_l(i,j), v_l = (psi_l(i+1,j) - psi_l(i-1,j)) * 0.5/dx (the reference's cd):

  rows 0, 1   energy[l]     1/2 sum_i (px^2 + py^2)
  rows 2, 3   enstrophy[l]  1/2 dx^2 sum_i zeta_l^2
  row  4      interface     1/2 dx^2 sum_i (psi_1 - psi_2)^2
  rows 5, 6   psi_mean[l]   (1/M) sum_i psi_l
  rows 7, 8   zeta_mean[l]  (1/M) sum_i zeta_l
  rows 9, 10  vort_flux[l]  (1/M) sum_i v_l zeta_l
  row  11     heat_flux     (1/M) sum_i 1/2 (v_1 + v_2) (psi_1 - psi_2)

Rows 0-4 sum over j to ``diagnostics()["energy"]``, ``["enstrophy"]`` and ``["interface"]``;
M dx^2 sum_j zeta_mean[l] is ``["zeta_sum"][l]``."""


def zonal_wind(records, dx):
    """The zonal-mean zonal wind of both layers from the ``psi_mean`` rows of profiles records:
    u_l(j) = -(psi_mean_l(j+1) - psi_mean_l(j-1)) * 0.5/dx, rows wrapping.  ``records``: a
    (..., 12, P) tensor or array with any leading dimensions; returns (..., 2, P) of its kind."""
    pm = records[..., 5:7, :]
    if isinstance(pm, np.ndarray):
        return -(np.roll(pm, -1, axis=-1) - np.roll(pm, 1, axis=-1)) * (0.5 / float(dx))
    return -(pm.roll(-1, -1) - pm.roll(1, -1)) * (0.5 / float(dx))


def profile_dict(record):
    """One (12, P) profiles record as a dict in the manner of :meth:`State.diagnostics`:
    ``energy``, ``enstrophy``, ``psi_mean``, ``zeta_mean`` and ``vort_flux`` hold the two layers'
    lines as a (2, P) block, ``interface`` and ``heat_flux`` one (P,) line."""
    return {"energy": record[0:2], "enstrophy": record[2:4], "interface": record[4], "psi_mean": record[5:7],
            "zeta_mean": record[7:9], "vort_flux": record[9:11], "heat_flux": record[11]}


SPECTRA_LINES = ("energy_1", "energy_2", "enstrophy_1", "enstrophy_2", "interface")
"""The rows of a spectra record (layers 1-based, as the reference counts them): rows 0-1 sum over
k to ``diagnostics()["energy"]``, rows 2-3 to ``["enstrophy"]``, row 4 to ``["interface"]``."""
SPECTRA_STRIP_CAP = _lib.QG_SPEC_MAX_STRIPS
"""Row strips of the spectra kernel: min(P, this), a function of P only (qg_mi355_spectra.h)."""


def spectra_wavenumbers(M, dx):
    """The zonal wavenumbers 2 pi k / (M dx), k = 0 .. M/2, of the columns of a spectra record."""
    return 2.0 * np.pi * np.arange(int(M) // 2 + 1) / (int(M) * float(dx))


ISO_LINES = SPECTRA_LINES
"""The rows of an isotropic or (kx, ky) spectrum (include/qg_mi355_spectra2d.h): those of
:data:`SPECTRA_LINES`, with the same sums."""


def iso_shells(M, P):
    """qg_iso_shells: the number NK of shells of an (M, P) grid (a host function: no device)."""
    nk = _lib.lib().qg_iso_shells(int(M), int(P))
    if nk < 0:
        raise _lib.QGError("qg_iso_shells", nk)
    return nk


def iso_wavenumbers(M, P, dx):
    """``(k, counts)`` of the columns of an isotropic spectrum: the shell centres
    k[n] = 2 pi n / (max(M, P) dx) in rad/m, and per shell the number of full-plane (kx, ky) cells
    it holds (qg_iso_shell_counts; they sum to M P) for normalising to a density."""
    nk = iso_shells(M, P)
    counts = (C.c_int64 * nk)()
    call("qg_iso_shell_counts", int(M), int(P), counts)
    return (2.0 * np.pi * np.arange(nk) / (max(int(M), int(P)) * float(dx)),
            np.frombuffer(counts, dtype=np.int64).copy())


def _spectra2d(name, handle, device, tdev, lead, model, full):
    torch = _torch()
    M, P = int(model.M), int(model.P)
    iso = torch.empty(tuple(lead) + (_lib.QG_SPEC_LINES, iso_shells(M, P)), dtype=torch.float64, device=tdev)
    out = torch.empty(tuple(lead) + (_lib.QG_SPEC_LINES, P, M // 2 + 1), dtype=torch.float64,
                      device=tdev) if full else None
    with torch.cuda.device(device):
        call(name, handle, _ptr(out) if full else None, _ptr(iso))
    return (out, iso) if full else iso


def _run_spectra(name, handle, device, tdev, shape, first_step, nsteps, every):
    torch = _torch()
    if int(every) < 1:
        raise ValueError(f"every = {every}: must be at least 1")
    n = max(int(nsteps), 0) // int(every)
    # (at least one record: a null pointer is refused also when no record is due)
    rec = torch.zeros((max(n, 1),) + tuple(shape), dtype=torch.float64, device=tdev)
    got = C.c_int64()
    with torch.cuda.device(device):
        call(name, handle, int(first_step), int(nsteps), int(every), _ptr(rec), n, C.byref(got))
    return rec[:got.value]


SPREAD_LEN = C.sizeof(_lib.QgSpread) // 8


def spread_dicts(records):
    """Rows of 16 doubles (a records tensor of :meth:`Ensemble.run_recorded`, or any sequence of
    rows) as dicts keyed by qg_spread's fields: per-layer lists, ``step`` and ``nmembers``."""
    rows = records.cpu().tolist() if hasattr(records, "cpu") else [list(r) for r in records]
    out = []
    for row in rows:
        d, k = {}, 0
        for f, t in _lib.QgSpread._fields_:
            n = getattr(t, "_length_", 0)
            if f != "reserved":
                d[f] = list(row[k:k + n]) if n else row[k]
            k += n or 1
        out.append(d)
    return out


def run_ensemble_no_output(m, nmembers, nsteps=None, seeds=None, record_every=None, **kw):
    """run_model_no_output for B members at once: init, floor(T/dt) steps; returns the Ensemble.
    (``members=``: per-member parameters, see :class:`Ensemble`.)  With ``record_every=k`` the
    spread record is taken on the device after every k-th step: returns (ens, records), see
    :meth:`Ensemble.run_recorded`."""
    ens = Ensemble(m, nmembers, **kw).initialise(seeds)
    total = int(np.floor(m.T / m.dt)) if nsteps is None else int(nsteps)
    if record_every is not None:
        return ens, ens.run_recorded(1, total, record_every)
    ens.run(1, total)
    return ens


# ---- stateless operators on (P+2, M+2) device matrices -----------------------------------
def _dims(u):
    P2, M2 = u.shape[-2:]
    return M2 - 2, P2 - 2


def laplace_5p(u, dx):
    torch = _torch()
    M, P = _dims(u)
    _check_field(u, M, P)
    out = torch.empty_like(u)
    call("qg_laplace_5p", _ptr(u), _ptr(out), M, P, float(dx), _stream_ptr())
    return out


def cd(u, dx):
    torch = _torch()
    M, P = _dims(u)
    _check_field(u, M, P)
    out = torch.empty_like(u)
    call("qg_cd", _ptr(u), _ptr(out), M, P, float(dx), _stream_ptr())
    return out


def J(dx, zeta, psi):
    torch = _torch()
    M, P = _dims(zeta)
    _check_field(zeta, M, P)
    _check_field(psi, M, P)
    out = torch.empty_like(zeta)
    call("qg_arakawa_J", _ptr(zeta), _ptr(psi), _ptr(out), M, P, float(dx), _stream_ptr())
    return out


def update_doubly_periodic_bc_(b):
    M, P = _dims(b)
    _check_field(b, M, P)
    call("qg_fill_ghosts", _ptr(b), M, P, _stream_ptr())
    return b


class PairSolver:
    """qg_solver handle: A_s x_s = proj_in . f for s = 0 (optionally pinned Poisson), 1."""

    def __init__(self, M, P, dx, alpha, pinned=(0, 0), proj_in=(1, 0, 0, 1), proj_out=(1, 0, 0, 1),
                 kind=_lib.QG_SOLVER_SPECTRAL, precond=_lib.QG_PRECOND_SPECTRAL):
        torch = _torch()
        self.M, self.P = M, P
        self._h = C.c_void_p()
        call("qg_solver_create", int(M), int(P), float(dx), (C.c_double * 2)(*alpha),
             (C.c_int * 2)(*pinned), (C.c_double * 4)(*proj_in), (C.c_double * 4)(*proj_out),
             int(kind), int(precond), int(torch.cuda.current_device()), _stream_ptr(), C.byref(self._h))

    def solve(self, f1, f2=None, out1=None, out2=None):
        torch = _torch()
        _check_field(f1, self.M, self.P)
        out1 = torch.empty_like(f1) if out1 is None else out1
        call("qg_solver_solve", self._h, _ptr(f1), _ptr(f2) if f2 is not None else None, _ptr(out1),
             _ptr(out2) if out2 is not None else None)
        return out1 if out2 is None else (out1, out2)

    def __del__(self):
        if getattr(self, "_h", None) and _lib._lib is not None:
            _lib._lib.qg_solver_destroy(self._h)
            self._h = None


def sp_solve_modified_helmholtz(M, P, dx, f, alpha, **kw):
    """laplacian.jl:78-86: solution x of construct_spA(M,P,dx,alpha) x = f, with ghosts."""
    s = PairSolver(M, P, dx, (float(alpha), -1.0), (0, 0), (1, 0, 0, 0), (1, 0, 0, 0), **kw)
    return s.solve(f)


def sp_solve_poisson(M, P, dx, f, **kw):
    """laplacian.jl:100-111: the pinned Poisson solve (x = 0 at interior (1,1))."""
    s = PairSolver(M, P, dx, (0.0, -1.0), (1, 0), (1, 0, 0, 0), (1, 0, 0, 0), **kw)
    return s.solve(f)
