"""The two tendency kernels (the LDS-ring kernel for large grids, the cache-resident one for
grids below ~1.2 M points; csrc/qg_tend_ring.hip, csrc/qg_tend_direct.hip) evaluate the same expressions in the same
order: forced one way and the other (qg_set_form(QG_FORM_TENDENCY, QG_TEND_RING / _DIRECT)),
five Euler + AB3 steps give bit-identical states, on a square grid and on a ragged one (odd P,
M not a multiple of the 64-point tile); the same for the certifying tendency of the PCG solver."""
import hashlib
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "julia-ocean-modelling_amd")]


def _run(qg, form, M, P, solver):
    with qg.forced_form(qg._lib.QG_FORM_TENDENCY, form):
        st = qg.run_model_no_output(qg.bench_model(M, P=P), nsteps=5, solver=solver)
        h = hashlib.sha1()
        for n in ("zeta", "psi", "f_store"):
            h.update(st.to_numpy(n).tobytes())
        st.close()
    return h.hexdigest()


@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("M,P", [(256, 256), (200, 37)])
def test_ring_and_direct_tendency_kernels_bitwise(M, P, solver):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd as qg
    assert _run(qg, qg._lib.QG_TEND_RING, M, P, solver) == _run(qg, qg._lib.QG_TEND_DIRECT, M, P, solver)

