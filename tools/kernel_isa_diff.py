"""Compare two builds of a HIP source file kernel by kernel on the ISA.

For a change that must leave existing kernels as they are (same bits, same speed): compile the
file before and after to gfx950 assembly and compare each function's instruction stream.

    F="-O3 -std=c++17 --offload-arch=gfx950 -Iinclude -S --cuda-device-only"
    git show REV:julia-ocean-modelling_amd/csrc/qg_spectral.hip > /tmp/old/qg_spectral.hip   # and its headers
    hipcc $F -I/tmp/old /tmp/old/qg_spectral.hip -o old.s
    hipcc $F -Ijulia-ocean-modelling_amd/csrc julia-ocean-modelling_amd/csrc/qg_spectral.hip -o new.s
    python tools/kernel_isa_diff.py old.s new.s        # (the Makefile's NOFMA files: add -ffp-contract=off)

A file split into several (or several files against their parent's one): compile each to its
own .s, concatenate them, and compare with the single old.s; the function labels summed over
the new files must also equal the old file's count (a kernel instantiated in two files would
show in neither list, only there).

    for f in julia-ocean-modelling_amd/csrc/qg_spec*.hip; do
        hipcc $F -Ijulia-ocean-modelling_amd/csrc $f -o new/$(basename $f .hip).s; done
    cat new/*.s > new.s
    python tools/kernel_isa_diff.py old.s new.s
    grep -c '^_Z[A-Za-z0-9_]*:' old.s new/*.s

Instructions are compared as text after dropping comments and directives and renumbering local
labels (their numbers depend on a function's position in the file).  A kernel template that
gained a trailing, empty parameter pack mangles differently (`...EJEEEv...DpT1_` for `...EEEv...`):
such names are matched to the old ones.  Prints the kernels that differ or are missing and the
counts; exit status 1 if an old kernel differs or is gone.  Functions only the new file has are
counted, not judged.

Record: the batched-ensemble change (qg_mi355_ensemble.h) left all 88 functions of
qg_spectral.hip and all 20 of qg_stencil.hip identical and added 20 + 1; the perturbed-parameter
change (qg_mi355_sweep.h) left all 108 + 21 identical and added 20 + 1 (profiles/sweep/).  The
split of qg_spectral.hip into one file per kernel family (qg_spec_*.hip: bluestein 15, carry 7,
gen 22, half 6, pow2 40, pow2_ens 36, twopoint 2, and qg_spectral.hip itself 0 functions) left
all 128 identical, differing or missing 0, new only 0, the labels summing to the old 128;
qg_stencil.hip (untouched) 22 identical.  With the generic and the split passes in files of
their own, the four generic kernels differed in the order of two scalar adds in the direct
DFT's loop (the families share dft_at); they share qg_spec_gen.hip for that reason.  The zonal
spectra (qg_mi355_spectra.h) left all 190 functions of the sixteen earlier files identical and
added the 20 of qg_spectra.hip (profiles/spectra/).  The profiles per latitude
(qg_mi355_profiles.h) left all 210 functions of the seventeen earlier files identical and added
the 12 of qg_profiles.hip (profiles/meridional/).  The 2-D and isotropic spectra
(qg_mi355_spectra2d.h) left all 222 functions of the eighteen earlier files identical and added
the 28 of qg_spectra2d.hip (profiles/spectra2d/isa_diff.txt).  The Lagrangian floats
(qg_mi355_floats.h) left all 257 functions of the twenty earlier files identical and added the 4 of
qg_floats.hip (profiles/floats/isa_diff.txt).  Moving the record families' entry points beside their
kernels (csrc/qg_owner.hpp, host code only) left every function of the seven files it touched
identical, differing or missing 0, new only 0, the labels equal: qg_spectra.hip 20,
qg_spectra2d.hip 28, qg_profiles.hip 12, qg_ens_stats.hip 4, qg_tracer.hip 7, qg_floats.hip 4,
qg_diag.hip 3 (78 in all).  The split of qg_stencil.hip into one file per tendency form (qg_ops.hip
7, qg_tend_ring.hip 9, qg_tend_pair.hip 1, qg_tend_direct.hip 5, qg_tend_launch.hip 0 functions) left
all 22 identical, differing or missing 0, new only 0, and qg_tracer.hip's 7 identical with the
shared arakawa_point (profiles/tend_split/isa_diff.txt); the ring and pair kernels written without
their prefetch-depth parameter (only PF = 1 exists) differed in all ten (tendency_kernel<256, 1,
double> 4527 -> 4546 instructions, tendency_pair_kernel 7516 -> 7576), so the parameter stays.
The split of qg_capi.hip by concern (qg_capi, qg_step, qg_ctx_io, qg_ctx_comm, qg_solver: host code,
0 functions each) with the operator entries moved into qg_ops.hip and the slot planner (qg_slots.hpp)
left qg_ops.hip 7, qg_tracer.hip 7, qg_comm.hip 5 and qg_pcg.hip 22 identical, differing or missing
0, new only 0, the labels equal (profiles/ctx_split/isa_diff.txt).  The restructured PcgSolver::solve
(openings, one direction step, named reductions: host code) left 17 of qg_pcg.hip's 22 functions
identical, the labels equal; the five that now share partial_tree<NV> differ, as intended, with the
additions per value in the same order: pcg_rank_sum 186 -> 190 instructions, pcg_rank_sumN<2> 180 ->
190, <4> 269 -> 279, <6> 357 -> 356, pcg_cert_latch_part 387 -> 388 (profiles/pcg_solve/isa_diff.txt).
The spectral solver's planner (csrc/qg_spec_plan.hpp: the row family, the transform plan, the chunk
rows, the carry geometry and the arena as host rules; the size constants moved there from
qg_spec_dev.hpp; launchers taking the family and the plan beside SpecArgs, whose layout is
untouched) left all 128 functions of the solver's files identical, differing or missing 0, new only
0, the labels equal file by file (bluestein 15, carry 7, gen 22, half 6, pow2 40, pow2_ens 36,
twopoint 2, qg_spectral.hip 0), and qg_pcg.hip's 22 identical, qg_ensemble.hip 0 functions
(profiles/spec_plan/isa_diff.txt).  The time statistics (qg_mi355_tstats.h) left all 261 functions
of the earlier files identical and added the 7 of qg_tstats.hip (profiles/tstats/isa_diff.txt).
"""
import re
import sys


def functions(path):
    out, cur, body = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, body = m.group(1), []
            out[cur] = body
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        t = re.sub(r"\s*;.*", "", line.strip())
        if not t or t.startswith("."):
            continue
        t = re.sub(r"\.LBB\d+_", ".LBB_", t)
        body.append(re.sub(r"\.L__unnamed_\d+|\.Ltmp\d+|\.str\.\d+", ".L", t))
    return out


def unpack_name(name):
    """The mangled name without an empty trailing template pack and its parameter expansion."""
    return re.sub(r"DpT\d_$", "", name.replace("JEEE", "EE"))


def main(old_path, new_path):
    # (both sides: the old file may already carry the packs)
    old = {unpack_name(k): v for k, v in functions(old_path).items()}
    new = {unpack_name(k): v for k, v in functions(new_path).items()}
    same = bad = 0
    for k in sorted(old):
        if k not in new:
            print("missing:", k)
            bad += 1
        elif old[k] != new[k]:
            print(f"differs: {k} ({len(old[k])} -> {len(new[k])} instructions)")
            bad += 1
        else:
            same += 1
    print(f"identical {same}, differing or missing {bad}, new only {len(set(new) - set(old))}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
