// The tendency's entry points (qg_common.hpp): each plans its launch (qg_tend_plan.hpp) and
// hands the plan to the form it names (qg_tend_forms.hpp).  The one device query, the resident
// workgroups of the chosen kernel, is made only for the balanced launches and cached per kernel.
#include "qg_tend_forms.hpp"

namespace qg {

namespace {

template <class T>
TendShape shape_of(const TendArgsT<T> &a, bool cert, int nmembers, int64_t cap) {
    return tend_shape(a.M, a.j0, a.j1, a.j2, a.j3, (int)sizeof(T), cert, nmembers, form(QG_FORM_TENDENCY),
                      form(QG_FORM_TENDENCY_TILE), cap);
}

// choose, ask the device where the choice needs it, size the grid
int plan_launch(const TendShape &sh, qg_tend_plan &p) {
    QG_CHECK(tend_choose(sh, p));
    int resident = 0;
    if (p.rows == 0) {
        if (p.kernel == QG_TEND_KERNEL_PAIR) QG_CHECK(tend_pair_resident(p, resident));
        else QG_CHECK(tend_ring_resident(p, sh.esize, sh.cert, resident));
    }
    return tend_grid(sh, resident, p);
}

template <class T>
int launch_tendency_t(const TendArgsT<T> &a, hipStream_t s) {
    if (a.j1 - a.j0 <= 0 && a.j3 - a.j2 <= 0) return QG_OK;
    qg_tend_plan p;
    QG_CHECK(plan_launch(shape_of(a, false, 0, 0), p));
    if (p.kernel == QG_TEND_KERNEL_DIRECT) return launch_tend_direct(a, p, s);
    if constexpr (sizeof(T) == 4) {
        if (p.kernel == QG_TEND_KERNEL_PAIR) return launch_tend_pair(a, p, s);
    }
    return launch_tend_ring(a, p, s);
}

}  // namespace

int launch_tendency(const TendArgsT<double> &a, hipStream_t s) { return launch_tendency_t(a, s); }
int launch_tendency(const TendArgsT<float> &a, hipStream_t s) { return launch_tendency_t(a, s); }

int launch_tendency_cert(const TendArgsT<double> &a, int64_t cap, int *nblk, hipStream_t s) {
    qg_tend_plan p;
    QG_CHECK(plan_launch(shape_of(a, true, 0, cap), p));
    *nblk = (int)p.blocks;
    if (p.blocks == 0) return QG_OK;
    return p.kernel == QG_TEND_KERNEL_DIRECT ? launch_tend_direct_cert(a, p, s) : launch_tend_ring_cert(a, p, s);
}

// the one-point tendency of rows [j0, j1) for nmembers members (one rank, F64; see the kernels);
// rec: a device table of nmembers records with the members' own parameters, or nullptr
static int launch_members(const TendArgsT<double> &a, int nmembers, int64_t member_stride, const TendMember *rec,
                          hipStream_t s) {
    if (nmembers < 1) return QG_ERR_INVALID_ARG;
    qg_tend_plan p;
    QG_CHECK(plan_launch(shape_of(a, false, nmembers, 0), p));
    return launch_tend_direct_members(a, p, member_stride, rec, s);
}

int launch_tendency_members(const TendArgsT<double> &a, int nmembers, int64_t member_stride, hipStream_t s) {
    return launch_members(a, nmembers, member_stride, nullptr, s);
}

int launch_tendency_sweep(const TendArgsT<double> &a, int nmembers, int64_t member_stride, const TendMember *rec,
                          hipStream_t s) {
    if (!rec) return QG_ERR_INVALID_ARG;
    return launch_members(a, nmembers, member_stride, rec, s);
}

}  // namespace qg

// the plan alone, for a caller-supplied resident-workgroup count (qg_mi355.h)
extern "C" int qg_tendency_plan(int64_t M, const int rows[4], int esize, int cert, int nmembers, int resident,
                                int64_t cap, qg_tend_plan *out) {
    using namespace qg;
    if (!rows || !out || resident < 1) return QG_ERR_INVALID_ARG;
    const TendShape sh = tend_shape(M, rows[0], rows[1], rows[2], rows[3], esize, cert != 0, nmembers,
                                    form(QG_FORM_TENDENCY), form(QG_FORM_TENDENCY_TILE), cap);
    QG_CHECK(tend_choose(sh, *out));
    return tend_grid(sh, resident, *out);
}
