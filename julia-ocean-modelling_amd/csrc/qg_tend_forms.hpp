// Host side of the three tendency forms: per form, the resident-workgroup count of the kernel a
// plan names and the launch of that plan (each defined in the file that holds the form's kernels
// -- no kernel is visible outside its file).  qg_tend_launch.hip plans (qg_tend_plan.hpp) and
// calls only these.
#pragma once

#include "qg_common.hpp"
#include "qg_tend_plan.hpp"

namespace qg {

// LDS ring, one point per thread (qg_tend_ring.hip; T = double, float); cert = the certifying
// instantiation
int tend_ring_resident(const qg_tend_plan &p, int esize, bool cert, int &resident);
template <class T>
int launch_tend_ring(const TendArgsT<T> &a, const qg_tend_plan &p, hipStream_t s);
int launch_tend_ring_cert(const TendArgsT<double> &a, const qg_tend_plan &p, hipStream_t s);
// two points per thread (qg_tend_pair.hip)
int tend_pair_resident(const qg_tend_plan &p, int &resident);
int launch_tend_pair(const TendArgsT<float> &a, const qg_tend_plan &p, hipStream_t s);
// cache-resident one-point form (qg_tend_direct.hip; T = double, float); rec = nullptr: members
// share a's parameters
template <class T>
int launch_tend_direct(const TendArgsT<T> &a, const qg_tend_plan &p, hipStream_t s);
int launch_tend_direct_cert(const TendArgsT<double> &a, const qg_tend_plan &p, hipStream_t s);
int launch_tend_direct_members(const TendArgsT<double> &a, const qg_tend_plan &p, int64_t member_stride,
                               const TendMember *rec, hipStream_t s);

// Resident workgroups per chip (CUs x per-CU occupancy) of a tendency kernel, asked once per
// kernel: `sl` is the caller's process-wide cache for that instantiation
template <class K>
int tend_slots(K kernel, int threads, int &sl) {
    if (sl) return QG_OK;
    int dev = 0, cus = 0, per = 0;
    QG_HIP(hipGetDevice(&dev));
    QG_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    QG_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, threads, 0));
    sl = cus * (per > 0 ? per : 1);
    return QG_OK;
}

inline dim3 tend_grid_dim(const qg_tend_plan &p) { return dim3((unsigned)p.nx, (unsigned)(p.nyA + p.nyB), (unsigned)p.nz); }

}  // namespace qg
