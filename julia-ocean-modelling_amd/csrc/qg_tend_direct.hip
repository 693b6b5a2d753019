// The cache-resident one-point form of the tendency (small grids, ensembles): one context,
// ensemble members, perturbed-parameter members and the certifying form.  Compiled with
// -ffp-contract=off; the same expressions in the same order as qg_tend_ring.hip.
#include "qg_tend_dev.hpp"
#include "qg_tend_forms.hpp"

namespace qg {

// ------------------------------------------------------------------------------------
// Cache-resident tendency (small grids).  When every field of the step fits in the 256 MB
// MALL, the LDS-ring kernel spends most of its time in the ring prologue and the
// per-row barriers of short strips.  Here each thread computes one output point straight
// from global memory: the 13-point psi diamond, the 3x3 zeta block and F(t-1), F(t-2), the
// neighbours' re-reads served by L1/L2/MALL; no LDS, no barriers.  Same expressions in the
// same order as tendency_kernel (lap at the five points, then the biharmonic), so the two
// kernels are bit-identical.  Block: 64 x-points (one wave) x 4 rows.
// ------------------------------------------------------------------------------------
// one point (i, j) of one layer: loads, tendency, AB3 update, stores; returns the centre
// values the certification uses (zeta, lap(psi), psi).  off: elements added to every field
// pointer of `a` (an ensemble member's block; 0 for a single context).  MEMBER: the record *mr's
// (visc, U, r, beta, wind) stand in for a's (a perturbed-parameter ensemble's member); a
// compile-time switch, so the other instantiations are the code they were
template <class T, bool MEMBER = false>
__device__ __forceinline__ void direct_point(const TendArgsT<T> &a, int layer, int i, int j, T &zc_out, T &L0_out,
                                             T &P0_out, const size_t off = 0, const TendMember *mr = nullptr) {
    const int M = (int)a.M, P = (int)a.P;
    const int64_t ld = a.ld;
    const T *psi = a.psi[layer] + off, *zeta = a.zeta[layer] + off;
    const RowSrcT<T> &prs = a.psi_rows[layer];
    const RowSrcT<T> &zrs = a.zeta_rows[layer];
    const T dx = (T)a.dx, idx = T(1) / dx, idx2 = idx * idx;
    const T cdc = T(0.5) * idx;
    const T den = T(12) * (dx * dx);
    const T visc = (T)(MEMBER ? mr->visc : a.visc), dtT = (T)a.dt, Ut = (T)(MEMBER ? mr->U : a.U),
            rt = (T)(MEMBER ? mr->r : a.r);
    const bool small = M < 8;
    auto wx = [&](int x) -> int {
        if (small) return ((x % M) + M) % M;
        return x < 0 ? x + M : (x >= M ? x - M : x);
    };
    auto rowp = [&](const T *base, const RowSrcT<T> &rs, int jj) -> const T * {
        if (jj >= 0 && jj < P) return base + fidx(1, jj + 1, ld);
        return rs.halo[jj < 0 ? jj + 2 : (jj - P) + 2] + off;
    };
    const T *pr[5], *zr[3];
#pragma unroll
    for (int d = 0; d < 5; ++d) pr[d] = rowp(psi, prs, j - 2 + d);
#pragma unroll
    for (int d = 0; d < 3; ++d) zr[d] = rowp(zeta, zrs, j - 1 + d);
    const int xm2 = wx(i - 2), xm1 = wx(i - 1), xp1 = wx(i + 1), xp2 = wx(i + 2);
    auto X = [&](int da) { return da == -2 ? xm2 : da == -1 ? xm1 : da == 0 ? i : da == 1 ? xp1 : xp2; };
    auto S = [&](int da, int db) { return pr[db + 2][X(da)]; };
    auto Z = [&](int da, int db) { return zr[db + 1][X(da)]; };
    auto lap = [&](int da, int db) {  // lap_row's expression at (i + da, j + db)
        return ((((S(da - 1, db) + S(da + 1, db)) - T(4) * S(da, db)) + S(da, db - 1)) + S(da, db + 1)) * idx2;
    };
    const T L0 = lap(0, 0);
    const T biharm = ((((lap(-1, 0) + lap(1, 0)) - T(4) * L0) + lap(0, -1)) + lap(0, 1)) * idx2;
    const T v_term = visc * biharm;
    const T J_term = arakawa_point<T>(Z, S, den);
    const T bl = (T)(MEMBER ? mr->beta[layer] : a.beta[layer]);
    const T beta_term = bl * (cdc * (S(1, 0) - S(-1, 0)));
    T last;
    if (layer == 0) last = Ut * (cdc * (Z(1, 0) - Z(-1, 0)));
    else last = rt * L0;
    T F = ((v_term - J_term) - beta_term) - last;
    if constexpr (MEMBER) {
        if (layer == 0 && mr->wind) F = F + (T)mr->wind[j];
    } else {
        if (layer == 0 && a.wind) F = F + (T)a.wind[j];
    }
    const T zcen = Z(0, 0);
    T zn, f1c = 0, f2c = 0;
    if (a.ab3) {
        const size_t o = (size_t)(j + 1) * ld + i + 1;
        f1c = ld_stream(a.fprev1[layer] + off + o);
        f2c = ld_stream(a.fprev2[layer] + off + o);
        zn = zcen + dtT * ((((T)(23.0 / 12.0) * F) - ((T)(16.0 / 12.0) * f1c)) + ((T)(5.0 / 12.0) * f2c));
    } else {
        zn = zcen + (dtT * F);
    }
    T *zo = a.zeta_out[layer] + off, *fo = a.f_out[layer] + off;
    const bool gr = a.write_ghost_rows;
    store_row_with_ghosts(zo + (size_t)(j + 1) * ld, ghost_row_target(zo, ld, P, j, gr), M, i, zn);
    store_row_with_ghosts(fo + (size_t)(j + 1) * ld, ghost_row_target(fo, ld, P, j, gr), M, i, F);
    if (a.ab3 && a.fshift1[layer]) {  // (see TendArgsT::fshift1)
        T *s1 = a.fshift1[layer] + off, *s2 = a.fshift2[layer] + off;
        store_row_with_ghosts(s1 + (size_t)(j + 1) * ld, ghost_row_target(s1, ld, P, j, gr), M, i, f1c);
        store_row_with_ghosts(s2 + (size_t)(j + 1) * ld, ghost_row_target(s2, ld, P, j, gr), M, i, f2c);
    }
    zc_out = zcen;
    L0_out = L0;
    P0_out = S(0, 0);
}

template <class T>
__global__ __launch_bounds__(256) void tendency_direct_kernel(TendArgsT<T> a, int nyA, int nyB) {
    const TendBlock tb = tend_block();
    const int layer = tb.z;
    const int M = (int)a.M;
    const int i = tb.x * 64 + (int)(threadIdx.x & 63);
    const int w = (int)(threadIdx.x >> 6);
    const int y = tb.y;
    const bool second = y >= nyA;
    const int r0 = second ? a.j2 : a.j0, r1 = second ? a.j3 : a.j1;
    const int j = r0 + 4 * (second ? y - nyA : y) + w;
    if (i >= M || j >= r1) return;  // no barriers below
    T zc, L0, P0;
    direct_point(a, layer, i, j, zc, L0, P0);
}

// Ensembles (qg_mi355_ensemble.h): the same point for every member of a batch in one launch.
// The grid is linear -- (strips of 64) x (blocks of 4 rows) x layer x member workgroups, member
// slowest, decoded from the XCD-aware logical id as tend_block() does -- so no factor has to fit
// a grid's 65 535-wide y or z extent.  Member b's fields lie b * mstride elements behind member
// 0's (direct_point's off); everything else (parameters, wind table) is shared.
struct MemberBlock {
    int x, y, layer, m;  // strip of 64, block of 4 rows, layer, member (workgroup-uniform)
};
__device__ __forceinline__ MemberBlock member_block(int nx, int ny) {
    const int b = xcd_logical_id();
    const int x = b % nx;
    int r = b / nx;
    const int y = r % ny;
    r /= ny;
    return {x, y, r & 1, r >> 1};
}

__global__ __launch_bounds__(256) void tendency_direct_ens_kernel(TendArgsT<double> a, int nx, int ny, int64_t mstride) {
    const MemberBlock mb = member_block(nx, ny);
    const size_t off = (size_t)mb.m * (size_t)mstride;
    const int i = mb.x * 64 + (int)(threadIdx.x & 63);
    const int j = a.j0 + 4 * mb.y + (int)(threadIdx.x >> 6);
    if (i >= (int)a.M || j >= a.j1) return;  // no barriers below
    double zc, L0, P0;
    direct_point(a, mb.layer, i, j, zc, L0, P0, off);
}

// Perturbed-parameter ensembles (qg_mi355_sweep.h): tendency_direct_ens_kernel with the five
// model scalars and the wind table of the workgroup's member read from its 64-byte record
// (workgroup-uniform: scalar loads) in place of the arguments'.  direct_point takes the record
// beside the arguments: a patched copy of them would leave the kernel-argument segment for
// scratch (472 bytes per lane on the compiler's resource report).  The point itself is
// direct_point, so a member's arithmetic is a single context's with those parameters.
// rec[m].wind is null for a member without wind: its F never sees the "+ w_j" (which would turn
// a -0.0 into +0.0).
__global__ __launch_bounds__(256) void tendency_direct_sweep_kernel(TendArgsT<double> a, int nx, int ny, int64_t mstride,
                                                                    const TendMember *rec) {
    const MemberBlock mb = member_block(nx, ny);
    const size_t off = (size_t)mb.m * (size_t)mstride;
    const int i = mb.x * 64 + (int)(threadIdx.x & 63);
    const int j = a.j0 + 4 * mb.y + (int)(threadIdx.x >> 6);
    if (i >= (int)a.M || j >= a.j1) return;  // no barriers below
    double zc, L0, P0;
    direct_point<double, true>(a, mb.layer, i, j, zc, L0, P0, off, rec + mb.m);
}

// The certifying form of the cache-resident kernel (PCG, one rank, small grids): each thread
// steps both layers of its point and forms the previous solve's residual terms there
// (tendency_kernel<CERT>'s per-point parts, layer 0's first); (b,b), (r,r) per block.
__global__ __launch_bounds__(256) void tendency_direct_cert_kernel(TendArgsT<double> a, int nyA, int nyB) {
    const TendBlock tb = tend_block();
    const int M = (int)a.M;
    const int i = tb.x * 64 + (int)(threadIdx.x & 63);
    const int w = (int)(threadIdx.x >> 6);
    const int y = tb.y;
    const bool second = y >= nyA;
    const int r0 = second ? a.j2 : a.j0, r1 = second ? a.j3 : a.j1;
    const int j = r0 + 4 * (second ? y - nyA : y) + w;
    double cv[4] = {0, 0, 0, 0};
    if (i < M && j < r1) {
        double part[2][4];
#pragma unroll
        for (int layer = 0; layer < 2; ++layer) {
            double zc, L0, P0;
            direct_point(a, layer, i, j, zc, L0, P0);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const double b = -(a.cert_in[2 * s + layer] * zc);
                part[layer][2 * s] = b;
                part[layer][2 * s + 1] = b + a.cert_pinv[2 * s + layer] * (L0 + a.cert_alpha[s] * P0);
            }
        }
        double bs[2], rs[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bs[s] = part[0][2 * s] + part[1][2 * s];
            rs[s] = part[0][2 * s + 1] + part[1][2 * s + 1];
        }
        if (a.cert_pin && i == 0 && j == 0) bs[0] = rs[0] = 0.0;  // identity row: b = x = 0
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            cv[2 * s] = bs[s] * bs[s];
            cv[2 * s + 1] = rs[s] * rs[s];
        }
    }
    // block sums, fixed order (wave shuffles, then the four wave totals in order)
    __shared__ double sv[4][4];
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double v = cv[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) sv[k][w] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const double v = ((sv[threadIdx.x][0] + sv[threadIdx.x][1]) + sv[threadIdx.x][2]) + sv[threadIdx.x][3];
        a.cert[4 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x) + threadIdx.x] = v;
    }
}

// ------------------------------------------------------------------------------------
// host side: the plan's grid of 64 x 4 blocks (the kernels assume DIRECT_W and DIRECT_ROWS)
// ------------------------------------------------------------------------------------
template <class T>
int launch_tend_direct(const TendArgsT<T> &a, const qg_tend_plan &p, hipStream_t s) {
    tendency_direct_kernel<T><<<tend_grid_dim(p), p.threads, 0, s>>>(a, p.nyA, p.nyB);
    QG_LAUNCH_CHECK();
    return QG_OK;
}
template int launch_tend_direct(const TendArgsT<double> &, const qg_tend_plan &, hipStream_t);
template int launch_tend_direct(const TendArgsT<float> &, const qg_tend_plan &, hipStream_t);

int launch_tend_direct_cert(const TendArgsT<double> &a, const qg_tend_plan &p, hipStream_t s) {
    tendency_direct_cert_kernel<<<tend_grid_dim(p), p.threads, 0, s>>>(a, p.nyA, p.nyB);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

int launch_tend_direct_members(const TendArgsT<double> &a, const qg_tend_plan &p, int64_t member_stride,
                               const TendMember *rec, hipStream_t s) {
    if (rec) tendency_direct_sweep_kernel<<<(unsigned)p.blocks, p.threads, 0, s>>>(a, p.nx, p.nyA, member_stride, rec);
    else tendency_direct_ens_kernel<<<(unsigned)p.blocks, p.threads, 0, s>>>(a, p.nx, p.nyA, member_stride);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

}  // namespace qg
