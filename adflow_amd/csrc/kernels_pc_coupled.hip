// ILU(0) of the assembled 7-point preconditioner matrix over the WHOLE level: one subdomain per process, the couplings across block
// interfaces inside M (adflow_gpu_pc_set_coupled(1); api.hip builds the tables, pc_build).
//
// Reference semantics: the PCApply of setupStandardKSP (adjointUtils.F90:1374-1562) with one ASM subdomain per process and overlap
// 0: the ILU of a process spans every block it owns, natural ordering = block after block in ascending nn, then k, j, i.  A column on
// a first-layer face halo whose donor is an owned cell of this process is the column of that donor cell (the 2-layer pattern of the
// level, as adflow_gpu_jacobian_mult reads it); a halo without such a donor stays outside M.  Fill 0 only.
//
// Arithmetic: neighbour n(d) of cell c in direction d (0..2: -i, -j, -k; 3..5: +i, +j, +k) is absent, LOWER (its number in the PETSc
// layout is smaller than c's) or UPPER -- which, no longer follows from d: the wrap behind a + face of a periodic brick leads to a
// lower cell, and across a rotated interface the way back from n to c is not the opposite direction.  As long as no two neighbours
// of a cell are neighbours of each other (the host refuses the level otherwise) elimination creates no entry inside the pattern
// but on the diagonal:
//   L_{c,n} = A_{c,n} D_n^-1 (n lower),   U_{c,n} = A_{c,n} (n upper),   D_c = A_cc (+ T) - sum_{n lower} L_{c,n} U_{n,c}
// with the six terms taken in the order of d, so two setups agree bit for bit, and on one block without self-interfaces the factor
// is the one of k_pc_factor bit for bit (the same loops in the same order).
//
// Storage: that of kernels_pc.hip -- position q of the order (set, block, k, j, i) holds fac[q + ((s nState + l) nState + ll) N] --
// with slot d = 0..5 of a cell holding L if d is lower and U if it is upper, slot 6 holding D^-1.  cw[q], one word per cell:
//   bits 0..5     direction d is lower
//   bits 6+3d..   the slot (0..5) in which the neighbour in direction d keeps its entry back to this cell: U_{n,c} of the
//                 factorisation and the blocks the transposed sweeps read, so one factor serves M^-1 r and M^-T r
// nbr[d N + q]: position of the neighbour in direction d, in whichever block it lies, -1: none.  The sets are the longest dependency
// path over the lower neighbours of the whole level; a sweep walks the six directions and takes those whose mask bit matches its
// side.  Position, mask word and factor block are a dependent chain: the six positions and the word are loaded before the first
// block, one neighbour block is live at a time.
#include "internal.h"

#define PCC_T 64          // one wave per workgroup, as kernels_pc.hip

#include "pc_block.h"

// one level set of the factorisation: lanes q0 .. q0 + cnt - 1.  The rows of the lower neighbours are complete (earlier launches)
template <int NS>
__global__ __launch_bounds__(PCC_T) void k_pcc_factor(PcTab T, int q0, int cnt)
{
    const int t = blockIdx.x * PCC_T + threadIdx.x;
    if (t >= cnt) return;
    const unsigned q = (unsigned)(q0 + t), q8 = q * 8u;
    const long N = T.ncell;
    const unsigned w = T.cw[q];
    const JmBlk b = T.blk[T.cblk[q]];
    const unsigned c8 = (unsigned)T.cbox[q] * 8u, nb8 = (unsigned)b.nbox * 8u;
    GPTR(double) F = (GPTR(double))T.fac;
    double D[NS * NS];
    {
        GPTR(const double) A = (GPTR(const double))(b.jac + (long)T.sten[6] * (NS * NS) * b.nbox);
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) D[e] = ldg(A, c8 + e * nb8);
    }
    if constexpr (NS >= 5) {
        // adflow_gpu_ank_pc_setup: dRdwPre + timeStepMat, as k_pc_factor adds it
        if (T.tsm) {
            const long m = T.vec[q];
            const double dtInv = T.tsm[m], rho = T.tsm[N + m];
            PCE(D, 0, 0) += dtInv;
            PCE(D, 4, 4) += dtInv;
#pragma unroll
            for (int l = 1; l < 4; ++l) {
                PCE(D, l, 0) += dtInv * T.tsm[(l + 1) * N + m];
                PCE(D, l, l) += dtInv * rho;
            }
            if (NS > 5) PCE(D, NS - 1, NS - 1) += dtInv * T.turbDiag;
        }
    } else if constexpr (NS == 1) {
        if (T.tsm) D[0] += T.tsm[T.vec[q]] * T.turbDiag;
    }
    for (int d = 0; d < 6; ++d) {
        const int n = T.nbr[(long)d * N + q];
        GPTR(double) Fs = F + (long)d * (NS * NS) * N;
        if (n < 0) {
#pragma unroll
            for (int e = 0; e < NS * NS; ++e) stg(Fs + e * N, q8, 0.0);
            continue;
        }
        GPTR(const double) A = (GPTR(const double))(b.jac + (long)T.sten[d] * (NS * NS) * b.nbox);
        if (!((w >> d) & 1u)) {                   // upper: U_{c,n} = A_{c,n}
#pragma unroll
            for (int e = 0; e < NS * NS; ++e) stg(Fs + e * N, q8, ldg(A, c8 + e * nb8));
            continue;
        }
        double X[NS * NS], L[NS * NS];
        // L_{c,n} = A_{c,n} D_n^-1: the lower neighbour wrote it into this slot when it held D_n (below), by a solve, as k_pc_factor
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) L[e] = ldg((GPTR(const double))Fs + e * N, q8);
        {
            // U_{n,c}: the neighbour holds it in the slot of ITS direction towards c, which differs from lane to lane
            const long back = (w >> (6 + 3 * d)) & 7u;
            GPTR(const double) Fu = F + back * (NS * NS) * N + n;
#pragma unroll
            for (int e = 0; e < NS * NS; ++e) X[e] = Fu[(long)e * N];
        }
        pc_schur_sub<NS>(D, L, X);
    }
    // the L blocks of the upper neighbours towards this cell, L_{c,q} = A_{c,q} D_q^-1, by a solve with D_q while it is at hand
    // (pc_right_solve), written into the slot in which c keeps its entry back to this cell; c's row reads it in a later set
    for (int d = 0; d < 6; ++d) {
        const int c = T.nbr[(long)d * N + q];
        if (c < 0 || ((w >> d) & 1u)) continue;
        const long back = (w >> (6 + 3 * d)) & 7u;
        const JmBlk bc = T.blk[T.cblk[c]];
        GPTR(const double) A = (GPTR(const double))(bc.jac + (long)T.sten[back] * (NS * NS) * bc.nbox);
        const unsigned cc8 = (unsigned)T.cbox[c] * 8u, nbc8 = (unsigned)bc.nbox * 8u;
        double X[NS * NS];
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) X[e] = ldg(A, cc8 + e * nbc8);             // A_{c,q}
        pc_right_solve<NS>(D, X);
        GPTR(double) Fs = F + back * (NS * NS) * N;
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) stg(Fs + e * N, (unsigned)c * 8u, X[e]);
    }
    if (!pc_invert<NS>(D)) T.flag[0] = (int)q + 1;      // any of the failing cells: the host names one of them
    GPTR(double) Fd = F + (long)6 * (NS * NS) * N;
#pragma unroll
    for (int e = 0; e < NS * NS; ++e) stg(Fd + e * N, q8, D[e]);
}

// one level set of a triangular sweep, the four sweeps of k_pc_sweep.  BACK = 0: ascending sets, the lower neighbours, input r;
// BACK = 1: descending sets, the upper neighbours, input ws, output also to z.
//   TR = 0:  forward  y_c = r_c - sum L_{c,n} y_n            backward  z_c = D_c^-1 (y_c - sum U_{c,n} z_n)      (slot d of c)
//   TR = 1:  forward  y_c = D_c^-T (r_c - sum U_{n,c}^T y_n)  backward  z_c = y_c - sum L_{n,c}^T z_n             (back slot of n)
// NV vectors at once as k_pc_sweep takes them: positions, word and factor blocks once, values and accumulators per vector.
template <int NS, int TR, int BACK, int NV = 1>
__global__ __launch_bounds__(PCC_T) void k_pcc_sweep(PcTab T, int q0, int cnt, const double* __restrict__ r, double* __restrict__ z,
                                                     long ldr, long ldz)
{
    const int t = blockIdx.x * PCC_T + threadIdx.x;
    if (t >= cnt) return;
    const unsigned q = (unsigned)(q0 + t), q8 = q * 8u;
    const long N = T.ncell;
    const unsigned N8 = (unsigned)N * 8u;
    int nb[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) nb[d] = T.nbr[(long)d * N + q];
    const unsigned w = T.cw[q];
    GPTR(const double) F = (GPTR(const double))T.fac;
    GPTR(double) W[NV];          // vector 0 in the work space of the factor, the others in its extra part
#pragma unroll
    for (int v = 0; v < NV; ++v) W[v] = (GPTR(double))(v == 0 ? T.ws : T.wsx + (long)(v - 1) * NS * N);
    const long m = (long)T.vec[q] * NS;
    double acc[NV][NS];
    if (BACK) {
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int l = 0; l < NS; ++l) acc[v][l] = ldg(W[v], q8 + l * N8);
    } else {
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int l = 0; l < NS; ++l) acc[v][l] = r[v * ldr + m + l];
    }
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        const int n = nb[d];
        if (n < 0 || (int)((w >> d) & 1u) == BACK) continue;      // forward: the lower neighbours, backward: the upper ones
        const unsigned n8 = (unsigned)n * 8u;
        double xv[NV][NS], bv[NS * NS];
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int l = 0; l < NS; ++l) xv[v][l] = ldg(W[v], n8 + l * N8);
        if (TR) {
            const long back = (w >> (6 + 3 * d)) & 7u;
            GPTR(const double) Fb = F + back * (NS * NS) * N + n;
#pragma unroll
            for (int e = 0; e < NS * NS; ++e) bv[e] = Fb[(long)e * N];
        } else {
            GPTR(const double) Fs = F + (long)d * (NS * NS) * N;
#pragma unroll
            for (int e = 0; e < NS * NS; ++e) bv[e] = ldg(Fs + e * N, q8);
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            if (TR) {
#pragma unroll
                for (int l = 0; l < NS; ++l)
#pragma unroll
                    for (int ll = 0; ll < NS; ++ll) acc[v][l] -= PCE(bv, ll, l) * xv[v][ll];
            } else {
#pragma unroll
                for (int l = 0; l < NS; ++l)
#pragma unroll
                    for (int ll = 0; ll < NS; ++ll) acc[v][ll] -= PCE(bv, ll, l) * xv[v][l];
            }
        }
    }
    if (TR != BACK) {
        GPTR(const double) Fd = F + (long)6 * (NS * NS) * N;
        double bv[NS * NS];
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) bv[e] = ldg(Fd + e * N, q8);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            double o[NS];
#pragma unroll
            for (int l = 0; l < NS; ++l) o[l] = 0.0;
            if (TR) {
#pragma unroll
                for (int l = 0; l < NS; ++l)
#pragma unroll
                    for (int ll = 0; ll < NS; ++ll) o[l] += PCE(bv, ll, l) * acc[v][ll];
            } else {
#pragma unroll
                for (int l = 0; l < NS; ++l)
#pragma unroll
                    for (int ll = 0; ll < NS; ++ll) o[ll] += PCE(bv, ll, l) * acc[v][l];
            }
#pragma unroll
            for (int l = 0; l < NS; ++l) acc[v][l] = o[l];
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int l = 0; l < NS; ++l) stg(W[v], q8 + l * N8, acc[v][l]);
    if (BACK) {
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int l = 0; l < NS; ++l) z[v * ldz + m + l] = acc[v][l];
    }
}

#define PCC_DISPATCH(nState, ...)                                                      \
    switch (nState) {                                                                  \
    case 1: { constexpr int NS_ = 1; __VA_ARGS__; } break;                             \
    case 5: { constexpr int NS_ = 5; __VA_ARGS__; } break;                             \
    case 6: { constexpr int NS_ = 6; __VA_ARGS__; } break;                             \
    default: return adf_fail("pc: no kernel for this nState");                         \
    }

int launch_pcc_factor(const PcTab& T, int nState, const std::vector<int>& setStart, hipStream_t s)
{
    for (size_t p = 0; p + 1 < setStart.size(); ++p) {
        const int q0 = setStart[p], cnt = setStart[p + 1] - q0;
        if (cnt <= 0) continue;
        PCC_DISPATCH(nState, hipLaunchKernelGGL((k_pcc_factor<NS_>), dim3((cnt + PCC_T - 1) / PCC_T), dim3(PCC_T), 0, s, T, q0, cnt))
    }
    return 0;
}

template <int NS, int TR, int NV>
static void pcc_apply_sets(const PcTab& T, const std::vector<int>& setStart, const double* r, double* z, long ldr, long ldz, hipStream_t s)
{
    const int np = (int)setStart.size() - 1;
    for (int p = 0; p < np; ++p) {
        const int q0 = setStart[p], cnt = setStart[p + 1] - q0;
        if (cnt > 0)
            hipLaunchKernelGGL((k_pcc_sweep<NS, TR, 0, NV>), dim3((cnt + PCC_T - 1) / PCC_T), dim3(PCC_T), 0, s, T, q0, cnt, r, z, ldr, ldz);
    }
    for (int p = np - 1; p >= 0; --p) {
        const int q0 = setStart[p], cnt = setStart[p + 1] - q0;
        if (cnt > 0)
            hipLaunchKernelGGL((k_pcc_sweep<NS, TR, 1, NV>), dim3((cnt + PCC_T - 1) / PCC_T), dim3(PCC_T), 0, s, T, q0, cnt, r, z, ldr, ldz);
    }
}

#define PCC_DISPATCH_NV(nv, ...) ADF_DISPATCH_NV(nv, return adf_fail("pc: no kernel for this number of vectors"), __VA_ARGS__)

int launch_pcc_apply(const PcTab& T, int nState, int transpose, const std::vector<int>& setStart, const double* r, double* z,
                     hipStream_t s, int nv, long ldr, long ldz)
{
    if (transpose) { PCC_DISPATCH(nState, PCC_DISPATCH_NV(nv, pcc_apply_sets<NS_, 1, NV_>(T, setStart, r, z, ldr, ldz, s))) }
    else { PCC_DISPATCH(nState, PCC_DISPATCH_NV(nv, pcc_apply_sets<NS_, 0, NV_>(T, setStart, r, z, ldr, ldz, s))) }
    return 0;
}
