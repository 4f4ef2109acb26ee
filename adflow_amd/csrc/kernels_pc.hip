// Block ILU(0) of the assembled 7-point preconditioner matrix, factored and applied on the device, and the vector kernels of the
// right-preconditioned GMRES that uses it (adflow_gpu_pc_setup / _pc_apply / _gmres_solve, api.hip).
//
// Reference semantics: the PCApply of setupStandardKSP (adjointUtils.F90:1374-1562) in the configuration PCBJACOBI (= PCASM with
// overlap 0), one subdomain per structured block, sub-preconditioner ILU with 0 levels in the natural ordering (k, j, i with i
// fastest) on BAIJ blocks of size nState.  A column on a halo cell, with or without a donor, is not part of a subdomain.
// (One subdomain for the level -- what the reference gives a process that owns several blocks, the couplings across its block
// interfaces inside M -- is adflow_gpu_pc_set_coupled(1): kernels_pc_coupled.hip, fill 0, the same storage.)
// Fill: natural ordering, fill <= 2.  This file is fill 0; ILU(1) and ILU(2) (adflow_gpu_pc_set_fill; the reference defaults to 2)
// are in kernels_pc_fill.hip and leave a factor that everything above the two launch_pc_* calls takes unchanged.
// Out of scope: fill > 2 and the RCM ordering (the reference's default ordering), ASM overlap between ranks, GMRES across ranks.
// (The pseudo-time diagonal term of ANK and the matrix-free operator: adflow_gpu_ank_pc_setup / _ank_solve, kernels_ank.hip.)
//
// Arithmetic: eliminating row c of a 7-point stencil in natural order with the rows c - e_i, c - e_j, c - e_k creates no entry
// inside the pattern but on the diagonal, so
//   D_c = A_cc - sum_lower A_{c,n} D_n^-1 A_{n,c},    L_{c,n} = A_{c,n} D_n^-1,    U_{c,n} = A_{c,n},    M = L (D + U)
// (L_{c,n} is formed by the thread of row n, by a solve with D_n before D_n is inverted -- pc_right_solve, pc_block.h -- and read by
// row c; only the sweeps multiply by the stored D^-1)
// and D_c needs the cells of the hyperplane i + j + k - 1 only: setup, forward and backward sweep run hyperplane by hyperplane,
// one plain launch per hyperplane that covers every block of the level, in stream order.  M^T = (D + U)^T L^T has the diagonal
// blocks D_c^T: the same factor serves M^-1 r and M^-T r.
//
// Storage (owned by the factor): the cells of the level sorted by (hyperplane, block, k, j, i); position q of that order holds
//   fac[q + ((s nState + l) nState + ll) N]   s = 0..2: L of the lower neighbour along i, j, k; 3..5: U of the upper neighbour;
//                                             6: D^-1;  (ll, l) = (row, column) of the block as in jac[]
// so the lanes of a wave stream every component plane coalesced (in the box layout the cells of a hyperplane are ldi - 1 apart).
// nbr[e N + q]: position of neighbour e (0..2 lower, 3..5 upper) or -1 outside the block; vec[q]: the cell's number in the PETSc
// layout.  Only the neighbour values of the vector are gathered (ws, hyperplane order, component-major); the transposed sweeps
// read the blocks at the neighbours' positions, which are monotone in q along a hyperplane.
//
// Several vectors at once (adflow_gpu_pc_apply_multi, adflow_gpu_gmres_solve_multi): k_pc_sweep takes a vector count NV = 1 .. 4 --
// the same launches per hyperplane, neighbour positions and factor blocks loaded once, neighbour values, accumulators and the D^-1
// product per vector (vector 0 in ws, the others in wsx, which the factor gets at its first multi-vector application).  The GMRES
// kernels have _multi twins with the column in blockIdx.y: every column keeps its own partial sums, added in the single solver's order.
#include "internal.h"

#define PC_T 64           // one wave per workgroup: a hyperplane of a few thousand cells still spreads over the CUs

#include "pc_block.h"

// one hyperplane of the factorisation: lanes q0 .. q0 + cnt - 1.  The rows of the lower neighbours are complete (earlier launches)
template <int NS>
__global__ __launch_bounds__(PC_T) void k_pc_factor(PcTab T, int q0, int cnt)
{
    const int t = blockIdx.x * PC_T + threadIdx.x;
    if (t >= cnt) return;
    const unsigned q = (unsigned)(q0 + t), q8 = q * 8u;
    const long N = T.ncell;
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
        // adflow_gpu_ank_pc_setup: dRdwPre + timeStepMat (FormJacobianANK, NKSolvers.F90:1996-1998), T = dtInv S formed from the
        // compact storage of kernels_ank.hip (PETSc cell order)
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
        // the turbulence KSP (FormJacobianANKTurb, NKSolvers.F90:2395-2406): dtInv turbResScale / turbCFLScale on the pivot; the
        // turbulence T stores dtInv only
        if (T.tsm) D[0] += T.tsm[T.vec[q]] * T.turbDiag;
    }
    for (int s = 0; s < 3; ++s) {
        const int n = T.nbr[(long)s * N + q];
        GPTR(double) Fs = F + (long)s * (NS * NS) * N;
        if (n < 0) {
#pragma unroll
            for (int e = 0; e < NS * NS; ++e) stg(Fs + e * N, q8, 0.0);
            continue;
        }
        const unsigned n8 = (unsigned)n * 8u;
        double X[NS * NS], L[NS * NS];
        // L_{c,n} = A_{c,n} D_n^-1: the lower neighbour wrote it into this slot when it held D_n (below), by a solve
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) L[e] = ldg((GPTR(const double))Fs + e * N, q8);
        {
            GPTR(const double) Fu = F + (long)(3 + s) * (NS * NS) * N;
#pragma unroll
            for (int e = 0; e < NS * NS; ++e) X[e] = ldg(Fu + e * N, n8);           // U_{n,c} = A_{n, n + e_s}
        }
        pc_schur_sub<NS>(D, L, X);
    }
    for (int s = 3; s < 6; ++s) {
        const bool in = T.nbr[(long)s * N + q] >= 0;
        GPTR(const double) A = (GPTR(const double))(b.jac + (long)T.sten[s] * (NS * NS) * b.nbox);
        GPTR(double) Fs = F + (long)s * (NS * NS) * N;
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) stg(Fs + e * N, q8, in ? ldg(A, c8 + e * nb8) : 0.0);
    }
    // the L blocks of the three upper neighbours c = q + e_s towards this cell, L_{c,q} = A_{c,q} D_q^-1, while D_q itself is at hand:
    // a solve with D_q (pc_right_solve), written into slot s of c, which c's row reads on a later hyperplane
    for (int s = 0; s < 3; ++s) {
        const int c = T.nbr[(long)(3 + s) * N + q];
        if (c < 0) continue;
        GPTR(const double) A = (GPTR(const double))(b.jac + (long)T.sten[s] * (NS * NS) * b.nbox);
        const unsigned cc8 = (unsigned)T.cbox[c] * 8u;
        double X[NS * NS];
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) X[e] = ldg(A, cc8 + e * nb8);              // A_{c,q}
        pc_right_solve<NS>(D, X);
        GPTR(double) Fs = F + (long)s * (NS * NS) * N;
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) stg(Fs + e * N, (unsigned)c * 8u, X[e]);
    }
    if (!pc_invert<NS>(D)) T.flag[0] = (int)q + 1;      // any of the failing cells: the host names one of them
    GPTR(double) Fd = F + (long)6 * (NS * NS) * N;
#pragma unroll
    for (int e = 0; e < NS * NS; ++e) stg(Fd + e * N, q8, D[e]);
}

// one hyperplane of a triangular sweep.  BACK = 0: ascending hyperplanes, lower neighbours, input r; BACK = 1: descending, upper
// neighbours, input ws, output also to z.
//   TR = 0:  forward  y_c = r_c - sum L_{c,n} y_n            backward  z_c = D_c^-1 (y_c - sum U_{c,n} z_n)      (blocks of c)
//   TR = 1:  forward  y_c = D_c^-T (r_c - sum U_{n,c}^T y_n)  backward  z_c = y_c - sum L_{n,c}^T z_n             (blocks of n)
// NV vectors at once (adflow_gpu_pc_apply_multi): neighbour position and factor block are loaded once, the neighbour values, the
// accumulators and the D^-1 product are per vector; column v of r and z starts v ldr / v ldz doubles behind column 0.  NV = 1 is the
// sweep of one vector as it always was.
template <int NS, int TR, int BACK, int NV = 1>
__global__ __launch_bounds__(PC_T) void k_pc_sweep(PcTab T, int q0, int cnt, const double* __restrict__ r, double* __restrict__ z, long ldr,
                                                   long ldz)
{
    const int t = blockIdx.x * PC_T + threadIdx.x;
    if (t >= cnt) return;
    const unsigned q = (unsigned)(q0 + t), q8 = q * 8u;
    const long N = T.ncell;
    const unsigned N8 = (unsigned)N * 8u;
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
    // the blocks of the sweep: TR = 0 the cell's own L (forward) / U (backward); TR = 1 the neighbour's U (forward) / L (backward)
    const int slot0 = (TR != BACK) ? 3 : 0;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int n = T.nbr[(long)((BACK ? 3 : 0) + s) * N + q];
        if (n < 0) continue;
        const unsigned n8 = (unsigned)n * 8u, at = TR ? n8 : q8;
        GPTR(const double) Fs = F + (long)(slot0 + s) * (NS * NS) * N;
        double xv[NV][NS], bv[NS * NS];
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int l = 0; l < NS; ++l) xv[v][l] = ldg(W[v], n8 + l * N8);
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) bv[e] = ldg(Fs + e * N, at);
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

#define PC_DISPATCH(nState, ...)                                                       \
    switch (nState) {                                                                  \
    case 1: { constexpr int NS_ = 1; __VA_ARGS__; } break;                             \
    case 5: { constexpr int NS_ = 5; __VA_ARGS__; } break;                             \
    case 6: { constexpr int NS_ = 6; __VA_ARGS__; } break;                             \
    default: return adf_fail("pc: no kernel for this nState");                         \
    }

int launch_pc_factor(const PcTab& T, int nState, const std::vector<int>& planeStart, hipStream_t s)
{
    for (size_t p = 0; p + 1 < planeStart.size(); ++p) {
        const int q0 = planeStart[p], cnt = planeStart[p + 1] - q0;
        if (cnt <= 0) continue;
        PC_DISPATCH(nState, hipLaunchKernelGGL((k_pc_factor<NS_>), dim3((cnt + PC_T - 1) / PC_T), dim3(PC_T), 0, s, T, q0, cnt))
    }
    return 0;
}

template <int NS, int TR, int NV>
static void pc_apply_planes(const PcTab& T, const std::vector<int>& planeStart, const double* r, double* z, long ldr, long ldz, hipStream_t s)
{
    const int np = (int)planeStart.size() - 1;
    for (int p = 0; p < np; ++p) {
        const int q0 = planeStart[p], cnt = planeStart[p + 1] - q0;
        if (cnt > 0)
            hipLaunchKernelGGL((k_pc_sweep<NS, TR, 0, NV>), dim3((cnt + PC_T - 1) / PC_T), dim3(PC_T), 0, s, T, q0, cnt, r, z, ldr, ldz);
    }
    for (int p = np - 1; p >= 0; --p) {
        const int q0 = planeStart[p], cnt = planeStart[p + 1] - q0;
        if (cnt > 0)
            hipLaunchKernelGGL((k_pc_sweep<NS, TR, 1, NV>), dim3((cnt + PC_T - 1) / PC_T), dim3(PC_T), 0, s, T, q0, cnt, r, z, ldr, ldz);
    }
}

#define PC_DISPATCH_NV(nv, ...) ADF_DISPATCH_NV(nv, return adf_fail("pc: no kernel for this number of vectors"), __VA_ARGS__)

int launch_pc_apply(const PcTab& T, int nState, int transpose, const std::vector<int>& planeStart, const double* r, double* z,
                    hipStream_t s, int nv, long ldr, long ldz)
{
    if (transpose) { PC_DISPATCH(nState, PC_DISPATCH_NV(nv, pc_apply_planes<NS_, 1, NV_>(T, planeStart, r, z, ldr, ldz, s))) }
    else { PC_DISPATCH(nState, PC_DISPATCH_NV(nv, pc_apply_planes<NS_, 0, NV_>(T, planeStart, r, z, ldr, ldz, s))) }
    return 0;
}

// ---- the vectors of GMRES: everything stays on the device, one download of a column of the Hessenberg matrix per step -----------
#define GM_T 256          // threads of a workgroup = the largest number of workgroups (partial sums) of a reduction
static_assert(GM_T == GM_PARTS, "gm_solve of api.hip sizes its buffers of partial sums for GM_T of them");

__device__ __forceinline__ double gm_block_sum(double v, double* red)
{
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = GM_T / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double out = red[0];
    __syncthreads();
    return out;
}

// One step of modified Gram-Schmidt per launch: h = sum of the partial sums hp[] the launch before left (every workgroup adds them
// in the same order; workgroup 0 stores h to *hOut), w -= h v, and the partial sums of <w, u> (u == NULL: <w, w>) go to out[].
// v == NULL: no update, only the dot product.  The dot with basis vector i + 1 needs the update with vector i: MGS allows no wider
// batch than this chain, which costs one launch per basis vector and no trip to the host.
__device__ __forceinline__ void gm_mgs_column(double* w, const double* v, const double* hp, const double* u, double* out, double* hOut,
                                              long n, double* red)
{
    const int tid = threadIdx.x;
    double h = 0.0;
    if (v) {
        h = gm_block_sum(tid < (int)gridDim.x ? hp[tid] : 0.0, red);
        if (blockIdx.x == 0 && tid == 0) *hOut = h;
    }
    double sum = 0.0;
    for (long i = (long)blockIdx.x * GM_T + tid; i < n; i += (long)gridDim.x * GM_T) {
        double wi = w[i];
        if (v) {
            wi -= h * v[i];
            w[i] = wi;
        }
        sum += wi * (u ? u[i] : wi);
    }
    sum = gm_block_sum(sum, red);
    if (tid == 0) out[blockIdx.x] = sum;
}

__global__ __launch_bounds__(GM_T) void k_gm_mgs(double* w, const double* v, const double* hp, const double* u, double* out,
                                                 double* hOut, long n)
{
    __shared__ double red[GM_T];
    gm_mgs_column(w, v, hp, u, out, hOut, n, red);
}

// The columns of adflow_gpu_gmres_solve_multi in lock-step: the same step for column blockIdx.y of w, v and u (ld doubles apart),
// with its own GM_PARTS partial sums in hp and out, added in the order of the single solver; its h goes to hOut[column]
__global__ __launch_bounds__(GM_T) void k_gm_mgs_multi(double* w, const double* v, const double* hp, const double* u, double* out,
                                                       double* hOut, long n, long ld)
{
    __shared__ double red[GM_T];
    const long c = blockIdx.y;
    gm_mgs_column(w + c * ld, v ? v + c * ld : nullptr, v ? hp + c * GM_PARTS : nullptr, u ? u + c * ld : nullptr, out + c * GM_PARTS,
                  v ? hOut + c : nullptr, n, red);
}

// the last partial sums of a chain
__global__ __launch_bounds__(GM_T) void k_gm_sum(const double* hp, int np, double* hOut)
{
    __shared__ double red[GM_T];
    const double h = gm_block_sum((int)threadIdx.x < np ? hp[threadIdx.x] : 0.0, red);
    if (threadIdx.x == 0) *hOut = h;
}

// y = a x + b y (b == 0: y is not read)
__global__ __launch_bounds__(GM_T) void k_gm_axpby(double* y, double a, const double* x, double b, long n)
{
    const long i = (long)blockIdx.x * GM_T + threadIdx.x;
    if (i >= n) return;
    y[i] = (b == 0.0) ? a * x[i] : a * x[i] + b * y[i];
}

// the same for the columns of a multi solve: partial sums of column c at hp + c GM_PARTS, its sum to hOut[c]
__global__ __launch_bounds__(GM_T) void k_gm_sum_multi(const double* hp, int np, double* hOut)
{
    __shared__ double red[GM_T];
    const double h = gm_block_sum((int)threadIdx.x < np ? hp[blockIdx.x * GM_PARTS + threadIdx.x] : 0.0, red);
    if (threadIdx.x == 0) hOut[blockIdx.x] = h;
}

// y_c = a_c x_c + b_c y_c for column c = blockIdx.y (b_c == 0: y_c is not read); a column with a_c = 0, b_c = 1 is not touched at all:
// that is how a column that has finished is left as it is
__global__ __launch_bounds__(GM_T) void k_gm_axpby_multi(double* y, long ldy, const double* x, long ldx, GmCoef k, long n)
{
    const long i = (long)blockIdx.x * GM_T + threadIdx.x;
    const int c = blockIdx.y;
    const double a = k.a[c], b = k.b[c];
    if (i >= n || (a == 0.0 && b == 1.0)) return;
    y[c * ldy + i] = (b == 0.0) ? a * x[c * ldx + i] : a * x[c * ldx + i] + b * y[c * ldy + i];
}

int gm_groups(long n)
{
    const long g = (n + 4L * GM_T - 1) / (4L * GM_T);
    return (int)(g < 1 ? 1 : g > GM_T ? GM_T : g);
}
void launch_gm_mgs(double* w, const double* v, const double* hp, const double* u, double* out, double* hOut, long n, hipStream_t s)
{
    hipLaunchKernelGGL(k_gm_mgs, dim3(gm_groups(n)), dim3(GM_T), 0, s, w, v, hp, u, out, hOut, n);
}
void launch_gm_sum(const double* hp, long n, double* hOut, hipStream_t s)
{
    hipLaunchKernelGGL(k_gm_sum, dim3(1), dim3(GM_T), 0, s, hp, gm_groups(n), hOut);
}
void launch_gm_axpby(double* y, double a, const double* x, double b, long n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_gm_axpby, dim3((unsigned)((n + GM_T - 1) / GM_T)), dim3(GM_T), 0, s, y, a, x, b, n);
}
void launch_gm_mgs_multi(double* w, const double* v, const double* hp, const double* u, double* out, double* hOut, long n, long ld,
                         int nvec, hipStream_t s)
{
    hipLaunchKernelGGL(k_gm_mgs_multi, dim3(gm_groups(n), nvec), dim3(GM_T), 0, s, w, v, hp, u, out, hOut, n, ld);
}
void launch_gm_sum_multi(const double* hp, long n, double* hOut, int nvec, hipStream_t s)
{
    hipLaunchKernelGGL(k_gm_sum_multi, dim3(nvec), dim3(GM_T), 0, s, hp, gm_groups(n), hOut);
}
void launch_gm_axpby_multi(double* y, long ldy, const double* x, long ldx, const GmCoef& k, long n, int nvec, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_gm_axpby_multi, dim3((unsigned)((n + GM_T - 1) / GM_T), nvec), dim3(GM_T), 0, s, y, ldy, x, ldx, k, n);
}
