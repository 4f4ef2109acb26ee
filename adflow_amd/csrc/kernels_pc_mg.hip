// The streaming kernels of the multigrid preconditioner (adflow_gpu_pc_set_mg, api.hip): the aggregation hierarchy of amg.F90 on the
// 7-point preconditioner matrix restricted to the columns inside each structured block, smoothed by the block ILU of kernels_pc.hip /
// kernels_pc_fill.hip on every level.
//
// Reference semantics (amg.F90): coarse sizes n -> n/2, (n+1)/2 if odd (:140-155); the fine cell (i, j, k), 0-based, belongs to the
// coarse cell (i/2, j/2, k/2) of the same block (:222-226); A_{l+1} = P^T A_l P with P the piecewise-constant prolongation, which is
// the sum MatSetValuesBlocked(..., ADD_VALUES) on the coarse indices produces (adjointUtils.F90:683-710); the cycle (:712-759) visits
// the coarse level first and smooths afterwards:  rhs' = P^T r;  sol' = smoother or cycle;  y = P sol';  res = r - A y;  y += S(res).
//
// Storage: every level owns its matrix in the box layout JmBlk describes -- component planes jac[c + ((s nState + l) nState + ll)
// nbox], c = (i+2) + (j+2) ldi + (k+2) ldk, two halo layers that nothing reads -- with the stencil entries s in the order of the
// assembly, so pc_build factors a level from its block list like the assembled matrix.  ldi and ldk are EVEN on every level the
// hierarchy owns and the planes start at even offsets from a 256-byte aligned base: the two fine cells (2I, 2I+1) of a coarse cell sit
// in one aligned 16-byte pair.  An entry whose column lies outside the block is ZERO on every level (the fine copy writes the zero,
// a sum over no terms keeps it), so no kernel below needs to know why an entry is absent.
// Vectors are in the PETSc layout (block, k, j, i, variable fastest) the sweeps of the factor take.
//
// One lane per cell with the lanes of a wave along i (JM_BX x JM_BY as the product kernels): every component plane is read coalesced.
#include "internal.h"

#define MG_BX 64
#define MG_BY 4

typedef double MgPair __attribute__((vector_size(16)));     // two consecutive doubles, one 16-byte load

struct MgCell {
    JmBlk b;
    int i, j, k;          // 0-based owned cell
    bool in;
};

// block, cell and bounds of a lane of the level-batched grid (x: i, y: j, z: block slot x k plane)
__device__ __forceinline__ MgCell mg_cell(const JmBlk* __restrict__ tab, int nzb)
{
    MgCell c;
    c.b = tab[blockIdx.z / nzb];
    c.i = blockIdx.x * MG_BX + threadIdx.x;
    c.j = blockIdx.y * MG_BY + threadIdx.y;
    c.k = (int)(blockIdx.z % nzb);
    c.in = c.i < c.b.nx && c.j < c.b.ny && c.k < c.b.nz;
    return c;
}

__device__ __forceinline__ unsigned mg_box(const JmBlk& b, int i, int j, int k) { return (unsigned)((i + 2) + (j + 2) * b.ldi + (k + 2) * b.ldk); }

// is the column of off-diagonal slot q (0..2: c - e_i, c - e_j, c - e_k; 3..5: c + e_i, c + e_j, c + e_k) inside the block
__device__ __forceinline__ bool mg_inside(const JmBlk& b, int i, int j, int k, int q)
{
    switch (q) {
    case 0: return i > 0;
    case 1: return j > 0;
    case 2: return k > 0;
    case 3: return i < b.nx - 1;
    case 4: return j < b.ny - 1;
    default: return k < b.nz - 1;
    }
}

// ---- 1. the fine copy: the seven blocks of every owned cell of the assembly (src) into the level-1 matrix of the hierarchy (dst),
// zero where the column lies outside the block; tsm != NULL: the pseudo-time term of ANK on the diagonal block, formed and added with
// the arithmetic of k_pc_factor (kernels_pc.hip), so a factor of the copy equals the shifted factor of the assembly bit for bit
template <int NS>
__global__ __launch_bounds__(MG_BX* MG_BY) void k_mg_fine_copy(const JmBlk* __restrict__ src, const JmBlk* __restrict__ dst, int nzb, PcMgSten S,
                                                               const double* __restrict__ tsm, double turbDiag, long N)
{
    const MgCell c = mg_cell(dst, nzb);
    if (!c.in) return;
    const JmBlk a = src[blockIdx.z / nzb];
    const unsigned cs8 = mg_box(a, c.i, c.j, c.k) * 8u, cd8 = mg_box(c.b, c.i, c.j, c.k) * 8u;
    const unsigned ns8 = (unsigned)a.nbox * 8u, nd8 = (unsigned)c.b.nbox * 8u;
    for (int q = 0; q < 6; ++q) {
        const bool in = mg_inside(c.b, c.i, c.j, c.k, q);
        GPTR(const double) A = (GPTR(const double))(a.jac + (long)S.s[q] * (NS * NS) * a.nbox);
        GPTR(double) B = (GPTR(double))(c.b.jac + (long)S.s[q] * (NS * NS) * c.b.nbox);
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) stg(B, cd8 + e * nd8, in ? ldg(A, cs8 + e * ns8) : 0.0);
    }
    double D[NS * NS];
    {
        GPTR(const double) A = (GPTR(const double))(a.jac + (long)S.s[6] * (NS * NS) * a.nbox);
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) D[e] = ldg(A, cs8 + e * ns8);
    }
    if (tsm) {
        const long m = c.b.vecOff + ((long)c.k * c.b.ny + c.j) * c.b.nx + c.i;
        if constexpr (NS >= 5) {
            const double dtInv = tsm[m], rho = tsm[N + m];
            D[0] += dtInv;
            D[4 * NS + 4] += dtInv;
#pragma unroll
            for (int l = 1; l < 4; ++l) {
                D[l] += dtInv * tsm[(l + 1) * N + m];          // (row l, column 0)
                D[l * NS + l] += dtInv * rho;
            }
            if (NS > 5) D[(NS - 1) * NS + NS - 1] += dtInv * turbDiag;
        } else {
            D[0] += tsm[m] * turbDiag;
        }
    }
    GPTR(double) B = (GPTR(double))(c.b.jac + (long)S.s[6] * (NS * NS) * c.b.nbox);
#pragma unroll
    for (int e = 0; e < NS * NS; ++e) stg(B, cd8 + e * nd8, D[e]);
}

// ---- 2. coarsening A_l (fine) -> A_{l+1} (coarse) in gather form: one lane per coarse cell (I, J, K) and component e of the blocks
// (blockIdx.y carries e above the j tiles) forms the seven entries of that component.  The children (2I + di, 2J + dj, 2K + dk) that
// exist are visited in ascending (dk, dj, di); of each child first the diagonal entry, then the slots q = 0 .. 5 (-i, -j, -k, +i, +j,
// +k).  Entry q of a child is added to the coarse DIAGONAL when its column is another child of the aggregate, else to the coarse entry
// q (it crosses that face of the aggregate, or lies outside the block and is zero).  One fixed order, no atomics: the result does not
// depend on the execution order.  The pair (2I, 2I+1) of a row is one 16-byte load; the second half is a halo cell when 2I+1 = nx and
// is then not used.
template <int NS>
__global__ __launch_bounds__(MG_BX* MG_BY) void k_mg_coarsen(const JmBlk* __restrict__ fine, const JmBlk* __restrict__ coarse, int nzb, int nyb,
                                                             PcMgSten S)
{
    const JmBlk cb = coarse[blockIdx.z / nzb];
    const int I = blockIdx.x * MG_BX + threadIdx.x;
    const int J = (int)(blockIdx.y % nyb) * MG_BY + threadIdx.y;
    const int e = (int)(blockIdx.y / nyb);
    const int K = (int)(blockIdx.z % nzb);
    if (I >= cb.nx || J >= cb.ny || K >= cb.nz) return;
    const JmBlk fb = fine[blockIdx.z / nzb];
    const bool has1 = 2 * I + 1 < fb.nx;
    double acc[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) acc[q] = 0.0;
    for (int dk = 0; dk < 2; ++dk) {
        const int k = 2 * K + dk;
        if (k >= fb.nz) break;
        for (int dj = 0; dj < 2; ++dj) {
            const int j = 2 * J + dj;
            if (j >= fb.ny) break;
            const unsigned c8 = mg_box(fb, 2 * I, j, k) * 8u;
            double v0[7], v1[7];
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                GPTR(const char) P = (GPTR(const char))(fb.jac + ((long)S.s[q] * (NS * NS) + e) * fb.nbox);
                const MgPair p = *(GPTR(const MgPair))(P + c8);
                v0[q] = p[0];
                v1[q] = p[1];
            }
            // a sibling exists along j / k towards -: dj == 1 / dk == 1; towards +: the other child of the pair exists
            const bool upJ = dj == 0 && j + 1 < fb.ny, upK = dk == 0 && k + 1 < fb.nz;
            // child di = 0
            acc[6] += v0[6];
            acc[0] += v0[0];
            if (dj) acc[6] += v0[1]; else acc[1] += v0[1];
            if (dk) acc[6] += v0[2]; else acc[2] += v0[2];
            if (has1) acc[6] += v0[3]; else acc[3] += v0[3];
            if (upJ) acc[6] += v0[4]; else acc[4] += v0[4];
            if (upK) acc[6] += v0[5]; else acc[5] += v0[5];
            if (has1) {   // child di = 1
                acc[6] += v1[6];
                acc[6] += v1[0];
                if (dj) acc[6] += v1[1]; else acc[1] += v1[1];
                if (dk) acc[6] += v1[2]; else acc[2] += v1[2];
                acc[3] += v1[3];
                if (upJ) acc[6] += v1[4]; else acc[4] += v1[4];
                if (upK) acc[6] += v1[5]; else acc[5] += v1[5];
            }
        }
    }
    const unsigned cc8 = mg_box(cb, I, J, K) * 8u;
#pragma unroll
    for (int q = 0; q < 7; ++q) stg((GPTR(double))(cb.jac + ((long)S.s[q] * (NS * NS) + e) * cb.nbox), cc8, acc[q]);
}

// ---- 3. restriction rhs(C) = sum of r over the children of C that exist, in ascending (dk, dj, di)
template <int NS>
__global__ __launch_bounds__(MG_BX* MG_BY) void k_mg_restrict(const JmBlk* __restrict__ fine, const JmBlk* __restrict__ coarse, int nzb,
                                                              const double* __restrict__ r, double* __restrict__ rhs)
{
    const MgCell c = mg_cell(coarse, nzb);
    if (!c.in) return;
    const JmBlk fb = fine[blockIdx.z / nzb];
    double acc[NS];
#pragma unroll
    for (int l = 0; l < NS; ++l) acc[l] = 0.0;
    for (int dk = 0; dk < 2; ++dk) {
        const int k = 2 * c.k + dk;
        if (k >= fb.nz) break;
        for (int dj = 0; dj < 2; ++dj) {
            const int j = 2 * c.j + dj;
            if (j >= fb.ny) break;
            for (int di = 0; di < 2; ++di) {
                const int i = 2 * c.i + di;
                if (i >= fb.nx) break;
                const long m = (fb.vecOff + ((long)k * fb.ny + j) * fb.nx + i) * NS;
#pragma unroll
                for (int l = 0; l < NS; ++l) acc[l] += r[m + l];
            }
        }
    }
    const long mc = (c.b.vecOff + ((long)c.k * c.b.ny + c.j) * c.b.nx + c.i) * NS;
#pragma unroll
    for (int l = 0; l < NS; ++l) rhs[mc + l] = acc[l];
}

// ---- 4. and 5. the residual of a level, one streaming pass over its matrix:  res(c) = r(c) - sum_q A_q x(column of q)  over the columns
// inside the block, q = 0 .. 5 then the diagonal.
//   PRO = 0: x is a vector of this level (the Richardson iterations beyond the first).
//   PRO = 1: x = P sol, never formed for the product: the value of a column is sol at its PARENT (i/2, j/2, k/2) of the coarse level,
//            and y(c) = sol(parent(c)) is stored on the way (steps 3 and 4 of the cycle in one pass).
//   TR = 0: A_q = block q of row c.   TR = 1 (the cycle on A^T): A_q = the transposed block of row c + d_q that points back at c, which
//           is its slot of the opposite direction.
template <int NS, int TR, int PRO>
__global__ __launch_bounds__(MG_BX* MG_BY) void k_mg_residual(const JmBlk* __restrict__ tab, const JmBlk* __restrict__ coarse, int nzb, PcMgSten S,
                                                              const double* __restrict__ r, const double* __restrict__ x,
                                                              double* __restrict__ y, double* __restrict__ res)
{
    const MgCell c = mg_cell(tab, nzb);
    if (!c.in) return;
    const JmBlk& b = c.b;
    int cnx = 0, cny = 0;
    long coff = 0;
    if (PRO) {
        const JmBlk cb = coarse[blockIdx.z / nzb];
        cnx = cb.nx; cny = cb.ny; coff = cb.vecOff;
    }
    // first entry of the value of the column (i, j, k) in x
    auto at = [&](int i, int j, int k) -> long {
        return PRO ? (coff + ((long)(k >> 1) * cny + (j >> 1)) * cnx + (i >> 1)) * NS : (b.vecOff + ((long)k * b.ny + j) * b.nx + i) * NS;
    };
    const long m = (b.vecOff + ((long)c.k * b.ny + c.j) * b.nx + c.i) * NS;
    const unsigned c8 = mg_box(b, c.i, c.j, c.k) * 8u, nb8 = (unsigned)b.nbox * 8u;
    double acc[NS];
#pragma unroll
    for (int l = 0; l < NS; ++l) acc[l] = r[m + l];
    for (int q = 0; q < 7; ++q) {
        int di = 0, dj = 0, dk = 0;
        if (q < 6) {
            if (!mg_inside(b, c.i, c.j, c.k, q)) continue;
            const int sg = q < 3 ? -1 : 1;
            di = (q % 3 == 0) ? sg : 0;
            dj = (q % 3 == 1) ? sg : 0;
            dk = (q % 3 == 2) ? sg : 0;
        }
        const long mx = at(c.i + di, c.j + dj, c.k + dk);
        // TR: row c + d_q, its slot towards c
        const int slot = S.s[(TR && q < 6) ? (q + 3) % 6 : q];
        const unsigned a8 = TR ? (unsigned)((int)c8 + (di + dj * b.ldi + dk * b.ldk) * 8) : c8;
        GPTR(const double) B = (GPTR(const double))(b.jac + (long)slot * (NS * NS) * b.nbox);
        double xv[NS], bv[NS * NS];
#pragma unroll
        for (int l = 0; l < NS; ++l) xv[l] = x[mx + l];
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) bv[e] = ldg(B, a8 + e * nb8);
        if (TR) {
#pragma unroll
            for (int l = 0; l < NS; ++l)
#pragma unroll
                for (int mm = 0; mm < NS; ++mm) acc[l] -= bv[l * NS + mm] * xv[mm];
        } else {
#pragma unroll
            for (int l = 0; l < NS; ++l)
#pragma unroll
                for (int ll = 0; ll < NS; ++ll) acc[ll] -= bv[l * NS + ll] * xv[l];
        }
        if (PRO && q == 6) {
#pragma unroll
            for (int l = 0; l < NS; ++l) y[m + l] = xv[l];
        }
    }
#pragma unroll
    for (int l = 0; l < NS; ++l) res[m + l] = acc[l];
}

// ---- launchers: the blocks of a level in one launch (block slot x k plane in gridDim.z, split when that exceeds the limit)
static dim3 mg_grid(int nslots, int nx, int ny, int nz, int ncomp = 1)
{
    return dim3((nx + MG_BX - 1) / MG_BX, ((ny + MG_BY - 1) / MG_BY) * ncomp, nz * nslots);
}

#define MG_DISPATCH(nState, ...)                                                       \
    switch (nState) {                                                                  \
    case 1: { constexpr int NS_ = 1; __VA_ARGS__; } break;                             \
    case 5: { constexpr int NS_ = 5; __VA_ARGS__; } break;                             \
    case 6: { constexpr int NS_ = 6; __VA_ARGS__; } break;                             \
    default: (void)adf_fail("pc_mg: no kernel for this nState"); break;                \
    }

void launch_mg_fine_copy(const JmBlk* src, const JmBlk* dst, int nslots, int maxnx, int maxny, int maxnz, int nState, const PcMgSten& S,
                         const double* tsm, double turbDiag, long N, hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz, launch_mg_fine_copy(src + s0_, dst + s0_, n_, maxnx, maxny, maxnz, nState, S, tsm, turbDiag, N, s));
    if (nslots <= 0) return;
    MG_DISPATCH(nState, hipLaunchKernelGGL((k_mg_fine_copy<NS_>), mg_grid(nslots, maxnx, maxny, maxnz), dim3(MG_BX, MG_BY, 1), 0, s, src, dst,
                                           maxnz, S, tsm, turbDiag, N))
}

// maxn*: the largest extents of the COARSE level
void launch_mg_coarsen(const JmBlk* fine, const JmBlk* coarse, int nslots, int maxnx, int maxny, int maxnz, int nState, const PcMgSten& S,
                       hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz, launch_mg_coarsen(fine + s0_, coarse + s0_, n_, maxnx, maxny, maxnz, nState, S, s));
    if (nslots <= 0) return;
    const int nyb = (maxny + MG_BY - 1) / MG_BY;
    MG_DISPATCH(nState, hipLaunchKernelGGL((k_mg_coarsen<NS_>), mg_grid(nslots, maxnx, maxny, maxnz, NS_ * NS_), dim3(MG_BX, MG_BY, 1), 0, s,
                                           fine, coarse, maxnz, nyb, S))
}

void launch_mg_restrict(const JmBlk* fine, const JmBlk* coarse, int nslots, int maxnx, int maxny, int maxnz, int nState, const double* r,
                        double* rhs, hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz, launch_mg_restrict(fine + s0_, coarse + s0_, n_, maxnx, maxny, maxnz, nState, r, rhs, s));
    if (nslots <= 0) return;
    MG_DISPATCH(nState, hipLaunchKernelGGL((k_mg_restrict<NS_>), mg_grid(nslots, maxnx, maxny, maxnz), dim3(MG_BX, MG_BY, 1), 0, s, fine,
                                           coarse, maxnz, r, rhs))
}

// coarse != NULL: x is the solution of the coarse level, prolonged on the fly, and y receives the prolonged vector
void launch_mg_residual(const JmBlk* tab, const JmBlk* coarse, int nslots, int maxnx, int maxny, int maxnz, int nState, int transpose,
                        const PcMgSten& S, const double* r, const double* x, double* y, double* res, hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz,
                launch_mg_residual(tab + s0_, coarse ? coarse + s0_ : coarse, n_, maxnx, maxny, maxnz, nState, transpose, S, r, x, y, res, s));
    if (nslots <= 0) return;
    const dim3 g = mg_grid(nslots, maxnx, maxny, maxnz), t(MG_BX, MG_BY, 1);
#define MG_RES(TR, PRO) \
    MG_DISPATCH(nState, hipLaunchKernelGGL((k_mg_residual<NS_, TR, PRO>), g, t, 0, s, tab, coarse, maxnz, S, r, x, y, res))
    if (coarse) {
        if (transpose) { MG_RES(1, 1) } else { MG_RES(0, 1) }
    } else {
        if (transpose) { MG_RES(1, 0) } else { MG_RES(0, 0) }
    }
#undef MG_RES
}
