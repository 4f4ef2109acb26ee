// The streaming kernels of the preconditioner Richardson iterations (adflow_gpu_pc_set_its, api.hip): the residual  t = b - A x  and
// t = b - A^T x  over the 7-point matrix of the WHOLE level on the copy the factor owns, and the kernel that takes that copy from the
// assembly.
//
// Reference semantics (setupStandardKSP, adjointUtils.F90:1374-1562): master_PC_KSP runs globalPreConIts Richardson iterations whose
// operator is the preconditioner matrix of the process, every subdomain a Richardson subksp of localPreConIts iterations on its own
// matrix around the ILU; the mg shell does the same (amg.F90:487-510, :534-615).  Richardson from a zero guess, scale 1, no norm: the
// recurrences are in api.hip (pc_apply_enqueue), this file is their product.
//
// Storage: cell-major component planes, mat[(q nState^2 + e) ncell + c], c = the natural number of the row (PETSc layout: block after
// block, then k, j, i), q = 0..5 the directions -i, -j, -k, +i, +j, +k and 6 the diagonal (T of ANK included), e = the component of
// the block as the assembly keeps it (e = l nState + ll: d row ll / d column l).  One lane per row with consecutive lanes on
// consecutive rows: every plane is read coalesced, 7 nState^2 x 8 B per cell and pass.  col[q ncell + c] = the natural number of the
// column of direction q, -1: none (the entry is stored as zero and never read).  cw[c]: bit q = the column of direction q lies behind
// a block face (masked for A_sub of a block-local factor); bits 6+3q..8+3q = the direction in which that column keeps its entry back
// to c, the mirror entry the transposed form reads.
//
// Both forms are gathers: row c of A^T x collects, from every neighbour n, the transposed block of row n that points at c.  No atomics,
// one fixed order (q = 0..5, then the diagonal): no result depends on the execution order.  Per lane nState accumulators per column
// and ONE block column (nState numbers) at a time; a block is read once for all columns of a group.
// Vectors are in the PETSc layout (cell, variable fastest); column v of b, x and t starts v ld doubles behind column 0.
#include "internal.h"

#define RICH_T 256

// ---- the copy: the seven blocks of every owned cell of the assembly into the planes above, zero where col names no column; tsm != NULL:
// the pseudo-time term of ANK on the diagonal block, formed and added with the arithmetic of k_pc_factor (kernels_pc.hip) and
// k_mg_fine_copy (kernels_pc_mg.hip).  Grid of the level-batched kernels: x along i, y along j, z = block slot x k plane.
template <int NS>
__global__ __launch_bounds__(64 * 4) void k_rich_copy(const JmBlk* __restrict__ src, int nzb, PcMgSten S, const double* __restrict__ tsm,
                                                      double turbDiag, long N, const int* __restrict__ col, double* __restrict__ mat)
{
    const JmBlk a = src[blockIdx.z / nzb];
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = (int)(blockIdx.z % nzb);
    if (i >= a.nx || j >= a.ny || k >= a.nz) return;
    const long m = a.vecOff + ((long)k * a.ny + j) * a.nx + i;
    const long cs = (i + 2) + (long)(j + 2) * a.ldi + (long)(k + 2) * a.ldk;
    for (int q = 0; q < 6; ++q) {
        const bool in = col[(long)q * N + m] >= 0;
        const double* A = a.jac + (long)S.s[q] * (NS * NS) * a.nbox + cs;
        double* B = mat + (long)q * (NS * NS) * N + m;
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) B[(long)e * N] = in ? A[(long)e * a.nbox] : 0.0;
    }
    double D[NS * NS];
    {
        const double* A = a.jac + (long)S.s[6] * (NS * NS) * a.nbox + cs;
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) D[e] = A[(long)e * a.nbox];
    }
    if (tsm) {
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
    double* B = mat + (long)6 * (NS * NS) * N + m;
#pragma unroll
    for (int e = 0; e < NS * NS; ++e) B[(long)e * N] = D[e];
}

// ---- the residual.  TR = 0: block q of row c.  TR = 1: the mirror entry of row n = col[q][c], transposed.  SUB: the columns behind
// block faces are left out (A_sub of a factor with one subdomain per block).
template <int NS, int TR, int NV>
__global__ __launch_bounds__(RICH_T) void k_rich_residual(PcRichTab T, int sub, const double* __restrict__ b, long ldb,
                                                          const double* __restrict__ x, long ldx, double* __restrict__ t, long ldt)
{
    const long N = T.ncell;
    const long c = (long)blockIdx.x * RICH_T + threadIdx.x;
    if (c >= N) return;
    const unsigned w = T.cw[c];
    const unsigned skip = sub ? (w & 63u) : 0u;
    double acc[NV][NS];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int l = 0; l < NS; ++l) acc[v][l] = b[v * ldb + c * NS + l];
    for (int q = 0; q < 7; ++q) {
        long n = c;
        int slot = 6;
        if (q < 6) {
            n = T.col[(long)q * N + c];
            if (n < 0 || ((skip >> q) & 1u)) continue;
            slot = TR ? (int)((w >> (6 + 3 * q)) & 7u) : q;
        }
        const double* B = T.mat + (long)slot * (NS * NS) * N + (TR ? n : c);
        double xv[NV][NS];
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int l = 0; l < NS; ++l) xv[v][l] = x[v * ldx + n * NS + l];
#pragma unroll
        for (int l = 0; l < NS; ++l) {
            double bv[NS];                          // one block column: d row ll / d column l, ll = 0 .. NS - 1
#pragma unroll
            for (int ll = 0; ll < NS; ++ll) bv[ll] = B[(long)(l * NS + ll) * N];
#pragma unroll
            for (int v = 0; v < NV; ++v)
#pragma unroll
                for (int ll = 0; ll < NS; ++ll) {
                    if (TR) acc[v][l] -= bv[ll] * xv[v][ll];
                    else acc[v][ll] -= bv[ll] * xv[v][l];
                }
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int l = 0; l < NS; ++l) t[v * ldt + c * NS + l] = acc[v][l];
}

#define RICH_DISPATCH(nState, ONFAIL, ...)                                             \
    switch (nState) {                                                                  \
    case 1: { constexpr int NS_ = 1; __VA_ARGS__; } break;                             \
    case 5: { constexpr int NS_ = 5; __VA_ARGS__; } break;                             \
    case 6: { constexpr int NS_ = 6; __VA_ARGS__; } break;                             \
    default: ONFAIL;                                                                   \
    }

void launch_rich_copy(const JmBlk* src, int nslots, int maxnx, int maxny, int maxnz, int nState, const PcMgSten& S, const double* tsm,
                      double turbDiag, long N, const int* col, double* mat, hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz, launch_rich_copy(src + s0_, n_, maxnx, maxny, maxnz, nState, S, tsm, turbDiag, N, col, mat, s));
    if (nslots <= 0) return;
    const dim3 g((maxnx + 63) / 64, (maxny + 3) / 4, maxnz * nslots);
    RICH_DISPATCH(nState, (void)adf_fail("pc_rich: no kernel for this nState"),
                  hipLaunchKernelGGL((k_rich_copy<NS_>), g, dim3(64, 4, 1), 0, s, src, maxnz, S, tsm, turbDiag, N, col, mat))
}

int launch_rich_residual(const PcRichTab& T, int nState, int transpose, int sub, int nv, const double* b, long ldb, const double* x,
                         long ldx, double* t, long ldt, hipStream_t s)
{
    if (T.ncell <= 0) return 0;
    const dim3 g((unsigned)((T.ncell + RICH_T - 1) / RICH_T), 1, 1), blk(RICH_T, 1, 1);
#define RICH_RES(TR)                                                                                                         \
    RICH_DISPATCH(nState, return adf_fail("pc_rich: no kernel for this nState"),                                             \
                  ADF_DISPATCH_NV(nv, return adf_fail("pc_rich: no kernel for this many vectors"),                           \
                                  hipLaunchKernelGGL((k_rich_residual<NS_, TR, NV_>), g, blk, 0, s, T, sub, b, ldb, x, ldx, t, ldt)))
    if (transpose) { RICH_RES(1) } else { RICH_RES(0) }
#undef RICH_RES
    return 0;
}
