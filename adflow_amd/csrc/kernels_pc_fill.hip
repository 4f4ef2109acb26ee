// Block ILU(1) and ILU(2) of the assembled 7-point preconditioner matrix in the natural ordering, factored and applied on the device
// (adflow_gpu_pc_set_fill, then adflow_gpu_pc_setup / _ank_pc_setup, api.hip).  Fill 0 stays with kernels_pc.hip.
//
// Reference semantics: PCFactorSetLevels(fill) of setupStandardKSP (adjointUtils.F90:1559) with matrixOrdering = "natural", one
// subdomain per structured block, halo columns dropped.
//
// Pattern: in the natural ordering the level-of-fill pattern of a structured block is a fixed stencil of offsets cut at the faces of
// the block -- 13 offsets at fill 1, 23 at fill 2 (api.hip derives them by the symbolic factorisation in offset space; at fill 3
// entries go missing near the faces, which is why fill > 2 is refused).  A row holds nLow = 6 or 11 lower entries, as many upper
// entries and the pivot block; each side is kept in ascending column order, so upper entry u mirrors lower entry nLow-1-u.
//
// Arithmetic: IKJ restricted to the pattern (Saad, Iterative Methods, alg. 10.4).  Row c starts as the assembled row (zero in the fill
// entries); for its lower entries n in ascending column order
//   L_{c,n} = row_{c,n} D_n^-1,     row_{c,m} -= L_{c,n} U_{n,m}  for the upper entries m of row n inside the pattern of row c
// and then D_c^-1.  A row of 23 blocks of nState^2 does not fit in registers: it lives in the factor's own storage from the start,
// and the thread holds one L block and one column of U and of the target at a time.  The slot (n, m) lands in depends on the two
// entry numbers only: PcTab::tgt.
//
// Scheduling: row c needs the complete rows of its lower entries.  The level sets of that dependency (longest path, computed on the
// host from the pattern) replace the hyperplanes i + j + k of fill 0 -- an entry at (+1,-1,0) lies on the hyperplane of its row.  One
// plain launch per level set covers every block of the level; the sweeps run the same sets up and down.
//
// Storage: as in kernels_pc.hip with more slots.  Position q of the order (level set, block, k, j, i) holds
//   fac[q + ((s nState + l) nState + ll) N]   s = 0..nLow-1: L; nLow..2 nLow-1: U; 2 nLow: D^-1
// so a wave streams every component plane coalesced; nbr[s N + q] is the position of the cell of off-diagonal slot s or -1 outside the
// block.  Plane offsets are 64-bit pointer arithmetic, the 32-bit byte offset spans the positions of one plane only: the factor may
// exceed 4 GiB as long as one vector of the level does not (checked in pc_setup_build).
//
// Several vectors at once: k_pcf_sweep takes the vector count NV = 1 .. 4 of k_pc_sweep -- the dependent chain of position and block
// loads of an entry is walked once per lane for all NV vectors.  Instantiated at fill 1 (13 entries); at fill 2 the sweeps exist for one
// vector and adflow_gpu_pc_apply_multi applies the factor column by column (no measurement stands behind a wider fill-2 sweep).
#include "internal.h"
#include "pc_block.h"

#define PCF_T 64          // one wave per workgroup, as kernels_pc.hip: a level set of a few thousand cells still spreads over the CUs

// one level set of the factorisation: lanes q0 .. q0 + cnt - 1.  The rows of the lower entries are complete (earlier launches)
template <int NS, int NE>
__global__ __launch_bounds__(PCF_T) void k_pcf_factor(PcTab T, int q0, int cnt)
{
    constexpr int NL = (NE - 1) / 2, NB = NS * NS;
    const int t = blockIdx.x * PCF_T + threadIdx.x;
    if (t >= cnt) return;
    const unsigned q = (unsigned)(q0 + t), q8 = q * 8u;
    const long N = T.ncell;
    const JmBlk b = T.blk[T.cblk[q]];
    const unsigned c8 = (unsigned)T.cbox[q] * 8u, nb8 = (unsigned)b.nbox * 8u;
    GPTR(double) F = (GPTR(double))T.fac;
    GPTR(double) Fd = F + (long)(2 * NL) * NB * N;
    // ---- the row as assembled: entries outside the block and fill entries start from zero
#pragma nounroll
    for (int s = 0; s < 2 * NL; ++s) {
        GPTR(double) Fs = F + (long)s * NB * N;
        const int a = T.asmEnt[s];
        if (a >= 0 && T.nbr[(long)s * N + q] >= 0) {
            GPTR(const double) A = (GPTR(const double))(b.jac + (long)a * NB * b.nbox);
#pragma unroll
            for (int e = 0; e < NB; ++e) stg(Fs + e * N, q8, ldg(A, c8 + e * nb8));
        } else {
#pragma unroll
            for (int e = 0; e < NB; ++e) stg(Fs + e * N, q8, 0.0);
        }
    }
    {
        double D[NB];
        GPTR(const double) A = (GPTR(const double))(b.jac + (long)T.asmEnt[2 * NL] * NB * b.nbox);
#pragma unroll
        for (int e = 0; e < NB; ++e) D[e] = ldg(A, c8 + e * nb8);
        // the pseudo-time term of ANK and the pivot shift of the turbulence KSP, exactly as k_pc_factor adds them
        if constexpr (NS >= 5) {
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
#pragma unroll
        for (int e = 0; e < NB; ++e) stg(Fd + e * N, q8, D[e]);
    }
    // ---- elimination with the rows of the lower entries, in ascending column order
#pragma nounroll
    for (int e = 0; e < NL; ++e) {
        const int n = T.nbr[(long)e * N + q];
        if (n < 0) continue;
        const unsigned n8 = (unsigned)n * 8u;
        GPTR(double) Fe = F + (long)e * NB * N;
        double L[NB];
        {
            double X[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) X[i] = ldg(Fd + i * N, n8);                 // D_n^-1
#pragma unroll
            for (int i = 0; i < NB; ++i) L[i] = 0.0;
#pragma unroll
            for (int m = 0; m < NS; ++m)
#pragma unroll
                for (int r = 0; r < NS; ++r) {
                    const double arm = ldg(Fe + (m * NS + r) * N, q8);               // row_{c,n}(r, m)
#pragma unroll
                    for (int l = 0; l < NS; ++l) PCE(L, r, l) += arm * PCE(X, m, l);
                }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) stg(Fe + i * N, q8, L[i]);
#pragma nounroll
        for (int u = 0; u < NL; ++u) {
            const int tg = T.tgt[e * NL + u];
            if (tg < 0) continue;
            if (tg < 2 * NL && T.nbr[(long)tg * N + q] < 0) continue;                // the target cell lies outside the block
            GPTR(const double) Fu = F + (long)(NL + u) * NB * N;                     // U_{n,m}
            GPTR(double) Ft = F + (long)tg * NB * N;
#pragma unroll
            for (int l = 0; l < NS; ++l) {                                           // column l of the target
                // the product L_{c,n} U_{n,m} is summed on its own and subtracted from the target ONCE: subtracting its nState terms
                // from the target one by one costs a digit on wall-clustered curved meshes (`annulus` x `ilu-fill`)
                double uc[NS], tc[NS], pr[NS];
#pragma unroll
                for (int m = 0; m < NS; ++m) uc[m] = ldg(Fu + (l * NS + m) * N, n8);
#pragma unroll
                for (int r = 0; r < NS; ++r) tc[r] = ldg(Ft + (l * NS + r) * N, q8);
#pragma unroll
                for (int r = 0; r < NS; ++r) pr[r] = 0.0;
#pragma unroll
                for (int m = 0; m < NS; ++m)
#pragma unroll
                    for (int r = 0; r < NS; ++r) pr[r] += PCE(L, r, m) * uc[m];
#pragma unroll
                for (int r = 0; r < NS; ++r) stg(Ft + (l * NS + r) * N, q8, tc[r] - pr[r]);
            }
        }
    }
    // ---- the pivot block
    double D[NB];
#pragma unroll
    for (int e = 0; e < NB; ++e) D[e] = ldg(Fd + e * N, q8);
    if (!pc_invert<NS>(D)) T.flag[0] = (int)q + 1;      // any of the failing cells: the host names one of them
#pragma unroll
    for (int e = 0; e < NB; ++e) stg(Fd + e * N, q8, D[e]);
}

// one level set of a triangular sweep, the four forms of k_pc_sweep (kernels_pc.hip) over nLow entries; one neighbour block is live
// at a time.  TR = 1 reads the blocks of the neighbours' rows: the entry of row n that points back to c is the mirror of the entry
// of row c that points to n.
// NV vectors at once exactly as k_pc_sweep takes them: the chain of position and block loads is shared, the vector loads and the
// products are per vector
template <int NS, int NE, int TR, int BACK, int NV = 1>
__global__ __launch_bounds__(PCF_T) void k_pcf_sweep(PcTab T, int q0, int cnt, const double* __restrict__ r, double* __restrict__ z, long ldr,
                                                     long ldz)
{
    constexpr int NL = (NE - 1) / 2, NB = NS * NS;
    const int t = blockIdx.x * PCF_T + threadIdx.x;
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
#pragma nounroll
    for (int e = 0; e < NL; ++e) {
        const int col = BACK ? NL + e : e;
        const int n = T.nbr[(long)col * N + q];
        if (n < 0) continue;
        const unsigned n8 = (unsigned)n * 8u, at = TR ? n8 : q8;
        const int slot = TR ? (BACK ? NL - 1 - e : 2 * NL - 1 - e) : col;
        GPTR(const double) Fs = F + (long)slot * NB * N;
        double xv[NV][NS], bv[NB];
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int l = 0; l < NS; ++l) xv[v][l] = ldg(W[v], n8 + l * N8);
#pragma unroll
        for (int i = 0; i < NB; ++i) bv[i] = ldg(Fs + i * N, at);
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
        GPTR(const double) Fd = F + (long)(2 * NL) * NB * N;
        double bv[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) bv[i] = ldg(Fd + i * N, q8);
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

#define PCF_DISPATCH(nState, nEnt, ...)                                                \
    switch ((nState) * 100 + (nEnt)) {                                                 \
    case 113: { constexpr int NS_ = 1, NE_ = 13; __VA_ARGS__; } break;                 \
    case 123: { constexpr int NS_ = 1, NE_ = 23; __VA_ARGS__; } break;                 \
    case 513: { constexpr int NS_ = 5, NE_ = 13; __VA_ARGS__; } break;                 \
    case 523: { constexpr int NS_ = 5, NE_ = 23; __VA_ARGS__; } break;                 \
    case 613: { constexpr int NS_ = 6, NE_ = 13; __VA_ARGS__; } break;                 \
    case 623: { constexpr int NS_ = 6, NE_ = 23; __VA_ARGS__; } break;                 \
    default: return adf_fail("pc: no kernel for this nState and fill");                \
    }

int launch_pcf_factor(const PcTab& T, int nState, int nEnt, const std::vector<int>& levelStart, hipStream_t s)
{
    for (size_t p = 0; p + 1 < levelStart.size(); ++p) {
        const int q0 = levelStart[p], cnt = levelStart[p + 1] - q0;
        if (cnt <= 0) continue;
        PCF_DISPATCH(nState, nEnt,
                     hipLaunchKernelGGL((k_pcf_factor<NS_, NE_>), dim3((cnt + PCF_T - 1) / PCF_T), dim3(PCF_T), 0, s, T, q0, cnt))
    }
    return 0;
}

template <int NS, int NE, int TR, int NV>
static void pcf_apply_sets(const PcTab& T, const std::vector<int>& levelStart, const double* r, double* z, long ldr, long ldz, hipStream_t s)
{
    const int np = (int)levelStart.size() - 1;
    for (int p = 0; p < np; ++p) {
        const int q0 = levelStart[p], cnt = levelStart[p + 1] - q0;
        if (cnt > 0)
            hipLaunchKernelGGL((k_pcf_sweep<NS, NE, TR, 0, NV>), dim3((cnt + PCF_T - 1) / PCF_T), dim3(PCF_T), 0, s, T, q0, cnt, r, z, ldr,
                               ldz);
    }
    for (int p = np - 1; p >= 0; --p) {
        const int q0 = levelStart[p], cnt = levelStart[p + 1] - q0;
        if (cnt > 0)
            hipLaunchKernelGGL((k_pcf_sweep<NS, NE, TR, 1, NV>), dim3((cnt + PCF_T - 1) / PCF_T), dim3(PCF_T), 0, s, T, q0, cnt, r, z, ldr,
                               ldz);
    }
}

#define PCF_DISPATCH_NV(nv, ...) ADF_DISPATCH_NV(nv, return adf_fail("pc: no kernel for this number of vectors"), __VA_ARGS__)

// several vectors at fill 1 only: the fill-2 sweeps (23 entries) are instantiated for one vector (api.hip serves fill 2 column by column)
template <int NS, int NE, int TR>
static int pcf_apply_nv(const PcTab& T, const std::vector<int>& levelStart, const double* r, double* z, long ldr, long ldz, hipStream_t s,
                        int nv)
{
    if constexpr (NE == 23) {
        if (nv != 1) return adf_fail("pc: the fill-2 sweeps take one vector");
        pcf_apply_sets<NS, NE, TR, 1>(T, levelStart, r, z, ldr, ldz, s);
    } else {
        PCF_DISPATCH_NV(nv, pcf_apply_sets<NS, NE, TR, NV_>(T, levelStart, r, z, ldr, ldz, s))
    }
    return 0;
}

int launch_pcf_apply(const PcTab& T, int nState, int nEnt, int transpose, const std::vector<int>& levelStart, const double* r,
                     double* z, hipStream_t s, int nv, long ldr, long ldz)
{
    if (transpose) { PCF_DISPATCH(nState, nEnt, return pcf_apply_nv<NS_, NE_, 1>(T, levelStart, r, z, ldr, ldz, s, nv)) }
    else { PCF_DISPATCH(nState, nEnt, return pcf_apply_nv<NS_, NE_, 0>(T, levelStart, r, z, ldr, ldz, s, nv)) }
    return 0;
}
