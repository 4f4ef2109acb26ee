// ILU(k), k = 0 .. 3, of the assembled 7-point preconditioner matrix over the WHOLE level on a general block pattern
// (adflow_gpu_pc_set_level_fill, then adflow_gpu_pc_setup / _ank_pc_setup; api.hip runs the symbolic factorisation and builds the
// tables, pc_level_tables).
//
// Reference semantics: the PCApply of setupStandardKSP (adjointUtils.F90:1374-1562) on one process: one ASM subdomain over every block
// the process owns, PCFactorSetLevels(fill), natural ordering = block after block in ascending nn, then k, j, i.  The columns are those
// of kernels_pc_coupled.hip: an owned cell is its own column, a first-layer face halo the owned cell it has as donor.
// Another ordering (adflow_gpu_pc_set_ordering: RCM, a caller's permutation) is a relabelling in the tables: wherever this file says
// "natural number" of a row or column, read its number in the ordering of the factor.  PclTab::vec alone leads back to the vectors.
//
// Pattern: across an interface the level-of-fill pattern is no stencil (kernels_pc_fill.hip) and elimination does not stay on the
// diagonal (kernels_pc_coupled.hip).  The host runs the symbolic ILU(k) on the cell graph once; a row holds its entries in ascending
// column order: nLow lower entries, the pivot block, the upper entries -- 7 to 37 of them at fill 2.
//
// Arithmetic: IKJ restricted to the pattern (Saad, Iterative Methods, alg. 10.4), exactly as k_pcf_factor: row c starts as the
// assembled row (zero in the fill entries, T on the diagonal); for its lower entries n in ascending column order
//   L_{c,n} = row_{c,n} D_n^-1,     row_{c,m} -= L_{c,n} U_{n,m}  for the upper entries m of row n inside the pattern of row c
// and then the LU factors of D_c (below).  Where (n, m) lands in row c is found by a two-pointer merge of the upper part of row n
// with the rest of row c, both sorted by the natural number of the column (PclTab::enat): two more integer loads per step and no table whose size is the sum over
// the lower entries of the upper lengths (up to 24 x 21 targets per row at fill 2).  The thread holds one L block and one column of U
// and of the target at a time.
//
// Scheduling: the level sets of the row dependencies (longest path over the lower entries of the whole level), one plain launch per
// set, one thread per row, workgroups of one wave; the sweeps run the same sets up and down.
//
// Storage: proportional to the pattern.  Position q of the order (set, natural number) belongs to slice q / 64 of its set -- the rows of
// one workgroup.  A slice of `st` rows (64, fewer at the end of a set) whose longest row has w entries holds w st entry slots from
// slot ebase on: entry j of lane t is slot ebase + j st + t of the integer tables, and its block is
//   fac[ebase nState^2 + ((j nState^2 + e) st + t)]        e = l nState + ll as in the sibling factors
// so a wave streams every component plane of its slice coalesced.  ebase nState^2 is 64-bit pointer arithmetic; the 32-bit byte
// offset spans one slice.  A row of another slice is reached through its own ebase, lane and stride (PclTab::ebase, rinfo).
// TR = 1 reads the blocks of the neighbours' rows: the entry of row n that points back to c is the mirror entry (PclTab::einfo).
#include "internal.h"
#include "pc_block.h"

// The pivot block of a row is kept as its LU factors with partial pivoting, not as its inverse: P D = L U in place (L unit lower, the
// diagonal of U as reciprocals), the row exchanges packed three bits each into PclTab::rpiv.  A solve costs the nState^2 products of
// the product with the inverse; where fill makes the factor ill-conditioned the inverse costs two digits that the solve keeps (a
// period of three cells at fill 1: the library was 69 x as far from the extended-precision run as a float64 numpy run with D^-1 as
// a product, in the sweeps alone -- DESIGN).  Every index is a compile-time constant, an exchange is a conditional swap.
template <int NS>
__device__ __forceinline__ bool pcl_lu(double (&a)[NS * NS], int& piv)
{
    bool ok = true;
    piv = 0;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        int p = k;
        double best = fabs(PCE(a, k, k));
#pragma unroll
        for (int r = k + 1; r < NS; ++r) {
            const double v = fabs(PCE(a, r, k));
            const bool g = v > best;
            p = g ? r : p;
            best = g ? v : best;
        }
        piv |= p << (3 * k);
#pragma unroll
        for (int r = k + 1; r < NS; ++r) {
            const bool sw = p == r;
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                const double t = PCE(a, k, c), u = PCE(a, r, c);
                PCE(a, k, c) = sw ? u : t;
                PCE(a, r, c) = sw ? t : u;
            }
        }
        const double pv = PCE(a, k, k);
        ok = ok && (fabs(pv) > 0.0) && (fabs(pv) <= 1.7976931348623157e308);
#pragma unroll
        for (int r = k + 1; r < NS; ++r) {
            const double f = PCE(a, r, k) / pv;
            PCE(a, r, k) = f;
#pragma unroll
            for (int c = k + 1; c < NS; ++c) PCE(a, r, c) -= f * PCE(a, k, c);
        }
        PCE(a, k, k) = 1.0 / pv;
    }
    return ok;
}

// b <- D^-1 b (TR = 0) or D^-T b (TR = 1) with the factors of pcl_lu
template <int NS, int TR>
__device__ __forceinline__ void pcl_lu_solve(const double (&a)[NS * NS], int piv, double (&b)[NS])
{
    if (!TR) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int p = (piv >> (3 * k)) & 7;
#pragma unroll
            for (int r = k + 1; r < NS; ++r) {
                const bool sw = p == r;
                const double t = b[k], u = b[r];
                b[k] = sw ? u : t;
                b[r] = sw ? t : u;
            }
        }
        // (the exchanges moved whole rows, those of L included: P b first, then the two triangles)
#pragma unroll
        for (int k = 0; k < NS; ++k)
#pragma unroll
            for (int r = k + 1; r < NS; ++r) b[r] -= PCE(a, r, k) * b[k];
#pragma unroll
        for (int k = NS - 1; k >= 0; --k) {
            double t = b[k];
#pragma unroll
            for (int m = k + 1; m < NS; ++m) t -= PCE(a, k, m) * b[m];
            b[k] = t * PCE(a, k, k);
        }
    } else {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            double t = b[k];
#pragma unroll
            for (int m = 0; m < k; ++m) t -= PCE(a, m, k) * b[m];
            b[k] = t * PCE(a, k, k);
        }
#pragma unroll
        for (int k = NS - 1; k >= 0; --k)
#pragma unroll
            for (int r = k + 1; r < NS; ++r) b[k] -= PCE(a, r, k) * b[r];
#pragma unroll
        for (int k = NS - 1; k >= 0; --k) {
            const int p = (piv >> (3 * k)) & 7;
#pragma unroll
            for (int r = k + 1; r < NS; ++r) {
                const bool sw = p == r;
                const double t = b[k], u = b[r];
                b[k] = sw ? u : t;
                b[r] = sw ? t : u;
            }
        }
    }
}

#define PCL_T 64          // one wave per workgroup, as kernels_pc.hip; the slices of the storage are the workgroups of a launch

// one level set of the factorisation: lanes q0 .. q0 + cnt - 1.  The rows of the lower entries are complete (earlier launches)
template <int NS>
__global__ __launch_bounds__(PCL_T) void k_pcl_factor(PclTab T, int q0, int cnt)
{
    constexpr int NB = NS * NS;
    const int t = blockIdx.x * PCL_T + threadIdx.x;
    if (t >= cnt) return;
    const unsigned q = (unsigned)(q0 + t);
    const int left = cnt - (int)blockIdx.x * PCL_T;
    const unsigned st = (unsigned)(left < PCL_T ? left : PCL_T), ln = threadIdx.x, ln8 = ln * 8u, st8 = st * 8u;
    const long N = T.ncell, eb = T.ebase[q];
    const int rc = T.rcnt[q], nl = rc & 0xffff, ne = rc >> 16;
    const int* __restrict__ ip = T.epos + eb;
    const int* __restrict__ ik = T.enat + eb;
    const int* __restrict__ ii = T.einfo + eb;
    GPTR(double) Fr = (GPTR(double))T.fac + eb * NB;
    const JmBlk b = T.blk[T.cblk[q]];
    const unsigned c8 = (unsigned)T.cbox[q] * 8u, nb8 = (unsigned)b.nbox * 8u;
    // ---- the row as assembled: fill entries start from zero, T goes on the diagonal
#pragma nounroll
    for (int j = 0; j < ne; ++j) {
        const int d = (ii[j * st + ln] >> 16) - 1;
        const unsigned o = (unsigned)(j * NB) * st8 + ln8;
        if (d < 0) {
#pragma unroll
            for (int e = 0; e < NB; ++e) stg(Fr, o + e * st8, 0.0);
            continue;
        }
        GPTR(const double) A = (GPTR(const double))(b.jac + (long)T.sten[d] * NB * b.nbox);
        double D[NB];
#pragma unroll
        for (int e = 0; e < NB; ++e) D[e] = ldg(A, c8 + e * nb8);
        if (j == nl) {
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
        }
#pragma unroll
        for (int e = 0; e < NB; ++e) stg(Fr, o + e * st8, D[e]);
    }
    // ---- elimination with the rows of the lower entries, in ascending column order
#pragma nounroll
    for (int jl = 0; jl < nl; ++jl) {
        const int n = ip[jl * st + ln];
        const long ebn = T.ebase[n];
        const int rin = T.rinfo[n], rcn = T.rcnt[n], nen = rcn >> 16;
        const unsigned lnn8 = (unsigned)(rin & 0xff) * 8u, stn = (unsigned)(rin >> 8), stn8 = stn * 8u;
        GPTR(const double) Fn = (GPTR(const double))T.fac + ebn * NB;
        const int* __restrict__ ikn = T.enat + ebn + (rin & 0xff);
        const unsigned ol = (unsigned)(jl * NB) * st8 + ln8;
        double L[NB];
        {
            // L_{c,n} = row_{c,n} D_n^-1, row by row: D_n^T y = row_{c,n}(r, :)^T with the factors of D_n
            double X[NB];
            const unsigned od = (unsigned)((rcn & 0xffff) * NB) * stn8 + lnn8;
            const int pv = T.rpiv[n];
#pragma unroll
            for (int i = 0; i < NB; ++i) X[i] = ldg(Fn, od + i * stn8);
#pragma unroll
            for (int i = 0; i < NB; ++i) L[i] = ldg(Fr, ol + i * st8);                   // row_{c,n}
#pragma unroll
            for (int r = 0; r < NS; ++r) {
                double y[NS];
#pragma unroll
                for (int m = 0; m < NS; ++m) y[m] = PCE(L, r, m);
                pcl_lu_solve<NS, 1>(X, pv, y);
#pragma unroll
                for (int m = 0; m < NS; ++m) PCE(L, r, m) = y[m];
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) stg(Fr, ol + i * st8, L[i]);
        // the upper entries a of row n against the entries b behind jl of row c: both ascend in the natural number of the column
        int a = (rcn & 0xffff) + 1, bq = jl + 1;
        if (a >= nen) continue;
        int ka = ikn[a * stn], kb = ik[bq * st + ln];
#pragma nounroll
        while (true) {
            if (ka == kb) {
                const unsigned ou = (unsigned)(a * NB) * stn8 + lnn8, ot = (unsigned)(bq * NB) * st8 + ln8;
#pragma unroll
                for (int l = 0; l < NS; ++l) {                                           // column l of the target
                    // the product L_{c,n} U_{n,m} is summed on its own and subtracted from the target ONCE (pc_schur_sub)
                    double uc[NS], tc[NS], pr[NS];
#pragma unroll
                    for (int m = 0; m < NS; ++m) uc[m] = ldg(Fn, ou + (l * NS + m) * stn8);
#pragma unroll
                    for (int r = 0; r < NS; ++r) tc[r] = ldg(Fr, ot + (l * NS + r) * st8);
#pragma unroll
                    for (int r = 0; r < NS; ++r) pr[r] = 0.0;
#pragma unroll
                    for (int m = 0; m < NS; ++m)
#pragma unroll
                        for (int r = 0; r < NS; ++r) pr[r] += PCE(L, r, m) * uc[m];
#pragma unroll
                    for (int r = 0; r < NS; ++r) stg(Fr, ot + (l * NS + r) * st8, tc[r] - pr[r]);
                }
            }
            // (the pivot of row c is in the pattern and every column of row n beyond it is larger than jl's: bq stays below ne while
            // a column of row n remains that is not larger than the last column of row c)
            const bool stepA = ka <= kb, stepB = kb <= ka;
            if (stepA && ++a >= nen) break;
            if (stepB && ++bq >= ne) break;
            if (stepA) ka = ikn[a * stn];
            if (stepB) kb = ik[bq * st + ln];
        }
    }
    // ---- the pivot block
    const unsigned od = (unsigned)(nl * NB) * st8 + ln8;
    double D[NB];
#pragma unroll
    for (int e = 0; e < NB; ++e) D[e] = ldg(Fr, od + e * st8);
    int pv;
    if (!pcl_lu<NS>(D, pv)) T.flag[0] = (int)q + 1;     // any of the failing cells: the host names one of them
    T.rpiv[q] = pv;
#pragma unroll
    for (int e = 0; e < NB; ++e) stg(Fr, od + e * st8, D[e]);
}

// one level set of a triangular sweep, the four forms of k_pcf_sweep with the entry counts of the row; one neighbour block is live at
// a time.  BACK = 0: ascending sets, the lower entries, input r; BACK = 1: descending sets, the upper entries, input ws, output also z.
//   TR = 0:  forward  y_c = r_c - sum L_{c,n} y_n            backward  z_c = D_c^-1 (y_c - sum U_{c,n} z_n)      (entry j of row c)
// D_c^-1 and D_c^-T are solves with the factors of the pivot block (pcl_lu_solve)
//   TR = 1:  forward  y_c = D_c^-T (r_c - sum U_{n,c}^T y_n)  backward  z_c = y_c - sum L_{n,c}^T z_n             (mirror entry of row n)
template <int NS, int TR, int BACK>
__global__ __launch_bounds__(PCL_T) void k_pcl_sweep(PclTab T, int q0, int cnt, const double* __restrict__ r, double* __restrict__ z)
{
    constexpr int NB = NS * NS;
    const int t = blockIdx.x * PCL_T + threadIdx.x;
    if (t >= cnt) return;
    const unsigned q = (unsigned)(q0 + t), q8 = q * 8u;
    const int left = cnt - (int)blockIdx.x * PCL_T;
    const unsigned st = (unsigned)(left < PCL_T ? left : PCL_T), ln = threadIdx.x, ln8 = ln * 8u, st8 = st * 8u;
    const long N = T.ncell, eb = T.ebase[q];
    const unsigned N8 = (unsigned)N * 8u;
    const int rc = T.rcnt[q], nl = rc & 0xffff, ne = rc >> 16;
    const int* __restrict__ ip = T.epos + eb;
    const int* __restrict__ ii = T.einfo + eb;
    GPTR(const double) Fr = (GPTR(const double))T.fac + eb * NB;
    GPTR(double) W = (GPTR(double))T.ws;
    const long m = (long)T.vec[q] * NS;
    double acc[NS];
    if (BACK) {
#pragma unroll
        for (int l = 0; l < NS; ++l) acc[l] = ldg(W, q8 + l * N8);
    } else {
#pragma unroll
        for (int l = 0; l < NS; ++l) acc[l] = r[m + l];
    }
    const int j0 = BACK ? nl + 1 : 0, j1 = BACK ? ne : nl;
#pragma nounroll
    for (int j = j0; j < j1; ++j) {
        const int n = ip[j * st + ln];
        const unsigned n8 = (unsigned)n * 8u;
        double xv[NS], bv[NB];
#pragma unroll
        for (int l = 0; l < NS; ++l) xv[l] = ldg(W, n8 + l * N8);
        if (TR) {
            const int mir = ii[j * st + ln] & 0xffff, rin = T.rinfo[n];
            const unsigned stn8 = (unsigned)(rin >> 8) * 8u, o = (unsigned)(mir * NB) * stn8 + (unsigned)(rin & 0xff) * 8u;
            GPTR(const double) Fn = (GPTR(const double))T.fac + T.ebase[n] * NB;
#pragma unroll
            for (int i = 0; i < NB; ++i) bv[i] = ldg(Fn, o + i * stn8);
        } else {
            const unsigned o = (unsigned)(j * NB) * st8 + ln8;
#pragma unroll
            for (int i = 0; i < NB; ++i) bv[i] = ldg(Fr, o + i * st8);
        }
        if (TR) {
#pragma unroll
            for (int l = 0; l < NS; ++l)
#pragma unroll
                for (int ll = 0; ll < NS; ++ll) acc[l] -= PCE(bv, ll, l) * xv[ll];
        } else {
#pragma unroll
            for (int l = 0; l < NS; ++l)
#pragma unroll
                for (int ll = 0; ll < NS; ++ll) acc[ll] -= PCE(bv, ll, l) * xv[l];
        }
    }
    if (TR != BACK) {
        const unsigned o = (unsigned)(nl * NB) * st8 + ln8;
        double bv[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) bv[i] = ldg(Fr, o + i * st8);
        pcl_lu_solve<NS, TR>(bv, T.rpiv[q], acc);
    }
#pragma unroll
    for (int l = 0; l < NS; ++l) stg(W, q8 + l * N8, acc[l]);
    if (BACK) {
#pragma unroll
        for (int l = 0; l < NS; ++l) z[m + l] = acc[l];
    }
}

#define PCL_DISPATCH(nState, ...)                                                      \
    switch (nState) {                                                                  \
    case 1: { constexpr int NS_ = 1; __VA_ARGS__; } break;                             \
    case 5: { constexpr int NS_ = 5; __VA_ARGS__; } break;                             \
    case 6: { constexpr int NS_ = 6; __VA_ARGS__; } break;                             \
    default: return adf_fail("pc: no kernel for this nState");                         \
    }

int launch_pcl_factor(const PclTab& T, int nState, const std::vector<int>& setStart, hipStream_t s)
{
    for (size_t p = 0; p + 1 < setStart.size(); ++p) {
        const int q0 = setStart[p], cnt = setStart[p + 1] - q0;
        if (cnt <= 0) continue;
        PCL_DISPATCH(nState, hipLaunchKernelGGL((k_pcl_factor<NS_>), dim3((cnt + PCL_T - 1) / PCL_T), dim3(PCL_T), 0, s, T, q0, cnt))
    }
    return 0;
}

template <int NS, int TR>
static void pcl_apply_sets(const PclTab& T, const std::vector<int>& setStart, const double* r, double* z, hipStream_t s)
{
    const int np = (int)setStart.size() - 1;
    for (int p = 0; p < np; ++p) {
        const int q0 = setStart[p], cnt = setStart[p + 1] - q0;
        if (cnt > 0) hipLaunchKernelGGL((k_pcl_sweep<NS, TR, 0>), dim3((cnt + PCL_T - 1) / PCL_T), dim3(PCL_T), 0, s, T, q0, cnt, r, z);
    }
    for (int p = np - 1; p >= 0; --p) {
        const int q0 = setStart[p], cnt = setStart[p + 1] - q0;
        if (cnt > 0) hipLaunchKernelGGL((k_pcl_sweep<NS, TR, 1>), dim3((cnt + PCL_T - 1) / PCL_T), dim3(PCL_T), 0, s, T, q0, cnt, r, z);
    }
}

int launch_pcl_apply(const PclTab& T, int nState, int transpose, const std::vector<int>& setStart, const double* r, double* z,
                     hipStream_t s)
{
    if (transpose) { PCL_DISPATCH(nState, pcl_apply_sets<NS_, 1>(T, setStart, r, z, s)) }
    else { PCL_DISPATCH(nState, pcl_apply_sets<NS_, 0>(T, setStart, r, z, s)) }
    return 0;
}
