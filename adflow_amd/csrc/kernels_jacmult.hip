// Products with the assembled matrix on the device: y = J x and y = J^T x for the stencil blocks adflow_gpu_fd_jacobian left on the
// level (kernels_jac.hip), on PETSc-layout vectors of nState entries per owned cell.
//
// Reference semantics: MatMult on the matrices of adjointUtils::setupStateResidualMatrix -- solveAdjoint's GMRES on dRdwT
// (adjointAPI.F90:661-863, MatMult :741 / :806; as shell operations dRdwTMatMult :1007 and dRdwMatMult :1050).  Block (ll, l) of
// stencil entry s at row cell (i,j,k) is d dw(i,j,k,ll) / d w(i-di(s), j-dj(s), k-dk(s), l); a column on a halo cell is the owned
// cell of the neighbouring block that halo has as donor, every other halo cell is no column (the insertion loop,
// adjointUtils.F90:560-700: globalCell >= 0).
//
// Storage: jac[c + ((s nState + l) nState + ll) nbox], c the box index with i fastest: lanes along i read every (s, l, ll) plane
// coalesced, and both products are ONE streaming pass over the matrix (nStencil nState^2 x 8 B per owned cell; the 2 nState doubles
// per cell of the vectors are below 1 % of that and stay in L2).
//   forward   : x -> halo'd array xs (zero halos), the 2-layer exchange fills the halos that have a donor, one lane per ROW cell
//               gathers  y(row) = sum_s B_s(row) x(row - d_s)
//   transposed: one lane per COLUMN cell of the whole halo'd box gathers  ys(col) = sum_s B_s(col + d_s)^T x(col + d_s)  over the
//               owned rows col + d_s (again coalesced in i, no atomics); the exchange then runs in reverse: every halo's value is
//               ADDED to its donor through a donor-sorted list (k_jac_halo_accumulate: one lane per donor, its halos in a fixed
//               order -- the result does not depend on the execution order)
// One stencil entry of a lane is nState^2 independent 8-byte loads (36 for RANS) issued together: 18 KB in flight per wave, several
// waves per SIMD -- the streaming regime without any staging.
//
// Several vectors at once (adflow_gpu_jacobian_mult_multi): both product kernels take a vector count NV = 1 .. 4 -- the nState^2 loads
// of a stencil entry are issued once and feed nState x NV accumulators, so NV products cost one pass over the matrix.  xs and ys hold
// the vectors one behind the other (vector v: components v nState .. of the same box layout); scatter, exchange, reverse accumulation
// and gather run per vector with the kernels of one vector (tables per vector), each donor still updated in its fixed order.
#include "internal.h"

#define JM_BX 64
#define JM_BY 4

// owned cells: PETSc-layout vector (block, k, j, i, variable fastest) -> component-major halo'd array
template <int NS>
__global__ __launch_bounds__(JM_BX* JM_BY) void k_jm_scatter(const JmBlk* __restrict__ tab, int nzb, const double* __restrict__ x)
{
    const JmBlk b = tab[blockIdx.z / nzb + 1];
    const int i = blockIdx.x * JM_BX + threadIdx.x + 2;
    const int j = blockIdx.y * JM_BY + threadIdx.y + 2;
    const int k = (int)(blockIdx.z % nzb) + 2;
    if (i > b.il || j > b.jl || k > b.kl) return;
    const long c = (long)i + (long)j * b.ldi + (long)k * b.ldk;
    const long m = b.vecOff + (((long)(k - 2) * b.ny + (j - 2)) * b.nx + (i - 2)) * NS;
    double v[NS];
#pragma unroll
    for (int l = 0; l < NS; ++l) v[l] = x[m + l];
#pragma unroll
    for (int l = 0; l < NS; ++l) b.xs[c + l * b.nbox] = v[l];
}

// owned cells: ys -> PETSc-layout vector
template <int NS>
__global__ __launch_bounds__(JM_BX* JM_BY) void k_jm_gather(const JmBlk* __restrict__ tab, int nzb, double* __restrict__ y)
{
    const JmBlk b = tab[blockIdx.z / nzb + 1];
    const int i = blockIdx.x * JM_BX + threadIdx.x + 2;
    const int j = blockIdx.y * JM_BY + threadIdx.y + 2;
    const int k = (int)(blockIdx.z % nzb) + 2;
    if (i > b.il || j > b.jl || k > b.kl) return;
    const long c = (long)i + (long)j * b.ldi + (long)k * b.ldk;
    const long m = b.vecOff + (((long)(k - 2) * b.ny + (j - 2)) * b.nx + (i - 2)) * NS;
    double v[NS];
#pragma unroll
    for (int l = 0; l < NS; ++l) v[l] = b.ys[c + l * b.nbox];
#pragma unroll
    for (int l = 0; l < NS; ++l) y[m + l] = v[l];
}

// y(row) = sum_s B_s(row) x(row - d_s): one lane per owned row cell, nState accumulators.  The columns of an owned row lie inside
// the halo'd box for every stencil of the assembly (offsets of at most two cells along an axis).
// The blocks of one stencil entry are addressed from a uniform base with 32-bit byte offsets (ldg): nState^2 planes of one block
// stay below 4 GiB (the launcher checks).
// NV vectors at once (adflow_gpu_jacobian_mult_multi): every block is loaded once and applied to the NV vectors, nState x NV
// accumulators per lane.  Vector v is the nState components of xs behind those of vector v - 1 and column v of y, ldy apart;
// NV = 1 is the product of one vector as it always was.
template <int NS, int NV = 1>
__global__ __launch_bounds__(JM_BX* JM_BY) void k_jac_mult(const JmBlk* __restrict__ tab, int nzb, JmStencil S, double* __restrict__ y,
                                                           long ldy)
{
    const JmBlk b = tab[blockIdx.z / nzb + 1];
    const int i = blockIdx.x * JM_BX + threadIdx.x + 2;
    const int j = blockIdx.y * JM_BY + threadIdx.y + 2;
    const int k = (int)(blockIdx.z % nzb) + 2;
    if (i > b.il || j > b.jl || k > b.kl) return;
    const int c = i + j * b.ldi + k * b.ldk;
    const unsigned nb8 = (unsigned)b.nbox * 8u;
    GPTR(const double) xs[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) xs[v] = (GPTR(const double))(b.xs + (long)v * NS * b.nbox);
    double acc[NV][NS];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int ll = 0; ll < NS; ++ll) acc[v][ll] = 0.0;
    for (int s = 0; s < S.n; ++s) {
        GPTR(const double) B = (GPTR(const double))(b.jac + (long)s * (NS * NS) * b.nbox);
        const unsigned cx = (unsigned)(c - (S.d[s][0] + S.d[s][1] * b.ldi + S.d[s][2] * b.ldk)) * 8u;
        double xv[NV][NS], bv[NS * NS];
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int l = 0; l < NS; ++l) xv[v][l] = ldg(xs[v], cx + l * nb8);
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) bv[e] = ldg(B, (unsigned)c * 8u + e * nb8);
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int l = 0; l < NS; ++l)
#pragma unroll
                for (int ll = 0; ll < NS; ++ll) acc[v][ll] += bv[l * NS + ll] * xv[v][l];
    }
    const long m = b.vecOff + (((long)(k - 2) * b.ny + (j - 2)) * b.nx + (i - 2)) * NS;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int ll = 0; ll < NS; ++ll) y[v * ldy + m + ll] = acc[v][ll];
}

// ys(col) = sum_s B_s(col + d_s)^T x(col + d_s) over the OWNED rows col + d_s, for every cell of the halo'd box (owned cells and
// both halo layers).  The rows of a wave share j and k: a stencil entry whose row plane lies outside the owned range is skipped by
// the whole wave, the i range by the lane.  NV vectors as in k_jac_mult; vector v of ys lies behind vector v - 1
template <int NS, int NV = 1>
__global__ __launch_bounds__(JM_BX* JM_BY) void k_jac_mult_t(const JmBlk* __restrict__ tab, int nzb, JmStencil S)
{
    const JmBlk b = tab[blockIdx.z / nzb + 1];
    const int i = blockIdx.x * JM_BX + threadIdx.x - 14;     // aligned rows (the box origin is shifted by ADF_PAD0)
    const int j = blockIdx.y * JM_BY + threadIdx.y;
    const int k = (int)(blockIdx.z % nzb);
    if (b.nx == 0 || i < 0 || i > b.ib || j > b.jb || k > b.kb) return;
    const int c = i + j * b.ldi + k * b.ldk;
    const unsigned nb8 = (unsigned)b.nbox * 8u;
    GPTR(const double) xs[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) xs[v] = (GPTR(const double))(b.xs + (long)v * NS * b.nbox);
    double acc[NV][NS];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int l = 0; l < NS; ++l) acc[v][l] = 0.0;
    for (int s = 0; s < S.n; ++s) {
        const int ri = i + S.d[s][0], rj = j + S.d[s][1], rk = k + S.d[s][2];
        if (rj < 2 || rj > b.jl || rk < 2 || rk > b.kl) continue;
        if (ri < 2 || ri > b.il) continue;
        GPTR(const double) B = (GPTR(const double))(b.jac + (long)s * (NS * NS) * b.nbox);
        const unsigned cr = (unsigned)(c + S.d[s][0] + S.d[s][1] * b.ldi + S.d[s][2] * b.ldk) * 8u;
        double xv[NV][NS], bv[NS * NS];
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int m = 0; m < NS; ++m) xv[v][m] = ldg(xs[v], cr + m * nb8);
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) bv[e] = ldg(B, cr + e * nb8);
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int l = 0; l < NS; ++l)
#pragma unroll
                for (int m = 0; m < NS; ++m) acc[v][l] += bv[l * NS + m] * xv[v][m];
    }
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int l = 0; l < NS; ++l) b.ys[c + (long)(v * NS + l) * b.nbox] = acc[v][l];
}

// the reverse exchange: target t (an owned cell, the donor of the forward exchange) += its sources in list order.  buf == NULL:
// the sources are halo cells of the blocks of this process; else entries of a received message (component-major, nbuf per component)
template <int NS>
__global__ void k_jac_halo_accumulate(const JmBlk* __restrict__ tab, const int* __restrict__ tBlk, const long* __restrict__ tOff,
                                      const int* __restrict__ seg, const int* __restrict__ sBlk, const long* __restrict__ sOff,
                                      const double* __restrict__ buf, int nbuf, int nu)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nu) return;
    const JmBlk& b = tab[tBlk[t]];
    double* ys = b.ys + tOff[t];
    const long nb = b.nbox;
    double a[NS];
#pragma unroll
    for (int l = 0; l < NS; ++l) a[l] = ys[l * nb];
    for (int e = seg[t]; e < seg[t + 1]; ++e) {
        if (buf) {
            const int q = sBlk[e];
#pragma unroll
            for (int l = 0; l < NS; ++l) a[l] += buf[(long)l * nbuf + q];
        } else {
            const JmBlk& h = tab[sBlk[e]];
            const double* hs = h.ys + sOff[e];
            const long hn = h.nbox;
#pragma unroll
            for (int l = 0; l < NS; ++l) a[l] += hs[l * hn];
        }
    }
#pragma unroll
    for (int l = 0; l < NS; ++l) ys[l * nb] = a[l];
}

static dim3 jm_own_grid(int nslots, int nx, int ny, int nz) { return dim3((nx + JM_BX - 1) / JM_BX, (ny + JM_BY - 1) / JM_BY, nz * nslots); }
static dim3 jm_box_grid(int nslots, int nx, int ny, int nz)
{
    return dim3((nx + 3 + 15 + JM_BX) / JM_BX, (ny + 4 + JM_BY - 1) / JM_BY, (nz + 4) * nslots);
}

#define JM_DISPATCH(KERNEL, GRID, ...)                                                                                          \
    switch (nState) {                                                                                                           \
    case 1: hipLaunchKernelGGL((KERNEL<1>), GRID, dim3(JM_BX, JM_BY, 1), 0, s, __VA_ARGS__); break;                             \
    case 5: hipLaunchKernelGGL((KERNEL<5>), GRID, dim3(JM_BX, JM_BY, 1), 0, s, __VA_ARGS__); break;                             \
    case 6: hipLaunchKernelGGL((KERNEL<6>), GRID, dim3(JM_BX, JM_BY, 1), 0, s, __VA_ARGS__); break;                             \
    default: (void)adf_fail("jacobian_mult: no kernel for this nState"); break;                                                 \
    }

void launch_jm_scatter(const JmBlk* tab, int nslots, int maxnx, int maxny, int maxnz, int nState, const double* x, hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz + 4, launch_jm_scatter(tab + s0_, n_, maxnx, maxny, maxnz, nState, x, s));
    if (nslots <= 0) return;
    JM_DISPATCH(k_jm_scatter, jm_own_grid(nslots, maxnx, maxny, maxnz), tab, maxnz, x)
}
void launch_jm_gather(const JmBlk* tab, int nslots, int maxnx, int maxny, int maxnz, int nState, double* y, hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz + 4, launch_jm_gather(tab + s0_, n_, maxnx, maxny, maxnz, nState, y, s));
    if (nslots <= 0) return;
    JM_DISPATCH(k_jm_gather, jm_own_grid(nslots, maxnx, maxny, maxnz), tab, maxnz, y)
}
// the two product kernels for nState and the nv = 1 .. JM_MAXW vectors of one pass over the matrix
#define JM_LAUNCH_NV(KERNEL, NS, GRID, ...)                                                                                     \
    ADF_DISPATCH_NV(nv, (void)adf_fail("jacobian_mult: no kernel for this number of vectors"),                                  \
                    hipLaunchKernelGGL((KERNEL<NS, NV_>), GRID, dim3(JM_BX, JM_BY, 1), 0, s, __VA_ARGS__))
#define JM_DISPATCH_NV(KERNEL, GRID, ...)                                                                                       \
    switch (nState) {                                                                                                           \
    case 1: JM_LAUNCH_NV(KERNEL, 1, GRID, __VA_ARGS__) break;                                                                   \
    case 5: JM_LAUNCH_NV(KERNEL, 5, GRID, __VA_ARGS__) break;                                                                   \
    case 6: JM_LAUNCH_NV(KERNEL, 6, GRID, __VA_ARGS__) break;                                                                   \
    default: (void)adf_fail("jacobian_mult: no kernel for this nState"); break;                                                 \
    }

void launch_jac_mult(const JmBlk* tab, int nslots, int maxnx, int maxny, int maxnz, int nState, const JmStencil& S, double* y, hipStream_t s,
                     int nv, long ldy)
{
    LEVEL_SPLIT(nslots, maxnz + 4, launch_jac_mult(tab + s0_, n_, maxnx, maxny, maxnz, nState, S, y, s, nv, ldy));
    if (nslots <= 0) return;
    JM_DISPATCH_NV(k_jac_mult, jm_own_grid(nslots, maxnx, maxny, maxnz), tab, maxnz, S, y, ldy)
}
void launch_jac_mult_t(const JmBlk* tab, int nslots, int maxnx, int maxny, int maxnz, int nState, const JmStencil& S, hipStream_t s, int nv)
{
    LEVEL_SPLIT(nslots, maxnz + 4, launch_jac_mult_t(tab + s0_, n_, maxnx, maxny, maxnz, nState, S, s, nv));
    if (nslots <= 0) return;
    JM_DISPATCH_NV(k_jac_mult_t, jm_box_grid(nslots, maxnx, maxny, maxnz), tab, maxnz + 4, S)
}

void launch_jac_halo_accumulate(const JmBlk* tab, const JmAccList& a, int nState, const double* buf, int nbuf, hipStream_t s)
{
    if (a.nu <= 0) return;
    const dim3 g((a.nu + 255) / 256), t(256);
    switch (nState) {
    case 1: hipLaunchKernelGGL((k_jac_halo_accumulate<1>), g, t, 0, s, tab, a.tBlk, a.tOff, a.seg, a.sBlk, a.sOff, buf, nbuf, a.nu); break;
    case 5: hipLaunchKernelGGL((k_jac_halo_accumulate<5>), g, t, 0, s, tab, a.tBlk, a.tOff, a.seg, a.sBlk, a.sOff, buf, nbuf, a.nu); break;
    case 6: hipLaunchKernelGGL((k_jac_halo_accumulate<6>), g, t, 0, s, tab, a.tBlk, a.tOff, a.seg, a.sBlk, a.sOff, buf, nbuf, a.nu); break;
    default: (void)adf_fail("jacobian_mult: no kernel for this nState"); break;
    }
}
