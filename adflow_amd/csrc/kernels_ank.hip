// The flow update of the approximate Newton-Krylov step on the device (adflow_gpu_ank_*, api.hip): vector glue for
// nState /= nw, the pseudo-time term T, the matrix-free operator and the step limiter.
//
// Reference semantics (src/NKSolver/NKSolvers.F90):
//   setWANK(wVec, 1, nState)   :2975-3011   w(i,j,k,1:nState) of the owned cells, no clipping of the turbulence variable
//   setRVecANK / setRVec       :2895-2933, :1262-1329   dw / volRef (coupled: turbulence entry * turbResScale)
//   computeTimeStepBlock       :2116-2329   ANK_charTimeStepType = 'None':  T = S / (ANK_CFL dtl volRef), S = dU/du the
//                                           state-to-conservative block (coupled: S(nt1,nt1) = turbResScale / ANK_turbCFLScale)
//   FormFunction_mf            :2468-2538   R(u) + T u, differenced by MatMFFD (default MATMFFD_DS step); here the linear part T v is
//                                           taken analytically:  y = (R(w + h v) - r0) / h + T v
//   physicalityCheckANK        :3013-3210   the largest step that changes density / energy by at most physLSTol (real mode)
//   the turbulence KSP (ANKTurbSolveKSP :3337-3627), nState = 1, the entry of a cell is nuTilde:
//   setWANK(wVecTurb, nt1, nt2) :2975-3011, setRVecANKTurb :2935-2973 (dw(itu1) / volRef turbResScale), FormJacobianANKTurb
//   :2395-2406 (the diagonal dtInv turbResScale / turbCFLScale), FormFunction_mf_turb :2540-2612, physicalityCheckANKTurb :3212-3335
//   computeUnsteadyResANK / ...Turb :2614-2786   the residual of the backtracking line search, R(w) - omega T deltaW, and its 2-norm
// Out of scope: the Turkel / VLR time-step types.
//
// Every pass is bandwidth-bound, one lane per owned cell.  Vectors are the PETSc layout (block, k, j, i, variable fastest) with
// nS = nState variables per cell: cell m of the level starts at m nS; the first cell of a block is BlkView::vecOff / nw.
// T is not stored as dense blocks: tsm[q N + m], q = 0 dtInv, 1 rho, 2..4 u, v, w of the state T was formed from (N = owned cells of
// the level) -- 40 B per cell instead of the 200 B of a dense 5 x 5 block; T v and the diagonal shift are formed on the fly.
#include "internal.h"
#include "nk_closures.h"

#define AK_BX 64
#define AK_BY 4
#define AK_T 256          // threads of a reduction workgroup = the largest number of partial results
static_assert(AK_T == ANK_PARTS, "the reduction buffer of api.hip is laid out for AK_T partial results");

struct AkCell { int i, j, k; long c, m; bool in; };

// the cell of this lane: box index c, PETSc cell number m
__device__ __forceinline__ AkCell ak_cell(const BlkView& b, int kz)
{
    AkCell q;
    q.i = blockIdx.x * AK_BX + threadIdx.x + 2;
    q.j = blockIdx.y * AK_BY + threadIdx.y + 2;
    q.k = kz + 2;
    q.in = q.i <= b.il && q.j <= b.jl && q.k <= b.kl;
    q.c = q.m = 0;
    if (q.in) {
        q.c = b.idx(q.i, q.j, q.k);
        q.m = b.vecOff / b.nw + ((long)(q.k - 2) * b.ny + (q.j - 2)) * b.nx + (q.i - 2);
    }
    return q;
}

// w(1:nS) = vec (hv == NULL) or vec + h hv with h = hdev[ANK_H]; CLOS: the closures of blocketteRes in the same pass, each lane reads
// back what it wrote itself (k_set_w_closures_level)
template <bool CLOS>
__global__ __launch_bounds__(AK_BX* AK_BY) void k_ank_set_w(const BlkView* __restrict__ tab, int nzb, int nS, const double* __restrict__ vec,
                                                            const double* __restrict__ hv, const double* __restrict__ hdev, KParams kp,
                                                            int* __restrict__ floored)
{
    const BlkView& b = tab[blockIdx.z / nzb + 1];
    const AkCell q = ak_cell(b, (int)(blockIdx.z % nzb));
    if (!q.in) return;
    const long m = q.m * nS;
    const double h = hv ? hdev[ANK_H] : 0.0;
    for (int l = 0; l < nS; ++l) b.w[q.c + l * b.nbox] = hv ? vec[m + l] + h * hv[m + l] : vec[m + l];
    if (CLOS) closures_cell<true>(b, q.i, q.j, q.k, kp, floored);
}

// vec(1:nS) = dw / volRef, the entry of the turbulence variable times turbScale
__global__ __launch_bounds__(AK_BX* AK_BY) void k_ank_get_r(const BlkView* __restrict__ tab, int nzb, int nS, double* __restrict__ vec,
                                                            double turbScale)
{
    const BlkView& b = tab[blockIdx.z / nzb + 1];
    const AkCell q = ak_cell(b, (int)(blockIdx.z % nzb));
    if (!q.in) return;
    const long m = q.m * nS;
    const double ovv = 1.0 / b.volRef[q.c];
    for (int l = 0; l < nS; ++l) {
        const double t = b.dw[q.c + l * b.nbox] * ovv;
        vec[m + l] = l < 5 ? t : t * turbScale;
    }
}

// dtInv = 1 / (cfl dtl volRef) and the state T is formed from
__global__ __launch_bounds__(AK_BX* AK_BY) void k_ank_time_step(const BlkView* __restrict__ tab, int nzb, double cfl, double* __restrict__ tsm, long N)
{
    const BlkView& b = tab[blockIdx.z / nzb + 1];
    const AkCell q = ak_cell(b, (int)(blockIdx.z % nzb));
    if (!q.in) return;
    tsm[q.m] = rcp_nr(cfl * b.dtl[q.c] * b.volRef[q.c]);
    for (int l = 0; l < 4; ++l) tsm[(l + 1) * N + q.m] = b.w[q.c + l * b.nbox];
}

// y = (dw / volRef - r0) / h + T v;  h == 0 (v = 0): y = 0
__global__ __launch_bounds__(AK_BX* AK_BY) void k_ank_quotient(const BlkView* __restrict__ tab, int nzb, int nS, const double* __restrict__ v,
                                                               const double* __restrict__ r0, const double* __restrict__ tsm, long N,
                                                               double turbDiag, double turbScale, const double* __restrict__ hdev,
                                                               double* __restrict__ y)
{
    const BlkView& b = tab[blockIdx.z / nzb + 1];
    const AkCell q = ak_cell(b, (int)(blockIdx.z % nzb));
    if (!q.in) return;
    const long m = q.m * nS;
    const double hinv = hdev[ANK_HINV];
    if (hdev[ANK_H] == 0.0) {
        for (int l = 0; l < nS; ++l) y[m + l] = 0.0;
        return;
    }
    const double ovv = 1.0 / b.volRef[q.c];
    const double dtInv = tsm[q.m], rho = tsm[N + q.m];
    const double v0 = v[m];
    for (int l = 0; l < nS; ++l) {
        double r = b.dw[q.c + l * b.nbox] * ovv;
        if (l >= 5) r *= turbScale;
        const double vl = v[m + l];
        double tv;
        if (l == 0 || l == 4) tv = dtInv * vl;
        else if (l < 4) tv = dtInv * (tsm[(l + 1) * N + q.m] * v0 + rho * vl);
        else tv = dtInv * turbDiag * vl;
        y[m + l] = (r - r0[m + l]) * hinv + tv;
    }
}

// ---- the turbulence KSP: one entry per cell (nuTilde) --------------------------------------------------------------------------------
// w(itu1) = vec (hv == NULL) or vec + h hv.  The flow variables do not move, so p and rlv stand; EDDY: the eddy viscosity of the cell
// is re-formed from rho, rlv and the new nuTilde by the function closures_cell uses -- about 5 values per cell instead of the state
template <bool EDDY>
__global__ __launch_bounds__(AK_BX* AK_BY) void k_ank_set_w_turb(const BlkView* __restrict__ tab, int nzb, const double* __restrict__ vec,
                                                                 const double* __restrict__ hv, const double* __restrict__ hdev, KParams kp)
{
    const BlkView& b = tab[blockIdx.z / nzb + 1];
    const AkCell q = ak_cell(b, (int)(blockIdx.z % nzb));
    if (!q.in) return;
    const double h = hv ? hdev[ANK_H] : 0.0;
    const double nut = hv ? vec[q.m] + h * hv[q.m] : vec[q.m];
    b.w[q.c + 5 * b.nbox] = nut;
    if (EDDY && kp.eddyModel && kp.updateEddy) b.rev[q.c] = sa_eddy_viscosity(kp, b.w[q.c], b.rlv[q.c], nut);
}

// vec = dw(itu1) / volRef turbScale (setRVecANKTurb)
__global__ __launch_bounds__(AK_BX* AK_BY) void k_ank_get_r_turb(const BlkView* __restrict__ tab, int nzb, double* __restrict__ vec, double turbScale)
{
    const BlkView& b = tab[blockIdx.z / nzb + 1];
    const AkCell q = ak_cell(b, (int)(blockIdx.z % nzb));
    if (!q.in) return;
    const double ovv = 1.0 / b.volRef[q.c];
    vec[q.m] = b.dw[q.c + 5 * b.nbox] * ovv * turbScale;
}

// the turbulence T: dtInv = 1 / (cfl dtl volRef) and nothing else, 8 B per cell
__global__ __launch_bounds__(AK_BX* AK_BY) void k_ank_time_step_turb(const BlkView* __restrict__ tab, int nzb, double cfl, double* __restrict__ tsm)
{
    const BlkView& b = tab[blockIdx.z / nzb + 1];
    const AkCell q = ak_cell(b, (int)(blockIdx.z % nzb));
    if (!q.in) return;
    tsm[q.m] = rcp_nr(cfl * b.dtl[q.c] * b.volRef[q.c]);
}

// y = (dw(itu1) / volRef turbScale - r0) / h + dtInv turbDiag v;  h == 0 (v = 0): y = 0
__global__ __launch_bounds__(AK_BX* AK_BY) void k_ank_quotient_turb(const BlkView* __restrict__ tab, int nzb, const double* __restrict__ v,
                                                                    const double* __restrict__ r0, const double* __restrict__ tsm,
                                                                    double turbDiag, double turbScale, const double* __restrict__ hdev,
                                                                    double* __restrict__ y)
{
    const BlkView& b = tab[blockIdx.z / nzb + 1];
    const AkCell q = ak_cell(b, (int)(blockIdx.z % nzb));
    if (!q.in) return;
    if (hdev[ANK_H] == 0.0) {
        y[q.m] = 0.0;
        return;
    }
    const double ovv = 1.0 / b.volRef[q.c];
    const double r = b.dw[q.c + 5 * b.nbox] * ovv * turbScale;
    y[q.m] = (r - r0[q.m]) * hdev[ANK_HINV] + tsm[q.m] * turbDiag * v[q.m];
}

// ---- reductions: partial results per workgroup, then one finishing workgroup that adds them in a fixed order ------------------------
template <int NV>
__device__ __forceinline__ void ak_block_sum(double (&v)[NV], double (*red)[AK_T])
{
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;          // AK_T x 1 and AK_BX x AK_BY workgroups alike
    for (int q = 0; q < NV; ++q) red[q][tid] = v[q];
    __syncthreads();
    for (int s = AK_T / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int q = 0; q < NV; ++q) red[q][tid] += red[q][tid + s];
        __syncthreads();
    }
    for (int q = 0; q < NV; ++q) v[q] = red[q][0];
    __syncthreads();
}

// partial sums of  w.v, |v|_1, |v|_2^2  to part[q AK_T + workgroup]
__global__ __launch_bounds__(AK_T) void k_ank_sums(const double* __restrict__ w, const double* __restrict__ v, long n, double* __restrict__ part)
{
    __shared__ double red[3][AK_T];
    double s[3] = {0.0, 0.0, 0.0};
    for (long i = (long)blockIdx.x * AK_T + threadIdx.x; i < n; i += (long)gridDim.x * AK_T) {
        const double vi = v[i];
        s[0] += w[i] * vi;
        s[1] += fabs(vi);
        s[2] += vi * vi;
    }
    ak_block_sum<3>(s, red);
    if (threadIdx.x == 0)
        for (int q = 0; q < 3; ++q) part[q * AK_T + blockIdx.x] = s[q];
}

// the step of MATMFFD_DS from the three sums: hdev[ANK_H] = h, hdev[ANK_HINV] = 1 / h (both 0 when v = 0), hdev[ANK_SUMS ..] = the sums
__global__ __launch_bounds__(AK_T) void k_ank_step(const double* __restrict__ part, int np, double errRel, double umin, double* __restrict__ hdev)
{
    __shared__ double red[3][AK_T];
    double s[3];
    for (int q = 0; q < 3; ++q) s[q] = (int)threadIdx.x < np ? part[q * AK_T + threadIdx.x] : 0.0;
    ak_block_sum<3>(s, red);
    if (threadIdx.x != 0) return;
    double dot = s[0];
    const double d = s[1], nrm2 = s[2];
    if (fabs(dot) < umin * d) dot = dot < 0.0 ? -umin * d : umin * d;
    const double h = nrm2 == 0.0 ? 0.0 : errRel * dot / nrm2;
    hdev[ANK_H] = h;
    hdev[ANK_HINV] = h == 0.0 ? 0.0 : 1.0 / h;
    hdev[ANK_SUMS] = s[0]; hdev[ANK_SUMS + 1] = d; hdev[ANK_SUMS + 2] = nrm2;
}

// the residual of the backtracking line search (computeUnsteadyResANK / ...Turb): r = setRVecANK / setRVec / setRVecANKTurb of the dw
// on the device minus omega T dW with T as stored, and the sum of r^2 over the workgroup to part[workgroup of the launch + partOff]:
// one pass over dw, volRef, tsm and dW.  Every workgroup writes its partial, one without cells a zero.
template <bool TURB>
__global__ __launch_bounds__(AK_BX* AK_BY) void k_ank_unsteady(const BlkView* __restrict__ tab, int nzb, int nS, const double* __restrict__ dW,
                                                               const double* __restrict__ tsm, long N, double turbDiag, double turbScale,
                                                               double omega, double* __restrict__ r, double* __restrict__ part, long partOff)
{
    __shared__ double red[1][AK_T];
    const BlkView& b = tab[blockIdx.z / nzb + 1];
    const AkCell q = ak_cell(b, (int)(blockIdx.z % nzb));
    double s[1] = {0.0};
    if (q.in) {
        const double ovv = 1.0 / b.volRef[q.c];
        const double dtInv = tsm[q.m];
        if (TURB) {
            const double steady = b.dw[q.c + 5 * b.nbox] * ovv * turbScale;
            const double val = steady - omega * (dtInv * turbDiag * dW[q.m]);
            r[q.m] = val;
            s[0] = val * val;
        } else {
            const long m = q.m * nS;
            const double rho = tsm[N + q.m], d0 = dW[m];
            for (int l = 0; l < nS; ++l) {
                const double t = b.dw[q.c + l * b.nbox] * ovv;
                const double steady = l < 5 ? t : t * turbScale;
                const double dl = dW[m + l];
                double tv;
                if (l == 0 || l == 4) tv = dtInv * dl;
                else if (l < 4) tv = dtInv * (tsm[(l + 1) * N + q.m] * d0 + rho * dl);
                else tv = dtInv * turbDiag * dl;
                const double val = steady - omega * tv;
                r[m + l] = val;
                s[0] += val * val;
            }
        }
    }
    ak_block_sum<1>(s, red);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        part[partOff + ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s[0];
}

// out[0] = sqrt(sum of np partials): lane t adds part[t], part[t + AK_T], ... in that order, then the tree of ak_block_sum
__global__ __launch_bounds__(AK_T) void k_ank_norm_finish(const double* __restrict__ part, long np, double* __restrict__ out)
{
    __shared__ double red[1][AK_T];
    double s[1] = {0.0};
    for (long i = threadIdx.x; i < np; i += AK_T) s[0] += part[i];
    ak_block_sum<1>(s, red);
    if (threadIdx.x == 0) out[0] = sqrt(s[0]);
}

// physicalityCheckANK / physicalityCheckANKTurb: the smallest ratio of the cells of a workgroup to part[workgroup]; a NaN ratio makes
// the partial NaN.  flow: density and energy (entries 0 and 4) take part; lt: the entry of the turbulence variable (5 coupled, 0 in
// the turbulence KSP), < 0 none
__global__ __launch_bounds__(AK_T) void k_ank_phys(const double* __restrict__ w, double* __restrict__ dw, long ncell, int nS, int flow, int lt,
                                                   double eps, double tol, double tolTurb, double turbThreshold, double* __restrict__ part)
{
    __shared__ double red[2][AK_T];
    double lam = 1.7976931348623157e308, bad = 0.0;
    for (long c = (long)blockIdx.x * AK_T + threadIdx.x; c < ncell; c += (long)gridDim.x * AK_T) {
        const long m = c * nS;
        for (int l = 0; flow && l < 5; l += 4) {
            const double ratio = fabs(w[m + l] / (dw[m + l] + eps)) * tol;
            if (ratio != ratio) bad = 1.0;
            lam = fmin(lam, ratio);
        }
        if (lt >= 0) {
            double ratio = (w[m + lt] / (dw[m + lt] + eps)) * tolTurb;
            if (ratio < turbThreshold) {
                if (ratio > 0.0) dw[m + lt] = w[m + lt] * tolTurb;
                ratio = 1.0;
            }
            if (ratio != ratio) bad = 1.0;
            lam = fmin(lam, ratio);
        }
    }
    const int tid = threadIdx.x;
    red[0][tid] = lam;
    red[1][tid] = bad;
    __syncthreads();
    for (int s = AK_T / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] = fmin(red[0][tid], red[0][tid + s]);
            red[1][tid] = fmax(red[1][tid], red[1][tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0) part[blockIdx.x] = red[1][0] != 0.0 ? __builtin_nan("") : red[0][0];
}

// lambda = min(start value, partials); NaN anywhere: 0
__global__ __launch_bounds__(AK_T) void k_ank_phys_finish(const double* __restrict__ part, int np, double lambda0, double* __restrict__ out)
{
    __shared__ double red[2][AK_T];
    const int tid = threadIdx.x;
    const double v = tid < np ? part[tid] : lambda0;
    red[0][tid] = v != v ? 0.0 : v;
    red[1][tid] = v != v ? 1.0 : 0.0;
    __syncthreads();
    for (int s = AK_T / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] = fmin(red[0][tid], red[0][tid + s]);
            red[1][tid] = fmax(red[1][tid], red[1][tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double lam = fmin(red[0][0], lambda0);
        out[0] = (red[1][0] != 0.0 || lambda0 != lambda0) ? 0.0 : lam;
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
static dim3 ak_grid(int nslots, int maxnx, int maxny, int maxnz)
{
    return dim3((maxnx + AK_BX - 1) / AK_BX, (maxny + AK_BY - 1) / AK_BY, maxnz * nslots);
}
int ank_groups(long n)
{
    const long g = (n + 4L * AK_T - 1) / (4L * AK_T);
    return (int)(g < 1 ? 1 : g > AK_T ? AK_T : g);
}

void launch_ank_set_w(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, int nS, const double* vec, const double* hv,
                      const double* hdev, const KParams* kp, int* floored, hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz + 4, launch_ank_set_w(tab + s0_, n_, maxnx, maxny, maxnz, nS, vec, hv, hdev, kp, floored, s));
    if (nslots <= 0) return;
    if (kp)
        hipLaunchKernelGGL(k_ank_set_w<true>, ak_grid(nslots, maxnx, maxny, maxnz), dim3(AK_BX, AK_BY, 1), 0, s, tab, maxnz, nS, vec, hv, hdev,
                           *kp, floored);
    else
        hipLaunchKernelGGL(k_ank_set_w<false>, ak_grid(nslots, maxnx, maxny, maxnz), dim3(AK_BX, AK_BY, 1), 0, s, tab, maxnz, nS, vec, hv, hdev,
                           KParams(), (int*)nullptr);
}
void launch_ank_get_r(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, int nS, double* vec, double turbScale, hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz + 4, launch_ank_get_r(tab + s0_, n_, maxnx, maxny, maxnz, nS, vec, turbScale, s));
    if (nslots <= 0) return;
    hipLaunchKernelGGL(k_ank_get_r, ak_grid(nslots, maxnx, maxny, maxnz), dim3(AK_BX, AK_BY, 1), 0, s, tab, maxnz, nS, vec, turbScale);
}
void launch_ank_time_step(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, double cfl, double* tsm, long N, hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz + 4, launch_ank_time_step(tab + s0_, n_, maxnx, maxny, maxnz, cfl, tsm, N, s));
    if (nslots <= 0) return;
    hipLaunchKernelGGL(k_ank_time_step, ak_grid(nslots, maxnx, maxny, maxnz), dim3(AK_BX, AK_BY, 1), 0, s, tab, maxnz, cfl, tsm, N);
}
void launch_ank_quotient(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, int nS, const double* v, const double* r0,
                         const double* tsm, long N, double turbDiag, double turbScale, const double* hdev, double* y, hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz + 4, launch_ank_quotient(tab + s0_, n_, maxnx, maxny, maxnz, nS, v, r0, tsm, N, turbDiag, turbScale, hdev, y, s));
    if (nslots <= 0) return;
    hipLaunchKernelGGL(k_ank_quotient, ak_grid(nslots, maxnx, maxny, maxnz), dim3(AK_BX, AK_BY, 1), 0, s, tab, maxnz, nS, v, r0, tsm, N, turbDiag,
                       turbScale, hdev, y);
}
// part: 3 AK_T doubles; hdev: 5 doubles
void launch_ank_step(const double* w, const double* v, long n, double errRel, double umin, double* part, double* hdev, hipStream_t s)
{
    const int g = ank_groups(n);
    hipLaunchKernelGGL(k_ank_sums, dim3(g), dim3(AK_T), 0, s, w, v, n, part);
    hipLaunchKernelGGL(k_ank_step, dim3(1), dim3(AK_T), 0, s, part, g, errRel, umin, hdev);
}
// part: AK_T doubles
void launch_ank_phys(const double* w, double* dw, long ncell, int nS, int flow, int lt, double eps, double tol, double tolTurb,
                     double turbThreshold, double lambda0, double* part, double* out, hipStream_t s)
{
    const int g = ank_groups(ncell);
    hipLaunchKernelGGL(k_ank_phys, dim3(g), dim3(AK_T), 0, s, w, dw, ncell, nS, flow, lt, eps, tol, tolTurb, turbThreshold, part);
    hipLaunchKernelGGL(k_ank_phys_finish, dim3(1), dim3(AK_T), 0, s, part, g, lambda0, out);
}

// ---- the turbulence KSP and the line-search residual -------------------------------------------------------------------------------------
void launch_ank_set_w_turb(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, const double* vec, const double* hv,
                           const double* hdev, const KParams* kp, hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz + 4, launch_ank_set_w_turb(tab + s0_, n_, maxnx, maxny, maxnz, vec, hv, hdev, kp, s));
    if (nslots <= 0) return;
    if (kp)
        hipLaunchKernelGGL(k_ank_set_w_turb<true>, ak_grid(nslots, maxnx, maxny, maxnz), dim3(AK_BX, AK_BY, 1), 0, s, tab, maxnz, vec, hv, hdev, *kp);
    else
        hipLaunchKernelGGL(k_ank_set_w_turb<false>, ak_grid(nslots, maxnx, maxny, maxnz), dim3(AK_BX, AK_BY, 1), 0, s, tab, maxnz, vec, hv, hdev,
                           KParams());
}
void launch_ank_get_r_turb(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, double* vec, double turbScale, hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz + 4, launch_ank_get_r_turb(tab + s0_, n_, maxnx, maxny, maxnz, vec, turbScale, s));
    if (nslots <= 0) return;
    hipLaunchKernelGGL(k_ank_get_r_turb, ak_grid(nslots, maxnx, maxny, maxnz), dim3(AK_BX, AK_BY, 1), 0, s, tab, maxnz, vec, turbScale);
}
void launch_ank_time_step_turb(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, double cfl, double* tsm, hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz + 4, launch_ank_time_step_turb(tab + s0_, n_, maxnx, maxny, maxnz, cfl, tsm, s));
    if (nslots <= 0) return;
    hipLaunchKernelGGL(k_ank_time_step_turb, ak_grid(nslots, maxnx, maxny, maxnz), dim3(AK_BX, AK_BY, 1), 0, s, tab, maxnz, cfl, tsm);
}
void launch_ank_quotient_turb(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, const double* v, const double* r0,
                              const double* tsm, double turbDiag, double turbScale, const double* hdev, double* y, hipStream_t s)
{
    LEVEL_SPLIT(nslots, maxnz + 4, launch_ank_quotient_turb(tab + s0_, n_, maxnx, maxny, maxnz, v, r0, tsm, turbDiag, turbScale, hdev, y, s));
    if (nslots <= 0) return;
    hipLaunchKernelGGL(k_ank_quotient_turb, ak_grid(nslots, maxnx, maxny, maxnz), dim3(AK_BX, AK_BY, 1), 0, s, tab, maxnz, v, r0, tsm, turbDiag,
                       turbScale, hdev, y);
}
// the workgroups (= partial sums) of launch_ank_unsteady over these slots
long ank_unsteady_groups(int nslots, int maxnx, int maxny, int maxnz)
{
    const dim3 g = ak_grid(1, maxnx, maxny, maxnz);
    return (long)g.x * g.y * g.z * (nslots > 0 ? nslots : 0);
}
// part: ank_unsteady_groups doubles; out (NULL: no norm): 1 double
void launch_ank_unsteady(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, int nS, int turb, const double* dW, const double* tsm,
                         long N, double turbDiag, double turbScale, double omega, double* r, double* part, double* out, hipStream_t s)
{
    const int per = level_slots_per_launch(maxnz + 4);
    long off = 0;
    for (int s0 = 0; s0 < nslots; s0 += per) {
        const int n = nslots - s0 < per ? nslots - s0 : per;
        if (turb)
            hipLaunchKernelGGL(k_ank_unsteady<true>, ak_grid(n, maxnx, maxny, maxnz), dim3(AK_BX, AK_BY, 1), 0, s, tab + s0, maxnz, nS, dW, tsm, N,
                               turbDiag, turbScale, omega, r, part, off);
        else
            hipLaunchKernelGGL(k_ank_unsteady<false>, ak_grid(n, maxnx, maxny, maxnz), dim3(AK_BX, AK_BY, 1), 0, s, tab + s0, maxnz, nS, dW, tsm, N,
                               turbDiag, turbScale, omega, r, part, off);
        off += ank_unsteady_groups(n, maxnx, maxny, maxnz);
    }
    if (out) hipLaunchKernelGGL(k_ank_norm_finish, dim3(1), dim3(AK_T), 0, s, part, off, out);
}
