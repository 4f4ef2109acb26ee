// Internal device data model of the MI355X residual engine (not part of the ABI).
//
// HBM layout: every per-cell, per-face and per-node array of a
// block lives in ONE uniform index box (0:ib,0:jb,0:kb), i fastest, SoA with the
// variable index slowest.  One linear offset  idx = i + j*ldi + k*ldk  addresses
// every array, and the six neighbours are idx±1, ±ldi, ±ldk.  Rows are padded to
// ldi (multiple of 16 doubles) and the box origin is shifted by PAD0 doubles so
// that the first OWNED cell of every row (i=2) starts a 128-byte line: a
// wavefront whose lane l handles cell i=2+l issues fully aligned 512-byte loads.
//   face arrays : sI(i,j,k,:) (face between cells i and i+1) stored at cell idx
//   node arrays : x(i,j,k,:), nodal gradients stored at cell idx (node = upper
//                 corner of cell (i,j,k), as in the reference, block.F90:363)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/adflow_gpu.h"

#define ADF_PAD0 14   // (PAD0 + 2) % 16 == 0

// pointer into HBM with an explicit global address space: pointers that reach a
// kernel through a table in memory are "generic" to the compiler and would be
// accessed with the slower flat_load/flat_store forms.
#ifdef HOSTSIM
#define GPTR(T) T*
#else
#define GPTR(T) T __attribute__((address_space(1)))*
#endif

// element access through a uniform base pointer and a 32-bit BYTE offset: the
// form `global_load v, v_off, s[base]` (scalar base + 32-bit vector offset) that
// needs no 64-bit address arithmetic per access.  Valid while one component of
// one block stays below 4 GiB (512 M doubles).
__device__ __forceinline__ double ldg(GPTR(const double) base, unsigned byteoff)
{
    return *(GPTR(const double))((GPTR(const char))base + byteoff);
}
__device__ __forceinline__ void stg(GPTR(double) base, unsigned byteoff, double v)
{
    *(GPTR(double))((GPTR(char))base + byteoff) = v;
}

// 1 / b and 1 / sqrt(x) for operands in the normal range: the hardware seed (v_rcp_f64 / v_rsq_f64, quarter rate) refined
// by ADF_NR Newton steps in FMA form, without the range handling, final residual correction and denormal scaling of the
// compiler's division / sqrt.  Callers multiply by the result; the flux kernels that use them are bound by FP64 issue.
// Measured on MI355X (tools/pmc_calib.bin probe, profiles/r02_a_probe.txt): raw seeds 4.6e-8 / 5.2e-8 relative, one step
// 2.1e-15 / 4.1e-15, two steps 1.1e-16 / 2.2e-16 -> ONE step is enough for the 1e-10 parity bar.
#ifndef ADF_NR
#define ADF_NR 1
#endif
#ifdef HOSTSIM
__device__ __forceinline__ double rcp_nr(double b) { return 1.0 / b; }
__device__ __forceinline__ double rsq_nr(double x) { return 1.0 / sqrt(x); }
#else
__device__ __forceinline__ double rcp_nr(double b)
{
    double x = __builtin_amdgcn_rcp(b);
#pragma unroll
    for (int it = 0; it < ADF_NR; ++it) {
        const double e = __builtin_fma(-b, x, 1.0);
        x = __builtin_fma(x, e, x);
    }
    return x;
}
__device__ __forceinline__ double rsq_nr(double x)
{
    double y = __builtin_amdgcn_rsq(x);
#pragma unroll
    for (int it = 0; it < ADF_NR; ++it) {
        const double t = x * y;
        const double e = __builtin_fma(-t, y, 1.0);      // 1 - x y^2
        y = __builtin_fma(0.5 * y, e, y);
    }
    return y;
}
#endif

// a / b for denominators in the normal range (clamped differences, densities, volumes, sound speeds): a * rcp_nr(b),
// 5 FP64 issue slots instead of the ~17 of the compiler's division (v_div_scale / v_div_fmas / v_div_fixup range handling)
__device__ __forceinline__ double fastdiv(double a, double b) { return a * rcp_nr(b); }

// sqrt(x) for x >= 0 in the normal range or exactly 0
#ifdef HOSTSIM
__device__ __forceinline__ double fastsqrt(double x) { return sqrt(x); }
__device__ __forceinline__ double fast_root6(double x) { return pow(x, 1.0 / 6.0); }
__device__ __forceinline__ double fast_exp_neg(double x) { return exp(x); }
__device__ __forceinline__ double fast_powa(double x, double a) { return pow(x, a); }
#else
__device__ __forceinline__ double fastsqrt(double x) { return x * rsq_nr(fmax(x, 1.e-300)); }
// x^(1/6) for x in the normal positive range: single-precision seed of z = x^(-1/6) (v_log_f32 / v_exp_f32), two Newton steps
// z <- z (7 - x z^6) / 6 in FP64 (quadratic: 1e-7 -> 4e-14 -> 1e-26), result x z^5.  ~25 issue slots instead of ~150 of pow().
// The argument is first scaled into [2^-6, 2^6) by a power of 2^6 taken from its exponent (x = x' 2^(6k), x^(1/6) = x'^(1/6) 2^k), so that
// the single-precision seed never under- / overflows: x reaches 1e-100 when the SA variable is negative and rr is far below zero (the
// reference bounds rr only from above, sa.F90).  x = 0 (gg^6 overflowed) gives 0 as the reference's power does.
__device__ __forceinline__ double fast_root6(double x)
{
    const int e = __builtin_amdgcn_frexp_exp(x);
    const int k = (e >= 0 ? e : e - 5) / 6;                 // floor(e / 6)
    const double xs = __builtin_ldexp(x, -6 * k);
    double z = (double)__builtin_amdgcn_exp2f(-(1.0f / 6.0f) * __builtin_amdgcn_logf((float)xs));
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double z2 = z * z, z6 = z2 * z2 * z2;
        z = z * __builtin_fma(-xs, z6, 7.0) * (1.0 / 6.0);
    }
    const double z2 = z * z;
    const double r = __builtin_ldexp(xs * (z2 * z2 * z), k);
    return (x == 0.0) ? 0.0 : r;
}
// x^a for x in the normal positive range and moderate a (the directional scaling of the spectral radii, adis = 0.67 by default):
// x = m 2^e with m in [0.707, 1.414); ln m = 2 atanh(s), s = (m - 1) / (m + 1), |s| <= 0.172, odd series to s^19 (truncation
// 1e-16); 2^(a log2 x) = 2^k exp(f ln 2) with the degree-13 Taylor polynomial on |f ln 2| <= 0.347 (4e-18).  ~50 issue slots
// instead of the ~200 of log() + exp().
__device__ __forceinline__ double fast_powa(double x, double a)
{
    int e = __builtin_amdgcn_frexp_exp(x);
    double m = __builtin_amdgcn_frexp_mant(x);          // [0.5, 1)
    if (m < 0.70710678118654752) { m *= 2.0; e -= 1; }
    const double s = (m - 1.0) * rcp_nr(m + 1.0);
    const double s2 = s * s;
    double p = 1.0 / 19.0;
    p = __builtin_fma(p, s2, 1.0 / 17.0);
    p = __builtin_fma(p, s2, 1.0 / 15.0);
    p = __builtin_fma(p, s2, 1.0 / 13.0);
    p = __builtin_fma(p, s2, 1.0 / 11.0);
    p = __builtin_fma(p, s2, 1.0 / 9.0);
    p = __builtin_fma(p, s2, 1.0 / 7.0);
    p = __builtin_fma(p, s2, 1.0 / 5.0);
    p = __builtin_fma(p, s2, 1.0 / 3.0);
    p = __builtin_fma(p, s2, 1.0);
    const double log2x = __builtin_fma(2.0 * s * p, 1.4426950408889634, (double)e);
    const double t = a * log2x;
    const double k = __builtin_rint(t);
    const double r = (t - k) * 6.93147180559945309417e-01;
    double q = 1.0 / 6227020800.0;
    q = __builtin_fma(q, r, 1.0 / 479001600.0);
    q = __builtin_fma(q, r, 1.0 / 39916800.0);
    q = __builtin_fma(q, r, 1.0 / 3628800.0);
    q = __builtin_fma(q, r, 1.0 / 362880.0);
    q = __builtin_fma(q, r, 1.0 / 40320.0);
    q = __builtin_fma(q, r, 1.0 / 5040.0);
    q = __builtin_fma(q, r, 1.0 / 720.0);
    q = __builtin_fma(q, r, 1.0 / 120.0);
    q = __builtin_fma(q, r, 1.0 / 24.0);
    q = __builtin_fma(q, r, 1.0 / 6.0);
    q = __builtin_fma(q, r, 0.5);
    q = __builtin_fma(q, r, 1.0);
    q = __builtin_fma(q, r, 1.0);
    return __builtin_ldexp(q, (int)k);
}
// exp(x) for x <= 0 (the ft2 term of Spalart-Allmaras): 0 below -700, else 2^k * P(r) with k = round(x log2 e), r = x - k ln 2
// in two pieces, Taylor polynomial of degree 13 on |r| <= ln2 / 2 (truncation 1e-17), ldexp.  ~25 slots instead of ~60.
__device__ __forceinline__ double fast_exp_neg(double x)
{
    if (x < -700.0) return 0.0;
    const double k = __builtin_rint(x * 1.4426950408889634);
    double r = __builtin_fma(-k, 6.93147180369123816490e-01, x);
    r = __builtin_fma(-k, 1.90821492927058770002e-10, r);
    double p = 1.0 / 6227020800.0;
    p = __builtin_fma(p, r, 1.0 / 479001600.0);
    p = __builtin_fma(p, r, 1.0 / 39916800.0);
    p = __builtin_fma(p, r, 1.0 / 3628800.0);
    p = __builtin_fma(p, r, 1.0 / 362880.0);
    p = __builtin_fma(p, r, 1.0 / 40320.0);
    p = __builtin_fma(p, r, 1.0 / 5040.0);
    p = __builtin_fma(p, r, 1.0 / 720.0);
    p = __builtin_fma(p, r, 1.0 / 120.0);
    p = __builtin_fma(p, r, 1.0 / 24.0);
    p = __builtin_fma(p, r, 1.0 / 6.0);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return __builtin_ldexp(p, (int)k);
}
#endif

// binary exponent of a finite x > 0 (frexp: x = f 2^e, 0.5 <= f < 1)
#ifdef HOSTSIM
__device__ __forceinline__ int exponent_of(double x) { int e; (void)frexp(x, &e); return e; }
#else
__device__ __forceinline__ int exponent_of(double x) { return __builtin_amdgcn_frexp_exp(x); }
#endif

// a b + c in one rounding (the dual form, kernels_ad.hip, is the plain product and sum)
__device__ __forceinline__ double adf_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
// high 32 bits of a double (the exponent test of the limiter's clamp, kernels_roe_march.hip; kernels_ad.hip holds the dual form)
__device__ __forceinline__ int adf_hiword(double x) { return __double2hiint(x); }

// a value that is the same in every lane of the wavefront, moved to a scalar register so that branches on it are scalar branches
#ifdef HOSTSIM
__device__ __forceinline__ int wave_uniform(int v) { return v; }
#else
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
#endif

// value of the neighbouring lane of the 64-wide wavefront: lane_up1 = lane-1
// (__shfl_up by 1), lane_dn1 = lane+1.  On gfx950 these are single DPP moves
// (v_mov_b32_dpp wave_shr:1 / wave_shl:1) per 32-bit half instead of a
// ds_bpermute through the LDS crossbar.  Lane 0 / 63 receive garbage.
#ifdef HOSTSIM
__device__ __forceinline__ double lane_up1(double v) { return __shfl_up(v, 1); }
__device__ __forceinline__ double lane_dn1(double v) { return __shfl_down(v, 1); }
__device__ __forceinline__ int lane_up1(int v) { return __shfl_up(v, 1); }
#else
__device__ __forceinline__ int lane_up1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, true); }
__device__ __forceinline__ int lane_dn1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, true); }
__device__ __forceinline__ double lane_up1(double v)
{
    return __hiloint2double(lane_up1(__double2hiint(v)), lane_up1(__double2loint(v)));
}
__device__ __forceinline__ double lane_dn1(double v)
{
    return __hiloint2double(lane_dn1(__double2hiint(v)), lane_dn1(__double2loint(v)));
}




#endif

typedef double adf_real8;      // a double that stays one where `double` is re-defined (kernels_ad.hip)
#define ADF_BLKVIEW BlkView
#define ADF_GEOM double
#include "blkview_def.h"
#undef ADF_GEOM
#undef ADF_BLKVIEW

// one boundary subface on the device (adflow_bc_subface with device copies of the BCData members)
struct BcFaceDev {
    int type, faceID, icBeg, icEnd, jcBeg, jcEnd;
    const double *norm, *rface, *uslip, *tns, *rho, *vx, *vy, *vz, *ps;
    const double *pt, *tt, *ht, *fdx, *fdy, *fdz;   // subsonic inflow with total conditions
    const double* turbInlet;                       // prescribed turbulence variable of inflow subfaces
    int inletTreatment, pad;
    double symNorm[3];     // BCData%symNorm of a symmetry plane (xhalo_block)
    double* tauq;          // viscous subfaces: viscSubface%tau(:,:,1:6), %q(:,:,1:3) over the OWNED face cells, component-major
};

// owned face cells of a subface (the node range inBeg+1..inEnd of viscSubfaceInfo, preprocessingAPI.F90:2520-2524)
__host__ __device__ inline void bc_owned_range(int faceID, int icBeg, int icEnd, int jcBeg, int jcEnd, int il, int jl, int kl, int r[4])
{
    const int amax = (faceID <= 2) ? jl : il, bmax = (faceID <= 4) ? kl : jl;
    r[0] = icBeg > 2 ? icBeg : 2;
    r[1] = icEnd < amax ? icEnd : amax;
    r[2] = jcBeg > 2 ? jcBeg : 2;
    r[3] = jcEnd < bmax ? jcEnd : bmax;
}

struct BcEntry { int slot, pad; BcFaceDev f; };     // one subface of the block in table slot `slot`
enum { BCP_SYMM1, BCP_SYMM2, BCP_WALL_ADIABATIC, BCP_WALL_ISOTHERMAL, BCP_FARFIELD, BCP_EXTRAP, BCP_EULERWALL,
       BCP_SUPERSONIC_INFLOW, BCP_SYMMPOLAR1, BCP_SYMMPOLAR2, BCP_SUBSONIC_OUTFLOW, BCP_SUBSONIC_INFLOW, BCP_ORDINAL };
struct BcPhase { int kind, first, count; long maxCells; };   // one launch: entries order[first .. first+count)

// porosity codes after the +1 shift used in `flags`
#define ADF_POR_NOFLUX 0
#define ADF_POR_BOUND 1
#define ADF_POR_NORMAL 2
__device__ __forceinline__ int flg_porI(uint8_t f) { return f & 3; }
__device__ __forceinline__ int flg_porJ(uint8_t f) { return (f >> 2) & 3; }
__device__ __forceinline__ int flg_porK(uint8_t f) { return (f >> 4) & 3; }
__device__ __forceinline__ double flg_blank(uint8_t f) { return (f & 64) ? 1.0 : 0.0; }

// per-call scalar parameters derived from adflow_opts on the host
struct KParams {
    int equations, spaceDiscr, limiter, orderTurb, turbProd;
    int viscous, eddyModel, dirScaling, useQCR, useRotationSA, useft2SA;
    int fineGrid;          // currentLevel == groundLevel
    int groundLevelIsOne;  // groundLevel == 1 (second-order turbulence advection only then)
    int doScaling;         // dirScaling && currentLevel <= groundLevel
    int onlyRadii;
    int coarseInit;        // initres: dw = wr instead of 0
    int updateEddy;        // currentLevel <= groundLevel: recompute rev in the stage update
    int fwMode;            // 0: fw not persistent (rFil==1, sfil==0, no store)  1: persistent fw
    int storeIntermed;     // store dtl / radii
    int dissApprox;        // lumped dissipation with the frozen sensor in b.ss (inviscidDissFlux*Approx)
    int viscFirst;         // the viscous march runs BEFORE the Roe march: it writes its flux sums into dw(2:5), the Roe march adds them and completes dw
    int radiiInMarch;      // the Euler march forms the spectral radii itself (no k_time_step pass in front)
    int metricFromX;       // marching kernels re-form the face normals from the node coordinates (as blocketteResCore, blockette.F90:854-960)
    int lumpedDiss;        // inputDiscretization::lumpedDiss (preconditioner assembly): first-order Roe upwind (fluxes.F90:1536)
    int approxSA;          // ADFLOW_RES_APPROX_SA: term1 of the SA source is zero (sa.F90:296); no dispatch key, the kernels select
    double sigma;
    double rFil, sfil;
    double vis2, vis4, vis2Coarse, adis, acousticScaleFactor, kappaCoef;
    double gammaConstant, gammaInf, pInf, pInfCorr, rhoInf, RGas, muRef, TRef, timeRef;
    double prandtl, prandtlTurb, SSuthDim, muSuthDim, TSuthDim;
    double sa_k, sa_cb1, sa_cb2, sa_cb3, sa_cv1, sa_cw1, sa_cw2, sa_cw3, sa_ct3, sa_ct4, sa_crot;
    double sa_qqFactor;    // 1 + (1-alfaTurb)/alfaTurb for implicit relaxation, else 1
    double sa_updFactor;   // alfaTurb for explicit relaxation, else 1
    double cfl, cflLimit, smoop, fcoll, turbResScale;
    double wInf[10];
    // matrix-free matvec (adflow_gpu_nk_residual_dev): the kernels that complete dw also write setRVec's entries dw / volRef
    // (NKSolvers.F90:1262-1376) of the PETSc-ordered residual vector (block offset BlkView::vecOff); NULL otherwise
    double* rvec;
    double rvecTurbScale;
    // the turbulence entry of rvec is written by the Roe march from the dw(itu1) the SA march left (both run in one queue, SA first):
    // the six entries of a cell go out together -- 48 contiguous bytes per cell instead of 40 + 8 from two kernels
    int rvecTurbFromDw;
    // Jacobian assembly (adflow_gpu_fd_jacobian on the marching kernels of the preconditioner matrix): the kernels that complete the
    // residual write the dense snapshot of the coloured evaluation -- resScale(dw), or its derivative part in forward mode -- INSTEAD
    // of dw (k_fd_snap / k_ad_snap read dw back and wrote the same numbers); NULL otherwise.  snapTab: per block slot the snapshot
    // array; component m of colour snapCol at ((snapCol snapN + m) nbox); state variable l is component l - snapL0
    const struct SnapSlot* snapTab;
    int snapCol, snapL0, snapN;
    double snapTurbScale;
};
struct SnapSlot { double* snap; };
// plain build: the scaled residual itself (k_fd_scatter forms the finite difference; kernels_ad.hip holds the form on dual numbers)
__device__ __forceinline__ void snap_put(GPTR(double) sn, unsigned c, double val) { stg(sn, c, val); }

// ---- face normals of a cell from its eight corner nodes, the formulas (and operand order) of metric_block
// (adjointExtra.F90:176-268, k_metric in kernels_geom.hip): a marching thread loads the two nodes (i, j, k) and (i, j-1, k) of
// its column per plane, takes the column i-1 by DPP and keeps the plane below: 6 loads instead of the 12 of sI, sJ(j-1), sJ, sK
struct NgNodes { double a[3], b[3]; };          // x(i, j, k) and x(i, j-1, k)

__device__ __forceinline__ void ngx_load_x(GPTR(const double) x, unsigned c, unsigned nb8, unsigned sj, NgNodes& n)
{
#pragma unroll
    for (int d = 0; d < 3; ++d) { n.a[d] = ldg(x, c + d * nb8); n.b[d] = ldg(x, c - sj + d * nb8); }
}

__device__ __forceinline__ void ngx_cross(double fact, const double p1[3], const double p2[3], const double q1[3], const double q2[3],
                                          double s[3])
{
    const double v1x = p1[0] - p2[0], v1y = p1[1] - p2[1], v1z = p1[2] - p2[2];
    const double v2x = q1[0] - q2[0], v2y = q1[1] - q2[1], v2z = q1[2] - q2[2];
    s[0] = fact * (v1y * v2z - v1z * v2y);
    s[1] = fact * (v1z * v2x - v1x * v2z);
    s[2] = fact * (v1x * v2y - v1y * v2x);
}

// sK of the node plane N alone (the plane below the first cell plane of a march)
__device__ __forceinline__ void ngx_normal_k(double fact, const NgNodes& N, double nK[3])
{
    double Na1[3], Nb1[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { Na1[d] = lane_up1(N.a[d]); Nb1[d] = lane_up1(N.b[d]); }
    ngx_cross(fact, N.a, Nb1, Na1, N.b, nK);                       // v1 = x(i,j,k) - x(l,m,k) ; v2 = x(l,j,k) - x(i,m,k)
}

// normals stored at the cell (i, j, k): sI, sJ(j-1), sJ, sK from the node planes k-1 (P) and k (N)
__device__ __forceinline__ void ngx_normals(double fact, const NgNodes& P, const NgNodes& N, double nI[3], double nJm[3], double nJ[3],
                                            double nK[3])
{
    double Na1[3], Nb1[3], Pa1[3], Pb1[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { Na1[d] = lane_up1(N.a[d]); Nb1[d] = lane_up1(N.b[d]); Pa1[d] = lane_up1(P.a[d]); Pb1[d] = lane_up1(P.b[d]); }
    ngx_cross(fact, P.a, N.b, N.a, P.b, nI);                       // v1 = x(i,j,n) - x(i,m,k) ; v2 = x(i,j,k) - x(i,m,n)
    ngx_cross(fact, P.a, Na1, Pa1, N.a, nJ);                       // v1 = x(i,j,n) - x(l,j,k) ; v2 = x(l,j,n) - x(i,j,k)
    ngx_cross(fact, P.b, Nb1, Pb1, N.b, nJm);                      // the same one row below
    ngx_cross(fact, N.a, Nb1, Na1, N.b, nK);
}


// coloured finite-difference Jacobian (kernels_jac.hip)
struct JacSpec {
    int nStencil, nState, lStart;     // lStart: first state variable (0-based) of the matrix
    int ca, cb, cc, cn, cm;           // colour(i,j,k) = (ca (i mod cm) + cb (j mod cm) + cc (k mod cm)) mod cn   (0-based)
    int st[33][3];                    // stencil offsets (row = perturbed cell + offset)
    int sc[33];                       // (ca di + cb dj + cc dk) mod cn of every entry (linear colourings)
};
void launch_fd_state(const BlkView& b, const double* wref, int l, int col, const JacSpec& J, double delta, hipStream_t s);
void launch_fd_state_closures(const BlkView& b, const double* wref, int l, int col, const JacSpec& J, double delta, const KParams& kp,
                              hipStream_t s, bool onlyL = false);
void launch_fd_snap(const BlkView& b, double* snap, const JacSpec& J, double turbResScale, hipStream_t s);
void launch_fd_scatter(const BlkView& b, const double* snap, double* jac, int l, const JacSpec& J, const double* dwref, double deltaInv,
                       hipStream_t s);
void launch_jac_rows(const BlkView& b, const double* jac, double* out, int nState, int nStencil, int k0, int nk, hipStream_t s);
void launch_fd_copy(const BlkView& b, double* dst, const double* src, int ncomp, hipStream_t s);
void launch_closures_halo(const BlkView& b, const KParams& kp, hipStream_t s);
void launch_fd_extract(const BlkView& b, double* dwref, double* jac, int l, int col, const JacSpec& J, double deltaInv, double turbResScale,
                       hipStream_t s);

// products with the assembled matrix (kernels_jacmult.hip): one block of the level as the product kernels see it.  xs / ys: the
// halo'd scratch arrays of nState components (box layout of the block); jac: the stencil blocks of the assembly
struct JmBlk {
    int nx, ny, nz, il, jl, kl, ib, jb, kb, ldi, ldk, pad;
    long nbox;
    long vecOff;          // first entry of the block in the vectors of the product: nState (not nw) entries per owned cell
    const double* jac;
    double *xs, *ys;
};
struct JmStencil { int n; int d[33][3]; };
// one reverse exchange as a donor-sorted list: target t (an owned cell) receives the sources seg[t] .. seg[t+1]-1 in list order
struct JmAccList {
    int nu = 0, nsrc = 0;
    int* tBlk = nullptr; long* tOff = nullptr; int* seg = nullptr;
    int* sBlk = nullptr;      // block slot of the source halo cell, or its position in the message
    long* sOff = nullptr;     // offset of the source halo cell (NULL: the sources are message entries)
};
void launch_jm_scatter(const JmBlk* tab, int nslots, int maxnx, int maxny, int maxnz, int nState, const double* x, hipStream_t s);
void launch_jm_gather(const JmBlk* tab, int nslots, int maxnx, int maxny, int maxnz, int nState, double* y, hipStream_t s);
// The vector count of the multi-vector kernels (1 .. 4) as the compile-time constant NV_ of the statement that follows; used by the
// launchers of kernels_jacmult.hip, kernels_pc.hip and kernels_pc_fill.hip inside their dispatch on nState.  ONFAIL: what a launcher
// does with a count it has no kernel for
#define ADF_DISPATCH_NV(nv, ONFAIL, ...)                                               \
    switch (nv) {                                                                      \
    case 1: { constexpr int NV_ = 1; __VA_ARGS__; } break;                             \
    case 2: { constexpr int NV_ = 2; __VA_ARGS__; } break;                             \
    case 3: { constexpr int NV_ = 3; __VA_ARGS__; } break;                             \
    case 4: { constexpr int NV_ = 4; __VA_ARGS__; } break;                             \
    default: ONFAIL;                                                                   \
    }
// nv = 1 .. JM_MAXW vectors in one pass over the matrix: vector v of xs / ys lies nState components behind vector v - 1, column v of y
// starts v ldy doubles behind column 0
enum { JM_MAXW = 4 };
void launch_jac_mult(const JmBlk* tab, int nslots, int maxnx, int maxny, int maxnz, int nState, const JmStencil& S, double* y, hipStream_t s,
                     int nv = 1, long ldy = 0);
void launch_jac_mult_t(const JmBlk* tab, int nslots, int maxnx, int maxny, int maxnz, int nState, const JmStencil& S, hipStream_t s,
                       int nv = 1);
void launch_jac_halo_accumulate(const JmBlk* tab, const JmAccList& a, int nState, const double* buf, int nbuf, hipStream_t s);

// block ILU of the 7-point matrix (kernels_pc.hip, kernels_pc_fill.hip): the factor of a level as its kernels see it.  Position q of
// the order of the factor (set, block, k, j, i) holds fac[q + ((s nState + l) nState + ll) ncell].  A set holds the cells whose lower
// entries all lie in earlier sets (longest path inside the block): the hyperplanes i + j + k at fill 0.  One builder (pc_build of
// api.hip) makes the tables of every fill from the offsets of the off-diagonal slots s, which the kernels of each fill number their
// own way; column s of nbr is the neighbour of slot s:
//   fill 0:    s = 0..2 L of the lower neighbour along i, j, k (columns c - e_i, c - e_j, c - e_k), 3..5 U of the upper neighbour along
//              i, j, k, 6 the inverted pivot block -- NOT ascending column order, where c - e_k would come first
//   fill 1, 2: nLow = (entries per row - 1) / 2 lower and as many upper entries, each side in ascending column order (c - e_k before
//              c - e_j before c - e_i; upper entry u is the mirror of lower entry nLow-1-u): s = 0..nLow-1 L, nLow..2 nLow-1 U, 2 nLow the
//              inverted pivot block
#include <vector>
struct PcTab {
    long ncell;           // owned cells of the level
    double* fac;
    double* ws;           // nState components in the order of the factor: the vector between and during the two sweeps
    const int* nbr;       // nbr[s ncell + q]: position of the neighbour of off-diagonal slot s (see above), -1 outside the block
    const int* vec;       // the cell's number in the PETSc layout (block, k, j, i)
    const int* cblk;      // setup only: slot of the cell's block in blk[] and its box index
    const int* cbox;
    const JmBlk* blk;
    int* flag;            // != 0: 1 + position of a cell whose pivot block is singular or not finite
    int sten[7];          // stencil entries of the assembly: the columns c - e_i, c - e_j, c - e_k, c + e_i, c + e_j, c + e_k, c
    const double* tsm;    // setup only: the pseudo-time term of ANK added to the diagonal blocks (kernels_ank.hip), NULL = none
    double turbDiag;      // S(nt1, nt1) = turbResScale / turbCFLScale of the coupled T
    // fill 1 and 2 only (kernels_pc_fill.hip); zero at fill 0
    int asmEnt[23];       // stencil entry of the assembly that slot s starts from, -1: a fill entry (starts from zero)
    signed char tgt[121]; // tgt[e nLow + u]: slot of this row that L_{c,n} U_{n,m} lands in (n: lower entry e, m: upper entry u
                          // of row n), -1: outside the pattern
    double* wsx;          // the work space of vectors 1 .. of a multi-vector application, laid out like ws; NULL until the first one
    // the factor over the whole level only (kernels_pc_coupled.hip); NULL otherwise
    const unsigned* cw;   // per cell: bits 0..5 "the neighbour of slot d is lower", bits 6+3d..8+3d the slot in which that neighbour
                          // keeps its entry back to this cell; nbr[] then names neighbours in any block of the level
};
int launch_pc_factor(const PcTab& T, int nState, const std::vector<int>& planeStart, hipStream_t s);
// nv = 1 .. PC_MAXW vectors through the same launches: column v of r and z starts v ldr / v ldz doubles behind column 0 and uses the
// work space ws (v = 0) or wsx (v - 1); nv = 1 is the application of one vector
enum { PC_MAXW = 4 };
int launch_pc_apply(const PcTab& T, int nState, int transpose, const std::vector<int>& planeStart, const double* r, double* z,
                    hipStream_t s, int nv = 1, long ldr = 0, long ldz = 0);
// ILU(0) over the whole level (kernels_pc_coupled.hip; adflow_gpu_pc_set_coupled): the same storage with slot d = 0..5 holding L or U
// as the mask of cw says, setStart = first position of every dependency level set of the level, and the end
int launch_pcc_factor(const PcTab& T, int nState, const std::vector<int>& setStart, hipStream_t s);
int launch_pcc_apply(const PcTab& T, int nState, int transpose, const std::vector<int>& setStart, const double* r, double* z,
                     hipStream_t s, int nv = 1, long ldr = 0, long ldz = 0);
// block ILU(1) / ILU(2) of the same matrix (kernels_pc_fill.hip): nEnt = 13 or 23 entries per row, levelStart = first position of
// every dependency level set in the order of the factor, and the end
int launch_pcf_factor(const PcTab& T, int nState, int nEnt, const std::vector<int>& levelStart, hipStream_t s);
int launch_pcf_apply(const PcTab& T, int nState, int nEnt, int transpose, const std::vector<int>& levelStart, const double* r,
                     double* z, hipStream_t s, int nv = 1, long ldr = 0, long ldz = 0);
// ILU(k) over the whole level on a general block pattern (kernels_pc_level.hip; adflow_gpu_pc_set_level_fill): the factor as its
// kernels see it.  "Number" below is the cell's number in the ordering of the factor: the natural one, RCM or the caller's
// (adflow_gpu_pc_set_ordering; api.hip relabels, the kernels do not know).  Position q of the order (set, number) is lane q % 64 of slice q / 64 of its set (counted from the first
// position of the set): the rows of one workgroup.  A slice of st rows whose longest row has w entries owns the w st entry slots from
// ebase on; entry j of lane t is slot ebase + j st + t of epos / enat / einfo, and its block is fac[ebase nState^2 + (j nState^2 + e) st + t].
// The entries of a row ascend in the number of their column: nLow lower entries, the pivot block (as its LU factors, kernels_pc_level.hip), the upper ones.
struct PclTab {
    long ncell;           // owned cells of the level
    double* fac;
    double* ws;           // nState components in the order of the factor: the vector between and during the two sweeps
    int* rpiv;            // per row: the row exchanges of the LU of its pivot block, three bits each (written by the factorisation)
    const long* ebase;   // per row: first entry slot of its slice (64-bit: the factor of the benchmark mesh has > 2^31 doubles)
    const int* rinfo;     // per row: lane (bits 0..7) and rows of its slice (bits 8..)
    const int* rcnt;      // per row: nLow (bits 0..15) and entries (bits 16..)
    const int* epos;      // per entry: position of the row of its column
    const int* enat;      // per entry: number of its column in the ordering of the factor (adflow_gpu_pc_set_ordering; the natural
                          // number by default), the key of the merge in k_pcl_factor
    const int* einfo;     // per entry: bits 0..15 the number of the mirror entry (n, c) in row n; bits 16..: 1 + the direction
                          // (0..5, 6: the diagonal) of the assembled entry it starts from, 0: a fill entry (starts from zero)
    const int* vec;       // the cell's number in the PETSc layout (block, k, j, i)
    const int* cblk;      // setup only: slot of the cell's block in blk[] and its box index
    const int* cbox;
    const JmBlk* blk;
    int* flag;            // != 0: 1 + position of a cell whose pivot block is singular or not finite
    int sten[7];          // stencil entries of the assembly, as PcTab::sten
    const double* tsm;    // setup only, as PcTab::tsm
    double turbDiag;
};
int launch_pcl_factor(const PclTab& T, int nState, const std::vector<int>& setStart, hipStream_t s);
int launch_pcl_apply(const PclTab& T, int nState, int transpose, const std::vector<int>& setStart, const double* r, double* z,
                     hipStream_t s);
// the multigrid preconditioner (kernels_pc_mg.hip): every level keeps its 7-point matrix in the box layout of JmBlk (jac = the blocks
// of the level, vecOff = the first CELL of the block in the vectors of the level) with the stencil entries of the assembly;
// PcMgSten: those entries in the order of PcTab::sten.  Tables hold one JmBlk per block, the same slot on every level; maxn*: the
// largest extents of the level the lanes run over
struct PcMgSten { int s[7]; };
void launch_mg_fine_copy(const JmBlk* src, const JmBlk* dst, int nslots, int maxnx, int maxny, int maxnz, int nState, const PcMgSten& S,
                         const double* tsm, double turbDiag, long N, hipStream_t s);
void launch_mg_coarsen(const JmBlk* fine, const JmBlk* coarse, int nslots, int maxnx, int maxny, int maxnz, int nState, const PcMgSten& S,
                       hipStream_t s);
void launch_mg_restrict(const JmBlk* fine, const JmBlk* coarse, int nslots, int maxnx, int maxny, int maxnz, int nState, const double* r,
                        double* rhs, hipStream_t s);
void launch_mg_residual(const JmBlk* tab, const JmBlk* coarse, int nslots, int maxnx, int maxny, int maxnz, int nState, int transpose,
                        const PcMgSten& S, const double* r, const double* x, double* y, double* res, hipStream_t s);
// the preconditioner Richardson iterations (kernels_pc_rich.hip; adflow_gpu_pc_set_its): the copy of the 7-point matrix of the whole
// level a factor owns, as its residual kernel sees it
struct PcRichTab {
    long ncell;           // owned cells of the level
    const double* mat;    // mat[(q nState^2 + e) ncell + c]: component e of the block of direction q (0..5: -i, -j, -k, +i, +j, +k; 6: the
                          // diagonal) of row c, c = the cell's number in the PETSc layout; zero where the direction has no column
    const int* col;       // col[q ncell + c]: the number of the column of direction q of row c, -1: none
    const unsigned* cw;   // per row: bit q = the column of direction q lies behind a block face; bits 6+3q..8+3q = the direction in which
                          // that column keeps its entry back to this row
};
// src: the blocks of the assembly (vecOff = first CELL of the block); S, tsm, turbDiag, N as launch_mg_fine_copy
void launch_rich_copy(const JmBlk* src, int nslots, int maxnx, int maxny, int maxnz, int nState, const PcMgSten& S, const double* tsm,
                      double turbDiag, long N, const int* col, double* mat, hipStream_t s);
// t = b - A x (transpose: A^T) for nv = 1 .. PC_MAXW columns ldb / ldx / ldt apart; sub: without the columns behind block faces
int launch_rich_residual(const PcRichTab& T, int nState, int transpose, int sub, int nv, const double* b, long ldb, const double* x,
                         long ldx, double* t, long ldt, hipStream_t s);
// the vectors of GMRES: one step of modified Gram-Schmidt per launch (partial sums in, partial sums out), see kernels_pc.hip
enum { GM_PARTS = 256 };  // the most partial sums one reduction leaves (GM_T of kernels_pc.hip): the size of a buffer of them
int gm_groups(long n);
void launch_gm_mgs(double* w, const double* v, const double* hp, const double* u, double* out, double* hOut, long n, hipStream_t s);
void launch_gm_sum(const double* hp, long n, double* hOut, hipStream_t s);
void launch_gm_axpby(double* y, double a, const double* x, double b, long n, hipStream_t s);
// the columns of a multi solve in lock-step (column c of a vector starts c ld doubles behind column 0; partial sums of column c at
// c GM_PARTS; hOut[c]); GmCoef: the coefficients of every column of one update, a = 0 with b = 1 leaves the column untouched
enum { GM_MAXV = 32 };    // the most columns of one call (ADFLOW_GPU_MAX_NVEC of the header)
struct GmCoef { double a[GM_MAXV], b[GM_MAXV]; };
void launch_gm_mgs_multi(double* w, const double* v, const double* hp, const double* u, double* out, double* hOut, long n, long ld,
                         int nvec, hipStream_t s);
void launch_gm_sum_multi(const double* hp, long n, double* hOut, int nvec, hipStream_t s);
void launch_gm_axpby_multi(double* y, long ldy, const double* x, long ldx, const GmCoef& k, long n, int nvec, hipStream_t s);
// approximate Newton-Krylov step (kernels_ank.hip): vectors of nS variables per owned cell; kp != NULL: with the closures of blocketteRes
struct KParams;
// The reduction buffer of the ANK entries (g_ank.red of api.hip), in doubles: partial results, one per workgroup of a reduction, then
// the scalars.  Two index spaces, two types: AnkRed are offsets into the buffer, AnkScal are offsets into its scalars.  The kernels
// take the partial results they write and `hdev` / `out`, pointers into the scalars; hdev = the buffer + ANK_RED_SCAL is indexed by
// ANK_H .. ANK_SUMS
enum { ANK_PARTS = 256 };                  // the most workgroups of a reduction (AK_T of kernels_ank.hip)
enum AnkScal {
    ANK_H = 0, ANK_HINV = 1,               // the MATMFFD_DS step h and 1 / h (both 0 when v = 0)
    ANK_SUMS = 2,                          // the three sums h was formed from
    ANK_LAMBDA = 5,                        // the step the physicality check allows
    ANK_NORM = 6,                          // the norm of the unsteady residual
    ANK_NSCAL = 8
};
enum AnkRed {
    ANK_RED_SUMS = 0,                      // 3 x ANK_PARTS partial sums of w.v, |v|_1, |v|_2^2 (launch_ank_step)
    ANK_RED_MIN = 3 * ANK_PARTS,           // ANK_PARTS partial minima (launch_ank_phys)
    ANK_RED_SCAL = 4 * ANK_PARTS,          // the ANK_NSCAL scalars
    ANK_RED = ANK_RED_SCAL + ANK_NSCAL     // doubles in all
};
int ank_groups(long n);
void launch_ank_set_w(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, int nS, const double* vec, const double* hv,
                      const double* hdev, const KParams* kp, int* floored, hipStream_t s);
void launch_ank_get_r(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, int nS, double* vec, double turbScale, hipStream_t s);
void launch_ank_time_step(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, double cfl, double* tsm, long N, hipStream_t s);
void launch_ank_quotient(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, int nS, const double* v, const double* r0,
                         const double* tsm, long N, double turbDiag, double turbScale, const double* hdev, double* y, hipStream_t s);
void launch_ank_step(const double* w, const double* v, long n, double errRel, double umin, double* part, double* hdev, hipStream_t s);
void launch_ank_phys(const double* w, double* dw, long ncell, int nS, int flow, int lt, double eps, double tol, double tolTurb,
                     double turbThreshold, double lambda0, double* part, double* out, hipStream_t s);
// the turbulence KSP (one entry per cell) and the line-search residual with its norm
void launch_ank_set_w_turb(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, const double* vec, const double* hv,
                           const double* hdev, const KParams* kp, hipStream_t s);
void launch_ank_get_r_turb(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, double* vec, double turbScale, hipStream_t s);
void launch_ank_time_step_turb(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, double cfl, double* tsm, hipStream_t s);
void launch_ank_quotient_turb(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, const double* v, const double* r0,
                              const double* tsm, double turbDiag, double turbScale, const double* hdev, double* y, hipStream_t s);
long ank_unsteady_groups(int nslots, int maxnx, int maxny, int maxnz);
void launch_ank_unsteady(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, int nS, int turb, const double* dW, const double* tsm,
                         long N, double turbDiag, double turbScale, double omega, double* r, double* part, double* out, hipStream_t s);

// surface integration (kernels_wallint.hip; adflow_gpu_wall_integrate): one wall subface of the level as the face kernel sees it
struct WiFace {
    int slot, faceID;         // block slot in the level's table, BCFaceID
    int r[4];                 // the owned face cells (bc_owned_range)
    int icBeg, jcBeg, ldn;    // BCData%norm: component c of cell (a, b) at (a - icBeg) + (b - jcBeg) ldn + c nnorm
    int inflow;               // flow subfaces: 1 on SubsonicInflow / SupersonicInflow (inFlowFact = -1); walls: 0
    long nnorm;
    const double* norm;       // NULL where no term reads it (y+ of a viscous wall under RANS does)
    const double* tauq;       // viscous walls: the stored stress (BcFaceDev::tauq); NULL on an Euler wall
    const signed char* iblank;   // per owned face cell, NULL = all ones
    double* fpv;              // BCData%Fp(3), %Fv(3), %area over the owned face cells, component-major
    long goff;                // the first owned face of the subface among all owned wall faces of the level (table order)
};
// the parameters of wallIntegrationFace, lengths already times LRef
struct WiPar {
    double pInf, pRef, gammaInf, MachCoef;
    double refPoint[3], axisPoint[3], axisDir[3], velDir[3];      // axisDir: the unit vector along the moment axis
    double sepOffset, sepSharpness, cavitationNumber, cavOffset, cavSharpness, cpminRho, cpminFamily;
    int computeCavitation, cavExponent, rans, pad;
};
// the quantities a workgroup of the face kernel reduces: sums, then the maximum of y+ and the minimum of Cp
enum { WI_FP = 0, WI_FV = 3, WI_MP = 6, WI_MV = 9, WI_SEP = 12, WI_SEPAVG = 13, WI_CAV = 16, WI_AXIS = 17, WI_CPMIN_KS = 18, WI_COF = 19,
       WI_YPLUS = 28, WI_CPMIN = 29, WI_NQ = 30 };
enum { WI_T = 256 };          // threads of a workgroup of both kernels
inline int wallint_groups_per_face(long maxOwned) { return (int)((maxOwned + WI_T - 1) / WI_T); }
// part: WI_NQ x (workgroups per subface x nface) doubles; member[g nface + f] != 0: subface f belongs to group g; out: nGroups x
// ADFLOW_WALLINT_STRIDE doubles on the device
void launch_wallint(const BlkView* tab, const WiFace* faces, int nface, long maxOwned, const WiPar& P, double* part,
                    const unsigned char* member, int nGroups, double* out, hipStream_t s);
// derivatives of the integration (adflow_gpu_wall_integrate_fwd / _bwd).  The transposed product is a coloured forward-mode sweep over
// the front of the evaluation: the colour of a cell is (i mod WI_CM) + WI_CM (j mod WI_CM) + WI_CM^2 (k mod WI_CM), local to its block,
// halos included.  A term of a face depends on cells at most WI_REACH from it in the plane of the wall and on the WI_DEPTH layers from
// the first halo to the third interior cell along the normal: a box of 5 x 5 x 4 cells, in which the cube of WI_CM = 5 gives every
// cell its own colour whichever way the wall faces.  The treatments implemented today (constant / linear pressure, normal momentum)
// reach one cell in the plane and the second interior layer; the box also holds what the reference's quadratic extrapolation would
// read (the third layer; at an edge of two walls a second cell in the plane).  DESIGN 8g has the price of that margin.
enum { WI_CM = 5, WI_NCOL = WI_CM * WI_CM * WI_CM, WI_REACH = 2, WI_DEPTH = 4 };
struct JmBlk;
void launch_wallint_credit(const WiFace* faces, int nface, long maxBox, const JmBlk* tab, long nt, int nRhs, int lq, int col,
                           const double* g, long ldg, hipStream_t s);

// flow integration (kernels_wallint.hip; adflow_gpu_flow_integrate): flowIntegrationFace over the in- and outflow subfaces of a level.
// The subfaces come in a WiFace table of their own (norm, tauq, fpv NULL), the groups in a membership table like that of the walls.
struct FiPar {
    double pInf, pRef, gammaInf, rhoRef, TRef, uRef, timeRef, RGas, rGasDim;
    double internalFlowFact;      // -1 for flowType == internalFlow, else 1
    double refPoint[3];           // LRef pointRef
};
// the quantities a workgroup of the flow face kernel reduces, all sums
enum { FI_MASSFLOW = 0, FI_MASSPTOT = 1, FI_MASSTTOT = 2, FI_MASSPS = 3, FI_MASSMN = 4, FI_MASSA = 5, FI_MASSRHO = 6, FI_MASSV = 7,
       FI_MASSN = 10, FI_MASSVI = 13, FI_AREA = 14, FI_AREAPTOT = 15, FI_AREAPS = 16, FI_FP = 17, FI_MP = 20, FI_FM = 23, FI_MM = 26,
       FI_COF = 29, FI_NQ = 38 };
// part: FI_NQ x (workgroups per subface x nface) doubles; member and out as for launch_wallint
void launch_flowint(const BlkView* tab, const WiFace* faces, int nface, long maxOwned, const FiPar& P, double* part,
                    const unsigned char* member, int nGroups, double* out, hipStream_t s);

// The level-batched launches fold (block slot, plane) into gridDim.z, which HIP limits to 65535: a launcher whose level has more
// slots than fit calls itself on consecutive slot ranges (the kernels index the table relative to the pointer they get).
extern int g_max_grid_z;          // 65535; tuning "max_grid_z" lowers it for the tests
extern int g_ra_pcr;              // kernels_smooth.hip, tuning "ra_pcr"
extern int g_dadi_pcr;            // kernels_smooth.hip, tuning "dadi_pcr"
inline int level_slots_per_launch(int planes)
{
    const int per = g_max_grid_z / (planes > 0 ? planes : 1);
    return per > 0 ? per : 1;
}
#define LEVEL_SPLIT(nslots, planes, CALL)                                                         \
    {                                                                                             \
        const int per_ = level_slots_per_launch(planes);                                          \
        if ((nslots) > per_) {                                                                    \
            for (int s0_ = 0; s0_ < (nslots); s0_ += per_) {                                      \
                const int n_ = ((nslots) - s0_ < per_) ? (nslots) - s0_ : per_;                   \
                CALL;                                                                             \
            }                                                                                     \
            return;                                                                               \
        }                                                                                         \
    }

// ---- kernel launchers (one translation unit per kernel family) -------------
void launch_time_step_level(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, const KParams& kp, hipStream_t s);
void launch_entropy(const BlkView& b, hipStream_t s);
void launch_inviscid_level(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, const KParams& kp, hipStream_t s);
void launch_initres(const BlkView& b, const KParams& kp, int l0, int l1, hipStream_t s);
void launch_viscous(const BlkView& b, const KParams& kp, hipStream_t s);
int viscous_is_tiled();
void launch_sa_march(const BlkView* tab, const int4* tiles, int ntiles, const KParams& kp, hipStream_t s, bool solve);
void launch_visc_march_approx(const BlkView* tab, const int4* tiles, int ntiles, const KParams& kp, hipStream_t s);
bool euler_march_radii_capable(int fwMode, int doScaling, double adis);
void launch_visc_gf(const BlkView* tab, const int4* tiles, int ntiles, const KParams& kp, bool storeGrad, hipStream_t s);
void adf_note_snap(int bits);   // api.hip: a launcher reports that its kernel wrote the flow (1) / turbulence (2) snapshot entries (KParams::snapTab)
int adf_fail(const char* what); // api.hip: a launcher reports an internal error (the text of the failed call); returns 1
void adf_note_rvec(int bits);   // api.hip: a launcher reports that its kernel wrote the flow (1) / turbulence (2) part of kp.rvec
int adf_round_size();          // api.hip: workgroups of a marching kernel resident at a time (2 x CUs)
void adf_phase_mark(int i);    // api.hip: optional HIP event between the phases of blocketteRes
void launch_coarse_coordinates_level(const BlkView* ctab, const BlkView* ftab, int nslots, int nx, int ny, int nz, hipStream_t s);
void launch_xhalo_level(const BlkView* tab, int nslots, int nx, int ny, int nz, hipStream_t s);
void launch_xhalo_symm(const BlkView* tab, const BcEntry* ent, const int* order, const BcPhase& ph, hipStream_t s);
void launch_wall_stress(const BlkView* tab, const BcEntry* ent, const int* order, const BcPhase& ph, const KParams& kp, bool formGrad,
                        hipStream_t s);
void launch_viscous_approx(const BlkView& b, const KParams& kp, hipStream_t s);
void launch_face_vectors(const BlkView& b, hipStream_t s);
void launch_sa_residual_level(const BlkView* tab, int nslots, int nx, int ny, int nz, const KParams& kp, hipStream_t s);
void launch_sa_solve_level(const BlkView* tab, int nslots, int nx, int ny, int nz, const KParams& kp, hipStream_t s, bool marchRes = false);
void launch_rk_save_level(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, hipStream_t s);
void launch_etot_owned(const BlkView& b, double gammaConstant, hipStream_t s);
void launch_scale_dw_level(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, double factor, int timesVol, hipStream_t s);
void launch_source_terms(const BlkView* tab, const int* blk, const long* off, int n, const double Ffact[3], double Qfact, int withBlank,
                         hipStream_t s);
void launch_low_speed_precond_level(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, const KParams& kp, hipStream_t s);
void launch_stage_update_level(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, const KParams& kp, double scale,
                               int fromWn, hipStream_t s);
void launch_res_averaging_level(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, const KParams& kp, hipStream_t s,
                                double scaleDtl = 0.0);
void launch_dadi_level(const BlkView* tab, int nslots, int nx, int ny, int nz, const KParams& kp, hipStream_t s, bool withUpdate = false);
void launch_halo_copy(const BlkView* tab, const int* donorBlk, const long* donorOff, const int* haloBlk, const long* haloOff,
                      int n, unsigned mask, hipStream_t s);
void launch_periodic(const BlkView* tab, const int* blk, const long* off, int n, const double rotMatrix[9], const double rotCenter[3],
                     const double translation[3], int coor, hipStream_t s);
void launch_halo_pack(const BlkView* tab, const int* blk, const long* off, int n, unsigned mask, double* buf, hipStream_t s);
void launch_halo_unpack(const BlkView* tab, const int* blk, const long* off, int n, unsigned mask, const double* buf,
                        hipStream_t s);
int launch_inviscid_march(const BlkView* tab, const int4* tiles, int ntiles, const KParams& kp, hipStream_t s);
int inviscid_march_enabled();
int launch_roe_march(const BlkView* tab, const int4* tiles, int ntiles, const KParams& kp, hipStream_t s);
// kernels_pc_march.hip: first-order Roe + thin-layer viscous flux in one march (the mean-flow residual of the preconditioner matrix)
void launch_pc_march(const BlkView* tab, const int4* tiles, int ntiles, const KParams& kp, int kch, hipStream_t s);
bool roe_march_takes(int limiter);   // kernels_roe_march.hip: called by plan_flow (flow_plan.h) only
void launch_euler_march(const BlkView* tab, const int4* tiles, int ntiles, const KParams& kp, hipStream_t s);
void euler_march_tiles(const BlkView& b, int* ntx, int* nty, int* ntz);
void launch_restrict_level(const BlkView* ctab, const BlkView* ftab, int nslots, int nx, int ny, int nz, const KParams& kp, hipStream_t s);
void launch_store_entry_state_level(const BlkView* ctab, int nslots, int nx, int ny, int nz, hipStream_t s);
void launch_forcing_level(const BlkView* ctab, int nslots, int nx, int ny, int nz, double fcoll, hipStream_t s);
void launch_corrections_level(const BlkView* ctab, int nslots, int nx, int ny, int nz, hipStream_t s);
void launch_prolong_update_level(const BlkView* ftab, const BlkView* ctab, int nslots, int nx, int ny, int nz, const KParams& kp,
                                 hipStream_t s);
void launch_set_w(const BlkView& b, const double* vec, double turbFloor, hipStream_t s);
void launch_get_r(const BlkView& b, double* vec, double turbScale, double* sums, hipStream_t s);
void launch_closures(const BlkView& b, const KParams& kp, hipStream_t s);
// level-batched forms (blockIdx.z = slot * planes + plane): one launch for every block of a level
void launch_closures_level(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, const KParams& kp, hipStream_t s,
                           int* floored = nullptr);
void launch_set_w_closures_level(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, const double* vec, double turbFloor,
                                 const KParams& kp, int* floored, hipStream_t s);
void launch_set_w_level(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, const double* vec, double turbFloor, hipStream_t s);
void launch_get_r_level(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, double* vec, double turbScale, double* sums, hipStream_t s);
void launch_entropy_level(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, hipStream_t s);
void launch_etot_owned_level(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, double gammaConstant, hipStream_t s,
                             const int* onlyIf = nullptr);
void launch_initres_level(const BlkView* tab, int nslots, int maxnx, int maxny, int maxnz, const KParams& kp, int l0, int l1, hipStream_t s);
void launch_res_norms(const BlkView& b, int nvar, double* out, hipStream_t s);
#include <vector>
void launch_apply_all_bc(const BlkView* tab, const BcEntry* ent, const int* order, const std::vector<BcPhase>& flow,
                         const KParams& kp, int second, int eulerWallTreatment, int viscWallTreatment, int outflowTreatment, int hScalingInlet,
                         hipStream_t s);
void launch_turb_bc_treatment(const BlkView* tab, int nslots, long maxFace, const BcEntry* ent, const int* order,
                              const std::vector<BcPhase>& ordinal, const KParams& kp, hipStream_t s);
void launch_apply_turb_bc(const BlkView* tab, const BcEntry* ent, const int* order, const std::vector<BcPhase>& ordinal,
                          const KParams& kp, int second, hipStream_t s);
void launch_bc_coarse_corrections(const BlkView* tab, const BcEntry* ent, const int* order, const std::vector<BcPhase>& ordinal,
                                  double fact, hipStream_t s);
void launch_corner_row_halos_level(const BlkView* tab, int nslots, const KParams& kp, hipStream_t s);
void launch_volume_metric(const BlkView& b, int rightHanded, hipStream_t s);
void launch_boundary_normals(const BlkView& b, const BcFaceDev* faces, int nBocos, hipStream_t s);
void launch_wall_distance(const BlkView& b, const int* ind, const double* uv, const double* xSurf, hipStream_t s);

// ---- forward-mode twins of the gather kernels (kernels_ad.hip)
// entry points of kernels_ad.hip (BlkView-layout views whose array pointers lead to dual numbers, blkview_def.h)
void ad_launch_from_real(const double* src, void* dst, long n, hipStream_t s);
void ad_launch_value(const void* src, double* dst, long n, int deriv, hipStream_t s);
void ad_launch_snap(const BlkView& b, const void* dwd, double* snap, const JacSpec& J, double turbResScale, hipStream_t s);
void ad_launch_closures_halo(const BlkView& adv, const KParams& kp, hipStream_t s);
void ad_launch_apply_all_bc(const BlkView* tab, const BcEntry* ent, const int* order, const std::vector<BcPhase>& flow, const KParams& kp,
                            int second, int eulerWallTreatment, int viscWallTreatment, int outflowTreatment, int hScalingInlet, hipStream_t s);
void ad_launch_turb_bc(const BlkView* tab, int nslots, long maxFace, const BcEntry* ent, const int* order, const std::vector<BcPhase>& ordinal,
                       const KParams& kp, int second, hipStream_t s);
void ad_launch_time_step_level(const BlkView* tab, int n, int nx, int ny, int nz, const KParams& kp, hipStream_t s);
void ad_launch_entropy_level(const BlkView* tab, int n, int nx, int ny, int nz, hipStream_t s);
void ad_launch_sa_residual_level(const BlkView* tab, int n, int nx, int ny, int nz, const KParams& kp, hipStream_t s);
void ad_launch_inviscid_level(const BlkView* tab, int n, int nx, int ny, int nz, const KParams& kp, hipStream_t s);
void ad_launch_viscous(const BlkView& adv, const KParams& kp, hipStream_t s);
void ad_launch_viscous_approx(const BlkView& adv, const KParams& kp, hipStream_t s);
void ad_launch_seed_closures(const BlkView& real, const BlkView& adv, int l, int col, const JacSpec& J, const KParams& kp, hipStream_t s,
                             bool onlyL);
// matrix-free products (adflow_gpu_jacfree_mult): the seed from the halo'd scratch array xs of the product, the result into the vector y
void ad_launch_seed_vector(const BlkView& real, const BlkView& adv, const double* xs, int lStart, int nState, const KParams& kp, hipStream_t s);
void ad_launch_jf_readout(const BlkView& adv, double* y, long vecOff, int lStart, int nState, double turbResScale, hipStream_t s);
void ad_launch_pc_march(const BlkView* tab, const int4* tiles, int ntiles, const KParams& kp, int kch, hipStream_t s);
void ad_launch_sa_march(const BlkView* tab, const int4* tiles, int ntiles, const KParams& kp, hipStream_t s);
void ad_launch_visc_gf(const BlkView* tab, const int4* tiles, int ntiles, const KParams& kp, hipStream_t s);
int ad_launch_roe_march(const BlkView* tab, const int4* tiles, int ntiles, const KParams& kp, hipStream_t s);
int ad_launch_inviscid_march(const BlkView* tab, const int4* tiles, int ntiles, const KParams& kp, hipStream_t s);
// the dual front of the surface integration (kernels_viscous.hip and kernels_wallint.hip in namespace adj): the nodal gradients of the
// wall node planes; the forward product (part: WI_NQ x workgroups dual numbers); the face kernel of the transposed product
void ad_launch_wall_node_grad(const BlkView* tab, const BcEntry* ent, const int* order, const BcPhase& ph, hipStream_t s);
void ad_launch_wallint_fwd(const BlkView* tab, const WiFace* faces, int nface, long maxOwned, const WiPar& P, const KParams& kp, void* part,
                           const unsigned char* member, int nGroups, double* out, double* outDot, hipStream_t s);
void ad_launch_wallint_bar(const BlkView* tab, const WiFace* faces, int nface, long maxOwned, const WiPar& P, const KParams& kp,
                           const double* wq, int nRhs, long ldg, double* g, hipStream_t s);
// the same for the flow subfaces (part: FI_NQ x workgroups dual numbers; wq: FI_NQ weights per set and subface)
void ad_launch_flowint_fwd(const BlkView* tab, const WiFace* faces, int nface, long maxOwned, const FiPar& P, void* part,
                           const unsigned char* member, int nGroups, double* out, double* outDot, hipStream_t s);
void ad_launch_flowint_bar(const BlkView* tab, const WiFace* faces, int nface, long maxOwned, const FiPar& P, const double* wq, int nRhs,
                           long ldg, double* g, hipStream_t s);
void ad_launch_selftest_math(int which, const double* x, const double* a, long n, double* y, double* dy, hipStream_t s);
void ad_launch_visc_march_approx(const BlkView* tab, const int4* tiles, int ntiles, const KParams& kp, hipStream_t s);
