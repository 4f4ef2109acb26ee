// The pointwise state closures that open blockette::blocketteRes, one owned cell (computePressureSimple / computeLamViscosity /
// computeEddyViscosity, blockette.F90:199-203, flowUtils.F90:867-925,1201-1300, turbUtils.F90:657-720): shared by the kernels that
// write the state from a PETSc vector and close it in the same pass (kernels_nk.hip, kernels_ank.hip).
#pragma once
#include "internal.h"

// computeEddyViscosity for Spalart-Allmaras (turbUtils.F90:657-720) of one cell: the one form of this arithmetic, shared by the
// closures below and by the turbulence state write of the ANK turbulence KSP (k_ank_set_w_turb), which re-forms nothing else
__device__ __forceinline__ double sa_eddy_viscosity(const KParams& kp, double rho, double rlv, double nuTilde)
{
    const double cv13 = kp.sa_cv1 * kp.sa_cv1 * kp.sa_cv1;
    const double rnuSA = nuTilde * rho;
    const double chi = rnuSA / rlv;
    const double chi3 = chi * chi * chi;
    return chi3 / (chi3 + cv13) * rnuSA;
}

template <bool ETOT = false>
__device__ __forceinline__ void closures_cell(const BlkView& b, int i, int j, int k, const KParams& kp, int* __restrict__ floored)
{
    const long c = b.idx(i, j, k);
    const long nb = b.nbox;
    const double rho = b.w[c], u = b.w[c + nb], v = b.w[c + 2 * nb], w = b.w[c + 3 * nb];
    const double gm1 = kp.gammaConstant - 1.0;
    const double v2 = u * u + v * v + w * w;
    double p = gm1 * (b.w[c + 4 * nb] - 0.5 * rho * v2);
    const double pFloor = 1.e-4 * kp.pInfCorr;
    const bool hitFloor = !(p >= pFloor);
    p = fmax(p, pFloor);
    b.p[c] = p;
    if (ETOT) {
        if (hitFloor) *floored = 1;
        else {
            const double ovgm1 = 1.0 / (kp.gammaConstant - 1.0);
            b.w[c + 4 * nb] = ovgm1 * p + 0.5 * rho * v2;
        }
    }
    if (kp.viscous) {
        const double muSuth = kp.muSuthDim / kp.muRef, TSuth = kp.TSuthDim / kp.TRef, SSuth = kp.SSuthDim / kp.TRef;
        const double T = p / (kp.RGas * rho);
        const double tt = T / TSuth;
        const double rlv = muSuth * ((TSuth + SSuth) / (T + SSuth)) * (tt * sqrt(tt));
        b.rlv[c] = rlv;
        if (kp.eddyModel && kp.updateEddy) b.rev[c] = sa_eddy_viscosity(kp, rho, rlv, b.w[c + 5 * nb]);
    }
}
