// Surface integration on the device: forces, moments and surface sensors of the wall subfaces of a level, the terms of
// surfaceIntegrations::wallIntegrationFace (surfaceIntegrations.F90:406-881) and the family minimum of Cp of computeCpMinFamily
// (:1363-1437).  One thread per owned face cell of every wall subface (EulerWall, NSWallAdiabatic, NSWallIsoThermal); blockIdx.y = the
// subface in the level's table of wall subfaces, the plane addressed like k_wall_stress (kernels_viscous.hip) through the strides of
// BlkView.  The kernels read what is on the device -- the halos as the last boundary-condition pass left them, tau as the last storing
// evaluation left it -- and write only the buffers of the integration.
//
// Reduction: deterministic, no atomics, the two-pass form of k_ank_unsteady / k_ank_norm_finish (kernels_ank.hip).  Every workgroup
// writes its WI_NQ partial results (the neutral element where it has no faces); k_wallint_finish adds the partials of the subfaces
// of a group in a fixed order.  The maxima (y+) and minima (Cp) go the same way.  Plain HIP: the __shared__ tree of ak_block_sum, one
// quantity after the other through one array, so that the emulator of tests/hostsim runs the same source.
//
// Forward mode (adflow_gpu_wall_integrate_fwd / _bwd; wallIntegrationFace_d, outputForward/surfaceIntegrations_d.f90:1096-1801):
// kernels_ad.hip compiles this source a second time inside namespace adj with `double` standing for the dual number of dual.h.  There
// the state arrays of the block are dual, the stress of a viscous face comes from visc_face on the dual nodal gradients of the wall
// node plane (nothing is stored: the plain tau and the per-face Fp / Fv / area stay as they are), the partial results carry value and
// derivative, and y+ and the minimum of Cp keep a zero derivative as in the reference.  k_wallint_faces_bar is the face kernel of the
// transposed product: the derivative parts of a face's terms contracted with the weights of its groups.
#ifndef ADF_AD_BUILD
#include "internal.h"
#endif

namespace {

// reduce v over the WI_T threads of the workgroup; OP 0: sum, 1: max, 2: min.  Every thread of the workgroup calls it.
template <int OP>
__device__ __forceinline__ double wi_reduce(double v, double* red)
{
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = WI_T / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const double a = red[tid], c = red[tid + s];
            red[tid] = OP == 0 ? a + c : (OP == 1 ? fmax(a, c) : fmin(a, c));
        }
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// the quantity that entry e of a group's output holds: localValues(e + 1) of constants.F90:454-500, entry 63 the minimum of Cp;
// -1: an entry the library does not compute (zero)
__device__ __forceinline__ int wi_quantity_of_entry(int e)
{
    if (e <= 11) return e;                          // iFp, iFv, iMp, iMv
    if (e == 12) return WI_SEP;                     // iSepSensor
    if (e <= 15) return WI_SEPAVG + (e - 13);       // iSepAvg
    if (e == 16) return WI_CAV;                     // iCavitation
    if (e == 17) return WI_YPLUS;                   // iyPlus
    if (e == 44) return WI_AXIS;                    // iAxisMoment
    if (e == 49) return WI_CPMIN_KS;                // iCpMin
    if (e >= 50 && e <= 58) return WI_COF + (e - 50);   // iCoForceX, iCoForceY, iCoForceZ
    if (e == 63) return WI_CPMIN;
    return -1;
}

// The terms v[WI_NQ] of owned face t (of n) of subface f.  PLAIN: the stress of a viscous face is the stored one, and the per-face
// Fp / Fv / area are written.  DUAL (kp given): the stress from visc_face, nothing written.
#ifdef ADF_AD_BUILD
#define WI_KP_PARAM const KParams &kp,
#else
#define WI_KP_PARAM
#endif
__device__ __forceinline__ void wi_face_terms(const BlkView& b, const WiFace& f, const WiPar& P, WI_KP_PARAM long t, long n, double v[WI_NQ])
{
    const int na = f.r[1] - f.r[0] + 1;
    const int a = f.r[0] + (int)(t % na), bb = f.r[2] + (int)(t / na);
    const long nb = b.nbox;
    const long si = 1, sj = b.ldi, sk = b.ldk;
    long cL, sd, s1, s2;
    const adf_real8* sN;
    switch (f.faceID) {
    case ADFLOW_IMIN: case ADFLOW_IMAX:
        cL = b.idx(f.faceID == ADFLOW_IMIN ? 1 : b.il, a, bb); sd = si; s1 = sj; s2 = sk; sN = b.sI;
        break;
    case ADFLOW_JMIN: case ADFLOW_JMAX:
        cL = b.idx(a, f.faceID == ADFLOW_JMIN ? 1 : b.jl, bb); sd = sj; s1 = si; s2 = sk; sN = b.sJ;
        break;
    default:
        cL = b.idx(a, bb, f.faceID == ADFLOW_KMIN ? 1 : b.kl); sd = sk; s1 = si; s2 = sj; sN = b.sK;
    }
    const bool isMin = (f.faceID == ADFLOW_IMIN || f.faceID == ADFLOW_JMIN || f.faceID == ADFLOW_KMIN);
    const double fact = isMin ? -1.0 : 1.0;
    const long c1 = isMin ? cL : cL + sd;       // the halo cell (pp1, ww1, rlv1)
    const long c2 = isMin ? cL + sd : cL;       // the first interior cell (pp2, ww2, rlv2, dd2Wall)
    const double p1 = b.p[c1], p2 = b.p[c2];
    const double ss[3] = {sN[cL], sN[cL + nb], sN[cL + 2 * nb]};
    // centroid of the face: its four nodes in the order the reference adds them
    double xco[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const adf_real8* xd = b.x + d * nb;
        xco[d] = 0.25 * (xd[cL - s1 - s2] + xd[cL - s2] + xd[cL - s1] + xd[cL]);
    }
    const double xc[3] = {xco[0] - P.refPoint[0], xco[1] - P.refPoint[1], xco[2] - P.refPoint[2]};
    const double ra[3] = {xco[0] - P.axisPoint[0], xco[1] - P.axisPoint[1], xco[2] - P.axisPoint[2]};
    const int ib = f.iblank ? (int)f.iblank[t] : 1;
    const double blk = ib > 0 ? (double)ib : 0.0;

    // pressure part (surfaceIntegrations.F90:523-621)
    const double pm1 = fact * (0.5 * (p2 + p1) - P.pInf) * P.pRef;
    double fo[3] = {pm1 * ss[0], pm1 * ss[1], pm1 * ss[2]};
    const double area = sqrt(ss[0] * ss[0] + ss[1] * ss[1] + ss[2] * ss[2]);
#ifndef ADF_AD_BUILD
    double* fpv = f.fpv;
#endif
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        v[WI_FP + d] = fo[d] * blk;
#ifndef ADF_AD_BUILD
        fpv[d * n + t] = fo[d];
#endif
    }
#ifndef ADF_AD_BUILD
    fpv[6 * n + t] = area;
#endif
    v[WI_MP + 0] = (xc[1] * fo[2] - xc[2] * fo[1]) * blk;
    v[WI_MP + 1] = (xc[2] * fo[0] - xc[0] * fo[2]) * blk;
    v[WI_MP + 2] = (xc[0] * fo[1] - xc[1] * fo[0]) * blk;
#pragma unroll
    for (int d = 0; d < 3; ++d)                  // COFSumFx / Fy / Fz: force component d times the centroid
#pragma unroll
        for (int e = 0; e < 3; ++e) v[WI_COF + 3 * d + e] = xco[e] * fo[d] * blk;
    {
        const double m0x = ra[1] * fo[2] - ra[2] * fo[1], m0y = ra[2] * fo[0] - ra[0] * fo[2], m0z = ra[0] * fo[1] - ra[1] * fo[0];
        v[WI_AXIS] = (m0x * P.axisDir[0] + m0y * P.axisDir[1] + m0z * P.axisDir[2]) * blk;
    }

    // separation sensor (:623-677)
    {
        double vel[3] = {b.w[c2 + nb], b.w[c2 + 2 * nb], b.w[c2 + 3 * nb]};
        const double vm = sqrt(vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]) + 1e-16;
#pragma unroll
        for (int d = 0; d < 3; ++d) vel[d] = vel[d] / vm;
        double sensor = -(vel[0] * P.velDir[0] + vel[1] * P.velDir[1] + vel[2] * P.velDir[2]);
        sensor = 1.0 / (1.0 + exp(-2.0 * P.sepSharpness * (sensor - P.sepOffset)));
        sensor = sensor * area * blk;
        v[WI_SEP] = sensor;
#pragma unroll
        for (int d = 0; d < 3; ++d) v[WI_SEPAVG + d] = sensor * xco[d];
    }

    // cavitation sensor and the KS sum of the minimum of Cp (:679-691); the family minimum itself (:1415-1423)
    {
        const double tmp = 2.0 / (P.gammaInf * P.MachCoef * P.MachCoef);
        const double Cp = tmp * (p2 - P.pInf);
        if (ib == 1) v[WI_CPMIN] = Cp;
        if (P.computeCavitation) {
            const double s1c = -Cp - P.cavitationNumber;
            double pw = 1.0;
            for (int m = 0; m < P.cavExponent; ++m) pw *= s1c;
            const double sens = pw / (1.0 + exp(2.0 * P.cavSharpness * (-s1c + P.cavOffset)));
            v[WI_CAV] = sens * area * blk;
            v[WI_CPMIN_KS] = exp(P.cpminRho * (-Cp + P.cpminFamily)) * blk;
        }
    }

    // viscous part (:698-854)
    if (f.tauq) {
#ifdef ADF_AD_BUILD
        double tq[9], acc[5];
        const uint8_t fl = b.flags[cL];
        const int por = (sd == si) ? flg_porI(fl) : (sd == sj ? flg_porJ(fl) : flg_porK(fl));
        visc_face(b, kp, cL, sd, s1, s2, sN, por, 1.0, acc, tq);
        const double txx = tq[0], tyy = tq[1], tzz = tq[2], txy = tq[3], txz = tq[4], tyz = tq[5];
#else
        const double* tq = f.tauq;
        const double txx = tq[t], tyy = tq[n + t], tzz = tq[2 * n + t], txy = tq[3 * n + t], txz = tq[4 * n + t], tyz = tq[5 * n + t];
#endif
        fo[0] = -fact * (txx * ss[0] + txy * ss[1] + txz * ss[2]) * P.pRef;
        fo[1] = -fact * (txy * ss[0] + tyy * ss[1] + tyz * ss[2]) * P.pRef;
        fo[2] = -fact * (txz * ss[0] + tyz * ss[1] + tzz * ss[2]) * P.pRef;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            v[WI_FV + d] = fo[d] * blk;
#ifndef ADF_AD_BUILD
            fpv[(3 + d) * n + t] = fo[d];
#endif
        }
        v[WI_MV + 0] = (xc[1] * fo[2] - xc[2] * fo[1]) * blk;
        v[WI_MV + 1] = (xc[2] * fo[0] - xc[0] * fo[2]) * blk;
        v[WI_MV + 2] = (xc[0] * fo[1] - xc[1] * fo[0]) * blk;
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int e = 0; e < 3; ++e) v[WI_COF + 3 * d + e] += xco[e] * fo[d] * blk;
        const double m0x = ra[1] * fo[2] - ra[2] * fo[1], m0y = ra[2] * fo[0] - ra[0] * fo[2], m0z = ra[0] * fo[1] - ra[1] * fo[0];
        v[WI_AXIS] += (m0x * P.axisDir[0] + m0y * P.axisDir[1] + m0z * P.axisDir[2]) * blk;
        if (P.rans) {
            // y+ from the tangential part of the stress vector (:826-851)
            const long in = (long)(a - f.icBeg) + (long)(bb - f.jcBeg) * f.ldn;
            const double nx = f.norm[in], ny = f.norm[in + f.nnorm], nz = f.norm[in + 2 * f.nnorm];
            double tx = txx * nx + txy * ny + txz * nz;
            double ty = txy * nx + tyy * ny + tyz * nz;
            double tz = txz * nx + tyz * ny + tzz * nz;
            const double fn = tx * nx + ty * ny + tz * nz;
            tx -= fn * nx; ty -= fn * ny; tz -= fn * nz;
            const double rho = 0.5 * (b.w[c2] + b.w[c1]);
            const double mul = 0.5 * (b.rlv[c2] + b.rlv[c1]);
            const double yplus = sqrt(rho * sqrt(tx * tx + ty * ty + tz * tz)) * b.d2wall[c2] / mul;
            v[WI_YPLUS] = yplus * blk;
        }
    } else {
#ifndef ADF_AD_BUILD
#pragma unroll
        for (int d = 0; d < 3; ++d) fpv[(3 + d) * n + t] = 0.0;
#endif
    }
#ifdef ADF_AD_BUILD
    // yplusMax and the minimum of Cp are not differentiated (wallintegrationface_d; cpmin_family is passive)
    v[WI_YPLUS].d = 0.0;
    v[WI_CPMIN].d = 0.0;
#endif
}

// ---- flowIntegrationFace (surfaceIntegrations.F90:894-1200) over the in- and outflow subfaces ---------------------------------------
// where owned face t of subface f lies (the decode of wi_face_terms as a function): (a, bb) its cell in the plane, cL the cell left of the face along the normal (the halo of a min
// face, the first interior cell of a max face), sd the stride along the normal, s1 / s2 those in the plane, sN the face normals, dir
// the direction 0 / 1 / 2
struct WiGeom {
    int a, bb, dir;
    bool isMin;
    long cL, sd, s1, s2;
    const adf_real8* sN;
};
__device__ __forceinline__ WiGeom wi_face_geom(const BlkView& b, const WiFace& f, long t)
{
    WiGeom G;
    const int na = f.r[1] - f.r[0] + 1;
    const int a = f.r[0] + (int)(t % na), bb = f.r[2] + (int)(t / na);
    const long si = 1, sj = b.ldi, sk = b.ldk;
    switch (f.faceID) {
    case ADFLOW_IMIN: case ADFLOW_IMAX:
        G.cL = b.idx(f.faceID == ADFLOW_IMIN ? 1 : b.il, a, bb); G.sd = si; G.s1 = sj; G.s2 = sk; G.sN = b.sI; G.dir = 0;
        break;
    case ADFLOW_JMIN: case ADFLOW_JMAX:
        G.cL = b.idx(a, f.faceID == ADFLOW_JMIN ? 1 : b.jl, bb); G.sd = sj; G.s1 = si; G.s2 = sk; G.sN = b.sJ; G.dir = 1;
        break;
    default:
        G.cL = b.idx(a, bb, f.faceID == ADFLOW_KMIN ? 1 : b.kl); G.sd = sk; G.s1 = si; G.s2 = sj; G.sN = b.sK; G.dir = 2;
    }
    G.a = a; G.bb = bb;
    G.isMin = (f.faceID == ADFLOW_IMIN || f.faceID == ADFLOW_JMIN || f.faceID == ADFLOW_KMIN);
    return G;
}

// the quantity that entry e of a group's output holds (localValues(e + 1)); -1: an entry the flow integration leaves zero
__device__ __forceinline__ int fi_quantity_of_entry(int e)
{
    if (e <= 2) return FI_FP + e;                       // iFp
    if (e == 18) return FI_MASSFLOW;                    // iMassFlow
    if (e == 19) return FI_MASSPTOT;                    // iMassPTot
    if (e == 20) return FI_MASSTTOT;                    // iMassTtot
    if (e == 21) return FI_MASSPS;                      // iMassPs
    if (e >= 22 && e <= 24) return FI_MP + (e - 22);    // iFlowMp
    if (e >= 25 && e <= 27) return FI_FM + (e - 25);    // iFlowFm
    if (e >= 28 && e <= 30) return FI_MM + (e - 28);    // iFlowMm
    if (e == 31) return FI_MASSMN;                      // iMassMN
    if (e == 35) return FI_MASSA;                       // iMassa
    if (e == 36) return FI_MASSRHO;                     // iMassRho
    if (e == 37) return FI_AREA;                        // iArea
    if (e >= 38 && e <= 40) return FI_MASSV + (e - 38); // iMassVx, iMassVy, iMassVz
    if (e >= 41 && e <= 43) return FI_MASSN + (e - 41); // iMassnx, iMassny, iMassnz
    if (e == 47) return FI_AREAPTOT;                    // iAreaPTot
    if (e == 48) return FI_AREAPS;                      // iAreaPs
    if (e >= 50 && e <= 58) return FI_COF + (e - 50);   // iCoForceX, iCoForceY, iCoForceZ
    if (e == 59) return FI_MASSVI;                      // iMassVi
    return -1;
}

// The terms v[FI_NQ] of owned face t of flow subface f, in the order of the reference.  The geometry, the blanking and the signs are
// plain numbers in both builds (adf_real8); what comes from the state is `double`
__device__ __forceinline__ void fi_face_terms(const BlkView& b, const WiFace& f, const FiPar& P, long t, double v[FI_NQ])
{
    const WiGeom G = wi_face_geom(b, f, t);
    const long nb = b.nbox, cL = G.cL;
    const adf_real8 fact = G.isMin ? 1.0 : -1.0;        // positive mass flow INTO the domain: the opposite of the wall forces
    const adf_real8 inFlowFact = f.inflow ? -1.0 : 1.0;
    const long c1 = G.isMin ? cL : cL + G.sd;           // the halo cell (ww1, pp1, gamma1)
    const long c2 = G.isMin ? cL + G.sd : cL;           // the first interior cell
    const adf_real8 ss[3] = {G.sN[cL], G.sN[cL + nb], G.sN[cL + 2 * nb]};
    const adf_real8 sF = b.sFace ? b.sFace[cL + G.dir * nb] : 0.0;      // addGridVelocities: sFaceI / J / K of the boundary face
    const int ib = f.iblank ? (int)f.iblank[t] : 1;
    const adf_real8 blk = ib > 0 ? (adf_real8)ib : 0.0;

    const double vxm = 0.5 * (b.w[c1 + nb] + b.w[c2 + nb]);
    const double vym = 0.5 * (b.w[c1 + 2 * nb] + b.w[c2 + 2 * nb]);
    const double vzm = 0.5 * (b.w[c1 + 3 * nb] + b.w[c2 + 3 * nb]);
    const double rhom = 0.5 * (b.w[c1] + b.w[c2]);
    double pm = 0.5 * (b.p[c1] + b.p[c2]);
    const double gammam = 0.5 * (b.gamma[c1] + b.gamma[c2]);

    const double vnm = vxm * ss[0] + vym * ss[1] + vzm * ss[2] - sF;
    const double vmag = sqrt(vxm * vxm + vym * vym + vzm * vzm) - sF;
    const double am = sqrt(gammam * pm / rhom);
    const double MNm = vmag / am;
    const adf_real8 cellArea = sqrt(ss[0] * ss[0] + ss[1] * ss[1] + ss[2] * ss[2]);
    const adf_real8 overCellArea = 1.0 / cellArea;
    v[FI_AREA] = cellArea * blk;

    // computePtot, computeTtot of flowUtils for constant cp
    const adf_real8 govgm1 = P.gammaInf / (P.gammaInf - 1.0), gm1ovg = 1.0 / govgm1;
    const double kin = 0.5 * (vxm * vxm + vym * vym + vzm * vzm);
    const double Ptot = pm * pow(1.0 + rhom * kin / (govgm1 * pm), govgm1);
    const double Ttot = pm / (rhom * P.RGas) * (1.0 + rhom * kin / (govgm1 * pm));

    const adf_real8 mReDim = sqrt(P.pRef * P.rhoRef);
    double mfl = rhom * vnm * blk * fact * mReDim;      // massFlowRateLocal
    v[FI_MASSFLOW] = mfl;
    pm = pm * P.pRef;
    v[FI_MASSPTOT] = Ptot * mfl * P.pRef;
    v[FI_MASSTTOT] = Ttot * mfl * P.TRef;
    v[FI_MASSRHO] = rhom * mfl * P.rhoRef;
    v[FI_MASSA] = am * mfl * P.uRef;
    v[FI_MASSPS] = pm * mfl;
    v[FI_MASSMN] = MNm * mfl;
    v[FI_AREAPTOT] = Ptot * P.pRef * cellArea * blk;
    v[FI_AREAPS] = pm * cellArea * blk;
    v[FI_MASSV + 0] = (vxm * P.uRef - sF * ss[0] * overCellArea) * mfl;
    v[FI_MASSV + 1] = (vym * P.uRef - sF * ss[1] * overCellArea) * mfl;
    v[FI_MASSV + 2] = (vzm * P.uRef - sF * ss[2] * overCellArea) * mfl;
    {
        const adf_real8 viConst = 2.0 * govgm1 * P.rGasDim;
        const double pratio = fmin(1.0, 1.0 / Ptot);
        const double viLocal = sqrt(viConst * (1.0 - pow(pratio, gm1ovg)) * Ttot * P.TRef);
        v[FI_MASSVI] = viLocal * mfl;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) v[FI_MASSN + d] = ss[d] * overCellArea * mfl;

    // centroid of the face: its four nodes in the order the reference adds them
    adf_real8 xco[3], xc[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const adf_real8* xd = b.x + d * nb;
        xco[d] = 0.25 * (xd[cL - G.s1 - G.s2] + xd[cL - G.s2] + xd[cL - G.s1] + xd[cL]);
        xc[d] = xco[d] - P.refPoint[d];
    }
    // pressure force, with the sign of the wall forces
    pm = -(pm - P.pInf * P.pRef) * fact * blk;
    double fo[3] = {pm * ss[0], pm * ss[1], pm * ss[2]};
#pragma unroll
    for (int d = 0; d < 3; ++d) v[FI_FP + d] = fo[d];
    v[FI_MP + 0] = xc[1] * fo[2] - xc[2] * fo[1];
    v[FI_MP + 1] = xc[2] * fo[0] - xc[0] * fo[2];
    v[FI_MP + 2] = xc[0] * fo[1] - xc[1] * fo[0];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int e = 0; e < 3; ++e) v[FI_COF + 3 * d + e] = xco[e] * fo[d];
    // momentum force: fact is applied again to undo it, the sign flips between in- and outflow and for internal flow
    mfl = mfl * fact / P.timeRef * blk / cellArea * P.internalFlowFact * inFlowFact;
    fo[0] = mfl * ss[0] * vxm;
    fo[1] = mfl * ss[1] * vym;
    fo[2] = mfl * ss[2] * vzm;
#pragma unroll
    for (int d = 0; d < 3; ++d) v[FI_FM + d] = fo[d];
    v[FI_MM + 0] = xc[1] * fo[2] - xc[2] * fo[1];
    v[FI_MM + 1] = xc[2] * fo[0] - xc[0] * fo[2];
    v[FI_MM + 2] = xc[0] * fo[1] - xc[1] * fo[0];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int e = 0; e < 3; ++e) v[FI_COF + 3 * d + e] += xco[e] * fo[d];
}

}  // namespace

// The terms of one face and their sums over the workgroup.  part[q nwg + workgroup], nwg = gridDim.x gridDim.y.
#ifdef ADF_AD_BUILD
#define WI_KP_ARG kp,
__global__ __launch_bounds__(WI_T) void k_wallint_faces(const BlkView* __restrict__ tab, const WiFace* __restrict__ faces, WiPar P,
                                                        KParams kp, double* __restrict__ part)
#else
#define WI_KP_ARG
__global__ __launch_bounds__(WI_T) void k_wallint_faces(const BlkView* __restrict__ tab, const WiFace* __restrict__ faces, WiPar P,
                                                        double* __restrict__ part)
#endif
{
    __shared__ double red[WI_T];
    const WiFace& f = faces[blockIdx.y];
    const BlkView& b = tab[f.slot];
    const int na = f.r[1] - f.r[0] + 1, nbb = f.r[3] - f.r[2] + 1;
    const long n = (na > 0 && nbb > 0) ? (long)na * nbb : 0;
    const long t = (long)blockIdx.x * WI_T + threadIdx.x;
    double v[WI_NQ];
#pragma unroll
    for (int q = 0; q < WI_NQ; ++q) v[q] = 0.0;
    v[WI_CPMIN] = 10000.0;                          // the start value of computeCpMinFamily
    if (t < n) wi_face_terms(b, f, P, WI_KP_ARG t, n, v);
    const long nwg = (long)gridDim.x * gridDim.y;
    const long wg = (long)blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
    for (int q = 0; q < WI_NQ; ++q) {
        const double r = q == WI_YPLUS ? wi_reduce<1>(v[q], red) : (q == WI_CPMIN ? wi_reduce<2>(v[q], red) : wi_reduce<0>(v[q], red));
        if (threadIdx.x == 0) part[q * nwg + wg] = r;
    }
}

// Entry blockIdx.y of group blockIdx.x: thread t takes the workgroups t, t + WI_T, ... of the face kernel in that order (those of the
// subfaces that belong to the group: member[group nface + subface]), then the tree.  gx: workgroups per subface.
// DUAL: the value parts go to out (where given), the derivative parts to outDot
#ifdef ADF_AD_BUILD
__global__ __launch_bounds__(WI_T) void k_wallint_finish(const double* __restrict__ part, const unsigned char* __restrict__ member,
                                                         int nface, int gx, adf_real8* __restrict__ out, adf_real8* __restrict__ outDot)
#else
__global__ __launch_bounds__(WI_T) void k_wallint_finish(const double* __restrict__ part, const unsigned char* __restrict__ member,
                                                         int nface, int gx, double* __restrict__ out)
#endif
{
    __shared__ double red[WI_T];
    const int g = blockIdx.x, e = blockIdx.y;
    const int q = wi_quantity_of_entry(e);
    const long dst = (long)g * ADFLOW_WALLINT_STRIDE + e;
    if (q < 0) {                                     // (the same branch in every thread of the workgroup)
        if (threadIdx.x == 0) {
#ifdef ADF_AD_BUILD
            if (out) out[dst] = 0.0;
            outDot[dst] = 0.0;
#else
            out[dst] = 0.0;
#endif
        }
        return;
    }
    const long nwg = (long)nface * gx;
    const double* pq = part + q * nwg;
    const unsigned char* mem = member + (long)g * nface;
    double s = q == WI_CPMIN ? 10000.0 : 0.0;
    for (long w = threadIdx.x; w < nwg; w += WI_T) {
        if (!mem[w / gx]) continue;
        const double pv = pq[w];
        s = q == WI_YPLUS ? fmax(s, pv) : (q == WI_CPMIN ? fmin(s, pv) : s + pv);
    }
    const double r = q == WI_YPLUS ? wi_reduce<1>(s, red) : (q == WI_CPMIN ? wi_reduce<2>(s, red) : wi_reduce<0>(s, red));
    if (threadIdx.x == 0) {
#ifdef ADF_AD_BUILD
        if (out) out[dst] = r.v;
        outDot[dst] = (q == WI_YPLUS || q == WI_CPMIN) ? 0.0 : r.d;
#else
        out[dst] = r;
#endif
    }
}

#ifdef ADF_AD_BUILD
// The face kernel of the transposed product.  One pass of the coloured sweep has seeded one state variable of the cells of one colour;
// the derivative part of a term of face t is then its derivative with respect to that variable of the ONE cell of the colour its
// stencil holds.  wq[(r nface + subface) WI_NQ + q]: the weight of quantity q of the subface in weight set r (the sum of outBar over the
// groups the subface belongs to); g[r ldg + goff + t]: the contracted derivative of face t, the quantities in their fixed order.
__global__ __launch_bounds__(WI_T) void k_wallint_faces_bar(const BlkView* __restrict__ tab, const WiFace* __restrict__ faces, WiPar P,
                                                            KParams kp, const adf_real8* __restrict__ wq, int nRhs, long ldg,
                                                            adf_real8* __restrict__ g)
{
    const WiFace& f = faces[blockIdx.y];
    const BlkView& b = tab[f.slot];
    const int na = f.r[1] - f.r[0] + 1, nbb = f.r[3] - f.r[2] + 1;
    const long n = (na > 0 && nbb > 0) ? (long)na * nbb : 0;
    const long t = (long)blockIdx.x * WI_T + threadIdx.x;
    if (t >= n) return;
    double v[WI_NQ];
#pragma unroll
    for (int q = 0; q < WI_NQ; ++q) v[q] = 0.0;
    wi_face_terms(b, f, P, kp, t, n, v);
    const int nface = gridDim.y;
    for (int r = 0; r < nRhs; ++r) {
        const adf_real8* w = wq + ((long)r * nface + blockIdx.y) * WI_NQ;
        adf_real8 s = 0.0;
#pragma unroll
        for (int q = 0; q < WI_NQ; ++q) s += w[q] * v[q].d;
        g[r * ldg + f.goff + t] = s;
    }
}

void launch_wallint_fwd(const BlkView* tab, const WiFace* faces, int nface, long maxOwned, const WiPar& P, const KParams& kp, void* part,
                        const unsigned char* member, int nGroups, adf_real8* out, adf_real8* outDot, hipStream_t s)
{
    const int gx = wallint_groups_per_face(maxOwned);
    if (nface > 0)
        hipLaunchKernelGGL(k_wallint_faces, dim3((unsigned)gx, (unsigned)nface, 1), dim3(WI_T, 1, 1), 0, s, tab, faces, P, kp, (double*)part);
    hipLaunchKernelGGL(k_wallint_finish, dim3((unsigned)nGroups, ADFLOW_WALLINT_STRIDE, 1), dim3(WI_T, 1, 1), 0, s, (const double*)part,
                       member, nface, gx, out, outDot);
}

void launch_wallint_bar(const BlkView* tab, const WiFace* faces, int nface, long maxOwned, const WiPar& P, const KParams& kp,
                        const adf_real8* wq, int nRhs, long ldg, adf_real8* g, hipStream_t s)
{
    if (nface <= 0) return;
    hipLaunchKernelGGL(k_wallint_faces_bar, dim3((unsigned)wallint_groups_per_face(maxOwned), (unsigned)nface, 1), dim3(WI_T, 1, 1), 0, s, tab,
                       faces, P, kp, wq, nRhs, ldg, g);
}
#else
// The crediting of the transposed product, one launch per pass (state variable lq of the vectors, colour col of the WI_CM^3 cube):
// a gather per cell, no atomics.  blockIdx.y = subface, the threads run over its box of cells -- WI_REACH beyond its owned faces in
// the plane, the first halo layer and the first three interior layers along the normal: every cell a term of one of its faces can
// depend on through the closures, the boundary conditions of this and of the adjacent faces and the nodal gradients.  The cell of the
// pass's colour takes the contracted derivatives g of the faces whose box holds it -- the faces of every wall subface of its block, in
// the order of the table -- and stores the sum as entry lq of ys in every weight set; a cell in the boxes of several subfaces is
// served by the thread of the first of them.  Halo cells are credited like owned ones: the reverse exchange adds them to their donors.
__global__ __launch_bounds__(WI_T) void k_wallint_credit(const WiFace* __restrict__ faces, int nface, const JmBlk* __restrict__ tab, long nt,
                                                         int nRhs, int lq, int col, const double* __restrict__ g, long ldg)
{
    const WiFace& f = faces[blockIdx.y];
    const JmBlk& b = tab[f.slot];
    const int na = f.r[1] - f.r[0] + 1 + 2 * WI_REACH, nbb = f.r[3] - f.r[2] + 1 + 2 * WI_REACH;
    const long t = (long)blockIdx.x * WI_T + threadIdx.x;
    if (t >= (long)na * nbb * WI_DEPTH) return;
    const int a = f.r[0] - WI_REACH + (int)(t % na), bb = f.r[2] - WI_REACH + (int)((t / na) % nbb), m = (int)(t / ((long)na * nbb));
    int i, j, k;
    switch (f.faceID) {
    case ADFLOW_IMIN: i = 1 + m; j = a; k = bb; break;
    case ADFLOW_IMAX: i = b.il + 1 - m; j = a; k = bb; break;
    case ADFLOW_JMIN: i = a; j = 1 + m; k = bb; break;
    case ADFLOW_JMAX: i = a; j = b.jl + 1 - m; k = bb; break;
    case ADFLOW_KMIN: i = a; j = bb; k = 1 + m; break;
    default: i = a; j = bb; k = b.kl + 1 - m;
    }
    if (i < 0 || i > b.ib || j < 0 || j > b.jb || k < 0 || k > b.kb) return;
    if ((i % WI_CM) + WI_CM * (j % WI_CM) + WI_CM * WI_CM * (k % WI_CM) != col) return;
    double s[ADFLOW_GPU_MAX_NVEC];
    for (int r = 0; r < nRhs; ++r) s[r] = 0.0;
    for (int f2 = 0; f2 < nface; ++f2) {
        const WiFace& h = faces[f2];
        if (h.slot != f.slot) continue;
        int a2, b2, m2;
        switch (h.faceID) {
        case ADFLOW_IMIN: m2 = i - 1; a2 = j; b2 = k; break;
        case ADFLOW_IMAX: m2 = b.il + 1 - i; a2 = j; b2 = k; break;
        case ADFLOW_JMIN: m2 = j - 1; a2 = i; b2 = k; break;
        case ADFLOW_JMAX: m2 = b.jl + 1 - j; a2 = i; b2 = k; break;
        case ADFLOW_KMIN: m2 = k - 1; a2 = i; b2 = j; break;
        default: m2 = b.kl + 1 - k; a2 = i; b2 = j;
        }
        if (m2 < 0 || m2 >= WI_DEPTH || a2 < h.r[0] - WI_REACH || a2 > h.r[1] + WI_REACH || b2 < h.r[2] - WI_REACH ||
            b2 > h.r[3] + WI_REACH)
            continue;
        if (f2 < (int)blockIdx.y) return;              // the thread of that subface serves the cell
        const int na2 = h.r[1] - h.r[0] + 1;
        const int alo = a2 - WI_REACH > h.r[0] ? a2 - WI_REACH : h.r[0], ahi = a2 + WI_REACH < h.r[1] ? a2 + WI_REACH : h.r[1];
        const int blo = b2 - WI_REACH > h.r[2] ? b2 - WI_REACH : h.r[2], bhi = b2 + WI_REACH < h.r[3] ? b2 + WI_REACH : h.r[3];
        for (int q = blo; q <= bhi; ++q)
            for (int p = alo; p <= ahi; ++p) {
                const long fi = h.goff + (p - h.r[0]) + (long)(q - h.r[2]) * na2;
                for (int r = 0; r < nRhs; ++r) s[r] += g[r * ldg + fi];
            }
    }
    const long c = (long)i + (long)j * b.ldi + (long)k * b.ldk;
    for (int r = 0; r < nRhs; ++r) tab[r * nt + f.slot].ys[c + (long)lq * b.nbox] = s[r];
}

void launch_wallint_credit(const WiFace* faces, int nface, long maxBox, const JmBlk* tab, long nt, int nRhs, int lq, int col,
                           const double* g, long ldg, hipStream_t s)
{
    if (nface <= 0) return;
    hipLaunchKernelGGL(k_wallint_credit, dim3((unsigned)((maxBox + WI_T - 1) / WI_T), (unsigned)nface, 1), dim3(WI_T, 1, 1), 0, s, faces,
                       nface, tab, nt, nRhs, lq, col, g, ldg);
}

void launch_wallint(const BlkView* tab, const WiFace* faces, int nface, long maxOwned, const WiPar& P, double* part,
                    const unsigned char* member, int nGroups, double* out, hipStream_t s)
{
    const int gx = wallint_groups_per_face(maxOwned);
    if (nface > 0)
        hipLaunchKernelGGL(k_wallint_faces, dim3((unsigned)gx, (unsigned)nface, 1), dim3(WI_T, 1, 1), 0, s, tab, faces, P, part);
    hipLaunchKernelGGL(k_wallint_finish, dim3((unsigned)nGroups, ADFLOW_WALLINT_STRIDE, 1), dim3(WI_T, 1, 1), 0, s, part, member, nface, gx,
                       out);
}
#endif

// ---- the flow subfaces: the face kernel, the finish kernel and their launches, as above; every quantity is a sum -------------------
__global__ __launch_bounds__(WI_T) void k_flowint_faces(const BlkView* __restrict__ tab, const WiFace* __restrict__ faces, FiPar P,
                                                        double* __restrict__ part)
{
    __shared__ double red[WI_T];
    const WiFace& f = faces[blockIdx.y];
    const BlkView& b = tab[f.slot];
    const int na = f.r[1] - f.r[0] + 1, nbb = f.r[3] - f.r[2] + 1;
    const long n = (na > 0 && nbb > 0) ? (long)na * nbb : 0;
    const long t = (long)blockIdx.x * WI_T + threadIdx.x;
    double v[FI_NQ];
#pragma unroll
    for (int q = 0; q < FI_NQ; ++q) v[q] = 0.0;
    if (t < n) fi_face_terms(b, f, P, t, v);
    const long nwg = (long)gridDim.x * gridDim.y;
    const long wg = (long)blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
    for (int q = 0; q < FI_NQ; ++q) {
        const double r = wi_reduce<0>(v[q], red);
        if (threadIdx.x == 0) part[q * nwg + wg] = r;
    }
}

#ifdef ADF_AD_BUILD
__global__ __launch_bounds__(WI_T) void k_flowint_finish(const double* __restrict__ part, const unsigned char* __restrict__ member,
                                                         int nface, int gx, adf_real8* __restrict__ out, adf_real8* __restrict__ outDot)
#else
__global__ __launch_bounds__(WI_T) void k_flowint_finish(const double* __restrict__ part, const unsigned char* __restrict__ member,
                                                         int nface, int gx, double* __restrict__ out)
#endif
{
    __shared__ double red[WI_T];
    const int g = blockIdx.x, e = blockIdx.y;
    const int q = fi_quantity_of_entry(e);
    const long dst = (long)g * ADFLOW_WALLINT_STRIDE + e;
    double s = 0.0;
    if (q >= 0) {                                    // (the same branch in every thread of the workgroup)
        const long nwg = (long)nface * gx;
        const double* pq = part + q * nwg;
        const unsigned char* mem = member + (long)g * nface;
        for (long w = threadIdx.x; w < nwg; w += WI_T)
            if (mem[w / gx]) s += pq[w];
        s = wi_reduce<0>(s, red);
    }
    if (threadIdx.x == 0) {
#ifdef ADF_AD_BUILD
        if (out) out[dst] = s.v;
        outDot[dst] = s.d;
#else
        out[dst] = s;
#endif
    }
}

#ifdef ADF_AD_BUILD
// the face kernel of the transposed product, as k_wallint_faces_bar: wq[(r nface + subface) FI_NQ + q]
__global__ __launch_bounds__(WI_T) void k_flowint_faces_bar(const BlkView* __restrict__ tab, const WiFace* __restrict__ faces, FiPar P,
                                                            const adf_real8* __restrict__ wq, int nRhs, long ldg, adf_real8* __restrict__ g)
{
    const WiFace& f = faces[blockIdx.y];
    const BlkView& b = tab[f.slot];
    const int na = f.r[1] - f.r[0] + 1, nbb = f.r[3] - f.r[2] + 1;
    const long n = (na > 0 && nbb > 0) ? (long)na * nbb : 0;
    const long t = (long)blockIdx.x * WI_T + threadIdx.x;
    if (t >= n) return;
    double v[FI_NQ];
    fi_face_terms(b, f, P, t, v);
    const int nface = gridDim.y;
    for (int r = 0; r < nRhs; ++r) {
        const adf_real8* w = wq + ((long)r * nface + blockIdx.y) * FI_NQ;
        adf_real8 s = 0.0;
#pragma unroll
        for (int q = 0; q < FI_NQ; ++q) s += w[q] * v[q].d;
        g[r * ldg + f.goff + t] = s;
    }
}

void launch_flowint_fwd(const BlkView* tab, const WiFace* faces, int nface, long maxOwned, const FiPar& P, void* part,
                        const unsigned char* member, int nGroups, adf_real8* out, adf_real8* outDot, hipStream_t s)
{
    const int gx = wallint_groups_per_face(maxOwned);
    if (nface > 0)
        hipLaunchKernelGGL(k_flowint_faces, dim3((unsigned)gx, (unsigned)nface, 1), dim3(WI_T, 1, 1), 0, s, tab, faces, P, (double*)part);
    hipLaunchKernelGGL(k_flowint_finish, dim3((unsigned)nGroups, ADFLOW_WALLINT_STRIDE, 1), dim3(WI_T, 1, 1), 0, s, (const double*)part,
                       member, nface, gx, out, outDot);
}

void launch_flowint_bar(const BlkView* tab, const WiFace* faces, int nface, long maxOwned, const FiPar& P, const adf_real8* wq, int nRhs,
                        long ldg, adf_real8* g, hipStream_t s)
{
    if (nface <= 0) return;
    hipLaunchKernelGGL(k_flowint_faces_bar, dim3((unsigned)wallint_groups_per_face(maxOwned), (unsigned)nface, 1), dim3(WI_T, 1, 1), 0, s, tab,
                       faces, P, wq, nRhs, ldg, g);
}
#else
void launch_flowint(const BlkView* tab, const WiFace* faces, int nface, long maxOwned, const FiPar& P, double* part,
                    const unsigned char* member, int nGroups, double* out, hipStream_t s)
{
    const int gx = wallint_groups_per_face(maxOwned);
    if (nface > 0)
        hipLaunchKernelGGL(k_flowint_faces, dim3((unsigned)gx, (unsigned)nface, 1), dim3(WI_T, 1, 1), 0, s, tab, faces, P, part);
    hipLaunchKernelGGL(k_flowint_finish, dim3((unsigned)nGroups, ADFLOW_WALLINT_STRIDE, 1), dim3(WI_T, 1, 1), 0, s, part, member, nface, gx,
                       out);
}
#endif
#undef WI_KP_PARAM
#undef WI_KP_ARG
