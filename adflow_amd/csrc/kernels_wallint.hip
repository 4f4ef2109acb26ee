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
#include "internal.h"

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

}  // namespace

// The terms of one face and their sums over the workgroup.  part[q nwg + workgroup], nwg = gridDim.x gridDim.y.
__global__ __launch_bounds__(WI_T) void k_wallint_faces(const BlkView* __restrict__ tab, const WiFace* __restrict__ faces, WiPar P,
                                                        double* __restrict__ part)
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
    if (t < n) {
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
        double* fpv = f.fpv;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            v[WI_FP + d] = fo[d] * blk;
            fpv[d * n + t] = fo[d];
        }
        fpv[6 * n + t] = area;
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
            const double* tq = f.tauq;
            const double txx = tq[t], tyy = tq[n + t], tzz = tq[2 * n + t], txy = tq[3 * n + t], txz = tq[4 * n + t], tyz = tq[5 * n + t];
            fo[0] = -fact * (txx * ss[0] + txy * ss[1] + txz * ss[2]) * P.pRef;
            fo[1] = -fact * (txy * ss[0] + tyy * ss[1] + tyz * ss[2]) * P.pRef;
            fo[2] = -fact * (txz * ss[0] + tyz * ss[1] + tzz * ss[2]) * P.pRef;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                v[WI_FV + d] = fo[d] * blk;
                fpv[(3 + d) * n + t] = fo[d];
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
#pragma unroll
            for (int d = 0; d < 3; ++d) fpv[(3 + d) * n + t] = 0.0;
        }
    }
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
__global__ __launch_bounds__(WI_T) void k_wallint_finish(const double* __restrict__ part, const unsigned char* __restrict__ member,
                                                         int nface, int gx, double* __restrict__ out)
{
    __shared__ double red[WI_T];
    const int g = blockIdx.x, e = blockIdx.y;
    const int q = wi_quantity_of_entry(e);
    double* dst = out + (long)g * ADFLOW_WALLINT_STRIDE + e;
    if (q < 0) {                                     // (the same branch in every thread of the workgroup)
        if (threadIdx.x == 0) *dst = 0.0;
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
    if (threadIdx.x == 0) *dst = r;
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
