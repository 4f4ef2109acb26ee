// The dense nState x nState block arithmetic shared by the block ILU kernels (kernels_pc.hip: fill 0; kernels_pc_fill.hip: fill 1, 2).
#pragma once

#define PCE(a, r, c) a[(c) * NS + (r)]

// a <- a^-1 by LU with partial pivoting on [a | 1] and back substitution, in registers (every index is a compile-time constant;
// a row exchange is a conditional swap).  Returns false when a pivot is zero or not finite.
template <int NS>
__device__ __forceinline__ bool pc_invert(double (&a)[NS * NS])
{
    double b[NS * NS];
#pragma unroll
    for (int e = 0; e < NS * NS; ++e) b[e] = (e % (NS + 1) == 0) ? 1.0 : 0.0;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
#pragma unroll
        for (int r = k + 1; r < NS; ++r) {
            const bool sw = fabs(PCE(a, r, k)) > fabs(PCE(a, k, k));
#pragma unroll
            for (int c = k; c < NS; ++c) {
                const double t = PCE(a, k, c), u = PCE(a, r, c);
                PCE(a, k, c) = sw ? u : t;
                PCE(a, r, c) = sw ? t : u;
            }
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                const double t = PCE(b, k, c), u = PCE(b, r, c);
                PCE(b, k, c) = sw ? u : t;
                PCE(b, r, c) = sw ? t : u;
            }
        }
        const double piv = PCE(a, k, k);
        ok = ok && (fabs(piv) > 0.0) && (fabs(piv) <= 1.7976931348623157e308);
#pragma unroll
        for (int r = k + 1; r < NS; ++r) {
            const double f = PCE(a, r, k) / piv;
#pragma unroll
            for (int c = k + 1; c < NS; ++c) PCE(a, r, c) -= f * PCE(a, k, c);
#pragma unroll
            for (int c = 0; c < NS; ++c) PCE(b, r, c) -= f * PCE(b, k, c);
        }
    }
#pragma unroll
    for (int k = NS - 1; k >= 0; --k) {
        const double piv = PCE(a, k, k);
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            double t = PCE(b, k, c);
#pragma unroll
            for (int m = k + 1; m < NS; ++m) t -= PCE(a, k, m) * PCE(b, m, c);
            PCE(b, k, c) = t / piv;
        }
    }
#pragma unroll
    for (int e = 0; e < NS * NS; ++e) a[e] = b[e];
    return ok;
}
