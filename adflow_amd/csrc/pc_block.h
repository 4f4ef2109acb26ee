// The dense nState x nState block arithmetic shared by the block ILU kernels (kernels_pc.hip: fill 0; kernels_pc_fill.hip: fill 1, 2).
#pragma once

#define PCE(a, r, c) a[(c) * NS + (r)]

// b <- a^-1 b by LU with partial pivoting on [a | b] and back substitution, in registers (every index is a compile-time constant;
// a row exchange is a conditional swap); a is destroyed.  Returns false when a pivot is zero or not finite.
template <int NS>
__device__ __forceinline__ bool pc_solve(double (&a)[NS * NS], double (&b)[NS * NS])
{
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
    return ok;
}

// a <- a^-1: pc_solve on [a | 1]
template <int NS>
__device__ __forceinline__ bool pc_invert(double (&a)[NS * NS])
{
    double b[NS * NS];
#pragma unroll
    for (int e = 0; e < NS * NS; ++e) b[e] = (e % (NS + 1) == 0) ? 1.0 : 0.0;
    const bool ok = pc_solve<NS>(a, b);
#pragma unroll
    for (int e = 0; e < NS * NS; ++e) a[e] = b[e];
    return ok;
}

// d <- d - l u, the Schur update of a pivot block: every entry of the product l u is summed on its own and subtracted from d ONCE.
// Subtracting the nState terms from d one by one, d -= l(:, m) u(m, :), is the same sum in another order, and on wall-clustered
// meshes it costs a digit: the factor over the level on `units-clustered-2^10` was 11 / 27 times as far from the extended-precision
// factorisation as a float64 numpy run, 1.9 / 3.7 with this form.  One column of the product is live at a time.
template <int NS>
__device__ __forceinline__ void pc_schur_sub(double (&d)[NS * NS], const double (&l)[NS * NS], const double (&u)[NS * NS])
{
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        double p[NS];
#pragma unroll
        for (int r = 0; r < NS; ++r) p[r] = 0.0;
#pragma unroll
        for (int m = 0; m < NS; ++m)
#pragma unroll
            for (int r = 0; r < NS; ++r) p[r] += PCE(l, r, m) * PCE(u, m, c);
#pragma unroll
        for (int r = 0; r < NS; ++r) PCE(d, r, c) -= p[r];
    }
}

// x <- x d^-1 by a SOLVE with d (d^T y = x^T, pc_solve), not by a product with the explicit inverse: for a pivot block whose inverse
// spans many orders of magnitude (a wall-clustered RANS cell: condition numbers of 1e11) the product x d^-1 loses a digit that the
// solve keeps, and the loss enters every later pivot through the Schur update.  d is left as it is.
template <int NS>
__device__ __forceinline__ void pc_right_solve(const double (&d)[NS * NS], double (&x)[NS * NS])
{
    double at[NS * NS], bt[NS * NS];
#pragma unroll
    for (int r = 0; r < NS; ++r)
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            PCE(at, r, c) = PCE(d, c, r);
            PCE(bt, r, c) = PCE(x, c, r);
        }
    pc_solve<NS>(at, bt);          // (a singular d is reported by the pc_invert that follows in the same thread)
#pragma unroll
    for (int r = 0; r < NS; ++r)
#pragma unroll
        for (int c = 0; c < NS; ++c) PCE(x, c, r) = PCE(bt, r, c);
}
