"""Checks of the block ILU(0) preconditioner (adflow_gpu_pc_setup / _pc_apply) and of adflow_gpu_gmres_solve shared by
tests/test_gpu_pc.py (real MI355X) and tests/test_hostsim_pc.py (the kernel-logic emulator).

The yardstick is a GENERAL incomplete factorisation in numpy: the stencil blocks the library hands out (engine.jacobianBlocks) are
restricted to the columns inside each structured block (PCBJACOBI, one subdomain per block: halo columns, with or without a donor,
are dropped), put into a block-sparse matrix in the natural ordering (i fastest), and factored by IKJ ILU restricted to the pattern
(Saad, Iterative Methods, alg. 10.4) -- nothing here knows that only the diagonal blocks of a 7-point stencil change, so the
comparison also confirms that equivalence.  It runs in float64 and in np.longdouble with the same code; the library's result is
compared with the longdouble one and may be at most 10 x as far from it as the float64 numpy run is."""
import numpy as np

import checks
from device_vectors import dev_call
import jacmult_checks as jm
from adflow_amd import capi
from adflow_amd.params import FlowParams, RANSEquations, dissScalar, upwind, vanAlbeda, minmod

EPS = 2.0 ** -52
MARGIN = 10.0
RANS = FlowParams(equations=RANSEquations, spaceDiscr=upwind, limiter=vanAlbeda)
_REF_BLOCKS = []


# ---- dense LU with partial pivoting in any numpy float type (np.linalg does not take longdouble) ------------------------------
def _lu(A):
    A = A.copy()
    n = A.shape[0]
    perm = np.arange(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            perm[[k, p]] = perm[[p, k]]
        if A[k, k] == 0 or not np.isfinite(A[k, k]):
            raise ZeroDivisionError("singular pivot block")
        A[k + 1:, k] /= A[k, k]
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:])
    return A, perm


def _lu_solve(lu, B):
    """A^-1 B for B of shape (n,) or (n, m)"""
    A, perm = lu
    X = B[perm].copy()
    n = A.shape[0]
    for k in range(1, n):
        X[k] -= A[k, :k] @ X[:k]
    for k in range(n - 1, -1, -1):
        if k < n - 1:
            X[k] -= A[k, k + 1:] @ X[k + 1:]
        X[k] /= A[k, k]
    return X


class NumpyILU0:
    """block Jacobi over the blocks of the level, each subdomain: IKJ ILU(0) on the block-sparse matrix of its in-block columns"""

    def __init__(self, op, dtype):
        self.op, self.dtype, self.ns = op, dtype, op.ns
        self.sub = {}
        for nn, (nx, ny, nz) in op.dims.items():
            rows = []
            Jb = op.J[nn]
            for k in range(nz):
                for j in range(ny):
                    for i in range(nx):
                        row = {}
                        for s in range(op.st.shape[0]):
                            ci, cj, ck = i - op.st[s, 0], j - op.st[s, 1], k - op.st[s, 2]
                            if 0 <= ci < nx and 0 <= cj < ny and 0 <= ck < nz:
                                row[(ck * ny + cj) * nx + ci] = np.array(Jb[i, j, k, :, :, s], dtype=dtype)
                        rows.append(row)
            self.sub[nn] = self._factor(rows)

    @staticmethod
    def _factor(rows):
        n = len(rows)
        lu, luT = [None] * n, [None] * n
        for i in range(n):
            row = rows[i]
            for k in sorted(c for c in row if c < i):
                Lik = _lu_solve(luT[k], row[k].T).T                  # A_ik A_kk^-1
                row[k] = Lik
                for j, Akj in rows[k].items():
                    if j > k and j in row:                           # restricted to the pattern of row i
                        row[j] = row[j] - Lik @ Akj
            lu[i], luT[i] = _lu(row[i]), _lu(row[i].T)
        cols = [[] for _ in range(n)]                                # the same entries by column, for the transposed sweeps
        for i in range(n):
            for c, B in rows[i].items():
                if c != i:
                    cols[c].append((i, B))
        return rows, cols, lu, luT

    def apply(self, r, transpose=False):
        op, ns = self.op, self.ns
        out = np.zeros(op.n, dtype=self.dtype)
        for nn, (rows, cols, lu, luT) in self.sub.items():
            n = len(rows)
            lo = op.off[nn] * ns
            x = np.array(np.asarray(r)[lo:lo + n * ns], dtype=self.dtype).reshape(n, ns)
            if not transpose:                                        # L y = r, U z = y
                for i in range(n):
                    for c, B in rows[i].items():
                        if c < i:
                            x[i] -= B @ x[c]
                for i in range(n - 1, -1, -1):
                    for c, B in rows[i].items():
                        if c > i:
                            x[i] -= B @ x[c]
                    x[i] = _lu_solve(lu[i], x[i])
            else:                                                    # U^T y = r, L^T z = y
                for i in range(n):
                    for c, B in cols[i]:
                        if c < i:                                    # U_ci^T
                            x[i] -= B.T @ x[c]
                    x[i] = _lu_solve(luT[i], x[i])
                for i in range(n - 1, -1, -1):
                    for c, B in cols[i]:
                        if c > i:                                    # L_ci^T
                            x[i] -= B.T @ x[c]
            out[lo:lo + n * ns] = x.reshape(-1)
        return out

    def pivot_conditions(self):
        """largest 2-norm condition number of a pivot block (printed when a comparison fails)"""
        worst = 0.0
        for nn, (rows, cols, lu, luT) in self.sub.items():
            for i in range(len(rows)):
                worst = max(worst, float(np.linalg.cond(np.array(rows[i][i], dtype=np.float64))))
        return worst


def assert_apply_matches(engine, op, seed, what, ilus=None):
    """z = M^-1 r and M^-T r of the library against the longdouble ILU(0): at most MARGIN x the error of the float64 numpy run, in
    the max-norm over the vector.  Returns {transpose: (r, z, error of the float64 run)} and the two factorisations"""
    f64, fld = ilus or (NumpyILU0(op, np.float64), NumpyILU0(op, np.longdouble))
    rng = np.random.default_rng(seed)
    out = {}
    for tr in (False, True):
        r = rng.uniform(-1.0, 1.0, op.n)
        z = engine.pcApply(r, 1, transpose=tr)
        zl = fld.apply(r, tr)
        e_np = float(np.abs(f64.apply(r, tr).astype(np.longdouble) - zl).max())
        e_lib = float(np.abs(z.astype(np.longdouble) - zl).max())
        print(f"{what} transpose={tr}: max|z - z_ld| = {e_lib:.3e}, float64 numpy {e_np:.3e}, ratio {e_lib / max(e_np, 1e-300):.3f}, "
              f"max|z| = {float(np.abs(zl).max()):.3e}")
        if not e_lib <= MARGIN * e_np:
            print(f"largest condition number of a pivot block: {f64.pivot_conditions():.3e}")
        assert e_lib <= MARGIN * e_np, (what, tr, e_lib, e_np)
        assert np.abs(zl).max() > 0.0
        out[tr] = (r, z, e_np)
    return out, (f64, fld)


NDRAW = 16
STATS = []          # one record per (what, transpose[, column]) of assert_apply_median: what the tables of DESIGN §5 are written from


def assert_apply_median(engine, op, seed, what, ilus=None, apply=None):
    """assert_apply_matches over NDRAW = 16 vectors per transpose instead of one draw.  e_lib_i and e_np_i are formed per vector exactly as
    there (max-norm over the vector, against the longdouble yardstick); asserted: median_i(e_lib_i / e_np_i) <= MARGIN, every
    e_np_i > 0, every result finite, max|z_ld| > 0.  The error of the float64 numpy run itself varies by a factor of 4 to 21 from one
    vector to the next, so a single draw can fail on a harmless change of input and can hide half a digit behind a lucky denominator;
    the median of 16 ratios does neither.  Printed and recorded (STATS), not asserted: the largest per-vector ratio,
    max e_lib / max e_np and the spread max e_np / min e_np -- the maxima carry the noise of the single draw.

    apply(R, transpose) -> (NDRAW, n) or (columns, NDRAW, n): how the NDRAW vectors R go through the library (default: pcApply one by
    one); with a leading axis every column is held to the statistic on its own, against the one yardstick run.
    Returns what assert_apply_matches returns, of the first vector of each transpose"""
    f64, fld = ilus or (NumpyILU0(op, np.float64), NumpyILU0(op, np.longdouble))
    rng = np.random.default_rng(seed)
    out = {}
    for tr in (False, True):
        R = rng.uniform(-1.0, 1.0, (NDRAW, op.n))
        Z = np.stack([engine.pcApply(r, 1, transpose=tr) for r in R]) if apply is None else np.asarray(apply(R, tr))
        cols = Z[None] if Z.ndim == 2 else Z
        assert cols.shape[1:] == R.shape, (cols.shape, R.shape)
        zl = [fld.apply(r, tr) for r in R]
        e_np = np.array([float(np.abs(f64.apply(r, tr).astype(np.longdouble) - z).max()) for r, z in zip(R, zl)])
        assert np.isfinite(cols).all() and np.isfinite(e_np).all() and all(np.isfinite(z).all() for z in zl), (what, tr)
        assert (e_np > 0.0).all(), (what, tr, e_np)
        assert all(np.abs(z).max() > 0.0 for z in zl)
        for c, Zc in enumerate(cols):
            e_lib = np.array([float(np.abs(z.astype(np.longdouble) - l).max()) for z, l in zip(Zc, zl)])
            ratio = e_lib / e_np
            rec = dict(what=what, transpose=tr, column=c if Z.ndim == 3 else None, median=float(np.median(ratio)), largest=float(ratio.max()),
                       max_over_max=float(e_lib.max() / e_np.max()), spread=float(e_np.max() / e_np.min()),
                       med_e_lib=float(np.median(e_lib)), med_e_np=float(np.median(e_np)))
            STATS.append(rec)
            print(f"{what} transpose={tr}" + (f" column {c}" if Z.ndim == 3 else "") + f", {NDRAW} vectors: median e_lib / e_np = "
                  f"{rec['median']:.3f} (bar {MARGIN:g}), largest {rec['largest']:.3f}, max e_lib / max e_np = {rec['max_over_max']:.3f}, "
                  f"max e_np / min e_np = {rec['spread']:.2f}; medians {rec['med_e_lib']:.3e} / {rec['med_e_np']:.3e}")
            if not rec["median"] <= MARGIN:
                print(f"largest condition number of a pivot block: {f64.pivot_conditions():.3e}")
            assert rec["median"] <= MARGIN, (what, tr, c, rec)
        out[tr] = (R[0], cols[0][0], float(e_np[0]))
    return out, (f64, fld)


def assert_identity(engine, op, first, seed):
    """<M^-1 r, s> = <r, M^-T s>: exact for the longdouble factorisation, so the two sides differ by the errors of the two
    applications -- each within MARGIN x the float64 run's e, against the 1-norm of the other vector -- and by the rounding of the
    two dot products"""
    rng = np.random.default_rng(seed)
    r, s = first[False][0], first[True][0]
    z, zt = first[False][1], first[True][1]
    lhs, rhs = float(np.dot(z, s)), float(np.dot(r, zt))
    bound = MARGIN * (first[False][2] * np.abs(s).sum() + first[True][2] * np.abs(r).sum()) \
        + op.n * EPS * float(np.dot(np.abs(z), np.abs(s)) + np.dot(np.abs(r), np.abs(zt)))
    print(f"identity: |<M^-1 r, s> - <r, M^-T s>| = {abs(lhs - rhs):.3e} (bound {bound:.3e}, |lhs| = {abs(lhs):.3e})")
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


def single_block(engine, dims, prm, spec, seed=107, **jac):
    """the preconditioner matrix by forward mode on one block with six boundary faces; returns (blk, operator)"""
    mk = {k: jac.pop(k) for k in ("stretch_k", "shape", "lengths") if k in jac}
    blk, rblk, prm = checks.setup_block_with_bc(engine, dims, prm, spec, seed, **mk)
    _REF_BLOCKS[:] = [rblk]          # the reference's flowDoms point into these arrays: alive as long as ref may be called
    engine.setupStateResidualMatrix(1, True, useAD=True, **jac)
    return blk, jm.operator_of(engine, {1: blk})


def check_single(engine, dims, prm, spec, seed=107, median=False, **jac):
    """median: after the comparison on one draw, the same factor under assert_apply_median"""
    blk, op = single_block(engine, dims, prm, spec, seed, **jac)
    engine.pcSetup(1)
    ns, npl, nb = engine.pcInfo()
    assert ns == op.ns and npl == sum(dims) - 2 and nb >= 7 * ns * ns * 8 * op.ncell, (ns, npl, nb)
    first, ilus = assert_apply_matches(engine, op, seed + 1, f"{dims} nState={ns}")
    assert_identity(engine, op, first, seed + 2)
    if median:
        assert_apply_median(engine, op, seed + 3, f"{dims} nState={ns}", ilus=ilus)
    return blk, op, first, ilus


def check_brick(engine, topo, prm, seed=223):
    """several blocks with interfaces: the couplings across blocks are absent from M"""
    blocks, op = jm.brick_operator(engine, topo, prm, seed)
    engine.pcSetup(1)
    assert engine.pcInfo()[1] == max(sum(d) - 2 for d in op.dims.values())
    first, _ = assert_apply_matches(engine, op, seed + 1, f"{len(blocks)} blocks")
    assert_identity(engine, op, first, seed + 2)
    rng = np.random.default_rng(seed + 3)
    for nn in sorted(op.dims)[:2]:
        lo, hi = op.off[nn] * op.ns, (op.off[nn] + int(np.prod(op.dims[nn]))) * op.ns
        for tr in (False, True):
            r = np.zeros(op.n)
            r[lo:hi] = rng.uniform(-1.0, 1.0, hi - lo)
            z = engine.pcApply(r, 1, transpose=tr)
            assert np.abs(z[lo:hi]).max() > 0.0
            assert not z[:lo].any() and not z[hi:].any(), ("M^-1 couples blocks", nn, tr)
    # the matrix itself does couple them: the product of the same vector is non-zero on other blocks
    y = engine.jacobianMult(r, 1)
    assert np.abs(np.concatenate([y[:lo], y[hi:]])).max() > 0.0


def check_persistence(engine, dims=(7, 5, 4)):
    """the factor owns its data: bit-equal z after the exact matrix replaced the preconditioner matrix on the device; released once;
    bit-equal again after a new setup"""
    blk, op = single_block(engine, dims, RANS, jm.WALL, 107, stretch_k=2.0)
    engine.pcSetup(1)
    rng = np.random.default_rng(271)
    r = rng.uniform(-1.0, 1.0, op.n)
    z = {tr: engine.pcApply(r, 1, transpose=tr) for tr in (False, True)}
    engine.setupStateResidualMatrix(1, False, useAD=True)                 # the 33-point matrix of the adjoint
    assert engine.jacobianInfo()[1].shape[0] == 33
    ws = engine.releaseWorkspace()
    for tr in (False, True):
        assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z[tr]), ("after the exact assembly", tr)
    assert ws > 0 and engine.releaseWorkspace() == 0                       # the work space call neither frees nor counts the factor
    for tr in (False, True):
        assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z[tr]), ("after release_workspace", tr)
    nbytes = engine.pcRelease()
    assert nbytes >= 7 * op.ns ** 2 * 8 * op.ncell, nbytes
    assert engine.pcRelease() == 0
    with __import__("pytest").raises(capi.AdflowGpuError, match="no factor"):
        engine.pcApply(r, 1)
    engine.setupStateResidualMatrix(1, True, useAD=True)
    engine.pcSetup(1)
    for tr in (False, True):
        assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z[tr]), ("after a new setup", tr)
    engine.pcRelease()


def check_refusals_and_side_effects(engine, dims=(7, 6, 5)):
    """every error with its message; state, residual and matrix untouched by every new call"""
    import ctypes
    import pytest
    lib = engine.lib
    engine.release_all()
    with pytest.raises(capi.AdflowGpuError, match="no assembled Jacobian"):
        engine.pcSetup(1)
    with pytest.raises(capi.AdflowGpuError, match="no factor"):
        engine.pcInfo()
    assert engine.pcRelease() == 0
    checks.setup_block_with_bc(engine, dims, FlowParams(spaceDiscr=dissScalar), jm.EULER, 227)
    engine.setupStateResidualMatrix(1, False, delta=1e-6)
    with pytest.raises(capi.AdflowGpuError, match="13-point stencil"):
        engine.pcSetup(1)
    rm = RANS.replace(limiter=minmod)
    blk, _, prm = checks.setup_block_with_bc(engine, dims, rm, jm.WALL, 227, stretch_k=2.0)
    ncell = int(np.prod(dims))
    x = np.random.default_rng(229).uniform(-1.0, 1.0, 6 * ncell)
    with pytest.raises(capi.AdflowGpuError, match="no factor"):
        engine.pcApply(x, 1)
    for kw, npts in ((dict(usePC=False), 33), (dict(usePC=True, viscPC=True), 27)):
        engine.setupStateResidualMatrix(1, delta=1e-6, **kw)
        assert engine.jacobianInfo()[1].shape[0] == npts
        with pytest.raises(capi.AdflowGpuError, match=f"{npts}-point stencil"):
            engine.pcSetup(1)
    engine.setupStateResidualMatrix(1, True, delta=1e-6)
    with pytest.raises(capi.AdflowGpuError, match="not the level of the assembly"):
        engine.pcSetup(2)
    engine.download_state(1, 1)
    w0, dw0, J0 = blk["w"].copy(), engine.download_residual(1, 1).copy(), engine.jacobianBlocks(1).copy()
    engine.pcSetup(1)
    z = engine.pcApply(x, 1)
    assert np.array_equal(engine.pcApply(x, 1), z)
    out = np.zeros_like(x)
    for args, msg in (((2, 0, x.ctypes.data, out.ctypes.data, x.size), "not the level of the factor"),
                      ((1, 0, None, out.ctypes.data, x.size), "is NULL"),
                      ((1, 1, x.ctypes.data, None, x.size), "is NULL"),
                      ((1, 0, x.ctypes.data, x.ctypes.data, x.size), "same vector"),
                      ((1, 1, x.ctypes.data, out.ctypes.data, x.size + 6), "rows"),
                      ((1, 0, x.ctypes.data, out.ctypes.data, 5 * ncell), "rows")):
        for fn in (lib.adflow_gpu_pc_apply, lib.adflow_gpu_pc_apply_dev):
            assert fn(*args) != 0, msg
            assert msg in lib.adflow_gpu_last_error().decode(), (msg, lib.adflow_gpu_last_error().decode())
    xs, its, r0, rn = engine.gmresSolve(x, 1, restart=30, maxIts=30, rtol=1e-6)
    assert 0 < its <= 30 and rn <= 2e-6 * r0
    with pytest.raises(capi.AdflowGpuError, match="same vector"):
        engine._chk(lib.adflow_gpu_gmres_solve(1, 0, x.ctypes.data, x.ctypes.data, x.size, 10, 10, 1e-6, 0.0, 0, None, None, None))
    with pytest.raises(capi.AdflowGpuError, match="rows"):
        engine._chk(lib.adflow_gpu_gmres_solve(1, 0, x.ctypes.data, out.ctypes.data, x.size - 6, 10, 10, 1e-6, 0.0, 0, None, None, None))
    engine.download_state(1, 1)
    assert np.array_equal(blk["w"], w0) and np.array_equal(engine.download_residual(1, 1), dw0)
    assert np.array_equal(engine.jacobianBlocks(1), J0)
    # the matrix changes its nState under the factor: the solver refuses, the factor still applies
    engine.setupStateResidualMatrix(1, True, frozenTurb=True, delta=1e-6)
    with pytest.raises(capi.AdflowGpuError, match="nState"):
        engine.gmresSolve(x, 1)
    with pytest.raises(capi.AdflowGpuError, match="nState"):
        engine.gmresSolve(x[:5 * ncell], 1)
    assert np.array_equal(engine.pcApply(x, 1), z)
    # a state that is not finite in one cell gives pivot blocks that are not finite: setup fails, names the block, keeps nothing
    engine.download_state(1, 1)
    w = blk["w"].copy(order="F")
    blk["w"][4, 3, 3, 0] = np.nan
    engine.upload_state(1, 1)
    engine.setupStateResidualMatrix(1, True, delta=1e-6)
    with pytest.raises(capi.AdflowGpuError, match=r"pivot block of cell \(\d+,\d+,\d+\) of block 1"):
        engine.pcSetup(1)
    with pytest.raises(capi.AdflowGpuError, match="no factor"):
        engine.pcApply(x, 1)
    assert engine.pcRelease() == 0
    blk["w"][...] = w
    engine.release_all()


# ---- GMRES -------------------------------------------------------------------------------------------------------------------
def scipy_gmres_iterations(A, ilu, b, transpose, rtol, restart, maxiter):
    """scipy's own GMRES on A M^-1 (the numpy ILU(0) as RIGHT preconditioner): the iterations it takes to rtol ||b||"""
    import scipy.sparse.linalg as sla
    n = b.size
    count = [0]
    AM = sla.LinearOperator((n, n), matvec=lambda v: A(np.asarray(ilu.apply(v, transpose), dtype=np.float64)), dtype=np.float64)

    def cb(_):
        count[0] += 1
    u, info = sla.gmres(AM, b, rtol=rtol, atol=0.0, restart=restart, maxiter=maxiter, callback=cb, callback_type="pr_norm")
    assert info == 0, ("scipy's gmres did not converge", info, count[0])
    return count[0]


def check_gmres_on_pc_matrix(engine, dims, cap, restart, seed=281):
    """(a) operator = the preconditioner matrix itself, both transposes: the true residual recomputed in numpy from the downloaded
    blocks is <= 2 rtol ||b|| at rtol = 1e-8; the iteration count is within `cap`, a number fixed beforehand from scipy's gmres with
    the numpy ILU(0) on the same inputs (asserted here as well: at least a factor 2 to spare); a converged x as guess: 0 iterations"""
    rtol = 1e-8
    blk, op = single_block(engine, dims, RANS, jm.WALL, 107, stretch_k=2.0)
    engine.pcSetup(1)
    f64 = NumpyILU0(op, np.float64)
    rng = np.random.default_rng(seed)
    for tr in (False, True):
        b = rng.uniform(-1.0, 1.0, op.n)
        k_ref = scipy_gmres_iterations(lambda v: op.apply(v, tr), f64, b, tr, rtol, restart, cap)
        x, its, r0, rn = engine.gmresSolve(b, 1, transpose=tr, restart=restart, maxIts=cap, rtol=rtol)
        true = float(np.linalg.norm(b - op.apply(x, tr)))
        nb = float(np.linalg.norm(b))
        print(f"gmres on the PC matrix {dims} transpose={tr}: {its} iterations (scipy {k_ref}, cap {cap}), ||b - A x|| / ||b|| = "
              f"{true / nb:.3e} (reported {rn / nb:.3e})")
        assert 2 * k_ref <= cap, ("the cap leaves no factor 2 over scipy's count", k_ref, cap)
        assert 0 < its <= cap, (its, cap)
        assert abs(r0 - nb) <= 1e-12 * nb
        assert true <= 2 * rtol * nb, (true, nb)
        assert abs(rn - true) <= 1e-3 * rtol * nb + 1e-6 * true
        # the converged x as initial guess, at the level (a) grants the true residual
        x2, its2, r02, rn2 = engine.gmresSolve(b, 1, transpose=tr, restart=restart, maxIts=cap, rtol=2 * rtol, x0=x)
        assert its2 == 0 and np.array_equal(x2, x), its2
        # an iteration limit is not an error
        x3, its3, _, rn3 = engine.gmresSolve(b, 1, transpose=tr, restart=2, maxIts=3, rtol=rtol)
        assert its3 == 3 and rn3 > rtol * nb


def assert_apply_dev_twin(engine, dv, n, seed, what):
    """adflow_gpu_pc_apply_dev on device vectors against adflow_gpu_pc_apply with the factor that stands, bit for bit"""
    rng = np.random.default_rng(seed)
    for tr in (False, True):
        r = rng.uniform(-1.0, 1.0, n)
        z = engine.pcApply(r, 1, transpose=tr)
        dr, dz = dv.put(r), dv.empty(n)
        dev_call(engine, dv, engine.pcApplyDev, dv.ptr(dr), dv.ptr(dz), n, 1, tr)
        assert np.abs(z).max() > 0.0
        assert np.array_equal(dv.get(dz), z), (what, tr)
        assert np.array_equal(dv.get(dr), r), (what, tr, "the right-hand side was written")


def check_dev_twins(engine, dv, topo, dims, cap, seed=293):
    """the _dev entries on device vectors (dv: device_vectors.HostVectors / TorchVectors) return bit for bit what their host twins return:
    pc_apply at fill 0 on the blocks of `topo` (sets of unequal length in one launch), both transposes; gmres_solve on one
    wall-bounded RANS block, both transposes, from zero and from a guess: x, its, rnorm0 and rnorm"""
    blocks, op = jm.brick_operator(engine, topo, FlowParams(spaceDiscr=upwind), seed)
    engine.pcSetup(1)
    assert engine.pcInfo2()[0] == 0
    assert_apply_dev_twin(engine, dv, op.n, seed + 1, f"{len(blocks)} blocks, fill 0")
    engine.pcRelease()
    blk, op = single_block(engine, dims, RANS, jm.WALL, 107, stretch_k=2.0)
    engine.pcSetup(1)
    rng = np.random.default_rng(seed + 2)
    for tr in (False, True):
        b = rng.uniform(-1.0, 1.0, op.n)
        db = dv.put(b)
        kw = dict(transpose=tr, restart=cap, maxIts=cap, rtol=1e-8)
        x, *host = engine.gmresSolve(b, 1, **kw)
        dx = dv.put(np.full(op.n, 7.0))                                 # without a guess whatever x holds is not read
        dev = dev_call(engine, dv, engine.gmresSolveDev, dv.ptr(db), dv.ptr(dx), op.n, 1, **kw)
        print(f"gmres_solve / _dev {dims} transpose={tr}: (its, rnorm0, rnorm) = {tuple(host)} / {dev}")
        assert 0 < host[0] <= cap
        assert tuple(host) == dev and np.array_equal(dv.get(dx), x), ("from zero", tr)
        # a guess three iterations old: uploaded by the host form, read in place by the _dev form
        x3, its3, _, _ = engine.gmresSolve(b, 1, transpose=tr, restart=2, maxIts=3, rtol=1e-8)
        assert its3 == 3
        x, *host = engine.gmresSolve(b, 1, x0=x3, **kw)
        dx = dv.put(x3)
        dev = dev_call(engine, dv, engine.gmresSolveDev, dv.ptr(db), dv.ptr(dx), op.n, 1, useGuess=True, **kw)
        assert host[0] > 0 and tuple(host) == dev and np.array_equal(dv.get(dx), x), ("from a guess", tr)
        assert np.array_equal(dv.get(db), b)
    engine.pcRelease()
    engine.releaseWorkspace()


def check_gmres_adjoint_order(engine, dims, cap, seed=283):
    """(b) the adjoint's order of calls on a wall-bounded RANS block: factor of the preconditioner matrix, then the exact 33-point
    matrix, transpose = 1, restart >= cap.  x against scipy's spsolve on the matrix of the REFERENCE's blocks, within the assembly's
    1e-10 max|J_ref| per entry propagated through the solve:
        ||x - x_ref|| <= (rtol ||b|| + 1e-10 max|J_ref| nStencil nState ||x_ref||_inf sqrt(n)) / sigma_min"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as sla
    from oracle import ref
    rtol = 1e-8
    blk, opc = single_block(engine, dims, RANS, jm.WALL, 107, stretch_k=2.0)
    engine.pcSetup(1)
    f64 = NumpyILU0(opc, np.float64)
    Jr = ref.ad_jacobian(blk.nx, blk.ny, blk.nz, False, False, False, False)
    engine.setupStateResidualMatrix(1, False, useAD=True)
    ns, st = engine.jacobianInfo()
    d = {1: (blk.nx, blk.ny, blk.nz)}
    opr = jm.LevelOperator({1: Jr}, d, st)
    n = opr.n
    # the reference matrix, transposed, column by column through the numpy operator
    AT = sp.csc_matrix(np.column_stack([opr.apply(e, True) for e in np.eye(n)]))
    rng = np.random.default_rng(seed)
    b = rng.uniform(-1.0, 1.0, n)
    x_ref = sla.spsolve(AT, b)
    smin = float(np.linalg.svd(AT.toarray(), compute_uv=False)[-1])
    k_ref = scipy_gmres_iterations(lambda v: AT @ v, f64, b, True, rtol, cap, cap)
    x, its, r0, rn = engine.gmresSolve(b, 1, transpose=True, restart=cap, maxIts=cap, rtol=rtol)
    nb = float(np.linalg.norm(b))
    bound = (rtol * nb + 1e-10 * np.abs(Jr).max() * st.shape[0] * ns * np.abs(x_ref).max() * np.sqrt(n)) / smin
    err = float(np.linalg.norm(x - x_ref))
    print(f"adjoint order {dims}: {its} iterations (scipy {k_ref}, cap {cap}), ||x - x_ref|| = {err:.3e} (bound {bound:.3e}), "
          f"sigma_min = {smin:.3e}, reported ||r|| / ||b|| = {rn / nb:.3e}")
    assert 2 * k_ref <= cap, ("the cap leaves no factor 2 over scipy's count", k_ref, cap)
    assert 0 < its <= cap, (its, cap)
    assert err <= bound, (err, bound)
    x2, its2, _, _ = engine.gmresSolve(b, 1, transpose=True, restart=cap, maxIts=cap, rtol=2 * rtol, x0=x)
    assert its2 == 0 and np.array_equal(x2, x), its2
    engine.pcRelease()
