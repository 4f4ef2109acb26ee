"""Checks of the multi-vector entries adflow_gpu_jacobian_mult_multi, _pc_apply_multi and _gmres_solve_multi shared by
tests/test_gpu_multi.py (real MI355X) and tests/test_hostsim_multi.py (the kernel-logic emulator).

Nothing new is measured against: every column of a multi call is held to the yardstick its single entry is held to -- the rounding
bound of jacmult_checks.assert_products_to_rounding for the product, MARGIN x the float64 numpy error against the longdouble
factorisation (pc_checks / pc_fill_checks) for the sweeps -- with the numpy operator and the numpy ILU classes reused as they are,
each reference computed once per case and shared by every width.  On top of that: one column is the single entry to the bit, a
column does not depend on its neighbours, and a column of the solver stops where its own single solve stops."""
import numpy as np

import ank_checks as ank
import checks
import jacmult_checks as jm
import pc_checks as pc
import pc_fill_checks as pcf
from device_vectors import dev_call
from jacmult_checks import operator_of, brick_operator        # noqa: F401  (the numpy operator of every case)
from pc_checks import NumpyILU0, single_block, MARGIN, EPS
from adflow_amd import capi
from adflow_amd.params import FlowParams, dissScalar, upwind, minmod

assert pcf.pc.MARGIN == MARGIN and jm.EPS == EPS
NVEC_PRODUCT = (2, 3, 4, 7)           # 7 = 4 + 3: two groups
NVEC_SWEEP = (2, 3, 4, 5)             # 5 = 4 + 1: the rest runs the kernels of one vector


def ilus_of(op, fill):
    return (NumpyILU0(op, np.float64), NumpyILU0(op, np.longdouble)) if fill == 0 else pcf.yardsticks(op, fill)


# ---- 1. the product ----------------------------------------------------------------------------------------------------------
def assert_products(engine, op, seed, what, nvecs=NVEC_PRODUCT):
    """every column of every width within jm.assert_products_to_rounding's bound  2 n eps (|B| |x|), n = nStencil nState, entry by
    entry, against the numpy operator of the downloaded blocks; the references of the widest call serve the narrower ones"""
    rng = np.random.default_rng(seed)
    nn = op.st.shape[0] * op.ns
    for tr in (False, True):
        X = rng.uniform(-1.0, 1.0, (max(nvecs), op.n))
        ref = [op.apply(x, tr) for x in X]
        bound = [2 * nn * EPS * op.apply(x, tr, absolute=True) for x in X]
        assert all(np.abs(r).max() > 0.0 for r in ref)
        for nvec in nvecs:
            Y = engine.jacobianMultMulti(X[:nvec], 1, transpose=tr)
            worst = max(float((np.abs(Y[c] - ref[c]) / np.maximum(bound[c], 1e-300)).max()) for c in range(nvec))
            print(f"{what} transpose={tr} nvec={nvec}: largest err / bound over the columns = {worst:.3f}")
            for c in range(nvec):
                assert (np.abs(Y[c] - ref[c]) <= bound[c]).all(), (what, tr, nvec, c)


def rans_exact_operator(engine, dims, seed=211):
    """one wall-bounded RANS block with six boundary faces and the exact forward-mode matrix: the widest (33-point) stencil"""
    blk, rblk, _ = checks.setup_block_with_bc(engine, dims, pc.RANS, jm.WALL, seed, stretch_k=2.0)
    pc._REF_BLOCKS[:] = [rblk]
    engine.setupStateResidualMatrix(1, False, useAD=True)
    assert engine.jacobianInfo()[1].shape[0] == 33
    return operator_of(engine, {1: blk})


def euler_jst_operator(engine, dims, seed=227):
    """the Euler scalar-JST preconditioner matrix (7-point, nState 5)"""
    blk, rblk, _ = checks.setup_block_with_bc(engine, dims, FlowParams(spaceDiscr=dissScalar), jm.EULER, seed)
    pc._REF_BLOCKS[:] = [rblk]
    engine.setupStateResidualMatrix(1, True, delta=1e-6)
    assert engine.jacobianInfo()[1].shape[0] == 7
    return operator_of(engine, {1: blk})


def check_padding_untouched(engine, op, seed, nvec=3, pad=5):
    """ld = n + 5: the doubles between the columns keep their sentinel in the result and the input is not written; the columns are
    what ld = n gives, bit for bit.  Product and application"""
    rng = np.random.default_rng(seed)
    n, ld, sentinel = op.n, op.n + pad, -7.25e300
    X = np.full(nvec * ld, sentinel)
    for c in range(nvec):
        X[c * ld:c * ld + n] = rng.uniform(-1.0, 1.0, n)
    cols = np.stack([X[c * ld:c * ld + n] for c in range(nvec)])
    X0 = X.copy()
    entries = [(engine.lib.adflow_gpu_jacobian_mult_multi, engine.jacobianMultMulti)]
    try:
        engine.pcInfo()
        entries.append((engine.lib.adflow_gpu_pc_apply_multi, engine.pcApplyMulti))
    except capi.AdflowGpuError:
        pass
    for fn, tight in entries:
        for tr in (0, 1):
            Y = np.full(nvec * ld, sentinel)
            engine._chk(fn(1, tr, nvec, X.ctypes.data, ld, Y.ctypes.data, ld, n))
            want = tight(cols, 1, transpose=bool(tr))
            for c in range(nvec):
                assert np.array_equal(Y[c * ld:c * ld + n], want[c]), (fn.__name__, tr, c)
                assert (Y[c * ld + n:(c + 1) * ld] == sentinel).all(), (fn.__name__, tr, c, "padding written")
            assert np.array_equal(X, X0), "the input was written"


def check_adjoint_identity_across_columns(engine, op, seed):
    """<J X_a, S_b> = <X_a, J^T S_b> for a != b, within jm.check_brick's bound 4 N eps <|J| |X_a|, |S_b|>"""
    rng = np.random.default_rng(seed)
    X, S = rng.uniform(-1.0, 1.0, (2, op.n)), rng.uniform(-1.0, 1.0, (2, op.n))
    JX, JTS = engine.jacobianMultMulti(X, 1), engine.jacobianMultMulti(S, 1, transpose=True)
    for a, b in ((0, 1), (1, 0)):
        lhs, rhs = float(np.dot(JX[a], S[b])), float(np.dot(X[a], JTS[b]))
        bound = 4 * op.n * EPS * float(np.dot(op.apply(X[a], absolute=True), np.abs(S[b])))
        print(f"adjoint identity columns ({a}, {b}): |<J X_a, S_b> - <X_a, J^T S_b>| = {abs(lhs - rhs):.3e} (bound {bound:.3e})")
        assert abs(lhs - rhs) <= bound, (a, b, lhs, rhs, bound)


def check_product_cases(engine, dims_rans, dims_euler, dims_turb, brick, ell):
    assert_products(engine, rans_exact_operator(engine, dims_rans), 401, f"RANS exact {dims_rans}")
    op = euler_jst_operator(engine, dims_euler)
    assert_products(engine, op, 403, f"Euler JST PC {dims_euler}")
    check_padding_untouched(engine, op, 405)
    rm = pc.RANS.replace(limiter=minmod)
    for jac in (dict(frozenTurb=True), dict(useTurbOnly=True)):
        _, op = single_block(engine, dims_turb, rm, jm.WALL, stretch_k=2.0, **jac)
        assert_products(engine, op, 407, f"{dims_turb} {jac}")
    _, op = brick_operator(engine, brick, FlowParams(spaceDiscr=dissScalar))
    assert_products(engine, op, 409, "periodic brick")
    check_adjoint_identity_across_columns(engine, op, 411)
    _, op = brick_operator(engine, ell, FlowParams(spaceDiscr=upwind), seed=251)
    assert_products(engine, op, 413, "rotated interfaces")
    check_adjoint_identity_across_columns(engine, op, 415)
    engine.releaseWorkspace()


# ---- 2. the sweeps -----------------------------------------------------------------------------------------------------------
def assert_sweeps(engine, op, fill, seed, what, nvecs=NVEC_SWEEP, ilus=None):
    """the factor that stands: every column of every width within MARGIN x the float64 numpy error against the longdouble
    factorisation, in the max-norm (the yardstick of pc.assert_apply_matches).  Returns {transpose: (R, longdouble Z, float64 errors)}"""
    f64, fld = ilus or ilus_of(op, fill)
    rng = np.random.default_rng(seed)
    out = {}
    for tr in (False, True):
        R = rng.uniform(-1.0, 1.0, (max(nvecs), op.n))
        zl = [fld.apply(r, tr) for r in R]
        e_np = [float(np.abs(f64.apply(r, tr).astype(np.longdouble) - z).max()) for r, z in zip(R, zl)]
        for nvec in nvecs:
            Z = engine.pcApplyMulti(R[:nvec], 1, transpose=tr)
            e_lib = [float(np.abs(Z[c].astype(np.longdouble) - zl[c]).max()) for c in range(nvec)]
            print(f"{what} fill {fill} transpose={tr} nvec={nvec}: e_lib / e_np per column = "
                  + ", ".join(f"{a / max(b, 1e-300):.3f}" for a, b in zip(e_lib, e_np)))
            for c in range(nvec):
                assert e_lib[c] <= MARGIN * e_np[c], (what, fill, tr, nvec, c, e_lib[c], e_np[c])
                assert np.abs(zl[c]).max() > 0.0
        out[tr] = (R, zl, e_np)
    return out


def check_sweeps_every_lane(engine, op, fill, seed, what, nvec=3):
    """a large case whose numpy yardstick is paid for ONE column: that column is put into each of the nvec positions of a call in
    turn (the others random), and in every position it is held to MARGIN x the float64 numpy error against the longdouble
    factorisation -- every vector lane of the kernel is checked against the yardstick at the cost of one column"""
    f64, fld = ilus_of(op, fill)
    rng = np.random.default_rng(seed)
    for tr in (False, True):
        R = rng.uniform(-1.0, 1.0, (nvec, op.n))
        zl = fld.apply(R[0], tr)
        e_np = float(np.abs(f64.apply(R[0], tr).astype(np.longdouble) - zl).max())
        assert np.abs(zl).max() > 0.0
        for pos in range(nvec):
            Z = engine.pcApplyMulti(np.roll(R, pos, axis=0), 1, transpose=tr)
            e_lib = float(np.abs(Z[pos].astype(np.longdouble) - zl).max())
            print(f"{what} fill {fill} transpose={tr} nvec={nvec}, position {pos}: e_lib / e_np = {e_lib / max(e_np, 1e-300):.3f}")
            assert e_lib <= MARGIN * e_np, (what, fill, tr, pos, e_lib, e_np)


def check_sweeps_all_fills(engine, op, seed, what, nvecs=NVEC_SWEEP, fills=(0, 1, 2)):
    for fill in fills:
        with pcf.fill_of(engine, fill):
            engine.pcSetup(1)
            assert engine.pcInfo2()[0] == fill
            assert_sweeps(engine, op, fill, seed + fill, what, nvecs)
            engine.pcRelease()


def check_sweeps_median(engine, dims, prm, spec, seed=107, nvec=3, fills=(0, 1), **jac):
    """pcApplyMulti with nvec columns on one block with six boundary faces, every column position held to pc.assert_apply_median: its 16
    vectors go through in 16 calls of nvec columns, call g carrying the vectors g, g + 1, .. (cyclically), so that every vector passes
    every column position once and the yardstick is run once per vector.  Column 0 of an nvec = 1 call is pcApply to the bit"""
    _, op = single_block(engine, dims, prm, spec, seed, **jac)

    def apply(R, transpose):
        K = len(R)
        Z = np.empty((nvec,) + R.shape)
        for g in range(K):
            idx = [(g + c) % K for c in range(nvec)]
            Zg = engine.pcApplyMulti(R[idx], 1, transpose=transpose)
            for c in range(nvec):
                Z[c, idx[c]] = Zg[c]
        return Z

    for fill in fills:
        with pcf.fill_of(engine, fill):
            engine.pcSetup(1)
            assert engine.pcInfo2()[0] == fill
            first, _ = pc.assert_apply_median(engine, op, seed + 1 + fill, f"{dims} {nvec} columns fill {fill}", ilus=ilus_of(op, fill),
                                              apply=apply)
            for tr in (False, True):
                r = first[tr][0]
                assert np.array_equal(engine.pcApplyMulti(r[None], 1, transpose=tr)[0], engine.pcApply(r, 1, transpose=tr)), (fill, tr)
            engine.pcRelease()


def check_blocks_stay_subdomains(engine, op, fill, seed):
    """column a is non-zero on block a only: it comes back zero on every other block, and non-zero on its own"""
    rng = np.random.default_rng(seed)
    nns = sorted(op.dims)[:3]
    span = {nn: (op.off[nn] * op.ns, (op.off[nn] + int(np.prod(op.dims[nn]))) * op.ns) for nn in nns}
    R = np.zeros((len(nns), op.n))
    for c, nn in enumerate(nns):
        R[c, span[nn][0]:span[nn][1]] = rng.uniform(-1.0, 1.0, span[nn][1] - span[nn][0])
    for tr in (False, True):
        Z = engine.pcApplyMulti(R, 1, transpose=tr)
        for c, nn in enumerate(nns):
            lo, hi = span[nn]
            assert np.abs(Z[c, lo:hi]).max() > 0.0
            assert not Z[c, :lo].any() and not Z[c, hi:].any(), ("M^-1 couples blocks", fill, tr, c)


def check_sweep_cases(engine, dims_rans, dims_turb):
    _, op = single_block(engine, dims_rans, pc.RANS, jm.WALL, 107, stretch_k=2.0)
    check_sweeps_all_fills(engine, op, 421, f"RANS {dims_rans}")
    rm = pc.RANS.replace(limiter=minmod)
    for jac in (dict(frozenTurb=True), dict(useTurbOnly=True)):
        _, op = single_block(engine, dims_turb, rm, jm.WALL, stretch_k=2.0, **jac)
        check_sweeps_all_fills(engine, op, 431, f"{dims_turb} {jac}")


def check_sweeps_rotated_interfaces(engine, ell):
    """four blocks of unequal size: sets of unequal length in one launch, and the blocks stay subdomains"""
    _, op = brick_operator(engine, ell, FlowParams(spaceDiscr=upwind), seed=251)
    for fill in (0, 1, 2):
        with pcf.fill_of(engine, fill):
            engine.pcSetup(1)
            assert_sweeps(engine, op, fill, 441 + fill, "rotated interfaces")
            check_blocks_stay_subdomains(engine, op, fill, 445)
            engine.pcRelease()
    engine.releaseWorkspace()


def check_factor_slots(engine, dims, seed=451):
    """a fill-2 factor in slot 1, a fill-0 factor in slot 0: the multi entry acts on the selected slot, and the single-vector results of
    both slots are bit-identical before and after"""
    _, op = single_block(engine, dims, pc.RANS, jm.WALL, 107, stretch_k=2.0)
    rng = np.random.default_rng(seed)
    R = rng.uniform(-1.0, 1.0, (3, op.n))
    try:
        engine.pcSelect(1)
        engine.pcSetFill(2)
        engine.pcSetup(1)
        engine.pcSelect(0)
        engine.pcSetup(1)
        assert engine.pcInfo2()[0] == 0
        before = {}
        for slot in (0, 1):
            engine.pcSelect(slot)
            before[slot] = {tr: [engine.pcApply(r, 1, transpose=tr) for r in R] for tr in (False, True)}
        assert not np.array_equal(before[0][False][0], before[1][False][0])
        for slot, fill in ((1, 2), (0, 0)):
            engine.pcSelect(slot)
            assert engine.pcInfo2()[0] == fill
            got = assert_sweeps(engine, op, fill, seed + slot, f"slot {slot}", nvecs=(3,))
            del got
        for slot in (0, 1):
            engine.pcSelect(slot)
            for tr in (False, True):
                for c, r in enumerate(R):
                    assert np.array_equal(engine.pcApply(r, 1, transpose=tr), before[slot][tr][c]), ("single result changed", slot, tr, c)
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcSetFill(0)
            engine.pcRelease()


def check_ank_factor(engine, dims=(7, 6, 5), seed=311):
    """a factor of adflow_gpu_ank_pc_setup applied to 3 columns against the numpy ILU of dRdwPre + T, built as pcf.check_ank builds it"""
    blk, op = single_block(engine, dims, pc.RANS, jm.WALL, seed, frozenTurb=True, stretch_k=2.0)
    engine.timeStep(1)
    engine.ankTimeStep(ank.CFL, ank.TURB_CFL_SCALE, False)
    ops = ank.shifted(op, {1: engine.ankTimeStepBlocks(1, False)})
    try:
        for fill in (0, 2):
            with pcf.fill_of(engine, fill):
                engine.ankPcSetup(1)
                assert engine.pcInfo2()[0] == fill
                assert_sweeps(engine, ops, fill, seed + fill, f"ANK factor {dims}", nvecs=(3,))
                engine.pcRelease()
    finally:
        engine.pcSelect(0)
        engine.pcRelease()
        engine.ankRelease()


# ---- 3. one column is the single entry; columns do not depend on each other ----------------------------------------------------
def check_one_column_and_independence(engine, dims, cap, seed=461):
    """nvec = 1 of every multi entry equals the single entry bit for bit; column 0 of a three-column call does not change by a bit
    when the other columns change; against the single entry on the same column the difference is printed and stays within the
    yardstick of the entry (the product's rounding bound / MARGIN x the float64 numpy error).  Fill 0 and fill 2"""
    _, op = single_block(engine, dims, pc.RANS, jm.WALL, 107, stretch_k=2.0)
    rng = np.random.default_rng(seed)
    A, B = rng.uniform(-1.0, 1.0, (3, op.n)), rng.uniform(-1.0, 1.0, (3, op.n))
    B[0] = A[0]
    nn = op.st.shape[0] * op.ns
    for tr in (False, True):
        y1 = engine.jacobianMult(A[0], 1, transpose=tr)
        assert np.array_equal(engine.jacobianMultMulti(A[:1], 1, transpose=tr)[0], y1), ("product, one column", tr)
        Ya, Yb = engine.jacobianMultMulti(A, 1, transpose=tr), engine.jacobianMultMulti(B, 1, transpose=tr)
        assert np.array_equal(Ya[0], Yb[0]), ("product: column 0 depends on its neighbours", tr)
        d = np.abs(Ya[0] - y1)
        print(f"product transpose={tr}: max|multi - single| = {d.max():.3e} (bit-equal: {not d.any()})")
        assert (d <= 2 * nn * EPS * op.apply(A[0], tr, absolute=True)).all()              # the bound of the numpy product
    for fill in (0, 2):
        with pcf.fill_of(engine, fill):
            engine.pcSetup(1)
            f64, fld = ilus_of(op, fill)
            for tr in (False, True):
                z1 = engine.pcApply(A[0], 1, transpose=tr)
                assert np.array_equal(engine.pcApplyMulti(A[:1], 1, transpose=tr)[0], z1), ("application, one column", fill, tr)
                Za, Zb = engine.pcApplyMulti(A, 1, transpose=tr), engine.pcApplyMulti(B, 1, transpose=tr)
                assert np.array_equal(Za[0], Zb[0]), ("application: column 0 depends on its neighbours", fill, tr)
                zl = fld.apply(A[0], tr)
                e_np = float(np.abs(f64.apply(A[0], tr).astype(np.longdouble) - zl).max())
                d = float(np.abs(Za[0] - z1).max())
                print(f"application fill {fill} transpose={tr}: max|multi - single| = {d:.3e} (bit-equal: {d == 0.0}), float64 numpy "
                      f"error {e_np:.3e}")
                assert d <= MARGIN * e_np
            kw = dict(restart=cap, maxIts=cap, rtol=1e-8)
            x1 = engine.gmresSolve(A[0], 1, **kw)
            X, its, r0, rn = engine.gmresSolveMulti(A[:1], 1, **kw)
            assert np.array_equal(X[0], x1[0]) and (int(its[0]), float(r0[0]), float(rn[0])) == x1[1:], ("solver, one column", fill)
            Xa, ia, _, _ = engine.gmresSolveMulti(A, 1, **kw)
            Xb, ib, _, _ = engine.gmresSolveMulti(B, 1, **kw)
            assert np.array_equal(Xa[0], Xb[0]) and ia[0] == ib[0], ("solver: column 0 depends on its neighbours", fill)
            engine.pcRelease()
    engine.releaseWorkspace()


# ---- 4. the solver -----------------------------------------------------------------------------------------------------------
def sparse_of(op, transpose):
    """the numpy operator as a scipy matrix (the columns of LevelOperator.apply, assembled entry by entry instead of n products)"""
    import scipy.sparse as sp
    ns = op.ns
    rr, cc, vv = [], [], []
    for nn, (nx, ny, nz) in op.dims.items():
        I, J_, K = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
        rows = (op.off[nn] + (K * ny + J_) * nx + I).ravel()
        for s in range(op.st.shape[0]):
            d = op.st[s]
            cols = op.colmap[nn][I + 2 - d[0], J_ + 2 - d[1], K + 2 - d[2]].ravel()
            ok = cols >= 0
            B = op.J[nn][..., s].reshape(nx * ny * nz, ns, ns)[ok]                          # (row, ll, l)
            r = rows[ok][:, None, None] * ns + np.arange(ns)[None, :, None]
            c = cols[ok][:, None, None] * ns + np.arange(ns)[None, None, :]
            rr.append(np.broadcast_to(r, B.shape).ravel()); cc.append(np.broadcast_to(c, B.shape).ravel()); vv.append(B.ravel())
    A = sp.csr_matrix((np.concatenate(vv), (np.concatenate(rr), np.concatenate(cc))), shape=(op.n, op.n))
    return (A.T if transpose else A).tocsc()


def product_rounding(op, x, b, transpose):
    """2-norm of the rounding bound of b - A x formed in floating point: 2 n eps (|A| |x|) of the product, entry by entry, and one
    rounding of the subtraction"""
    nn = op.st.shape[0] * op.ns
    return float(np.linalg.norm(2 * nn * EPS * op.apply(x, transpose, absolute=True) + EPS * np.abs(b)))


def assert_columns_match_single_solves(engine, op, B, transpose, cap, what, x_ref=None, restart=None, rtol=1e-8, atol=0.0, X0=None,
                                       skip=()):
    """every column of one multi solve against adflow_gpu_gmres_solve on that column alone: the same iteration count, within the
    cap; rnorm0 and rnorm against the norms recomputed in numpy, to the rounding bound of the product.  That bound has two parts,
    both jm.assert_products_to_rounding's rule 2 n eps (|a| . |b|) for a dot product of length n: the residual vector b - A x
    (product_rounding: n = nStencil nState per entry), and the norm itself, which is the dot product <r, r> of length N = op.n in two
    summation orders -- 2 N eps <r, r> on the square, N eps ||r|| on its root;
    with x_ref (scipy's spsolve on the same matrix): the error is at most twice the single solve's plus that rounding bound.
    Returns (X, its, singles)"""
    restart = restart or cap
    kw = dict(transpose=transpose, restart=restart, maxIts=cap, rtol=rtol, atol=atol)
    X, its, r0, rn = engine.gmresSolveMulti(B, 1, x0=X0, **kw)
    assert np.isfinite(X).all() and np.isfinite(r0).all() and np.isfinite(rn).all()
    singles = []
    for c, b in enumerate(B):
        xs, its_s, r0s, rns = engine.gmresSolve(b, 1, x0=None if X0 is None else X0[c], **kw)
        singles.append((xs, its_s))
        if c in skip:
            continue
        nb = float(np.linalg.norm(b))
        start = b if X0 is None else b - op.apply(X0[c], transpose)
        true = float(np.linalg.norm(b - op.apply(X[c], transpose)))
        pr = product_rounding(op, X[c], b, transpose) + op.n * EPS * true
        pr0 = (0.0 if X0 is None else product_rounding(op, X0[c], b, transpose)) + op.n * EPS * float(np.linalg.norm(start))
        msg = f"{what} transpose={transpose} column {c}: {its[c]} iterations (single {its_s}, cap {cap}), ||b - A x|| / ||b|| = {true / nb:.3e}"
        if x_ref is not None:
            e_m, e_s = float(np.linalg.norm(X[c] - x_ref[c])), float(np.linalg.norm(xs - x_ref[c]))
            msg += f", ||x - x_ref||: multi {e_m:.3e}, single {e_s:.3e}"
        print(msg)
        assert its[c] == its_s and 0 < its[c] <= cap, (what, c, its[c], its_s, cap)
        assert abs(r0[c] - float(np.linalg.norm(start))) <= pr0, (what, c, r0[c], pr0)
        assert abs(rn[c] - true) <= pr, (what, c, rn[c], true, pr)
        if x_ref is not None:
            assert e_m <= 2 * e_s + pr, (what, c, e_m, e_s, pr)
    return X, its, singles


def check_gmres_on_pc_matrix(engine, dims, cap, seed=471):
    """3 right-hand sides on the preconditioner matrix itself (cap and restart of test_gmres_on_the_pc_matrix), fill 0 and 2, both
    transposes; then the uneven cases: a converged column, a zero column, a small restart"""
    import scipy.sparse.linalg as sla
    _, op = single_block(engine, dims, pc.RANS, jm.WALL, 107, stretch_k=2.0)
    rng = np.random.default_rng(seed)
    B = rng.uniform(-1.0, 1.0, (3, op.n)) * np.array([1.0, 1e-3, 40.0])[:, None]
    for fill in (0, 2):
        with pcf.fill_of(engine, fill):
            engine.pcSetup(1)
            for tr in (False, True):
                lu = sla.splu(sparse_of(op, tr))
                x_ref = [lu.solve(b) for b in B]
                assert_columns_match_single_solves(engine, op, B, tr, cap, f"PC matrix {dims} fill {fill}", x_ref)
            if fill == 0:
                check_uneven(engine, op, B, cap)
                # 8 columns: two groups of 4 inside every application and product of the solver, coefficients beyond the fourth
                B8 = rng.uniform(-1.0, 1.0, (8, op.n))
                assert_columns_match_single_solves(engine, op, B8, True, cap, f"8 columns, PC matrix {dims}")
            engine.pcRelease()
    engine.releaseWorkspace()


def check_uneven(engine, op, B, cap, rtol=1e-8):
    """with the factor that stands.  (a) useGuess = 1, column 0 starts from the converged solution of an earlier solve at the level
    check_gmres_on_pc_matrix of pc_checks grants it (2 rtol), the others from zero: its[0] == 0 and X[0] unchanged to the bit, the
    others as their single solves.  (b) a column b = 0: x = 0, its = 0, nothing that is not finite.  (c) restart 5: restarts
    happen while the columns need different iteration counts (the columns differ in size by orders of magnitude and share one
    atol, so their tolerances max(rtol ||b_c||, atol) differ relative to ||b_c||)"""
    x0, its0, _, _ = engine.gmresSolve(B[0], 1, restart=cap, maxIts=cap, rtol=rtol)
    assert 0 < its0 <= cap
    X0 = np.zeros_like(B)
    X0[0] = x0
    X, its, _ = assert_columns_match_single_solves(engine, op, B, False, cap, "converged column 0", rtol=2 * rtol, X0=X0, skip=(0,))
    assert its[0] == 0 and np.array_equal(X[0], x0), ("the converged column was touched", its[0])
    Bz = B.copy()
    Bz[1] = 0.0
    X, its, r0, rn = engine.gmresSolveMulti(Bz, 1, restart=cap, maxIts=cap, rtol=rtol)
    assert its[1] == 0 and not X[1].any() and r0[1] == 0.0 and rn[1] == 0.0
    assert np.isfinite(X).all() and np.isfinite(r0).all() and np.isfinite(rn).all()
    for c in (0, 2):
        xs, its_s, _, _ = engine.gmresSolve(Bz[c], 1, restart=cap, maxIts=cap, rtol=rtol)
        assert its[c] == its_s
    atol = 1e-4 * float(np.linalg.norm(B[0]))
    X, its, singles = assert_columns_match_single_solves(engine, op, B, False, 4 * cap, "restart 5", restart=5, atol=atol)
    assert len(set(int(i) for i in its)) > 1 and max(its) > 5, ("the columns were meant to need different counts over restarts", its)


def check_gmres_adjoint_order(engine, dims, cap, seed=283):
    """the adjoint's order of calls (pc.check_gmres_adjoint_order): the factor of the preconditioner matrix, then the exact 33-point
    matrix, transpose = 1, 3 right-hand sides, fill 0 and 2; x_ref is scipy's solve on the downloaded matrix"""
    import scipy.sparse.linalg as sla
    rng = np.random.default_rng(seed)
    for fill in (0, 2):
        blk, opc = single_block(engine, dims, pc.RANS, jm.WALL, 107, stretch_k=2.0)
        with pcf.fill_of(engine, fill):
            engine.pcSetup(1)
            engine.setupStateResidualMatrix(1, False, useAD=True)
            op = operator_of(engine, {1: blk})
            assert op.st.shape[0] == 33
            B = rng.uniform(-1.0, 1.0, (3, op.n))
            lu = sla.splu(sparse_of(op, True))
            assert_columns_match_single_solves(engine, op, B, True, cap, f"adjoint order {dims} fill {fill}", [lu.solve(b) for b in B])
            engine.pcRelease()
    engine.releaseWorkspace()


# ---- 5. refusals and side effects ----------------------------------------------------------------------------------------------
def check_refusals_and_side_effects(engine, dims=(7, 6, 5)):
    """every refusal with its message, named by the multi entry; state, residual, matrix and factor untouched; the extra work
    space of the factor appears in pc_info with the first multi application, not before, and leaves with the factor"""
    lib = engine.lib
    mult = (lib.adflow_gpu_jacobian_mult_multi, lib.adflow_gpu_jacobian_mult_multi_dev)
    appl = (lib.adflow_gpu_pc_apply_multi, lib.adflow_gpu_pc_apply_multi_dev)
    solv = (lib.adflow_gpu_gmres_solve_multi, lib.adflow_gpu_gmres_solve_multi_dev)
    tail = (10, 10, 1e-6, 0.0, 0, None, None, None)

    def refused(fns, args, msg, who):
        for fn in fns:
            assert fn(*args) != 0, (fn.__name__, msg)
            err = lib.adflow_gpu_last_error().decode()
            assert msg in err and who in err, (fn.__name__, msg, err)

    engine.release_all()
    engine.pcSelect(0)
    ncell = int(np.prod(dims))
    n = 6 * ncell
    rng = np.random.default_rng(229)
    X, Y = rng.uniform(-1.0, 1.0, (3, n)), np.zeros((3, n))
    px, py = X.ctypes.data, Y.ctypes.data
    refused(mult, (1, 0, 3, px, n, py, n, n), "no assembled Jacobian", "jacobian_mult_multi")
    refused(appl, (1, 0, 3, px, n, py, n, n), "no factor", "pc_apply_multi")
    refused(solv, (1, 0, 3, px, n, py, n, n) + tail, "no assembled Jacobian", "gmres_solve_multi")
    blk, _, prm = checks.setup_block_with_bc(engine, dims, pc.RANS.replace(limiter=minmod), jm.WALL, 227, stretch_k=2.0)
    engine.setupStateResidualMatrix(1, True, delta=1e-6)
    refused(appl, (1, 0, 3, px, n, py, n, n), "no factor", "pc_apply_multi")
    refused(solv, (1, 0, 3, px, n, py, n, n) + tail, "no factor", "gmres_solve_multi")
    engine.download_state(1, 1)
    w0, dw0, J0 = blk["w"].copy(), engine.download_residual(1, 1).copy(), engine.jacobianBlocks(1).copy()
    engine.pcSetup(1)
    bytes0 = engine.pcInfo()[2]
    single = {tr: ([engine.jacobianMult(x, 1, transpose=tr) for x in X], [engine.pcApply(x, 1, transpose=tr) for x in X])
              for tr in (False, True)}
    xs = engine.gmresSolve(X[0], 1, restart=30, maxIts=30, rtol=1e-6)
    assert engine.pcInfo()[2] == bytes0, "single calls must not grow the factor"
    for fns, who in ((mult, "jacobian_mult_multi"), (appl, "pc_apply_multi"), (solv, "gmres_solve_multi")):
        t = tail if fns is solv else ()
        refused(fns, (1, 0, 0, px, n, py, n, n) + t, "nvec = 0", who)
        refused(fns, (1, 0, -2, px, n, py, n, n) + t, "nvec = -2", who)
        refused(fns, (1, 0, capi.MAX_NVEC + 1, px, n, py, n, n) + t, "nvec", who)
        refused(fns, (1, 1, 3, px, n - 1, py, n, n) + t, "ld >= n", who)
        refused(fns, (1, 0, 3, px, n, py, n - 6, n) + t, "ld >= n", who)
        refused(fns, (1, 0, 3, px, n, px, n, n) + t, "overlap", who)
        refused(fns, (1, 0, 2, px, n, px + 8 * n, n, n) + t, "column 1 of the input and column 0 of the result overlap", who)
        refused(fns, (1, 0, 2, px, n, px + 8 * (n - 1), 2 * n, n) + t, "overlap", who)
        refused(fns, (2, 0, 3, px, n, py, n, n) + t, "not the level of", who)
        refused(fns, (1, 0, 3, None, n, py, n, n) + t, "is NULL", who)
        refused(fns, (1, 1, 3, px, n, None, n, n) + t, "is NULL", who)
        refused(fns, (1, 0, 3, px, n + 6, py, n + 6, n + 6) + t, "rows", who)
        refused(fns, (1, 0, 3, px, n, py, n, 5 * ncell) + t, "rows", who)
    refused(solv, (1, 0, 3, px, n, py, n, n, 0, 10, 1e-6, 0.0, 0, None, None, None), "restart = 0", "gmres_solve_multi")
    bad = X.copy()
    bad[2, 17] = np.nan
    refused(solv[:1], (1, 0, 3, bad.ctypes.data, n, py, n, n) + tail, "column 2 is not finite", "gmres_solve_multi")
    assert engine.pcInfo()[2] == bytes0, "a refused call must not grow the factor"
    # the calls themselves: the factor grows by the work space of the other vectors of the widest group, once
    Z2 = engine.pcApplyMulti(X[:2], 1)
    grown2 = engine.pcInfo()[2]
    assert grown2 == bytes0 + 1 * n * 8, (bytes0, grown2)
    Z3 = engine.pcApplyMulti(X, 1)
    grown3 = engine.pcInfo()[2]
    assert grown3 == bytes0 + 2 * n * 8, (bytes0, grown3)
    assert np.array_equal(Z3[:2], Z2)
    assert np.array_equal(engine.pcApplyMulti(X[:2], 1), Z2) and engine.pcInfo()[2] == grown3
    engine.jacobianMultMulti(X, 1, transpose=True)
    Xm, its, r0, rn = engine.gmresSolveMulti(X, 1, restart=30, maxIts=30, rtol=1e-6)
    assert (its > 0).all() and (its <= 30).all() and (rn <= 2e-6 * r0).all() and engine.pcInfo()[2] == grown3
    # state, residual, matrix and factor untouched: the single-vector results are bit-identical
    engine.download_state(1, 1)
    assert np.array_equal(blk["w"], w0) and np.array_equal(engine.download_residual(1, 1), dw0)
    assert np.array_equal(engine.jacobianBlocks(1), J0)
    for tr in (False, True):
        for c, x in enumerate(X):
            assert np.array_equal(engine.jacobianMult(x, 1, transpose=tr), single[tr][0][c]), ("product after the multi calls", tr, c)
            assert np.array_equal(engine.pcApply(x, 1, transpose=tr), single[tr][1][c]), ("application after the multi calls", tr, c)
    xs2 = engine.gmresSolve(X[0], 1, restart=30, maxIts=30, rtol=1e-6)
    assert np.array_equal(xs2[0], xs[0]) and xs2[1:] == xs[1:]
    # the matrix changes its nState under the factor: the solver refuses, the factor still applies
    engine.setupStateResidualMatrix(1, True, frozenTurb=True, delta=1e-6)
    refused(solv, (1, 0, 3, px, n, py, n, n) + tail, "nState", "gmres_solve_multi")
    assert np.array_equal(engine.pcApplyMulti(X[:2], 1), Z2)
    assert engine.pcRelease() == grown3 and engine.pcRelease() == 0
    refused(appl, (1, 0, 3, px, n, py, n, n), "no factor", "pc_apply_multi")
    engine.release_all()


# ---- 6. the _dev twins and the enqueue-only mode ---------------------------------------------------------------------------------
def check_dev_twins_and_async(engine, dv, ell, dims, cap, seed=481):
    """the _dev forms on device vectors (ld = n + 3) return bit for bit what the host forms return; with adflow_gpu_set_async(1) a
    chain product -> application (slot 0, fill 0) -> application (slot 1, fill 2) -> product with one synchronise at the end equals
    the same chain with a synchronise after every call"""
    rng = np.random.default_rng(seed)
    nvec, pad = 3, 3

    def columns(d, n):
        flat = dv.get(d)
        return np.stack([flat[c * (n + pad):c * (n + pad) + n] for c in range(nvec)])

    def put(A):
        n = A.shape[1]
        flat = np.full(nvec * (n + pad), 3.5)
        for c in range(nvec):
            flat[c * (n + pad):c * (n + pad) + n] = A[c]
        return dv.put(flat)

    _, op = brick_operator(engine, ell, FlowParams(spaceDiscr=upwind), seed)
    n, ld = op.n, op.n + pad
    try:
        engine.pcSelect(1)
        engine.pcSetFill(2)
        engine.pcSetup(1)
        engine.pcSelect(0)
        engine.pcSetup(1)
        X = rng.uniform(-1.0, 1.0, (nvec, n))
        dX = put(X)
        for tr in (False, True):
            dY = put(np.zeros((nvec, n)))
            dev_call(engine, dv, engine.jacobianMultMultiDev, dv.ptr(dX), ld, dv.ptr(dY), ld, nvec, n, 1, tr)
            assert np.array_equal(columns(dY, n), engine.jacobianMultMulti(X, 1, transpose=tr)), ("product _dev", tr)
            for slot in (0, 1):
                engine.pcSelect(slot)
                dZ = put(np.zeros((nvec, n)))
                dev_call(engine, dv, engine.pcApplyMultiDev, dv.ptr(dX), ld, dv.ptr(dZ), ld, nvec, n, 1, tr)
                assert np.array_equal(columns(dZ, n), engine.pcApplyMulti(X, 1, transpose=tr)), ("application _dev", tr, slot)
                assert (dv.get(dZ)[n:ld] == 3.5).all(), "padding written"
            assert np.array_equal(columns(dX, n), X), "the input was written"
        # the chain, synchronised after every call and enqueue-only
        out = {}
        for mode in (0, 1):
            d = [put(X)] + [put(np.zeros((nvec, n))) for _ in range(4)]
            dv.sync()
            engine.set_async(bool(mode))
            try:
                engine.pcSelect(0)
                engine.jacobianMultMultiDev(dv.ptr(d[0]), ld, dv.ptr(d[1]), ld, nvec, n, 1, False)
                engine.pcApplyMultiDev(dv.ptr(d[1]), ld, dv.ptr(d[2]), ld, nvec, n, 1, False)
                engine.pcSelect(1)
                engine.pcApplyMultiDev(dv.ptr(d[2]), ld, dv.ptr(d[3]), ld, nvec, n, 1, True)
                engine.jacobianMultMultiDev(dv.ptr(d[3]), ld, dv.ptr(d[4]), ld, nvec, n, 1, True)
                engine.sync()
            finally:
                engine.set_async(False)
                engine.pcSelect(0)
            out[mode] = [columns(q, n) for q in d[1:]]
        for a, b in zip(out[0], out[1]):
            assert np.abs(a).max() > 0.0 and np.array_equal(a, b), "the enqueue-only chain differs"
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcSetFill(0)
            engine.pcRelease()
    # the solver on one wall-bounded RANS block
    _, op = single_block(engine, dims, pc.RANS, jm.WALL, 107, stretch_k=2.0)
    engine.pcSetup(1)
    n, ld = op.n, op.n + pad
    B = rng.uniform(-1.0, 1.0, (nvec, n))
    kw = dict(transpose=True, restart=cap, maxIts=cap, rtol=1e-8)
    X, *host = engine.gmresSolveMulti(B, 1, **kw)
    dB, dX = put(B), put(np.full((nvec, n), 7.0))
    dev = dev_call(engine, dv, engine.gmresSolveMultiDev, dv.ptr(dB), ld, dv.ptr(dX), ld, nvec, n, 1, **kw)
    assert all(np.array_equal(h, d) for h, d in zip(host, dev)) and np.array_equal(columns(dX, n), X), "solver _dev"
    assert (dv.get(dX)[n:ld] == 3.5).all() and np.array_equal(columns(dB, n), B)
    engine.pcRelease()
    engine.releaseWorkspace()
