"""Checks of the flow update of the approximate Newton-Krylov step on the device (adflow_gpu_ank_*: vector glue, the pseudo-time term
T, the shifted ILU(0), the matrix-free operator, the solve and the step limiter) shared by tests/test_gpu_ank.py (real MI355X) and
tests/test_hostsim_ank.py (the kernel-logic emulator).  cfl = 5 throughout: T is comparable to the matrix.

Yardsticks: T from the formulas of computeTimeStepBlock restated in numpy on the library's downloaded w, dtl and volRef; the shifted
factor against pc_checks.NumpyILU0 on the downloaded blocks + T; the operator against J v + T v with the library's forward-mode blocks
applied in numpy, next to the reference's own difference quotient (two oracle.ref.blockette_res_core evaluations with the same flags
and the same step h); the step limiter against a numpy restatement of physicalityCheckANK."""
import numpy as np
import pytest

import checks
from device_vectors import dev_call
import jacmult_checks as jm
import pc_checks as pc
from adflow_amd import capi
from adflow_amd.params import FlowParams, EulerEquations, RANSEquations, dissMatrix, dissScalar, upwind

EPS = 2.0 ** -52
CFL = 5.0
MARGIN = pc.MARGIN
ERR_REL, UMIN = 1.490116119384766e-08, 1e-6
EULER_JST = FlowParams(spaceDiscr=dissScalar)
RANS_UPWIND = pc.RANS
RANS_JST = pc.RANS.replace(spaceDiscr=dissScalar)
RANS_COUPLED = pc.RANS.replace(turbResScale=1.0e3)          # turbResScale and turbCFLScale both /= 1
TURB_CFL_SCALE = 2.5
# Euler faces for the checks that compare with the FORWARD-MODE matrix: applyAllBC_block_d of the reference (BCExtra_d.F90:10-139,
# reproduced by the library's assembly) differentiates symmetry, walls, farfield and the subsonic kinds, NOT extrapolation and the
# supersonic kinds -- their halos enter a forward-mode matrix with a zero derivative, by the reference's design.  On jm.EULER (faces
# 4 and 6: extrapolation, supersonic outflow) such a matrix is therefore not the derivative of the residual next to those faces, and
# J v + T v is a yardstick only where every face of the block is of a differentiated kind: those two faces are farfield here.
EULER_AD = {1: -6, 2: -6, 3: -5, 4: -6, 5: -1, 6: -6}
_KEEP = []          # the reference's flowDoms point into these arrays: alive as long as ref may be called


# ---- vectors <-> blocks ------------------------------------------------------------------------------------------------------
def owned_vector(blocks, name, ns):
    """the owned cells of `name` of every block in the PETSc order (block, k, j, i, variable fastest), ns variables"""
    return np.concatenate([np.ascontiguousarray(np.transpose(blocks[nn].owned(name)[..., :ns], (2, 1, 0, 3))).reshape(-1)
                           for nn in sorted(blocks)])


def state_vector(engine, blocks, ns):
    for nn in blocks:
        engine.download_state(nn, 1)
    return owned_vector(blocks, "w", ns)


def ds_step(w, v):
    """PETSc's default MATMFFD_DS step"""
    s, d, q = float(np.dot(w, v)), float(np.abs(v).sum()), float(np.dot(v, v))
    if q == 0.0:
        return 0.0
    if abs(s) < UMIN * d:
        s = -UMIN * d if s < 0.0 else UMIN * d
    return ERR_REL * s / q


# ---- 1. the pseudo-time term -------------------------------------------------------------------------------------------------
def numpy_T(engine, blocks, prm, coupled, cfl=CFL, turbCFLScale=TURB_CFL_SCALE):
    """{nn: (nState, nState, nx, ny, nz)} from the formulas: dtInv = 1 / (cfl dtl volRef), T = dtInv S"""
    out = {}
    for nn, blk in blocks.items():
        engine.download_state(nn, 1)
        dtl = engine.download_array(capi.ARR_DTL, np.zeros((blk.ie, blk.je, blk.ke), order="F"), nn, 1)[1:blk.nx + 1, 1:blk.ny + 1, 1:blk.nz + 1]
        w = blk.owned("w")
        ns = blk.nw if coupled else 5
        dtInv = 1.0 / ((cfl * dtl) * blk.owned("volRef"))
        T = np.zeros((ns, ns) + dtl.shape)
        T[0, 0] = T[4, 4] = dtInv
        for l in (1, 2, 3):
            T[l, 0] = dtInv * w[..., l]
            T[l, l] = dtInv * w[..., 0]
        if ns > 5:
            T[5, 5] = dtInv * (prm.turbResScale / turbCFLScale)
        out[nn] = T
    return out


def assert_T_block(Tl, Tn, what):
    """the library's T of one block against the formula's: the structural zeros are zero, 16 eps on the rest; returns the largest
    relative difference"""
    assert Tl.shape == Tn.shape, (Tl.shape, Tn.shape)
    zero = Tn == 0.0
    nz = np.zeros(Tl.shape[:2], bool)
    nz[0, 0] = nz[4, 4] = True
    for l in (1, 2, 3):
        nz[l, 0] = nz[l, l] = True
    if Tl.shape[0] > 5:
        nz[5, 5] = True
    assert not Tl[~nz].any(), (what, "structural zeros")
    rel = np.abs(Tl[nz] - Tn[nz]) / np.abs(Tn[nz])
    print(f"T {what}: nState = {Tl.shape[0]}, max relative difference {rel.max() / EPS:.2f} eps, max|T| = {np.abs(Tl).max():.3e}")
    assert rel.max() <= 16 * EPS, (what, rel.max() / EPS)
    assert np.abs(Tl[nz]).min() > 0.0 and not (zero & nz[:, :, None, None, None]).any()
    return float(rel.max())


def assert_T(engine, blocks, prm, coupled, what):
    engine.timeStep(1)
    engine.ankTimeStep(CFL, TURB_CFL_SCALE, coupled)
    Tn = numpy_T(engine, blocks, prm, coupled)
    for nn in blocks:
        assert_T_block(engine.ankTimeStepBlocks(nn, coupled), Tn[nn], f"{what} block {nn}")
    return Tn


def T_times(Tn, blocks, v):
    ns = next(iter(Tn.values())).shape[0]
    out, off = np.zeros_like(v), 0
    for nn in sorted(blocks):
        n = blocks[nn].ncells * ns
        x = np.transpose(v[off:off + n].reshape(blocks[nn].nz, blocks[nn].ny, blocks[nn].nx, ns), (2, 1, 0, 3))
        y = np.einsum("abijk,ijkb->ijka", Tn[nn], x)
        out[off:off + n] = np.ascontiguousarray(np.transpose(y, (2, 1, 0, 3))).reshape(-1)
        off += n
    return out


def check_T_single(engine, dims, prm, spec, coupled, seed=307, **mk):
    blk, r, prm = checks.setup_block_with_bc(engine, dims, prm, spec, seed, **mk)
    _KEEP[:] = [r]
    assert_T(engine, {1: blk}, prm, coupled, f"{dims} coupled={coupled}")
    engine.ankRelease()


# ---- 2. the shifted factor -----------------------------------------------------------------------------------------------------
def shifted(op, Tn):
    """the numpy operator with T added to the diagonal blocks"""
    s0 = int(np.where((op.st == 0).all(axis=1))[0][0])
    J = {nn: B.copy() for nn, B in op.J.items()}
    for nn in J:
        J[nn][..., s0] += np.transpose(Tn[nn], (2, 3, 4, 0, 1))
    out = jm.LevelOperator(J, op.dims, op.st)
    out.colmap = op.colmap
    return out


def assert_shifted_factor(engine, blocks, op, prm, coupled, seed, what, matches=None):
    """pcApply after ankPcSetup against NumpyILU0 of J + T (pc_checks' rule); then pcSetup on the same matrix is bit-identical to
    the application taken before any ANK entry was called.  matches: the comparison (default pc_checks.assert_apply_matches, one draw)"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(-1.0, 1.0, op.n)
    engine.pcSetup(1)
    plain = {tr: engine.pcApply(r, 1, transpose=tr) for tr in (False, True)}
    Tn = assert_T(engine, blocks, prm, coupled, what)
    ops = shifted(op, Tn)
    engine.ankPcSetup(1)
    ns, npl, nb = engine.pcInfo()
    assert ns == op.ns and npl == max(sum(d) - 2 for d in op.dims.values())
    first, ilus = (matches or pc.assert_apply_matches)(engine, ops, seed + 1, f"shifted factor, {what}")
    assert not np.array_equal(engine.pcApply(r, 1), plain[False]), "T does not reach the factor"
    engine.pcSetup(1)
    for tr in (False, True):
        assert np.array_equal(engine.pcApply(r, 1, transpose=tr), plain[tr]), ("pcSetup after the ANK entries", tr)
    return Tn, ops, ilus


def check_shifted_single(engine, dims, seed=311):
    """RANS decoupled single block, ADFLOW_JAC_PC | FROZEN_TURB | USE_AD"""
    blk, op = pc.single_block(engine, dims, RANS_UPWIND, jm.WALL, seed, frozenTurb=True, stretch_k=2.0)
    assert_shifted_factor(engine, {1: blk}, op, RANS_UPWIND, False, seed, f"RANS decoupled {dims}")
    engine.pcRelease()
    engine.ankRelease()


def check_shifted_block(engine, dims, prm, spec, coupled, seed=311, matches=None, **mk):
    """one block with six boundary faces: decoupled (frozen turbulence, nState 5) or coupled (nState 6, T with the turbulence entry)"""
    blk, op = pc.single_block(engine, dims, prm, spec, seed, frozenTurb=not coupled, **mk)
    assert op.ns == (6 if coupled else 5)
    try:
        assert_shifted_factor(engine, {1: blk}, op, prm, coupled, seed, f"{dims} coupled={coupled}", matches=matches)
    finally:
        engine.pcRelease()
        engine.ankRelease()


def check_shifted_ell(engine, topo, seed=313):
    blocks, op = jm.brick_operator(engine, topo, FlowParams(spaceDiscr=upwind), seed)
    assert_shifted_factor(engine, blocks, op, FlowParams(spaceDiscr=upwind), False, seed, f"{len(blocks)} blocks, Euler")
    engine.pcRelease()
    engine.ankRelease()


# ---- 3. the operator -----------------------------------------------------------------------------------------------------------
class RefResidual:
    """R(w) of FormFunction_mf on ONE block with boundary subfaces, every arithmetic step the reference's own routine: setWANK and
    setRVecANK / setRVec restated in numpy, closures, boundary conditions, whalo2, blocketteResCore with the flags"""

    def __init__(self, r, prm, ns, approx):
        self.r, self.prm, self.ns, self.approx = r, prm, ns, approx
        self.turb = ns > 5

    def prepare(self, w):
        from oracle import ref
        r = self.r
        r.owned("w")[..., :self.ns] = np.transpose(w.reshape(r.nz, r.ny, r.nx, self.ns), (2, 1, 0, 3))
        ref.call_level("setPointers", 1, 1)
        ref.call("computePressureSimple", 0)
        ref.call("computeLamViscosity", 0)
        ref.call("computeEddyViscosity", 0)
        if self.turb:
            ref.call("bcTurbTreatment")
            ref.call("applyAllTurbBCThisBlock", 1)
        ref.call("applyAllBC_block", 1)
        ref.call_level("whalo2", 1, 1, self.ns)
        ref.call_level("setPointers", 1, 1)

    def freeze_sensor(self):
        from oracle import ref
        r, prm = self.r, self.prm
        if prm.equations == EulerEquations or prm.spaceDiscr == dissMatrix:
            sens = r["p"].copy(order="F")
        else:
            sens = np.asfortranarray(r["p"] / r["w"][..., 0] ** r["gamma"])
        r.a["shockSensor"] = sens
        ref.load().ref_set_ptr(b"shockSensor", sens.ctypes.data)
        ref.commit_block(1, 1)                        # setPointers re-aims the block pointers from flowDoms

    def __call__(self, w, freeze=False):
        from oracle import ref
        self.prepare(w)
        if freeze:
            self.freeze_sensor()
        ref.blockette_res_core(False, True, self.turb, diss_approx=self.approx, visc_approx=self.approx)
        r = self.r
        res = r.owned("dw")[..., :self.ns] / r.owned("volRef")[..., None]
        if self.turb:
            res[..., 5] *= self.prm.turbResScale
        return np.ascontiguousarray(np.transpose(res, (2, 1, 0, 3))).reshape(-1)


def setup_operator(engine, dims, prm, spec, coupled, approx, seed, **mk):
    """one block with six boundary faces: the matrix whose product is the yardstick (forward mode, the residual flavour of the
    operator), T, and the base of the matrix-free operator at the block's state.  Returns (blk, reference residual, J, T, w0)"""
    blk, r, prm = checks.setup_block_with_bc(engine, dims, prm, spec, seed, **mk)
    _KEEP[:] = [r]
    rans = prm.equations == RANSEquations
    ns = blk.nw if coupled else 5
    engine.setupStateResidualMatrix(1, usePC=approx, frozenTurb=rans and not coupled, useAD=True)
    op = jm.operator_of(engine, {1: blk})
    assert op.ns == ns
    Tn = assert_T(engine, {1: blk}, prm, coupled, f"{dims}")
    w0 = state_vector(engine, {1: blk}, ns)
    Rref = RefResidual(r, prm, ns, approx)
    Rref.r0 = Rref(w0, freeze=approx)
    if approx:
        engine.referenceShockSensor(1)
    engine.ankSetBase(w0, coupled, dissApprox=approx, viscApprox=approx)
    return blk, Rref, op, Tn, w0


def assert_product(what, y, v, h, op, Tn, blk, quotient):
    """the bar of the operator: max|y - (J v + T v)| <= MARGIN x the same distance of the reference's own difference quotient with
    the same step, quotient(h, v) = (R(w + h v) - r0) / h.  Returns (the yardstick product, the bar, the library's distance)"""
    Tv = T_times(Tn, {1: blk}, v)
    yard = op.apply(v) + Tv
    yref = quotient(h, v) + Tv
    e_lib, e_ref = float(np.abs(y - yard).max()), float(np.abs(yref - yard).max())
    print(f"operator {what}: h = {h:.3e}, max|y - (J + T) v| = {e_lib:.3e}, reference quotient {e_ref:.3e}, ratio "
          f"{e_lib / max(e_ref, 1e-300):.3f}, max|y| = {np.abs(yard).max():.3e}, max|T v| = {np.abs(Tv).max():.3e}")
    assert e_lib <= MARGIN * e_ref, (what, e_lib, e_ref)
    assert np.abs(yard).max() > 0.0
    return yard, MARGIN * e_ref, e_lib


def assert_operator(engine, blk, Rref, op, Tn, w0, seed, what):
    """max|ankMult(v) - (J v + T v)| <= MARGIN x the same distance of the reference's own difference quotient (same flags, same h)"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, w0.size)
    y = engine.ankMult(v)
    h = engine.ankLastH()
    hn = ds_step(w0, v)
    assert abs(h - hn) <= 1e-12 * abs(hn), (h, hn)
    yard, _, e_lib = assert_product(what, y, v, h, op, Tn, blk, lambda h, v: (Rref(w0 + h * v) - Rref.r0) / h)
    return v, y, e_lib / float(np.abs(yard).max())


def check_operator(engine, dims, prm, spec, coupled, approx, seed=331, edge_cases=False, **mk):
    blk, Rref, op, Tn, w0 = setup_operator(engine, dims, prm, spec, coupled, approx, seed, **mk)
    out = assert_operator(engine, blk, Rref, op, Tn, w0, seed + 1, f"{dims} coupled={coupled} approx={approx}")
    if edge_cases:
        assert not engine.ankMult(np.zeros_like(w0)).any() and engine.ankLastH() == 0.0
        # the umin branch: v orthogonal to w up to a residue far below umin |v|_1, of either sign
        rng = np.random.default_rng(seed + 2)
        for sign in (1.0, -1.0):
            v = rng.uniform(-1.0, 1.0, w0.size)
            v -= np.dot(v, w0) / np.dot(w0, w0) * w0
            v += sign * 0.01 * UMIN * np.abs(v).sum() / np.dot(w0, w0) * w0
            s, d = float(np.dot(w0, v)), float(np.abs(v).sum())
            assert 0.0 < abs(s) < 0.1 * UMIN * d and np.sign(s) == sign
            y = engine.ankMult(v)
            h, hn = engine.ankLastH(), ds_step(w0, v)
            assert abs(hn - sign * ERR_REL * UMIN * d / float(np.dot(v, v))) <= 4 * EPS * abs(hn)     # the umin branch decided
            assert abs(h - hn) <= 1e-12 * abs(hn), (sign, h, hn)
            assert np.isfinite(y).all() and np.abs(y).max() > 0.0
    engine.ankRelease()
    return out


def check_tile_sized(engine, dims, seed=383):
    """the shifted factor of the preconditioner matrix first (the adjoint's order of calls: it survives the exact assembly), then the
    exact operator at size and a short solve on it"""
    blk, r, prm = checks.setup_block_with_bc(engine, dims, RANS_UPWIND, jm.WALL, seed, stretch_k=2.0)
    _KEEP[:] = [r]
    engine.setupStateResidualMatrix(1, True, frozenTurb=True, useAD=True)
    engine.timeStep(1)
    engine.ankTimeStep(CFL)
    engine.ankPcSetup(1)
    assert engine.pcInfo()[:2] == (5, sum(dims) - 2)
    engine.setupStateResidualMatrix(1, False, frozenTurb=True, useAD=True)
    op = jm.operator_of(engine, {1: blk})
    Tn = numpy_T(engine, {1: blk}, prm, False)
    w0 = state_vector(engine, {1: blk}, 5)
    Rref = RefResidual(r, prm, 5, False)
    Rref.r0 = Rref(w0)
    engine.ankSetBase(w0)
    assert_operator(engine, blk, Rref, op, Tn, w0, seed + 1, f"{dims} RANS decoupled exact")
    engine.ankSetW(w0)
    b = engine.ankGetR()
    x, its, r0, rn = engine.ankSolve(b, 1, restart=5, maxIts=5, rtol=1e-12)
    print(f"ankSolve {dims}: {its} iterations, rnorm0 = {r0:.3e}, rnorm = {rn:.3e}")
    assert its == 5 and rn < r0 and engine.pcInfo()[1] == 132
    engine.pcRelease()
    engine.ankRelease()
    engine.releaseWorkspace()


# ---- 4. the solve ----------------------------------------------------------------------------------------------------------------
def check_solve(engine, dims, prm, spec, cap, seed=347, **mk):
    """flavour b (DISS_APPROX | VISC_APPROX against ADFLOW_JAC_PC | USE_AD), b = ankGetR of the base state, rtol = 1e-4,
    restart = maxIts = cap.  A = J + T from the downloaded blocks: scipy's gmres with the shifted NumpyILU0 as right preconditioner
    needs at most cap / 2 iterations, the library at most cap; ||b - A x|| <= 2 rtol ||b|| in numpy -- the 2 covers the recurrence
    bound plus the operator's distance from A, which the operator checks measure at about 1e-7 relative, far below rtol; the
    reported rnorm agrees with a numpy evaluation through ankMult to 1e-10 relative.

    The Euler case runs on EULER_AD (see there): with extrapolation / supersonic-outflow faces the forward-mode A lacks, by the
    reference's design, the dependence of those halos on the interior that the matrix-free operator carries, and ||b - A x|| then
    measures that difference (5.5e-02 ||b|| on jm.EULER), not the solve."""
    rtol = 1e-4
    blk, Rref, op, Tn, w0 = setup_operator(engine, dims, prm, spec, False, True, seed, **mk)
    ops = shifted(op, Tn)
    engine.ankPcSetup(1)
    b = engine.ankGetR()
    nb = float(np.linalg.norm(b))
    assert nb > 0.0 and np.abs(b - Rref.r0).max() <= 1e-9 * np.abs(Rref.r0).max()
    x, its, r0, rn = engine.ankSolve(b, 1, restart=cap, maxIts=cap, rtol=rtol)
    assert_solve(f"ankSolve {dims}", its, r0, b, x, ops, cap, rtol)
    rn_np = float(np.linalg.norm(b - engine.ankMult(x)))
    print(f"ankSolve {dims}: reported {rn / nb:.3e}, through ankMult {rn_np / nb:.3e}")
    assert abs(rn - rn_np) <= 1e-10 * rn_np, (rn, rn_np)
    engine.pcRelease()
    engine.ankRelease()


def assert_solve(what, its, r0, b, x, ops, cap, rtol):
    """the bars of a solve on the numpy operator ops = J + T: scipy's gmres with the shifted NumpyILU0 as right preconditioner needs
    at most cap / 2 iterations, the library at most cap; rnorm0 = ||b|| to 1e-12; ||b - A x|| <= 2 rtol ||b||"""
    nb = float(np.linalg.norm(b))
    k_ref = pc.scipy_gmres_iterations(lambda v: ops.apply(v), pc.NumpyILU0(ops, np.float64), b, False, rtol, cap, cap)
    true = float(np.linalg.norm(b - ops.apply(x)))
    print(f"{what}: {its} iterations (scipy {k_ref}, cap {cap}), ||b - A x|| / ||b|| = {true / nb:.3e} (bar {2 * rtol:.0e})")
    assert 2 * k_ref <= cap, ("the cap leaves no factor 2 over scipy's count", k_ref, cap)
    assert 0 < its <= cap, (its, cap)
    assert abs(r0 - nb) <= 1e-12 * nb
    assert true <= 2 * rtol * nb, (true, nb)


# ---- 5. the step limiter ---------------------------------------------------------------------------------------------------------
def numpy_physicality(w, dw, ns, coupled, lam, tol, tolTurb, stepFactor, stepMin):
    eps = 1e-25
    W, D = w.reshape(-1, ns), dw.reshape(-1, ns).copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        ratios = [np.abs(W[:, l] / (D[:, l] + eps)) * tol for l in (0, 4)]
        if coupled and ns > 5:
            rt = (W[:, 5] / (D[:, 5] + eps)) * tolTurb
            low = rt < stepFactor * stepMin
            clip = low & (rt > 0.0)
            D[clip, 5] = W[clip, 5] * tolTurb
            ratios.append(np.where(low, 1.0, rt))
    allr = np.concatenate(ratios + [np.array([lam])])
    return (0.0 if np.isnan(allr).any() else float(allr.min())), D.reshape(-1), (clip if coupled and ns > 5 else None)


def check_physicality(engine, topo, coupled, seed=359):
    prm = RANS_UPWIND
    blocks, _ = checks.setup_brick(engine, topo, prm, seed)
    ns = 6 if coupled else 5
    tol, tolTurb, stepFactor, stepMin = 0.2, 0.99, 1.0, 0.01
    rng = np.random.default_rng(seed)
    w = owned_vector(blocks, "w", ns)
    ncell = w.size // ns
    assert ncell > 4 * 256                                            # more than one workgroup, a partial last one
    base = 1e-3 * rng.uniform(-1.0, 1.0, w.size) * np.abs(w)
    W = w.reshape(-1, ns)

    def case(edit, lam0=1.0):
        dw = base.copy()
        edit(dw.reshape(-1, ns))
        lam, out = engine.ankPhysicalityCheck(w, dw, lam0, coupled, tol, tolTurb, stepFactor, stepMin)
        lam_np, out_np, clip = numpy_physicality(w, dw, ns, coupled, lam0, tol, tolTurb, stepFactor, stepMin)
        assert abs(lam - lam_np) <= 4 * EPS * abs(lam_np), (lam, lam_np)
        if clip is not None:
            assert np.array_equal(out.reshape(-1, ns)[clip, 5], W[clip, 5] * tolTurb)
        assert np.array_equal(out, out_np, equal_nan=True)
        return lam, dw, out, clip

    lam, *_ = case(lambda D: None)
    assert lam == 1.0                                                 # small updates: the start value stands
    assert case(lambda D: None, lam0=0.5)[0] == 0.5
    c1, c2, c3 = ncell // 3, ncell - 7, 5

    def density(D):
        D[c1, 0] = -10.0 * W[c1, 0]                                   # a density update ten times the density
        D[c2, 4] = 4.0 * W[c2, 4]                                     # an energy update that limits less
    lam, *_ = case(density)
    assert abs(lam - tol / 10.0) <= 1e-12

    def energy(D):
        D[c2, 4] = 4.0 * W[c2, 4]
    lam, *_ = case(energy)
    assert abs(lam - tol / 4.0) <= 1e-12
    if coupled:
        def turb(D):
            D[c3, 5] = 200.0 * W[c3, 5]                               # positive with a ratio below the threshold: clipped to w tolTurb, no limit
            D[c1, 5] = -2.0 * W[c1, 5]                                # negative, ratio -0.495: below the threshold, not positive: kept, no limit
            D[c2, 5] = 3.0 * W[c2, 5]                                 # ratio 0.33 above the threshold: limits
            D[c2 - 1, 5] = 1e4 * W[c2 - 1, 5]                         # ratio ~1e-4 below it, positive: clipped
        lam, dw, out, clip = case(turb)
        assert abs(lam - tolTurb / 3.0) <= 1e-12
        assert clip[c3] and clip[c2 - 1] and not clip[c1] and not clip[c2] and clip.sum() == 2
        assert out.reshape(-1, ns)[c1, 5] == dw.reshape(-1, ns)[c1, 5]

    def nan(D):
        D[c1, 4] = np.nan
    assert case(nan)[0] == 0.0
    if coupled:
        def nan_t(D):
            D[c2, 5] = np.nan
        assert case(nan_t)[0] == 0.0
    engine.ankRelease()


# ---- 6. the _dev entries against their host twins -----------------------------------------------------------------------------------
def check_dev_twins(engine, dv, dims=(7, 6, 5), kind="flow", cap=16, seed=431):
    """every adflow_gpu_ank_*_dev entry on device vectors (dv: device_vectors.HostVectors / TorchVectors) returns bit for bit what its host twin
    returns from the same inputs and the same device state -- the two forms run the same kernels with the same launch geometry and
    fixed-order reductions.  kind: 'flow' (nState 5), 'coupled' (6) or 'turb' (1) on one wall-bounded RANS block; the state on the
    device (w, p, rlv, rev with their halos) is put back before each call of a pair."""
    import ctypes
    lib = engine.lib
    coupled, turb = kind == "coupled", kind == "turb"
    blk, r, prm = checks.setup_block_with_bc(engine, dims, RANS_COUPLED if coupled else RANS_UPWIND, jm.WALL, seed, stretch_k=2.0)
    _KEEP[:] = [r]
    ns = 1 if turb else blk.nw if coupled else 5
    flags = engine._ankFlags(coupled, turb=turb, approxSA=turb)
    kflags = engine._ankFlags(coupled, turb=turb)
    engine.setupStateResidualMatrix(1, True, frozenTurb=kind == "flow", useTurbOnly=turb, useAD=True, approxSA=turb)
    engine.timeStep(1)
    engine.ankTimeStep(CFL, TURB_CFL_SCALE, coupled=coupled, turb=turb)
    engine.ankPcSetup(1)
    engine.ankSetBase(state_vector(engine, {1: blk}, blk.nw), coupled=True)       # p, rlv and rev of the state on the device
    engine.download_state(1, 1)
    start = {name: blk[name].copy() for name in ("w", "p", "rlv", "rev")}
    w0 = owned_vector({1: blk}, "w", blk.nw)[5::blk.nw].copy() if turb else owned_vector({1: blk}, "w", ns)
    n = w0.size
    rng = np.random.default_rng(seed)

    def reset():
        for name, a in start.items():
            blk[name][...] = a
        engine.upload_state(1, 1)

    def chk(rc):
        engine._chk(rc)

    def state():
        engine.download_state(1, 1)
        return blk["w"].copy()

    def evaluate():
        engine.blocketteRes(1, updateIntermed=False, flowRes=not turb, turbRes=turb or coupled, halo=True, closures=True)

    # set_w and get_r: the state each form leaves, and the vector each form takes from the residual of that state
    w1 = w0 * (1.0 + 1e-3 * rng.uniform(-1.0, 1.0, n))
    reset()
    engine.ankSetW(w1, coupled=coupled, turb=turb)
    s_host = state()
    evaluate()
    r_host = engine.ankGetR(coupled=coupled, turb=turb)
    reset()
    d_w1, d_r = dv.put(w1), dv.empty(n)
    chk(dev_call(engine, dv, lib.adflow_gpu_ank_set_w_dev, dv.ptr(d_w1), n, kflags))
    assert np.array_equal(state(), s_host, equal_nan=True), (kind, "ank_set_w_dev")
    evaluate()
    chk(dev_call(engine, dv, lib.adflow_gpu_ank_get_r_dev, dv.ptr(d_r), n, kflags))
    assert np.abs(r_host).max() > 0.0
    assert np.array_equal(dv.get(d_r), r_host), (kind, "ank_get_r_dev")

    # set_base (through the r0 it keeps), mult and last_h
    v = rng.uniform(-1.0, 1.0, n)
    reset()
    engine.ankSetBase(w0, coupled, turb=turb, approxSA=turb)
    r0_host = engine.ankGetR(coupled=coupled, turb=turb)
    y_host, h_host = engine.ankMult(v), engine.ankLastH()
    reset()
    d_w0, d_v, d_y = dv.put(w0), dv.put(v), dv.empty(n)
    chk(dev_call(engine, dv, lib.adflow_gpu_ank_set_base_dev, dv.ptr(d_w0), n, flags))
    assert np.array_equal(engine.ankGetR(coupled=coupled, turb=turb), r0_host), (kind, "ank_set_base_dev")
    dev_call(engine, dv, engine.ankMultDev, dv.ptr(d_v), dv.ptr(d_y), n)
    print(f"ank_mult / _dev {kind} {dims}: h = {h_host:.17e} / {engine.ankLastH():.17e}, max|y| = {np.abs(y_host).max():.3e}")
    assert h_host != 0.0 and np.abs(y_host).max() > 0.0
    assert engine.ankLastH() == h_host and np.array_equal(dv.get(d_y), y_host), (kind, "ank_mult_dev")

    # solve: b = the residual of the base state
    b = r0_host
    kw = dict(restart=cap, maxIts=cap, rtol=1e-4)
    reset()
    engine.ankSetBase(w0, coupled, turb=turb, approxSA=turb)
    x_host, *host = engine.ankSolve(b, 1, **kw)
    reset()
    engine.ankSetBase(w0, coupled, turb=turb, approxSA=turb)
    d_b, d_x = dv.put(b), dv.put(np.full(n, 7.0))
    dev = dev_call(engine, dv, engine.ankSolveDev, dv.ptr(d_b), dv.ptr(d_x), n, 1, **kw)
    print(f"ank_solve / _dev {kind} {dims}: (its, rnorm0, rnorm) = {tuple(host)} / {dev}")
    assert 0 < host[0] <= cap
    assert tuple(host) == dev and np.array_equal(dv.get(d_x), x_host), (kind, "ank_solve_dev")

    # the step limiter: a density update that limits, turbulence updates that are clipped (written back) and one that limits
    dw = 1e-3 * rng.uniform(-1.0, 1.0, n) * np.abs(w0)
    D, W = dw.reshape(-1, ns), w0.reshape(-1, ns)
    ncell = D.shape[0]
    if not turb:
        D[ncell // 3, 0] = -10.0 * W[ncell // 3, 0]
    if turb or coupled:
        D[5, ns - 1] = 200.0 * W[5, ns - 1]
        D[ncell - 7, ns - 1] = 1e4 * W[ncell - 7, ns - 1]
        D[ncell // 2, ns - 1] = 3.0 * W[ncell // 2, ns - 1]
    lam_host, out_host = engine.ankPhysicalityCheck(w0, dw, 1.0, coupled, turb=turb)
    d_dw, lam = dv.put(dw), ctypes.c_double(1.0)
    chk(dev_call(engine, dv, lib.adflow_gpu_ank_physicality_check_dev, dv.ptr(d_w0), dv.ptr(d_dw), n, kflags, 0.2, 0.99, 1.0, 0.01,
                 ctypes.byref(lam)))
    print(f"ank_physicality_check / _dev {kind}: lambda = {lam_host!r} / {lam.value!r}, {int((out_host != dw).sum())} entries clipped")
    assert 0.0 < lam_host < 1.0 and (out_host != dw).any() == (turb or coupled)
    assert lam.value == lam_host and np.array_equal(dv.get(d_dw), out_host), (kind, "ank_physicality_check_dev")

    # the line-search residual, with and without its norm
    dW, omega = 1e-3 * rng.uniform(-1.0, 1.0, n) * np.abs(w0), 0.7
    reset()
    engine.ankSetW(w0 - omega * dW, coupled=coupled, turb=turb)
    rr_host, nrm_host = engine.ankUnsteadyRes(dW, omega, coupled=coupled, turb=turb, approxSA=turb)
    d_dW = dv.put(dW)
    for norm in (True, False):
        reset()
        engine.ankSetW(w0 - omega * dW, coupled=coupled, turb=turb)
        d_rr = dv.put(np.full(n, 7.0))
        nrm = dev_call(engine, dv, engine.ankUnsteadyResDev, dv.ptr(d_dW), omega, dv.ptr(d_rr), n, flags, norm)
        assert np.array_equal(dv.get(d_rr), rr_host), (kind, "ank_unsteady_res_dev", norm)
        assert nrm == (nrm_host if norm else None), (kind, nrm, nrm_host)
    assert nrm_host > 0.0
    engine.pcRelease()
    engine.ankRelease()
    engine.releaseWorkspace()


def check_nk_residual_dev_twin(engine, dv, dims=(7, 6, 5), seed=433):
    """adflow_gpu_nk_residual_dev with two device vectors against adflow_gpu_nk_residual (one staging buffer for w and r), bit for
    bit, on one wall-bounded RANS block; some turbulence entries lie below the floor of setW"""
    blk, r, prm = checks.setup_block_with_bc(engine, dims, RANS_UPWIND, jm.WALL, seed, stretch_k=2.0)
    _KEEP[:] = [r]
    engine.download_state(1, 1)
    rng = np.random.default_rng(seed)
    w = owned_vector({1: blk}, "w", blk.nw)
    w *= 1.0 + 1e-3 * rng.uniform(-1.0, 1.0, w.size)
    w[5::7 * blk.nw] = 0.0
    engine.upload_state(1, 1)
    r_host = engine.FormFunction_mf(w)
    engine.upload_state(1, 1)
    d_w, d_r = dv.put(w), dv.empty(w.size)
    engine._chk(dev_call(engine, dv, engine.lib.adflow_gpu_nk_residual_dev, dv.ptr(d_w), dv.ptr(d_r), w.size))
    assert np.abs(r_host).max() > 0.0 and np.isfinite(r_host).all()
    assert np.array_equal(dv.get(d_r), r_host) and np.array_equal(dv.get(d_w), w)


# ---- 7. refusals and side effects ------------------------------------------------------------------------------------------------
def check_refusals_and_side_effects(engine, dims=(7, 6, 5)):
    lib = engine.lib
    engine.release_all()
    rm = RANS_JST
    ncell = int(np.prod(dims))

    def sequence(with_ank):
        """the same calls with or without the ANK entries in between; returns what must not depend on them"""
        blk, r, prm = checks.setup_block_with_bc(engine, dims, rm, jm.WALL, 367, stretch_k=2.0)
        _KEEP[:] = [r]
        out = {}
        w5 = state_vector(engine, {1: blk}, 5)
        w6 = state_vector(engine, {1: blk}, 6)
        rng = np.random.default_rng(373)
        x = rng.uniform(-1.0, 1.0, 5 * ncell)
        engine.setupStateResidualMatrix(1, True, frozenTurb=True, useAD=True)
        if with_ank:
            engine.timeStep(1)
            engine.ankTimeStep(CFL)
            engine.ankPcSetup(1)
            engine.referenceShockSensor(1)
            engine.ankSetBase(w5, dissApprox=True, viscApprox=True)
            engine.ankMult(x)
            xs, its, _, _ = engine.ankSolve(engine.ankGetR(), 1, restart=20, maxIts=20, rtol=1e-3)
            assert its > 0
            lam, _ = engine.ankPhysicalityCheck(w5, xs)
            assert 0.0 <= lam <= 1.0
            engine.ankSetW(w5)                                        # the state back from the perturbed one
        else:
            engine.timeStep(1)
            engine.referenceShockSensor(1)
            engine.setW(w6.copy())                                    # the plain counterpart of ankSetW: the same values, the same caches invalidated
        engine.blocketteRes(1, updateIntermed=False, flowRes=True, turbRes=True, halo=True, closures=True)
        out["blockRes"] = engine.download_residual(1, 1).copy()
        engine.pcSetup(1)
        out["gmres"] = engine.gmresSolve(x, 1, restart=20, maxIts=20, rtol=1e-6)
        out["nk"] = engine.FormFunction_mf(w6.copy())
        out["ws"] = engine.releaseWorkspace()
        return out, blk, w5, x

    plain, *_ = sequence(False)
    ank, blk, w5, x = sequence(True)
    print("blockRes after the ANK sequence: max difference", np.abs(plain["blockRes"] - ank["blockRes"]).max(), "of", np.abs(plain["blockRes"]).max(),
          "at", np.unravel_index(np.abs(plain["blockRes"] - ank["blockRes"]).argmax(), plain["blockRes"].shape))
    assert np.array_equal(plain["blockRes"], ank["blockRes"]), "ankSetW(w) + blockRes after a full ANK sequence"
    assert np.array_equal(plain["gmres"][0], ank["gmres"][0]) and plain["gmres"][1:] == ank["gmres"][1:], "gmresSolve"
    assert np.array_equal(plain["nk"], ank["nk"]), "nkResidual"
    assert plain["ws"] == ank["ws"] > 0, "releaseWorkspace's byte count"
    held = engine.ankRelease()
    assert held >= 8 * (5 * ncell + 2 * 5 * ncell) and engine.ankRelease() == 0
    # every refusal with its cause
    y = np.zeros_like(x)
    with pytest.raises(capi.AdflowGpuError, match="no pseudo-time term"):
        engine.ankPcSetup(1)
    with pytest.raises(capi.AdflowGpuError, match="no pseudo-time term"):
        engine.ankTimeStepBlocks(1)
    with pytest.raises(capi.AdflowGpuError, match="no base state"):
        engine.ankMult(x)
    with pytest.raises(capi.AdflowGpuError, match="no base state"):
        engine.ankSolve(x, 1)
    with pytest.raises(capi.AdflowGpuError, match="no base state"):
        engine.ankLastH()
    engine.timeStep(1)
    engine.ankTimeStep(CFL, TURB_CFL_SCALE, coupled=True)
    with pytest.raises(capi.AdflowGpuError, match="nState = 6, the assembled matrix has nState = 5"):
        engine.ankPcSetup(1)                                          # a coupled T against an ADFLOW_JAC_FROZEN_TURB matrix
    with pytest.raises(capi.AdflowGpuError, match="not the level of the assembly"):
        engine.ankPcSetup(2)
    engine.ankSetBase(w5)
    with pytest.raises(capi.AdflowGpuError, match="pseudo-time term was formed for nState = 6"):
        engine.ankMult(x)
    engine.ankTimeStep(CFL)
    engine.pcRelease()
    with pytest.raises(capi.AdflowGpuError, match="no factor"):
        engine.ankSolve(x, 1)
    engine.setupStateResidualMatrix(1, True, useAD=True)               # nState = 6
    engine.pcSetup(1)
    with pytest.raises(capi.AdflowGpuError, match="factor was set up for nState = 6, the base state has nState = 5"):
        engine.ankSolve(x, 1)
    engine.setupStateResidualMatrix(1, False, frozenTurb=True, delta=1e-6)
    with pytest.raises(capi.AdflowGpuError, match="33-point stencil"):
        engine.ankPcSetup(1)
    for fn, args, msg in ((lib.adflow_gpu_ank_mult, (x.ctypes.data, x.ctypes.data, x.size), "same vector"),
                          (lib.adflow_gpu_ank_mult_dev, (x.ctypes.data, None, x.size), "is NULL"),
                          (lib.adflow_gpu_ank_mult, (x.ctypes.data, y.ctypes.data, x.size + 5), "rows"),
                          (lib.adflow_gpu_ank_set_w, (x.ctypes.data, 6 * ncell, 0), "nState = 5"),
                          (lib.adflow_gpu_ank_set_base, (x.ctypes.data, 5 * ncell, capi.ANK_COUPLED), "nState = 6"),
                          (lib.adflow_gpu_ank_set_base, (x.ctypes.data, 5 * ncell, 8), "flags"),
                          (lib.adflow_gpu_ank_time_step, (1, 0.0, 1.0, 0), "cfl"),
                          (lib.adflow_gpu_ank_solve, (2, x.ctypes.data, y.ctypes.data, x.size, 5, 5, 1e-3, 0.0, None, None, None), "level 2"),
                          (lib.adflow_gpu_ank_solve, (1, x.ctypes.data, x.ctypes.data, x.size, 5, 5, 1e-3, 0.0, None, None, None), "same vector"),
                          (lib.adflow_gpu_ank_physicality_check, (x.ctypes.data, x.ctypes.data, x.size, 0, 0.2, 0.99, 1.0, 0.01, None), "lambda is NULL")):
        assert fn(*args) != 0, msg
        assert msg in lib.adflow_gpu_last_error().decode(), (msg, lib.adflow_gpu_last_error().decode())
    engine.release_all()
    assert engine.ankRelease() == 0                                   # released with the blocks
