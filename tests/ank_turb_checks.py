"""Checks of the turbulence half of the approximate Newton-Krylov step on the device (approxSA, the turbulence KSP behind
ADFLOW_ANK_TURB, the line-search residual adflow_gpu_ank_unsteady_res, the two factor slots), shared by tests/test_gpu_ank_turb.py
(real MI355X) and tests/test_hostsim_ank_turb.py (the kernel-logic emulator).  cfl = 5 and turbCFLScale = 2.5 as in ank_checks.

Yardsticks: the reference's own blocketteResCore with approxSA set; T_t from its formula in numpy; the shifted factor against
pc_checks.NumpyILU0 of J_t + T_t; the operator against J_t v + T_t v with the library's forward-mode TURB_ONLY blocks applied in
numpy, next to the reference's own difference quotient with the same h; the step limiter against a numpy restatement of
physicalityCheckANKTurb; the unsteady residual against numpy on the downloaded dw, volRef and T."""
import contextlib

import numpy as np
import pytest

import ank_checks as ank
import checks
import jacmult_checks as jm
import pc_checks as pc
from adflow_amd import capi
from util import TOL, LOCAL_TOL, rel_err, rel_err_local, owned

EPS, CFL, TCS, MARGIN = ank.EPS, ank.CFL, ank.TURB_CFL_SCALE, ank.MARGIN
RANS = pc.RANS
_KEEP = ank._KEEP


@contextlib.contextmanager
def ref_approx_sa(on=True):
    """the reference's approxSA for the calls inside; ref.set_params / bind_block reset it, so it is set after the setup"""
    from oracle import ref
    ref.load().ref_set_int(b"approxSA", 1 if on else 0)
    try:
        yield
    finally:
        ref.load().ref_set_int(b"approxSA", 0)


def setup(engine, dims, seed, prm=RANS):
    blk, r, prm = checks.setup_block_with_bc(engine, dims, prm, jm.WALL, seed, stretch_k=2.0)
    _KEEP[:] = [r]
    return blk, r, prm


def turb_vector(blocks):
    return np.concatenate([np.ascontiguousarray(np.transpose(blocks[nn].owned("w")[..., 5], (2, 1, 0))).reshape(-1) for nn in sorted(blocks)])


def turb_field(blk, vec):
    return np.transpose(vec.reshape(blk.nz, blk.ny, blk.nx), (2, 1, 0))


# ---- 1. the approxSA residual ------------------------------------------------------------------------------------------------
def check_approx_sa_residual(engine, dims, seed=401):
    from oracle import ref
    blk, r, prm = setup(engine, dims, seed)
    ref.blockette_res_core(False, False, True)
    full_ref = owned(blk, r["dw"][..., 5]).copy()
    with ref_approx_sa():
        ref.blockette_res_core(False, False, True)
        approx_ref = owned(blk, r["dw"][..., 5]).copy()
    differs = full_ref != approx_ref
    assert differs.any()
    try:
        for sm in (1, 0):
            engine.set_tuning("sa_march", sm)
            engine.blocketteRes(1, updateIntermed=False, flowRes=False, turbRes=True)
            plain = owned(blk, engine.download_residual(1, 1)[..., 5]).copy()
            engine.blocketteRes(1, updateIntermed=False, flowRes=False, turbRes=True, approxSA=True)
            flagged = owned(blk, engine.download_residual(1, 1)[..., 5]).copy()
            e, el = rel_err(flagged, approx_ref), rel_err_local(flagged, approx_ref)
            e0 = rel_err(plain, full_ref)
            print(f"approxSA residual {dims} sa_march={sm}: relative {e:.3e}, local {el:.3e}; without the flag {e0:.3e}; "
                  f"{int(differs.sum())} of {differs.size} cells differ in the reference")
            assert e <= TOL and el <= max(LOCAL_TOL, 1e4 * TOL), (sm, e, el)
            assert e0 <= TOL, (sm, e0)
            assert (plain != flagged)[differs].all(), "the flag does not reach every cell where the reference's two results differ"
            engine.blocketteRes(1, updateIntermed=False, flowRes=False, turbRes=True)
            assert np.array_equal(owned(blk, engine.download_residual(1, 1)[..., 5]), plain), "the unflagged call after a flagged one"
    finally:
        engine.set_tuning("sa_march", 1)


def check_turb_first_order(engine, dims, seed=403):
    from adflow_amd.params import firstOrder, secondOrder
    out = {}
    for order, flag in ((secondOrder, True), (firstOrder, False), (secondOrder, False)):
        blk, r, prm = setup(engine, dims, seed, RANS.replace(orderTurb=order))
        engine.blocketteRes(1, updateIntermed=False, flowRes=False, turbRes=True, turbFirstOrder=flag)
        out[(order, flag)] = owned(blk, engine.download_residual(1, 1)[..., 5]).copy()
        if flag:          # the option is back: an unflagged call is second order again
            engine.blocketteRes(1, updateIntermed=False, flowRes=False, turbRes=True)
            again = owned(blk, engine.download_residual(1, 1)[..., 5]).copy()
    assert np.array_equal(out[(secondOrder, True)], out[(firstOrder, False)])
    assert not np.array_equal(out[(secondOrder, False)], out[(firstOrder, False)])
    assert np.array_equal(again, out[(secondOrder, False)])


# ---- 2. the approxSA assembly ------------------------------------------------------------------------------------------------
def check_approx_sa_assembly(engine, dims=(10, 7, 6), seed=405):
    """TURB_ONLY | PC | APPROX_SA by finite differences and by forward mode against the reference's routines with approxSA = 1 (the
    rules of checks.check_fd_jacobian / check_ad_jacobian: relative to the largest entry, 1e-9 at delta = 1e-5, 1e-10 forward mode)"""
    from oracle import ref
    blk, r, prm = setup(engine, dims, seed)
    with ref_approx_sa():
        Jfd = ref.fd_jacobian(blk.nx, blk.ny, blk.nz, True, False, True, False, False, 1e-5)
        Jad = ref.ad_jacobian(blk.nx, blk.ny, blk.nz, True, False, True, False)
    Jad_full = ref.ad_jacobian(blk.nx, blk.ny, blk.nz, True, False, True, False)
    assert np.abs(Jad - Jad_full).max() > 1e-6 * np.abs(Jad).max()          # the switch matters to the matrix
    for useAD, Jr, tol in ((False, Jfd, 1e-9), (True, Jad, 1e-10)):
        engine.setupStateResidualMatrix(1, True, useTurbOnly=True, delta=1e-5, useAD=useAD, approxSA=True)
        Jg = engine.jacobianBlocks(1, 1)
        assert Jg.shape == Jr.shape
        err = np.abs(Jg - Jr).max() / np.abs(Jr).max()
        print(f"approxSA TURB_ONLY matrix {dims} useAD={useAD}: {err:.3e} of the largest entry")
        assert err <= tol, (useAD, err)
    engine.setupStateResidualMatrix(1, True, useTurbOnly=True, useAD=True)
    errf = np.abs(engine.jacobianBlocks(1, 1) - Jad_full).max() / np.abs(Jad_full).max()
    assert errf <= 1e-10, errf                                               # and the unflagged assembly is the full one
    with ref_approx_sa():
        Jc = ref.ad_jacobian(blk.nx, blk.ny, blk.nz, True, False, False, False)
    engine.setupStateResidualMatrix(1, True, useAD=True, approxSA=True)
    Jg = engine.jacobianBlocks(1, 1)
    err = np.abs(Jg - Jc).max() / np.abs(Jc).max()
    errm = np.abs(Jg[..., :5, :5, :] - Jc[..., :5, :5, :]).max() / np.abs(Jc[..., :5, :5, :]).max()
    print(f"approxSA coupled PC matrix {dims}: {err:.3e}, mean-flow blocks {errm:.3e}")
    assert err <= 1e-10 and errm <= 1e-10, (err, errm)


# ---- 3. the turbulence T and the shifted factor ----------------------------------------------------------------------------------
def numpy_T_turb(engine, blocks, prm):
    Tf = ank.numpy_T(engine, blocks, prm, False)
    return {nn: (Tf[nn][0, 0] * (prm.turbResScale / TCS))[None, None] for nn in blocks}


def assert_T_turb(engine, blocks, prm, what):
    engine.timeStep(1)
    engine.ankTimeStep(CFL, TCS, turb=True)
    Tn = numpy_T_turb(engine, blocks, prm)
    for nn in blocks:
        assert_T_turb_block(engine.ankTimeStepBlocks(nn, turb=True), Tn[nn], blocks[nn], f"{what} block {nn}")
    return Tn


def assert_T_turb_block(Tl, Tn, blk, what):
    """the library's T_t of one block against the formula's: 16 eps"""
    assert Tl.shape == Tn.shape == (1, 1, blk.nx, blk.ny, blk.nz)
    rel = np.abs(Tl - Tn) / np.abs(Tn)
    print(f"T_t {what}: max relative difference {rel.max() / EPS:.2f} eps")
    assert rel.max() <= 16 * EPS and np.abs(Tl).min() > 0.0


def turb_operator(engine, blk, approxSA):
    engine.setupStateResidualMatrix(1, True, useTurbOnly=True, useAD=True, approxSA=approxSA)
    op = jm.operator_of(engine, {1: blk})
    assert op.ns == 1
    return op


def check_shifted_factor(engine, dims, seed=407):
    blk, r, prm = setup(engine, dims, seed)
    op = turb_operator(engine, blk, True)
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, op.n)
    engine.pcSetup(1)
    plain = {tr: engine.pcApply(x, 1, transpose=tr) for tr in (False, True)}
    with pytest.raises(capi.AdflowGpuError, match="no pseudo-time term of the turbulence KSP"):
        engine.ankPcSetup(1)
    engine.timeStep(1)
    engine.ankTimeStep(CFL)                                              # a flow T alone does not serve a TURB_ONLY matrix
    with pytest.raises(capi.AdflowGpuError, match="no pseudo-time term of the turbulence KSP"):
        engine.ankPcSetup(1)
    Tflow = engine.ankTimeStepBlocks(1)
    Tn = assert_T_turb(engine, {1: blk}, prm, f"{dims}")
    assert np.array_equal(engine.ankTimeStepBlocks(1), Tflow)            # side by side
    engine.ankPcSetup(1)
    assert engine.pcInfo()[:2] == (1, sum(dims) - 2)
    pc.assert_apply_matches(engine, ank.shifted(op, Tn), seed + 1, f"shifted turbulence factor {dims}")
    assert not np.array_equal(engine.pcApply(x, 1), plain[False]), "T does not reach the factor"
    engine.pcSetup(1)
    for tr in (False, True):
        assert np.array_equal(engine.pcApply(x, 1, transpose=tr), plain[tr]), ("pcSetup after the ANK entries", tr)
    engine.pcRelease()
    engine.ankRelease()


# ---- 4. the operator -------------------------------------------------------------------------------------------------------------
class RefTurbResidual:
    """R_t(w) of FormFunction_mf_turb on one block: setWANK(nt1, nt2) and setRVecANKTurb restated in numpy, everything between them the
    reference's own routines (blocketteResCore without the flow residual)"""

    def __init__(self, r, prm):
        self.r, self.prm = r, prm

    def __call__(self, wt):
        from oracle import ref
        r = self.r
        r.owned("w")[..., 5] = turb_field(r, wt)
        ref.call_level("setPointers", 1, 1)
        ref.call("computePressureSimple", 0)
        ref.call("computeLamViscosity", 0)
        ref.call("computeEddyViscosity", 0)
        ref.call("bcTurbTreatment")
        ref.call("applyAllTurbBCThisBlock", 1)
        ref.call("applyAllBC_block", 1)
        ref.call_level("whalo2", 1, 1, 6)
        ref.call_level("setPointers", 1, 1)
        ref.blockette_res_core(False, False, True)
        res = r.owned("dw")[..., 5] / r.owned("volRef") * self.prm.turbResScale
        return np.ascontiguousarray(np.transpose(res, (2, 1, 0))).reshape(-1)


def setup_turb_operator(engine, dims, approxSA, seed, prm=RANS):
    blk, r, prm = setup(engine, dims, seed, prm)
    op = turb_operator(engine, blk, approxSA)
    Tn = assert_T_turb(engine, {1: blk}, prm, f"{dims}")
    engine.download_state(1, 1)
    w0 = turb_vector({1: blk})
    Rref = RefTurbResidual(r, prm)
    with ref_approx_sa(approxSA):
        Rref.r0 = Rref(w0)
    # pressure and laminar viscosity on the device from the closures of the state write (the turbulence entries keep them)
    engine.ankSetBase(ank.state_vector(engine, {1: blk}, 6), coupled=True)
    engine.ankSetBase(w0, turb=True, approxSA=approxSA)
    return blk, Rref, op, Tn, w0


def check_operator(engine, dims, approxSA, seed=409, edge_cases=False, prm=RANS):
    blk, Rref, op, Tn, w0 = setup_turb_operator(engine, dims, approxSA, seed, prm)
    what = f"turbulence operator {dims} approxSA={approxSA}"
    b = engine.ankGetR(turb=True)
    assert np.abs(b - Rref.r0).max() <= 1e-9 * np.abs(Rref.r0).max()
    engine.download_state(1, 1)
    rev_base, rlv_base, p_base = blk.owned("rev").copy(), blk.owned("rlv").copy(), blk.owned("p").copy()
    rng = np.random.default_rng(seed + 1)
    v = rng.uniform(-1.0, 1.0, w0.size)
    y = engine.ankMult(v)
    h, hn = engine.ankLastH(), ank.ds_step(w0, v)
    assert abs(h - hn) <= 1e-12 * abs(hn), (h, hn)
    # the eddy viscosity the turbulence state write left against ank_set_w + the full closures for w + h v
    engine.download_state(1, 1)
    rev_fast, rlv_fast, p_fast = blk.owned("rev").copy(), blk.owned("rlv").copy(), blk.owned("p").copy()
    assert np.array_equal(turb_vector({1: blk}), w0 + h * v)
    assert np.array_equal(rlv_fast, rlv_base) and np.array_equal(p_fast, p_base), "the turbulence state write moved p or rlv"
    assert not np.array_equal(rev_fast, rev_base)
    # the issue's rule, every owned cell: the state write with the full closures_cell first (it leaves p, rlv and rev of w + h v),
    # then the turbulence state write of the same nuTilde, which reads that rho and rlv: rev is bit-equal, p and rlv stand
    w6 = ank.state_vector(engine, {1: blk}, 6)
    assert np.array_equal(w6[5::6], w0 + h * v)
    engine.ankSetBase(w6, coupled=True)
    engine.download_state(1, 1)
    rev_full, rlv_full, p_full = blk.owned("rev").copy(), blk.owned("rlv").copy(), blk.owned("p").copy()
    engine.ankSetBase(w0 + h * v, turb=True, approxSA=approxSA)
    engine.download_state(1, 1)
    assert np.array_equal(blk.owned("rlv"), rlv_full) and np.array_equal(blk.owned("p"), p_full)
    assert np.array_equal(blk.owned("rev"), rev_full), "eddy viscosity of the turbulence state write against the full closures"
    ulp = np.abs(rev_fast - rev_full) / (EPS * np.abs(rev_full))
    print(f"{what}: rev after the product against the full closures of the re-formed energy: at most {ulp.max():.1f} ulp")
    assert ulp.max() <= 8.0          # (rlv there comes from an energy whalo2 re-formed: E -> p -> E rounding, a few ulp through rlv and chi^3)
    engine.ankSetBase(w0, turb=True, approxSA=approxSA)
    def quotient(h, v):
        with ref_approx_sa(approxSA):
            return (Rref(w0 + h * v) - Rref.r0) / h
    _, bar, e_lib = ank.assert_product(what, y, v, h, op, Tn, blk, quotient)
    e_ref = bar / MARGIN
    if edge_cases:
        assert not engine.ankMult(np.zeros_like(w0)).any() and engine.ankLastH() == 0.0
    engine.ankSetW(w0, turb=True)
    engine.ankRelease()
    return e_lib, e_ref


# ---- 5. the solve ----------------------------------------------------------------------------------------------------------------
def check_solve(engine, dims, cap, seed=411):
    rtol = 1e-4
    blk, Rref, op, Tn, w0 = setup_turb_operator(engine, dims, True, seed)
    ops = ank.shifted(op, Tn)
    engine.ankPcSetup(1)
    b = engine.ankGetR(turb=True)
    nb = float(np.linalg.norm(b))
    assert nb > 0.0
    x, its, r0, rn = engine.ankSolve(b, 1, restart=cap, maxIts=cap, rtol=rtol)
    ank.assert_solve(f"ankSolve(turb) {dims}", its, r0, b, x, ops, cap, rtol)
    rn_np = float(np.linalg.norm(b - engine.ankMult(x)))
    print(f"ankSolve(turb) {dims}: reported {rn / nb:.3e}, through ankMult {rn_np / nb:.3e}")
    assert abs(rn - rn_np) <= 1e-10 * rn_np, (rn, rn_np)
    engine.ankSetW(w0, turb=True)
    engine.pcRelease()
    engine.ankRelease()


# ---- 6. the step limiter ---------------------------------------------------------------------------------------------------------
def numpy_physicality_turb(w, dw, lam, tolTurb, stepFactor, stepMin):
    eps = 1e-25
    D = dw.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        rt = (w / (D + eps)) * tolTurb
        low = rt < stepFactor * stepMin
        clip = low & (rt > 0.0)
        D[clip] = w[clip] * tolTurb
        allr = np.concatenate([np.where(low, 1.0, rt), np.array([lam])])
    return (0.0 if np.isnan(allr).any() else float(allr.min())), D, clip


def check_physicality(engine, topo, seed=413):
    blocks, _ = checks.setup_brick(engine, topo, RANS, seed)
    tolTurb, stepFactor, stepMin = 0.99, 1.0, 0.01
    thr = stepFactor * stepMin
    rng = np.random.default_rng(seed)
    w = turb_vector(blocks)
    n = w.size
    assert n > 4 * 256 and (w > 0.0).all()
    base = -1e-3 * rng.uniform(0.1, 1.0, n) * w                          # updates that raise nuTilde: w - lambda dw grows

    def case(edit, lam0=1.0):
        dw = base.copy()
        edit(dw)
        lam, out = engine.ankPhysicalityCheck(w, dw, lam0, turb=True, physLSTolTurb=tolTurb, stepFactor=stepFactor, stepMin=stepMin)
        lam_np, out_np, clip = numpy_physicality_turb(w, dw, lam0, tolTurb, stepFactor, stepMin)
        assert lam == lam_np, (lam, lam_np)
        assert np.array_equal(out, out_np, equal_nan=True)
        return lam, dw, out, clip

    lam, _, out, clip = case(lambda D: None)
    assert lam == 1.0 and not clip.any()                                  # negative ratios: below the threshold, not positive: kept
    assert case(lambda D: None, lam0=0.5)[0] == 0.5
    c1, c2, c3 = n // 3, n - 7, 5

    def edges(D):
        D[c1] = w[c1] * tolTurb / (thr * (1.0 - 1e-3))                    # ratio just below the threshold, positive: clipped, no limit
        D[c2] = w[c2] * tolTurb / (thr * (1.0 + 1e-3))                    # just above: limits the step
        D[c3] = 3.0 * w[c3]                                               # ratio 0.33: limits less
    lam, dw, out, clip = case(edges)
    assert clip[c1] and not clip[c2] and not clip[c3] and clip.sum() == 1
    assert out[c1] == w[c1] * tolTurb and out[c2] == dw[c2]
    assert thr <= lam <= thr * (1.0 + 2e-3)

    def nan(D):
        D[c2] = np.nan
    assert case(nan)[0] == 0.0
    engine.ankRelease()


# ---- 7. the unsteady residual ----------------------------------------------------------------------------------------------------
def assert_unsteady(what, rr, nrm, dwd, blk, prm, Tn, dW, omega, kind):
    """the line-search residual rr = R(w) - omega T dW and its norm against numpy on the downloaded dw (the steady residual of the
    state), volRef and T: 8 eps (|R| + |omega T dW|) entry by entry, the norm to n eps"""
    coupled, turb = kind == "coupled", kind == "turb"
    ns = 1 if turb else (6 if coupled else 5)
    if turb:
        st_np = owned(blk, dwd[..., 5]) / blk.owned("volRef") * prm.turbResScale
        st_np = np.ascontiguousarray(np.transpose(st_np, (2, 1, 0))).reshape(-1)
    else:
        st_np = owned(blk, dwd[..., :ns]) / blk.owned("volRef")[..., None]
        if coupled:
            st_np[..., 5] *= prm.turbResScale
        st_np = np.ascontiguousarray(np.transpose(st_np, (2, 1, 0, 3))).reshape(-1)
    TdW = ank.T_times(Tn, {1: blk}, dW)
    r_np = st_np - omega * TdW
    bound = 8 * EPS * (np.abs(st_np) + abs(omega) * np.abs(TdW))
    worst = float((np.abs(rr - r_np) / np.maximum(bound, 1e-300)).max())
    n = rr.size
    print(f"{what}: worst |r - r_np| / bound = {worst:.3f}, norm {nrm:.6e}, relative to numpy "
          f"{abs(nrm - np.linalg.norm(rr)) / np.linalg.norm(rr) / EPS:.2f} eps (bound {n} eps)")
    assert (np.abs(rr - r_np) <= bound).all(), worst
    assert np.abs(TdW).max() > 0.0 and np.abs(st_np).max() > 0.0
    assert abs(nrm - float(np.linalg.norm(rr))) <= n * EPS * float(np.linalg.norm(rr))


def check_unsteady(engine, dims, kind, seed=415, prm=None):
    """kind: 'flow' (decoupled), 'coupled' or 'turb'"""
    coupled, turb = kind == "coupled", kind == "turb"
    prm = prm or (ank.RANS_COUPLED if coupled else RANS)
    blk, r, prm = setup(engine, dims, seed, prm)
    ns = 1 if turb else (6 if coupled else 5)
    engine.timeStep(1)
    engine.ankTimeStep(CFL, TCS, coupled=coupled, turb=turb)
    Tn = numpy_T_turb(engine, {1: blk}, prm) if turb else ank.numpy_T(engine, {1: blk}, prm, coupled)
    w0 = turb_vector({1: blk}) if turb else ank.state_vector(engine, {1: blk}, ns)
    rng = np.random.default_rng(seed)
    dW = 1e-3 * rng.uniform(-1.0, 1.0, w0.size) * np.abs(w0)
    omega = 0.7
    engine.ankSetW(w0 - omega * dW, coupled=coupled, turb=turb)
    rr, nrm = engine.ankUnsteadyRes(dW, omega, coupled=coupled, turb=turb)
    # dw on the device is the steady residual of that state
    dwd = engine.download_residual(1, 1).copy()
    assert_unsteady(f"unsteady residual {kind} {dims}", rr, nrm, dwd, blk, prm, Tn, dW, omega, kind)
    # (the evaluation is blocketteRes: its whalo2 re-forms the owned energy from the pressure, so the caller's state goes in again)
    engine.ankSetW(w0 - omega * dW, coupled=coupled, turb=turb)
    rr2, nrm2 = engine.ankUnsteadyRes(dW, omega, coupled=coupled, turb=turb)
    assert nrm2 == nrm and np.array_equal(rr2, rr)
    r0, _ = engine.ankUnsteadyRes(dW, 0.0, coupled=coupled, turb=turb)
    assert np.array_equal(r0, engine.ankGetR(coupled=coupled, turb=turb)), "omega = 0 against ankGetR"
    # the evaluation in front of the pass is blocketteRes(useFlowRes, useTurbRes) with its closures, boundary conditions and whalo2
    # at the caller's state, with the residual flags passed on: dw against that call of the library itself, bit for bit
    lo, hi = (5, 6) if turb else (0, ns)
    for fl in (dict(), dict(approxSA=True, turbFirstOrder=True), dict(dissApprox=True, viscApprox=True, useBlockettes=True)):
        if fl.get("dissApprox"):
            engine.referenceShockSensor(1)
        engine.ankSetW(w0 - omega * dW, coupled=coupled, turb=turb)
        engine.ankUnsteadyRes(dW, omega, coupled=coupled, turb=turb, **fl)
        got = owned(blk, engine.download_residual(1, 1))[..., lo:hi].copy()
        if not fl:
            assert np.array_equal(got, owned(blk, dwd)[..., lo:hi])
        engine.ankSetW(w0 - omega * dW, coupled=coupled, turb=turb)
        engine.blocketteRes(1, updateIntermed=False, flowRes=not turb, turbRes=turb or coupled, halo=True, closures=True, **fl)
        want = owned(blk, engine.download_residual(1, 1))[..., lo:hi]
        assert np.array_equal(got, want), ("the evaluation of ankUnsteadyRes", kind, fl)
        if (fl.get("approxSA") and (turb or coupled)) or (fl.get("dissApprox") and not turb):
            assert not np.array_equal(got, owned(blk, dwd)[..., lo:hi]), ("the flags do not reach the evaluation", kind, fl)
    engine.ankSetW(w0, coupled=coupled, turb=turb)
    engine.ankRelease()


def check_dev_twins(engine, dv, dims, cap):
    """the _dev entries of the turbulence kind (nState 1, approxSA) against their host twins, bit for bit: ank_checks.check_dev_twins"""
    ank.check_dev_twins(engine, dv, dims, "turb", cap, seed=421)


# ---- 8. the factor slots ---------------------------------------------------------------------------------------------------------
def check_slots(engine, dims, seed=417):
    blk, r, prm = setup(engine, dims, seed)
    ncell = int(np.prod(dims))
    rng = np.random.default_rng(seed)
    x5, x1 = rng.uniform(-1.0, 1.0, 5 * ncell), rng.uniform(-1.0, 1.0, ncell)
    engine.download_state(1, 1)
    wt = turb_vector({1: blk})
    engine.timeStep(1)
    engine.ankTimeStep(CFL)
    engine.ankTimeStep(CFL, TCS, turb=True)
    engine.setupStateResidualMatrix(1, True, frozenTurb=True, useAD=True)
    engine.pcSelect(0)
    engine.ankPcSetup(1)
    z5 = engine.pcApply(x5, 1)
    ns0, _, bytes0 = engine.pcInfo()
    engine.setupStateResidualMatrix(1, True, useTurbOnly=True, useAD=True, approxSA=True)
    engine.pcSelect(1)
    with pytest.raises(capi.AdflowGpuError, match="no factor"):
        engine.pcInfo()
    engine.ankPcSetup(1)
    z1 = engine.pcApply(x1, 1)
    ns1, _, bytes1 = engine.pcInfo()
    assert (ns0, ns1) == (5, 1) and bytes0 > bytes1 > 0
    engine.pcSelect(0)
    assert np.array_equal(engine.pcApply(x5, 1), z5) and engine.pcInfo()[2] == bytes0
    engine.ankSetBase(wt, turb=True, approxSA=True)
    with pytest.raises(capi.AdflowGpuError, match="factor was set up for nState = 5, the base state has nState = 1"):
        engine.ankSolve(x1, 1)
    engine.pcSelect(1)
    assert np.array_equal(engine.pcApply(x1, 1), z1)
    x, its, _, _ = engine.ankSolve(engine.ankGetR(turb=True), 1, restart=5, maxIts=5, rtol=1e-2)
    assert its > 0 and np.isfinite(x).all()
    engine.ankSetW(wt, turb=True)
    with pytest.raises(capi.AdflowGpuError, match="slot 2"):
        engine.pcSelect(2)
    assert engine.pcRelease() == bytes1 and engine.pcRelease() == 0
    engine.pcSelect(0)
    assert engine.pcInfo()[2] == bytes0 and np.array_equal(engine.pcApply(x5, 1), z5)
    engine.pcSelect(1)
    engine.pcSetup(1)
    engine.pcSelect(0)
    engine.release_all()                                                   # both slots go with the blocks
    for s in (0, 1):
        engine.pcSelect(s)
        assert engine.pcRelease() == 0
    engine.pcSelect(0)


# ---- 9. refusals and side effects --------------------------------------------------------------------------------------------------
def check_refusals_and_side_effects(engine, dims=(7, 5, 4), seed=419):
    lib = engine.lib
    blk, r, prm = setup(engine, dims, seed)
    ncell = int(np.prod(dims))
    rng = np.random.default_rng(seed)
    engine.download_state(1, 1)
    wt = turb_vector({1: blk})
    w5 = ank.state_vector(engine, {1: blk}, 5)
    x1, x5 = rng.uniform(-1.0, 1.0, ncell), rng.uniform(-1.0, 1.0, 5 * ncell)
    import ctypes
    y1, nrmv = np.zeros(ncell), ctypes.c_double(0.0)
    nrm = ctypes.byref(nrmv)
    T, C = capi.ANK_TURB, capi.ANK_COUPLED
    for fn, args, msg in ((lib.adflow_gpu_ank_set_w, (x1.ctypes.data, ncell, T | C), "excludes ADFLOW_ANK_COUPLED"),
                          (lib.adflow_gpu_ank_time_step, (1, CFL, TCS, T | C), "excludes ADFLOW_ANK_COUPLED"),
                          (lib.adflow_gpu_ank_set_w, (x1.ctypes.data, ncell + 1, T), "nState = 1"),
                          (lib.adflow_gpu_ank_set_base, (x5.ctypes.data, 5 * ncell, T), "nState = 1"),
                          (lib.adflow_gpu_ank_time_step, (1, CFL, 0.0, T), "turbCFLScale"),
                          (lib.adflow_gpu_ank_unsteady_res, (x1.ctypes.data, 0.5, y1.ctypes.data, ncell, T, nrm), "no pseudo-time term of the turbulence KSP"),
                          (lib.adflow_gpu_ank_unsteady_res, (x5.ctypes.data, 0.5, x5.ctypes.data, 5 * ncell, 0, nrm), "same vector"),
                          (lib.adflow_gpu_ank_download_time_step_turb, (1, y1.ctypes.data, T), "no pseudo-time term of the turbulence KSP"),
                          (lib.adflow_gpu_ank_physicality_check, (x1.ctypes.data, y1.ctypes.data, ncell, T | 32, 0.2, 0.99, 1.0, 0.01, nrm), "flags"),
                          (lib.adflow_gpu_pc_select, (-1,), "slot -1")):
        assert fn(*args) != 0, msg
        assert msg in lib.adflow_gpu_last_error().decode(), (msg, lib.adflow_gpu_last_error().decode())
    with pytest.raises(capi.AdflowGpuError, match="no base state"):
        engine.ankMult(x1)
    with pytest.raises(capi.AdflowGpuError, match="no base state of the turbulence KSP"):
        engine.ankSelectBase(turb=True)
    # the flow kind's T and base survive every turbulence entry, and the other way round
    engine.timeStep(1)
    engine.ankTimeStep(CFL)
    Tflow = engine.ankTimeStepBlocks(1)
    def turb_halos():
        """nuTilde and the eddy viscosity of the halos as the library's own turbulence evaluation at wt leaves them (the decoupled
        flow operator applies no turbulence boundary condition, as blocketteRes(useTurbRes = F))"""
        engine.ankSetW(wt, turb=True)
        engine.blocketteRes(1, updateIntermed=False, flowRes=False, turbRes=True, halo=True, closures=True)

    turb_halos()
    engine.ankSetBase(w5)
    y5 = engine.ankMult(x5)
    engine.ankSetW(w5)
    engine.setupStateResidualMatrix(1, True, useTurbOnly=True, useAD=True)
    J0 = engine.jacobianBlocks(1, 1).copy()
    engine.download_state(1, 1)
    state0 = blk["w"].copy()
    w6 = ank.state_vector(engine, {1: blk}, 6)
    engine.blocketteRes(1, updateIntermed=False, flowRes=True, turbRes=True, halo=True, closures=True)
    res0 = owned(blk, engine.download_residual(1, 1)).copy()
    engine.setW(w6.copy())                                               # (the evaluation's whalo2 re-forms the owned energy)
    engine.ankTimeStep(CFL, TCS, turb=True)
    Tturb = engine.ankTimeStepBlocks(1, turb=True)
    engine.ankSetBase(wt, turb=True)
    with pytest.raises(capi.AdflowGpuError, match="rows"):
        engine.ankMult(x5)                                               # the base set last is the turbulence one
    yt = engine.ankMult(x1)
    engine.ankPhysicalityCheck(wt, x1, turb=True)
    engine.ankSetW(wt, turb=True)
    engine.ankUnsteadyRes(x1, 0.5, turb=True)
    engine.ankUnsteadyRes(x5, 0.5)
    assert np.array_equal(engine.ankTimeStepBlocks(1), Tflow) and np.array_equal(engine.ankTimeStepBlocks(1, turb=True), Tturb)
    assert np.array_equal(engine.jacobianBlocks(1, 1), J0), "matrix"
    engine.download_state(1, 1)
    wa, wb = owned(blk, blk["w"]), owned(blk, state0)
    assert np.array_equal(wa[..., [0, 1, 2, 3, 5]], wb[..., [0, 1, 2, 3, 5]]), "state"
    assert (np.abs(wa[..., 4] - wb[..., 4]) <= 4 * EPS * np.abs(wb[..., 4])).all(), "energy: only whalo2's E -> p -> E rounding"
    engine.setW(w6.copy())
    engine.blocketteRes(1, updateIntermed=False, flowRes=True, turbRes=True, halo=True, closures=True)
    res1 = owned(blk, engine.download_residual(1, 1))
    print("residual after the turbulence entries: max difference", np.abs(res1 - res0).max(), "of", np.abs(res0).max())
    assert np.array_equal(res1, res0), "residual"
    assert np.array_equal(engine.ankMult(x1), yt)
    turb_halos()                                                         # (the product left nuTilde perturbed)
    engine.ankSelectBase(turb=False)                                     # the flow base as it was stored: w0, r0 and T untouched
    assert np.array_equal(engine.ankMult(x5), y5)
    engine.ankSetW(w5)
    held = engine.ankRelease()
    assert held >= 8 * (5 * ncell + ncell + 2 * 5 * ncell + 2 * ncell) and engine.ankRelease() == 0
    # Euler: no turbulence KSP
    checks.setup_block_with_bc(engine, (7, 6, 5), ank.EULER_JST, jm.EULER, seed + 1)
    assert lib.adflow_gpu_ank_set_w(x1.ctypes.data, 7 * 6 * 5, T) != 0
    assert "needs the RANS equations" in lib.adflow_gpu_last_error().decode()
    engine.release_all()
