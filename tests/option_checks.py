"""Every option of FlowParams away from its default (test infrastructure shared by tests/test_gpu_options.py, real MI355X, and
tests/test_hostsim_options.py, the kernel-logic emulator).

The other tiers compare every kernel with the reference's Fortran almost always at the default options and at one flight
condition; a kernel that carried a default where it should read the option would pass them all.  Here every option GROUP is moved
to values that are no default, equal to no other option's value and not "nice", and handed to the entries that read it THROUGH THE
EXISTING CHECKERS (checks.py, ank_checks.py, ank_turb_checks.py) at their existing bars: no tolerance is introduced here.

Guards, so that no case passes for nothing:
  * sensitivity(): the reference's own output of the checker, recorded while the checker runs, with the override and with the
    defaults ON THE SAME INPUT (frozen_inputs: blocks and boundary data are built from the override's record both times), must differ
    by MOVED = 1e4 TOL in the checker's global measure.  It needs the reference only, so it runs in the emulator tier.
  * NO_EFFECT names, with the line of the reference that shows it, the options that a path does not read; a test asserts that none
    of them moves anything after all.
  * farfield_classes(): recount of the four characteristic classes of bcFarfield from the normals, face velocities and free stream
    the reference is run on; the supersonic cases assert that every class is present before they compare."""
import contextlib

import numpy as np

import ank_checks
import ank_turb_checks
import checks
import fuzz_parity
import jacmult_checks
import pc_checks
import util
from adflow_amd import capi, synth
from adflow_amd.params import (FlowParams, EulerEquations, NSEquations, RANSEquations, dissScalar, dissMatrix, upwind, vanAlbeda, noLimiter,
                               RungeKutta, DADI, noResAveraging, alternateResAveraging, alwaysResAveraging, firstOrder, secondOrder,
                               vorticity)
from adflow_amd.topology import BrickTopology

MOVED = 1e4 * util.TOL
_KEEP = []          # the reference's flowDoms point into these arrays: alive as long as ref may be called

# ---- the reference's stage sets (setStageCoeffMultistage of the reference, inputParamRoutines.F90:3576-3635): {nRKStages: (etaRK, cdisRK)}.
# Five stages: the default.  Four stages blend the dissipation with 1/2 in the second stage and then freeze it over two stages; the
# others recompute it in every stage.
STAGE_SETS = fuzz_parity.STAGE_SETS


def stage_set(n):
    eta, cdis = STAGE_SETS[n]
    return dict(nRKStages=n, etaRK=list(eta), cdisRK=list(cdis))


# ---- boundary sets: faces 1..6 = iMin, iMax, jMin, jMax, kMin, kMax; -1 symmetry, -3 / -4 adiabatic / isothermal wall, -5 Euler wall,
# -6 far field, -7 / -9 supersonic in- / outflow, -8 / -10 subsonic in- / outflow, -15 extrapolation
WALL = {1: -6, 2: -6, 3: -1, 4: -1, 5: -3, 6: -6}
EULER_AD = dict(ank_checks.EULER_AD)
EULER_KINDS = [{1: -1, 2: -6, 3: -5, 4: -15, 5: -1, 6: -9}, {1: -7, 2: -6, 3: -8, 4: -8, 5: -10, 6: -5}]
VISC_KINDS = [{1: -6, 2: -6, 3: -1, 4: -4, 5: -3, 6: -6}, {1: -9, 2: -7, 3: -3, 4: -8, 5: -4, 6: -15}]
FARFIELD = {f: -6 for f in range(1, 7)}
BRICK_WALL = {1: -6, 2: -6, 3: -1, 4: -6, 5: -3, 6: -6}
TILE, SMALL, JAC = (70, 9, 6), (10, 8, 6), (8, 6, 5)
JAC_EXACT = (5, 4, 3)          # the exact matrix takes 35 colours, and the reference's forward mode is slow

# ---- the option groups.  Every value differs from its default and from every other value here, so that a swap is seen as well.
# SAct4 = 0.07, not the 0.7 the issue suggests: the synthetic states hold chi >= 3, where ft2 = ct3 exp(-ct4 chi^2) with ct4 = 0.7 is below
# 3e-3 and neither ct3 nor ct4 moves the reference's residual by 1e4 TOL.
# turbProd takes two of its three values: with katoLaunder the reference's SA model stops the program (sa.F90:136-139).
GAS = dict(gammaConstant=1.3, prandtl=0.9, prandtlTurb=0.6, SSuthDim=120.0, TSuthDim=291.15, muSuthDim=1.827e-5)
REFSTATE = dict(pInfDim=101325.0, rhoInfDim=1.225, TInfDim=288.15, RGasDim=296.8)
SA = dict(SAKappa=0.38, SAcb1=0.15, SAcb2=0.7, SAsigma=0.8, SAcv1=6.5, SAcw2=0.25, SAcw3=1.7, SAct3=1.1, SAct4=0.07, SAcrot=1.5,
          eddyVisInfRatio=0.21)
DISSIPATION = dict(vis2=0.4, vis4=0.03, adis=0.5, acousticScaleFactor=0.5, dirScaling=False, sigma=0.11)
MULTIGRID = dict(fcoll=0.6, cflCoarse=0.7, vis2Coarse=0.3, cflLimit=1.2)
GROUPS = {
    "gas": GAS,
    "gas-viscous": dict(GAS, muSuthDim=1.0),                       # viscous-dominated: the viscous part cannot hide
    "refstate": REFSTATE,
    "sa": dict(SA, useft2SA=True),
    "sa-rotation": dict(SA, useft2SA=False, useRotationSA=True),
    "sa-vorticity": dict(SA, turbProd=vorticity),
    "dissipation": DISSIPATION,
    "dissipation-scaled": dict(DISSIPATION, dirScaling=True),      # for the entries whose reference scales unconditionally
    "kappa-1": dict(kappaCoef=-1.0),
    "kappa0": dict(kappaCoef=0.0),
    "kappa.5": dict(kappaCoef=0.5),
    "mach.05": dict(Mach=0.05),
    "mach1.3": dict(Mach=1.3),
    "mach2": dict(Mach=2.0),
    "alpha-7": dict(Mach=2.0, alphaDeg=-7.0),
    "alpha35": dict(Mach=1.3, alphaDeg=35.0),
    "sideslip": dict(Mach=2.0, alphaDeg=-7.0, betaDeg=23.0),       # all three free-stream velocity components non-zero
    "rk1": stage_set(1), "rk2": stage_set(2), "rk3": stage_set(3), "rk4": stage_set(4), "rk6": stage_set(6),
    "cfl.9": dict(cfl=0.9),
    "cfl3": dict(cfl=3.0),
    "smoop-always": dict(smoop=0.7, resAveraging=alwaysResAveraging),
    "smoop-alternate": dict(smoop=0.7, resAveraging=alternateResAveraging),
    "multigrid": MULTIGRID,
    "turb-explicit": dict(turbRelax=1, alfaTurb=0.6),
    "turb-implicit": dict(turbRelax=2, alfaTurb=0.6),
    "turbresscale": dict(turbResScale=300.0),
    # the second flight condition of check_flight_condition_change (FLIGHT_B), for the single-block assemblies: inside the chain the
    # matrix has no reference
    "flight-b": dict(Mach=0.62, alphaDeg=4.3, **REFSTATE, cfl=1.1, cflCoarse=0.7, SAcb1=0.15, SAcv1=6.5),
}

# ---- options that a path does not read: (option, entry) -> the line of the reference that shows it.  Not a place for failures: an option
# that the reference reads and the library does not is a bug.
NO_EFFECT = {
    ("SAcrot", "res-rans-rotation"): "sa.F90:273: sst + rsaCrot * min(zero, sqrt(two * strainMag2)); the minimum is always zero",
    ("SAct1", "res-rans-upwind"): "paramTurb.F90:10 imports rsaCt1; no routine of the SA model reads it (the trip term is not implemented)",
    ("SAct2", "res-rans-upwind"): "paramTurb.F90:10 imports rsaCt2; no routine of the SA model reads it (the trip term is not implemented)",
    ("betaTurb", "sa-solve"): "vf.F90:624-629, 1035: only the v2-f model's DD-ADI solve relaxes with betaTurb; sa.F90 reads alfaTurb",
    ("turbResScale", "res-rans-upwind"): "blockette.F90:755-852 leaves dw unscaled; only the vector entries scale (NKSolvers.F90:1262-1376)",
}
_RLV_IN = ("blockette.F90:755-852 takes rlv and rev as inputs; RGas, muRef and TRef are read by computeLamViscosity (flowUtils.F90:1201-1300) "
           "and the isothermal wall (BCRoutines.F90 bcNSWallIsothermal) only")
_NO_BC = "a residual without boundary subfaces reads w, never the free stream: the record only changes the state the mesh generator builds"
NO_EFFECT.update({      # whole GROUPS on entries that the guard found do not read them (the first name is then a key of GROUPS)
    ("refstate", "res-ns-scalar"): _RLV_IN, ("refstate", "res-rans-upwind"): _RLV_IN,
    ("refstate", "rk-euler"): "the Euler path reads no viscosity and no gas constant (flowUtils.F90:1201: computeLamViscosity returns for Euler)",
    ("refstate", "bc-euler-0"): "BCRoutines.F90:57-221: symmetry, far field, Euler wall, extrapolation and supersonic outflow read no gas constant",
    ("refstate", "ank-T"): "solverUtils.F90 timeStep_block: the viscous radii read rlv and rev, which setup_block_with_bc hands over as inputs",
    ("sa", "bc-rans-0"): "BCRoutines.F90:57-221 applyAllBC_block writes the mean flow, rlv and rev only; the turbulence variable is turbBCRoutines'",
    ("sa", "bc-rans-wall"): "BCRoutines.F90:57-221 applyAllBC_block writes the mean flow, rlv and rev only; the turbulence variable is turbBCRoutines'",
    ("turb-explicit", "dadi-rans"): "smoothers.F90:383-693 DADISmoother updates the mean flow; turbSolveDDADI is called by the cycle (multiGrid.F90)",
    ("turbresscale", "ank-T"): "solverUtils.F90 timeStep_block does not scale; computeTimeStepMat (NKSolvers.F90) applies turbResScale to its own diagonal",
    ("mach.05", "res-euler-scalar"): _NO_BC, ("mach.05", "res-rans-upwind"): _NO_BC, ("alpha35", "res-euler-upwind"): _NO_BC,
})
NO_EFFECT_VALUES = {"SAcrot": 1.5, "SAct1": 1.3, "SAct2": 2.6, "betaTurb": 0.35, "turbResScale": 300.0}

# every option on its own: option -> (value, entries of which at least one must move).  The stage sets, turbProd and the switches of the
# SA model are varied in GROUPS only.
_SA_RES, _CLOSURES = ["res-rans-upwind"], ["res-bc"]
SINGLE_OPTIONS = {
    "gammaConstant": (1.3, ["bc-farfield"]), "prandtl": (0.9, ["res-ns-scalar"]), "prandtlTurb": (0.6, _SA_RES),
    "SSuthDim": (120.0, _CLOSURES), "TSuthDim": (291.15, _CLOSURES), "muSuthDim": (1.827e-5, _CLOSURES),
    "pInfDim": (101325.0, _CLOSURES), "rhoInfDim": (1.225, _CLOSURES), "TInfDim": (288.15, _CLOSURES), "RGasDim": (296.8, _CLOSURES),
    "SAKappa": (0.38, _SA_RES), "SAcb1": (0.15, _SA_RES), "SAcb2": (0.7, _SA_RES), "SAsigma": (0.8, _SA_RES), "SAcv1": (6.5, _SA_RES),
    "SAcw2": (0.25, _SA_RES), "SAcw3": (1.7, _SA_RES), "SAct3": (1.1, ["res-rans-ft2"]), "SAct4": (0.07, _SA_RES),
    "eddyVisInfRatio": (0.21, ["sa-solve-bc", "res-bc"]),
    "vis2": (0.4, ["res-euler-scalar"]), "vis4": (0.03, ["res-euler-scalar"]), "adis": (0.5, ["res-euler-scalar"]),
    "acousticScaleFactor": (0.5, ["res-euler-scalar"]), "dirScaling": (False, ["res-euler-scalar"]), "sigma": (0.11, ["res-approx-scalar"]),
    "kappaCoef": (0.5, ["res-euler-unlimited"]),
    "Mach": (1.3, ["bc-farfield"]), "alphaDeg": (35.0, ["bc-farfield"]), "betaDeg": (23.0, ["bc-farfield"]),
    "etaRK": ([0.21, 0.19, 0.35, 0.45, 1.0], ["rk-euler"]), "cdisRK": ([1.0, 0.5, 0.3, 0.2, 0.1], ["rk-euler"]),
    "cfl": (0.9, ["rk-euler"]), "smoop": (0.7, ["rk-averaged"]), "cflLimit": (1.2, ["rk-averaged"]),
    "fcoll": (0.6, ["mg2-rk"]), "cflCoarse": (0.7, ["mg2-rk"]), "vis2Coarse": (0.3, ["mg2-rk"]),
    "turbRelax": (1, ["sa-solve"]), "alfaTurb": (0.6, ["sa-solve"]), "turbResScale": (300.0, ["nk-rans"]),
}
# options that the other tiers vary (the issue's list), and fields of the record that are no option of a path
VARIED_ELSEWHERE = ("equations", "turbProd", "useQCR", "useRotationSA", "useft2SA", "spaceDiscr", "spaceDiscrCoarse", "limiter", "orderTurb",
                    "smoother", "nRKStages", "resAveraging", "nSubiterations", "nSubIterTurb", "eulerWallBCTreatment", "viscWallBCTreatment",
                    "outflowTreatment", "lowSpeedPreconditioner", "hScalingInlet", "exchangePressureEarly", "LRef", "ordersConverged")
NOT_AN_OPTION = ("turbModel", "unsupported", "currentLevel", "groundLevel", "rkStage", "rFil")

MARCH_KEYS = ("pc_fused", "roe_march", "inviscid_march", "viscous_tiled", "sa_march", "euler_march")
TUNING_DEFAULTS = {"pc_fused": 1, "jac_snap": 1, "split_eval": 1, **fuzz_parity.KERNEL_DEFAULTS}


@contextlib.contextmanager
def dispatch(engine, marches):
    """marches = True: the default dispatch; False: the marching kernels switched off by their tuning keys, so that the gather kernels
    behind them run.  The keys are restored on the way out."""
    try:
        if not marches:
            for k in MARCH_KEYS:
                engine.set_tuning(k, 0)
        yield
    finally:
        for k in MARCH_KEYS:
            engine.set_tuning(k, TUNING_DEFAULTS[k])


# ---- the guard's instruments -------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def recording(compare=True):
    """the REFERENCE's side of every comparison the checkers make inside: the second argument of checks.rel_err (assert_dw, assert_state,
    assert_rvec, ...) and the reference's difference quotient of the ANK operator checks.  Entries whose checker compares otherwise
    (the Jacobian assemblies) append their reference array themselves (extra).
    compare = False: the comparisons themselves are switched off (rel_err and rel_err_local record and return 0), so that what the
    library gives plays no part in what is recorded (mesh_checks.reference_floor)."""
    rec = []
    real_rel_err, real_local, real_product = checks.rel_err, checks.rel_err_local, ank_checks.assert_product

    def rel_err(a, b, *k):
        rec.append(np.array(b, dtype=np.float64, copy=True))
        return real_rel_err(a, b) if compare else 0.0

    def assert_product(what, y, v, h, op, Tn, blk, quotient):
        def q(h_, v_):
            out = quotient(h_, v_)
            rec.append(np.array(out, copy=True))
            return out
        return real_product(what, y, v, h, op, Tn, blk, q)

    checks.rel_err, ank_checks.assert_product = rel_err, assert_product
    if not compare:
        checks.rel_err_local = rel_err
    try:
        yield rec
    finally:
        checks.rel_err, checks.rel_err_local, ank_checks.assert_product = real_rel_err, real_local, real_product


@contextlib.contextmanager
def frozen_inputs(prm_in):
    """blocks and boundary data built from prm_in whatever record the checker passes on: the two runs of the guard see the same mesh,
    state and boundary data, and differ in the options alone (the array gamma, which the host fills from gammaConstant, among them)"""
    real_block, real_bocos = synth.make_block, synth.make_bocos

    def make_block(nx, ny, nz, prm, *a, **k):
        blk = real_block(nx, ny, nz, prm_in.replace(equations=prm.equations), *a, **k)
        if prm.gammaConstant != prm_in.gammaConstant:
            # the host's array gamma IS the option gammaConstant, in library and reference alike, and the pressure is what the closures
            # make of the conserved state with it (entries differ in where they re-form a pressure that disagrees with the energy)
            w = blk["w"]
            blk["gamma"][...] = prm.gammaConstant
            blk["p"] = np.asfortranarray((prm.gammaConstant - 1.0) * (w[..., 4] - 0.5 * w[..., 0] * (w[..., 1] ** 2 + w[..., 2] ** 2 + w[..., 3] ** 2)))
        return blk

    def make_bocos(blk, prm, *a, **k):
        return real_bocos(blk, prm_in.replace(equations=prm.equations), *a, **k)

    synth.make_block, synth.make_bocos, checks.make_block = make_block, make_bocos, make_block
    try:
        yield
    finally:
        synth.make_block, synth.make_bocos, checks.make_block = real_block, real_bocos, real_block


def movement(rec1, rec0):
    """the largest change of a recorded reference array in the checkers' global measure max|a - b| / max|b|"""
    assert min(len(rec1), len(rec0)) > 0
    worst = 0.0          # (the stage sets: check_rk_residual_sequence compares one pair of arrays per stage; the common stages count)
    for a, b in zip(rec1, rec0):
        assert a.shape == b.shape
        assert np.isfinite(a).all() and np.isfinite(b).all(), "the reference's own output is not finite: choose another input"
        worst = max(worst, float(util.rel_err(a, b)))
    return worst


# ---- the entries: name -> (base options, run(engine, prm, marches) -> reference arrays the recorder does not see) ------------------------
def _res(eq, sd):
    def run(engine, prm, marches):
        dims = TILE if marches else SMALL
        checks.check_block_res(engine, dims, prm, seed=3, **({"stretch_k": 2.0} if eq != EulerEquations else {}))
    return dict(equations=eq, spaceDiscr=sd, vis4=0.1 if sd == dissMatrix else 0.0156), run


def _res_approx(engine, prm, marches):
    checks.check_block_res_approx(engine, TILE if marches else SMALL, prm, stretch_k=2.0)


def _res_bc(engine, prm, marches):
    nx = 35 if marches else 5
    n = checks.check_blockette_res_with_bc(engine, BrickTopology(2, 1, 1, nx, 8, 6, periodic=(False, False, False)), prm, BRICK_WALL,
                                           stretch_k=2.0)
    assert n > 0


def _bc(eq, spec, **mk):
    def run(engine, prm, marches):
        for second in (True, False):
            checks.check_apply_bc(engine, SMALL, prm, spec, secondHalo=second, **mk)
    return dict(equations=eq), run


def _rk(engine, prm, marches):
    checks.check_rk_smoother(engine, BrickTopology(2, 1, 1, 12, 8, 6), prm, nsweeps=2,
                             **({"stretch_k": 2.0} if prm.equations != EulerEquations else {}))


def _rk_sequence(engine, prm, marches):
    checks.check_rk_residual_sequence(engine, TILE if marches else SMALL, prm)


def _dadi(engine, prm, marches):
    checks.check_dadi_smoother(engine, BrickTopology(2, 1, 1, 12, 8, 6), prm,
                               **({"stretch_k": 2.0} if prm.equations != EulerEquations else {}))


V2, V3, W3 = [0, 1, 0, -1], [0, 1, 0, 1, 0, -1, 0, -1], [0, 1, 0, 1, 0, -1, 0, 1, 0, -1, 0, -1, 0]


def _mg(cycling, nlevels, bc_spec=None):
    def run(engine, prm, marches):
        mk = {"stretch_k": 2.0} if prm.equations != EulerEquations else {}
        topo = BrickTopology(1, 1, 1, 16, 8, 8) if bc_spec or nlevels == 3 else BrickTopology(2, 1, 1, 12, 8, 8)
        checks.check_mg_cycle(engine, topo, prm, cycling, ncycles=2, nlevels=nlevels, bc_spec=bc_spec, **mk)
    return run


def _nk(bc_spec):
    def run(engine, prm, marches):
        mk = {"stretch_k": 2.0} if prm.equations != EulerEquations else {}
        checks.check_nk_residual(engine, BrickTopology(1 if bc_spec else 2, 1, 1, 12, 8, 6), prm, bc_spec=bc_spec, **mk)
    return run


def _jac(ad, spec, **flags):
    def run(engine, prm, marches):
        mk = {"stretch_k": 2.0} if prm.equations != EulerEquations else {}
        chk = checks.check_ad_jacobian if ad else checks.check_fd_jacobian
        Jg, Jr, st = chk(engine, JAC if flags.get("usePC", True) else JAC_EXACT, prm, spec, **flags, **mk)
        return [Jr]
    return run


def _sa_solve(engine, prm, marches):
    checks.check_sa_solve(engine, BrickTopology(2, 1, 1, 12, 8, 6), prm, stretch_k=2.0)


def _sa_solve_bc(engine, prm, marches):
    checks.check_sa_solve_with_bc(engine, (12, 8, 6), prm, {1: -6, 2: -15, 3: -1, 4: -4, 5: -3, 6: -9}, stretch_k=2.0)


def _ank_T(engine, prm, marches):
    coupled = prm.equations == RANSEquations
    blk, r, prm = checks.setup_block_with_bc(engine, (7, 6, 5), prm, WALL if coupled else EULER_AD, 307,
                                             **({"stretch_k": 2.0} if coupled else {}))
    _KEEP[:] = [r]
    # the yardstick of assert_T restates computeTimeStepBlock on the LIBRARY's dtl: the reference's own time step next to it
    from oracle import ref
    ref.call_level("timeStep", 1, 0)
    ank_checks.assert_T(engine, {1: blk}, prm, coupled, "option")
    dtl = engine.download_array(capi.ARR_DTL, np.zeros((blk.ie, blk.je, blk.ke), order="F"), 1, 1)
    inner = (slice(1, blk.nx + 1),) + (slice(1, blk.ny + 1),) + (slice(1, blk.nz + 1),)
    assert checks.rel_err(dtl[inner], r["dtl"][inner]) <= util.TOL
    engine.ankRelease()


def _ank_operator(engine, prm, marches):
    rans = prm.equations == RANSEquations
    # (the combinations the ANK tier checks: the coupled operator against the exact matrix, the Euler one against the preconditioner's)
    ank_checks.check_operator(engine, JAC_EXACT if rans else (7, 6, 5), prm, WALL if rans else EULER_AD, rans, not rans,
                              **({"stretch_k": 2.0} if rans else {}))


def _ank_turb(engine, prm, marches):
    ank_turb_checks.check_operator(engine, (7, 6, 5), False, prm=prm)


RANS_DADI = dict(equations=RANSEquations, smoother=DADI, resAveraging=noResAveraging, cfl=1.5, nSubiterations=2, nSubIterTurb=2)
RANS_UP = dict(equations=RANSEquations, spaceDiscr=upwind, limiter=vanAlbeda)
ENTRIES = {
    **{f"res-{en}-{sn}": _res(eq, sd) for en, eq in (("euler", EulerEquations), ("ns", NSEquations), ("rans", RANSEquations))
       for sn, sd in (("upwind", upwind), ("scalar", dissScalar), ("matrix", dissMatrix))},
    "res-rans-order2": (dict(RANS_UP, orderTurb=secondOrder), _res(RANSEquations, upwind)[1]),
    "res-rans-rotation": (dict(RANS_UP, useRotationSA=True), _res(RANSEquations, upwind)[1]),
    "res-rans-ft2": (dict(RANS_UP, SAct4=0.07), _res(RANSEquations, upwind)[1]),
    # kappaCoef is read by the unlimited reconstruction only (fluxes.F90: limiter = noLimiter)
    "res-euler-unlimited": (dict(spaceDiscr=upwind, limiter=noLimiter), _res(EulerEquations, upwind)[1]),
    "res-rans-unlimited": (dict(RANS_UP, limiter=noLimiter), _res(RANSEquations, upwind)[1]),
    "res-bc-unlimited": (dict(RANS_UP, limiter=noLimiter), _res_bc),
    "fd-exact-unlimited": (dict(RANS_UP, limiter=noLimiter), _jac(False, WALL, usePC=False)),
    "ad-exact-unlimited": (dict(RANS_UP, limiter=noLimiter), _jac(True, WALL, usePC=False)),
    "res-approx-scalar": (dict(equations=RANSEquations, spaceDiscr=dissScalar), _res_approx),
    "res-approx-matrix": (dict(equations=NSEquations, spaceDiscr=dissMatrix), _res_approx),
    "res-bc": (dict(RANS_UP), _res_bc),
    "res-bc-scalar": (dict(equations=RANSEquations, spaceDiscr=dissScalar), _res_bc),
    "bc-euler-0": _bc(EulerEquations, EULER_KINDS[0]), "bc-euler-1": _bc(EulerEquations, EULER_KINDS[1]),
    "bc-rans-0": _bc(RANSEquations, VISC_KINDS[0], stretch_k=2.0), "bc-rans-1": _bc(RANSEquations, VISC_KINDS[1], stretch_k=2.0),
    "bc-rans-wall": _bc(RANSEquations, WALL, stretch_k=2.0),
    "bc-farfield": _bc(EulerEquations, FARFIELD),
    "rk-euler": (dict(smoother=RungeKutta), _rk), "rk-rans": (dict(equations=RANSEquations, smoother=RungeKutta, resAveraging=noResAveraging), _rk),
    "rk-averaged": (dict(smoother=RungeKutta, resAveraging=alwaysResAveraging), _rk),
    "rk-sequence": (dict(smoother=RungeKutta), _rk_sequence),
    "dadi-euler": (dict(smoother=DADI, resAveraging=noResAveraging, cfl=1.5), _dadi), "dadi-rans": (dict(RANS_DADI), _dadi),
    "mg2-rk": (dict(), _mg(V2, 2)), "mg3-rk-v": (dict(), _mg(V3, 3)), "mg3-rk-w": (dict(), _mg(W3, 3)),
    "mg2-dadi": (dict(smoother=DADI, resAveraging=noResAveraging, cfl=1.5), _mg(V2, 2)),
    "mg3-dadi-w": (dict(smoother=DADI, resAveraging=noResAveraging, cfl=1.5), _mg(W3, 3)),
    "mg2-ns": (dict(equations=NSEquations, resAveraging=noResAveraging), _mg(V2, 2)),
    "mg2-rans": (dict(RANS_DADI), _mg(V2, 2)),
    "mg2-farfield": (dict(), _mg(V2, 2, bc_spec=FARFIELD)),
    "nk-rans": (dict(RANS_UP), _nk(None)),
    "nk-rans-bc": (dict(RANS_UP), _nk(WALL)), "nk-farfield": (dict(), _nk(FARFIELD)),
    "fd-pc": (dict(RANS_UP), _jac(False, WALL, usePC=True)), "fd-exact": (dict(RANS_UP), _jac(False, WALL, usePC=False)),
    "ad-pc": (dict(RANS_UP), _jac(True, WALL, usePC=True)), "ad-exact": (dict(RANS_UP), _jac(True, WALL, usePC=False)),
    "fd-pc-scalar": (dict(equations=RANSEquations, spaceDiscr=dissScalar), _jac(False, WALL, usePC=True)),
    "ad-exact-scalar": (dict(equations=RANSEquations, spaceDiscr=dissScalar), _jac(True, WALL, usePC=False)),
    "fd-turb": (dict(RANS_UP), _jac(False, WALL, usePC=True, useTurbOnly=True)),
    "ad-turb": (dict(RANS_UP), _jac(True, WALL, usePC=True, useTurbOnly=True)),
    "fd-pc-farfield": (dict(spaceDiscr=upwind, limiter=vanAlbeda), _jac(False, FARFIELD, usePC=True)),
    "fd-exact-farfield": (dict(spaceDiscr=upwind, limiter=vanAlbeda), _jac(False, FARFIELD, usePC=False)),
    "ad-pc-farfield": (dict(spaceDiscr=upwind, limiter=vanAlbeda), _jac(True, FARFIELD, usePC=True)),
    "ad-exact-farfield": (dict(spaceDiscr=upwind, limiter=vanAlbeda), _jac(True, FARFIELD, usePC=False)),
    "sa-solve": (dict(equations=RANSEquations, nSubIterTurb=2), _sa_solve),
    "sa-solve-bc": (dict(equations=RANSEquations, nSubIterTurb=2, orderTurb=secondOrder), _sa_solve_bc),
    "ank-T": (dict(RANS_UP, turbResScale=1.0e3), _ank_T),
    "ank-operator": (dict(RANS_UP, turbResScale=1.0e3), _ank_operator),
    "ank-turb": (dict(RANS_UP), _ank_turb),
}
# entries without a residual march behind them run once; the others under both dispatches
BOTH_DISPATCHES = tuple(n for n in ENTRIES if n.startswith(("res-", "nk-", "fd-", "ad-")))

RES_ALL = [n for n in ENTRIES if n.startswith("res-") and n.count("-") == 2 and n.split("-")[1] in ("euler", "ns", "rans")
           and n.split("-")[2] in ("upwind", "scalar", "matrix")]
JAC4 = ["fd-pc", "fd-exact", "ad-pc", "ad-exact"]
GAS_ENTRIES = RES_ALL + ["res-bc", "bc-euler-0", "bc-euler-1", "bc-rans-0", "bc-rans-1", "rk-euler", "rk-rans", "dadi-euler", "dadi-rans",
                         "mg2-ns", "nk-rans-bc"] + JAC4 + ["ank-T", "ank-operator"]
# (group, entries): the table of the issue
PLAN = [
    ("gas", GAS_ENTRIES), ("gas-viscous", ["res-ns-scalar", "res-rans-upwind", "res-bc", "fd-pc", "ad-exact"]),
    # (the reference state enters through the closures and the isothermal wall: entries that take rlv as an input do not read it)
    ("refstate", ["res-bc", "bc-euler-1", "bc-rans-0", "bc-rans-1", "rk-rans", "dadi-rans", "mg2-ns", "nk-rans-bc"] + JAC4 + ["ank-operator"]),
    # (applyAllBC_block leaves the turbulence variable alone: its boundary conditions and eddyVisInfRatio run in sa-solve-bc and res-bc)
    ("sa", ["res-rans-upwind", "res-rans-order2", "sa-solve", "sa-solve-bc", "res-bc", "fd-pc", "ad-exact", "fd-turb", "ad-turb",
            "ank-turb"]),
    ("sa-rotation", ["res-rans-upwind", "res-bc", "ad-pc"]),
    ("sa-vorticity", ["res-rans-upwind", "res-bc", "ad-exact"]),
    ("dissipation", ["res-euler-scalar", "res-rans-scalar", "res-ns-matrix", "res-approx-scalar", "res-approx-matrix", "rk-euler", "fd-pc-scalar",
                     "ad-exact-scalar"]),
    ("dissipation-scaled", ["res-bc-scalar"]),
    ("kappa-1", ["res-euler-unlimited", "res-rans-unlimited", "res-bc-unlimited", "fd-exact-unlimited", "ad-exact-unlimited"]),
    ("kappa0", ["res-euler-unlimited", "res-rans-unlimited"]), ("kappa.5", ["res-rans-unlimited", "ad-exact-unlimited"]),
    ("rk1", ["rk-euler", "rk-rans"]), ("rk2", ["rk-euler", "rk-rans", "rk-sequence"]),
    ("rk3", ["rk-euler", "rk-rans", "rk-sequence"]), ("rk4", ["rk-euler", "rk-rans", "rk-sequence", "mg2-rk"]),
    ("rk6", ["rk-euler", "rk-rans", "rk-sequence"]),
    ("cfl.9", ["rk-euler", "dadi-rans"]), ("cfl3", ["rk-euler", "rk-rans"]),
    ("smoop-always", ["rk-euler"]), ("smoop-alternate", ["rk-euler", "mg2-rk"]),
    ("multigrid", ["mg2-rk", "mg3-rk-v", "mg3-rk-w", "mg2-dadi", "mg3-dadi-w"]),
    # (DADISmoother does not call the turbulence solve: the multigrid cycle that closes with it does)
    ("turb-explicit", ["sa-solve", "sa-solve-bc", "mg2-rans"]), ("turb-implicit", ["sa-solve", "sa-solve-bc", "mg2-rans"]),
    ("turbresscale", ["nk-rans", "nk-rans-bc", "ank-operator", "ank-turb"]),
    ("flight-b", ["fd-pc", "ad-pc", "res-bc"]),
    # section 3 of the issue: the free stream
    ("mach.05", ["res-euler-scalar", "res-rans-upwind", "bc-farfield", "bc-rans-0"]),
    ("mach1.3", ["bc-farfield", "bc-euler-0", "mg2-farfield"]),
    ("mach2", ["bc-farfield", "bc-rans-0", "nk-farfield", "fd-pc-farfield", "fd-exact-farfield", "ad-pc-farfield", "ad-exact-farfield"]),
    ("alpha-7", ["bc-farfield"]), ("alpha35", ["bc-farfield", "res-euler-upwind"]), ("sideslip", ["bc-farfield", "nk-farfield"]),
]
CASES = [(g, e) for g, es in PLAN for e in es]
# the three free-stream pairs on a residual without boundary conditions run for the STATE at that Mach number and angle; no option is read
# there, so they stand in NO_EFFECT and not under the guard
GUARDED = [c for c in CASES if c not in NO_EFFECT]


def no_effect_options(name):
    return dict(GROUPS[name]) if name in GROUPS else {name: NO_EFFECT_VALUES[name]}


def params_of(group, entry):
    """the record of a case: the entry's base options with the group's overrides on top"""
    return FlowParams(**{**ENTRIES[entry][0], **GROUPS[group]})


def run_case(engine, group, entry, dispatches=(True, False)):
    """the parity of one (group, entry) pair through the entry's checker, under both dispatches where a march stands in front"""
    prm = params_of(group, entry)
    for marches in (dispatches if entry in BOTH_DISPATCHES else dispatches[:1]):
        with dispatch(engine, marches):
            ENTRIES[entry][1](engine, prm, marches)


def reference_record(engine, entry, prm, prm_in):
    with frozen_inputs(prm_in), recording() as rec, dispatch(engine, False):
        extra = ENTRIES[entry][1](engine, prm, False)
    return rec + [np.array(a, copy=True) for a in (extra or [])]


def sensitivity(engine, entry, over):
    """how far the reference's output of the entry's checker moves between the options `over` and the defaults, on the SAME input
    (built from the record with `over`)"""
    base = ENTRIES[entry][0]
    prm = FlowParams(**{**base, **over})
    rec1 = reference_record(engine, entry, prm, prm)
    rec0 = reference_record(engine, entry, FlowParams(**base), prm)
    return movement(rec1, rec0)


# ---- far field: the four characteristic classes ------------------------------------------------------------------------------------------
def farfield_classes(faces, prm):
    """recount of bcFarfield's branches (BCRoutines.F90: vn0 = wInf . n - rface against -c0, 0, c0) over every far-field subface:
    {supersonic inflow, subsonic inflow, subsonic outflow, supersonic outflow}"""
    w = prm.wInf()
    c0 = np.sqrt(prm.gammaInf * prm.pInfCorr / w[0])
    n = dict(sup_in=0, sub_in=0, sub_out=0, sup_out=0)
    for f in faces:
        if f["bcType"] != -6:
            continue
        nrm = f["norm"]
        vn0 = w[1] * nrm[..., 0] + w[2] * nrm[..., 1] + w[3] * nrm[..., 2] - (f["rface"] if f.get("rface") is not None else 0.0)
        n["sup_in"] += int((vn0 <= -c0).sum())
        n["sub_in"] += int(((vn0 > -c0) & (vn0 <= 0.0)).sum())
        n["sub_out"] += int(((vn0 > 0.0) & (vn0 <= c0)).sum())
        n["sup_out"] += int((vn0 > c0).sum())
    return n


def farfield_faces(dims, prm, spec, seed, **mk):
    """the subfaces that check_apply_bc (seed) / setup_block_with_bc (seed) build for this case"""
    p = prm.replace(currentLevel=1, groundLevel=1)
    blk = synth.make_block(*dims, p, seed=seed, **mk)
    return synth.make_bocos(blk, p, spec, seed=seed + 1)[0]


def check_supersonic_farfield_bc(engine, group, dims=SMALL, seed=51, all_classes=True):
    """applyAllBC_block with six far-field faces (every face with a face velocity rface) and both halo rings"""
    prm = FlowParams(**GROUPS[group])
    n = farfield_classes(farfield_faces(dims, prm, FARFIELD, seed), prm)
    if all_classes:
        assert min(n.values()) > 0, n
    for second in (True, False):
        checks.check_apply_bc(engine, dims, prm, FARFIELD, secondHalo=second, seed=seed)
    return n


def check_supersonic_farfield_res(engine, marches=True):
    """the whole wall-bounded blocketteRes on a 2 x 2 x 1 brick whose outside is far field, at Mach 2"""
    prm = FlowParams(**GROUPS["mach2"], spaceDiscr=upwind)
    topo = BrickTopology(2, 2, 1, 6, 5, 4, periodic=(False, False, False))
    with dispatch(engine, marches):
        checks.check_blockette_res_with_bc(engine, topo, prm, FARFIELD)
    prm = FlowParams(**GROUPS["mach2"], **RANS_UP)
    with dispatch(engine, marches):
        return checks.check_blockette_res_with_bc(engine, topo, prm, {**FARFIELD, 5: -3}, stretch_k=2.0)


def check_supersonic_farfield_jacobian(engine, ad, usePC, seed=101):
    prm = FlowParams(**GROUPS["mach2"], spaceDiscr=upwind, limiter=vanAlbeda)
    n = farfield_classes(farfield_faces(JAC, prm, FARFIELD, seed), prm)
    assert min(n.values()) > 0, n
    chk = checks.check_ad_jacobian if ad else checks.check_fd_jacobian
    chk(engine, JAC, prm, FARFIELD, usePC=usePC, seed=seed)
    return n


# ---- a change of flight condition on registered blocks ---------------------------------------------------------------------------------
# (Runge-Kutta is the multigrid smoother of the case, so that the RK sweep of the chain needs no change of options: between two runs
# the record differs in the flight-condition fields alone, and those alone must retire the captured cycle)
FLIGHT_A = dict(RANS_UP, smoother=RungeKutta, resAveraging=noResAveraging, nSubIterTurb=2)
FLIGHT_B = dict(FLIGHT_A, **GROUPS["flight-b"])
GMRES_CAP, GMRES_RTOL = 60, 1e-8          # the cap: fixed beforehand, at least twice scipy's count with the numpy ILU(0) (asserted)


class FlightChain:
    """BrickTopology(2, 1, 1, 8, 6, 4), wall-bounded RANS, two multigrid levels, registered ONCE; run(prm) sets the options (the only
    set_options of a run), uploads the start state again and runs the chain blocketteRes, one RK sweep, three multigrid cycles (captured
    and then replayed on the device), preconditioner-matrix assembly + pcSetup + gmresSolve, one ANK flow step.  compare: against the
    reference's routines for the residual, the sweep, every cycle and the ANK right-hand side (TOL); the factor against the numpy
    ILU(0) of the downloaded matrix and the GMRES solution against scipy's count and the true residual (pc_checks' bars, MARGIN); the
    pseudo-time term against ank_checks' formula.  The eight iterations of the ANK solve have no yardstick of their own beyond that
    right-hand side (ank_checks.check_solve holds the converged solve to one).  The matrix ITSELF has no reference here: the
    reference's assembly (ref.ad_jacobian) takes one block; its parity under these options is what the fd-pc / ad-pc cases of PLAN
    check (the group flight-b is this chain's second condition), and here it must be bit for bit the matrix of a fresh registration.  Every comparison comes after the outputs of its stage
    are taken and leaves the device state alone or is followed by a stage that sets it again."""

    def __init__(self, engine, prm_start):
        self.engine = engine
        self.topo = BrickTopology(2, 1, 1, 8, 6, 4, periodic=(False, False, False))
        # the start state is built from ONE record (prm_start) for every run: only the options differ between the runs
        self.levels, self.rlevels = checks.setup_multilevel_brick(engine, self.topo, prm_start, 2, seed=23, brick_spec=BRICK_WALL, stretch_k=2.0)
        self.start = [{nn: {n: b[n].copy(order="F") for n in ("w", "p", "rlv", "rev", "gamma")} for nn, b in lev.items()} for lev in self.levels]

    def restart(self, prm):
        from oracle import ref
        self.engine.set_options(prm)
        ref.set_params(prm.replace(currentLevel=1, groundLevel=1))
        for lv, (lev, rlev) in enumerate(zip(self.levels, self.rlevels), start=1):
            for nn in sorted(lev):
                for n, a in self.start[lv - 1][nn].items():
                    lev[nn][n][...] = a
                    rlev[nn][n][...] = a
                self.engine.upload_state(nn, lv)

    def run(self, prm, compare):
        from oracle import ref
        e, fine, rfine = self.engine, self.levels[0], self.rlevels[0]
        out = {}
        self.restart(prm)
        # 1. blocketteRes with closures, boundary conditions and the exchange
        e.blocketteRes(level=1, updateIntermed=True, flowRes=True, turbRes=True, halo=True, closures=True)
        out["res"] = [e.download_residual(nn, 1).copy() for nn in sorted(fine)]
        if compare:
            for nn in sorted(rfine):
                ref.call_level("setPointers", 1, nn)
                ref.call("computePressureSimple", 0)
                ref.call("computeLamViscosity", 0)
                ref.call("computeEddyViscosity", 0)
                ref.call("bcTurbTreatment")
                ref.call("applyAllTurbBCThisBlock", 1)
                ref.call("applyAllBC_block", 1)
            ref.call_level("whalo2", 1, 1, prm.nw)
            for i, nn in enumerate(sorted(rfine)):
                ref.call_level("setPointers", 1, nn)
                ref.blockette_res_core(True, True, True)
                checks.assert_dw(fine[nn], out["res"][i], rfine[nn]["dw"], 6, what=f"flight chain: blocketteRes block {nn}")
        # 2. one Runge-Kutta sweep
        e.timeStep(1, False)
        e.residual(1, 0)
        e.RungeKuttaSmoother(1)
        if compare:
            ref.load().ref_set_int(b"rkStage", 0)
            ref.call_level("timeStep", 1, 0)
            ref.call_level("initres", 1, 1, 5)
            ref.call_level("residual", 1)
            ref.call_level("RungeKuttaSmoother", 1)
            checks.assert_state(e, fine, rfine, prm, "flight chain: RK sweep", rlv_first_halo_only=True, rlv_no_edges=True)
        out["rk"] = self.state()
        # 3. three multigrid cycles
        if compare:
            ref.set_cycling(V2)
            ref.load().ref_set_int(b"rkStage", 0)
            ref.call_level("timeStep", 1, 0)
            ref.call_level("initres", 1, 1, 5)
            ref.call_level("residual", 1)
        e.timeStep(1, False)
        e.residual(1, 0)
        for n in range(3):
            e.executeMGCycle(V2)
            if compare:
                ref.call_level("executeMGCycle", 1)
                checks.assert_state(e, fine, rfine, prm, f"flight chain: cycle {n}", rlv_first_halo_only=True, rlv_no_edges=True)
                for nn in sorted(fine):
                    checks.assert_dw(fine[nn], e.download_residual(nn, 1), rfine[nn]["dw"], 5, what=f"flight chain: dw after cycle {n}")
        out["mg"] = self.state() + [e.download_residual(nn, 1).copy() for nn in sorted(fine)]
        # 4. the preconditioner matrix, its factor and a solve
        e.setupStateResidualMatrix(1, usePC=True, frozenTurb=True, useAD=True)
        out["jac"] = [e.jacobianBlocks(nn, 1).copy() for nn in sorted(fine)]
        e.pcSetup(1)
        rng = np.random.default_rng(5)
        b = rng.uniform(-1.0, 1.0, 5 * sum(bl.ncells for bl in fine.values()))
        x, its, r0, rn = e.gmresSolve(b, 1, restart=GMRES_CAP, maxIts=GMRES_CAP, rtol=GMRES_RTOL)
        out["gmres"] = [np.asarray(x).copy(), np.array([float(its), r0, rn])]
        if compare:
            op = jacmult_checks.operator_of(e, fine, self.topo.patterns(2)[0])
            jacmult_checks.assert_products_to_rounding(e, op, 7, "flight chain: matrix product")
            _, (f64, _) = pc_checks.assert_apply_matches(e, op, 9, "flight chain: ILU(0) factor")
            k_ref = pc_checks.scipy_gmres_iterations(lambda v: op.apply(v), f64, b, False, GMRES_RTOL, GMRES_CAP, GMRES_CAP)
            true, nb = float(np.linalg.norm(b - op.apply(x))), float(np.linalg.norm(b))
            print(f"flight chain: gmres {its} iterations (scipy {k_ref}), ||b - A x|| / ||b|| = {true / nb:.3e}")
            assert 2 * k_ref <= GMRES_CAP and 0 < its <= GMRES_CAP, (its, k_ref)
            assert abs(r0 - nb) <= 1e-12 * nb and true <= 2 * GMRES_RTOL * nb, (r0, nb, true)
        # 5. one ANK flow step: time step, shifted factor, matrix-free solve
        e.timeStep(1)
        e.ankTimeStep(ank_checks.CFL)
        e.ankPcSetup(1)
        if compare:       # (downloads only: the solve below leaves the perturbed state on the device)
            Tn = ank_checks.numpy_T(e, fine, prm, False)
            for nn in fine:
                ank_checks.assert_T_block(e.ankTimeStepBlocks(nn, False), Tn[nn], f"flight chain block {nn}")
            w6 = ank_checks.state_vector(e, fine, 6)
        w0 = ank_checks.state_vector(e, fine, 5)
        e.ankSetBase(w0)
        rhs = e.ankGetR()
        x, its, r0, rn = e.ankSolve(rhs, 1, restart=8, maxIts=8, rtol=1e-3)
        out["ank"] = [rhs.copy(), np.asarray(x).copy(), np.array([float(its), r0, rn])]
        if compare:
            # the right-hand side is FormFunction_mf of the state the cycles left: the reference's routines on the same vector
            rRef = checks.nk_reference(rfine, prm, w6, bc_spec=BRICK_WALL)
            checks.assert_rvec(rhs, np.ascontiguousarray(rRef.reshape(-1, 6)[:, :5]).reshape(-1), 5, what="flight chain: ANK right-hand side")
            nrm = float(np.linalg.norm(rhs))
            assert abs(r0 - nrm) <= 1e-12 * nrm and 0 < its <= 8 and rn < r0, (its, r0, rn, nrm)
        e.pcRelease()
        e.ankRelease()
        return out

    def state(self):
        out = []
        for nn in sorted(self.levels[0]):
            self.engine.download_state(nn, 1)
            b = self.levels[0][nn]
            out += [b[n].copy() for n in ("w", "p", "rlv", "rev")]
        return out


def assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert len(a[k]) == len(b[k])
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert np.array_equal(x, y, equal_nan=True), (what, k, i, float(np.nanmax(np.abs(x - y))))


def check_flight_condition_change(engine):
    """options A (the defaults of the case) -> B -> A on blocks that stay registered: (a) every output under B is the reference's under
    B, (b) bit for bit what a fresh registration under B gives, (c) back under A the chain reproduces its first run bit for bit"""
    A, B = FlowParams(**FLIGHT_A), FlowParams(**FLIGHT_B)
    try:
        chain = FlightChain(engine, A)
        a1 = chain.run(A, compare=True)
        b1 = chain.run(B, compare=True)                  # (a)
        a2 = chain.run(A, compare=False)
        assert_same_bits(a2, a1, "back under A")      # (c)
        moved = max(float(util.rel_err(x, y)) for x, y in zip(b1["res"] + b1["mg"], a1["res"] + a1["mg"]))
        assert moved >= MOVED, ("the change of flight condition does not change the chain", moved)
        engine.release_all()
        fresh = FlightChain(engine, B)                   # registered under B: no call of this registration ever saw A ...
        fresh.start = chain.start                        # ... and the start state of the first chain (its boundary data hold no option)
        b2 = fresh.run(B, compare=False)
        assert_same_bits(b1, b2, "B after A against B on a fresh registration")      # (b)
    finally:
        engine.pcRelease()
        engine.ankRelease()
