"""TEST INFRASTRUCTURE.  The entries of the library on the mesh families of tests/mesh_families.py, through the checkers that
exist (checks.py, ank_checks.py, pc_checks.py and the checkers of everything built on the assembled matrix: pc_fill_checks.py,
pc_coupled_checks.py, pc_mg_checks.py, multi_checks.py, jacmult_checks.py, jacfree_checks.py): no comparison of its own.  Every checker call goes through `on`: first the
family's recount on a block -- or on every block of the brick, through frame -- built with the very keywords and topology the checker
gets, then the checker under a spy that asserts that each block it builds itself carries the case's shape and lengths, so that
neither a later edit nor a keyword filter inside a checker can quietly turn the mesh back into a cube.

    CASES      the meshes: the four families and the three `units` cases
    ENTRIES    name -> run(engine, case, big); big: the residual tier at the project's partial-tile shapes (GPU), else the
               emulator tier's small ones
    POLE_OUT   the entries left out on `pole`, where the reference itself would divide by zero: none

tests/test_gpu_meshes.py runs CASES x ENTRIES on the MI355X, tests/test_hostsim_meshes.py on the emulator, together with the
conditioning floor of every pair (reference_floor)."""
import contextlib

import numpy as np

import ank_checks
import checks
import jacfree_checks
import jacmult_checks
import mesh_families as mf
import multi_checks
import pc_checks
import pc_coupled_checks
import pc_fill_checks
import pc_mg_checks
from adflow_amd import synth
from adflow_amd.params import (FlowParams, NSEquations, RANSEquations, dissScalar, dissMatrix, upwind, vanAlbeda, minmod, DADI,
                               noResAveraging, alternateResAveraging)
from adflow_amd.topology import LatticeBlock, LatticeTopology
from option_checks import dispatch, recording

BIG_DIMS = [(70, 9, 12), (63, 6, 35)]        # a partial 64-column tile with a partial 4-row tile; 63 wide with 35 planes
SMALL_DIMS = [(12, 8, 6)]
SMALL = (12, 8, 6)
JAC, JAC_EXACT = (7, 6, 5), (6, 5, 4)
WARP = 0.2                                   # the geometry checkers' warp, relative to the local edge length (checks.local_warp)


class Case:
    """a mesh of the tier: family (or None: the default map), severity keywords, lengths"""

    def __init__(self, name, family, lengths=None, **severity):
        self.name, self.family, self.lengths, self.severity = name, family, lengths, severity

    def mk(self, visc=False, **severity):
        """make_block's keywords; severity: overrides for one entry (the conditioning floor)"""
        out = {}
        if self.family is not None:
            out["shape"] = mf.family(self.family, **{**self.severity, **severity})
        if self.lengths is not None:
            out["lengths"] = self.lengths
        if visc and self.family not in ("annulus", "clustered"):      # (those two bring their own wall clustering)
            out["stretch_k"] = 2.0
        return out

    def gate(self, dims, prm, mk):
        """the recount, on a block made as the checker will make it; returns it"""
        blk = synth.make_block(*dims, prm, **mk)
        n = mf.recount(blk)
        if self.family is not None:
            mf.assert_family(blk, self.family)
        if self.lengths is not None:
            # the unit of length: the mesh is the unscaled one times `lengths`, exactly (powers of two), and far from O(1)
            unit = synth.make_block(*dims, prm, **{k: v for k, v in mk.items() if k != "lengths"})
            assert np.array_equal(blk["x"], unit["x"] * np.asarray(self.lengths))
            assert np.abs(np.log2(np.asarray(self.lengths))).max() >= 4.0
            if len(set(self.lengths)) > 1:      # unequal lengths: the cells are stretched, far beyond what the unscaled mesh has
                assert n["aspect"] > 4.0 * mf.recount(unit)["aspect"], n
        return n

    def gate_brick(self, topo, prm, mk):
        """the recount over the blocks of a brick built through frame, as its checker builds them (topo.make_block); returns it"""
        blocks = [topo.make_block(g, prm, seed=g + 1, **mk) for g in range(topo.nblocks)]
        n, whole = mf.recount_brick(blocks)
        if self.family is not None:
            assert all(b.shape is mk["shape"] and np.all(b["vol"][2:-2, 2:-2, 2:-2] > 0.0) for b in blocks)
            assert mf.THRESHOLDS[self.family](n, whole), (self.family, n)
        if self.lengths is not None:
            unit = [topo.make_block(g, prm, seed=g + 1, **{k: v for k, v in mk.items() if k != "lengths"}) for g in range(topo.nblocks)]
            assert all(np.array_equal(b["x"], u["x"] * np.asarray(self.lengths)) for b, u in zip(blocks, unit))
            assert np.abs(np.log2(np.asarray(self.lengths))).max() >= 4.0
            if len(set(self.lengths)) > 1:
                assert n["aspect"] > 4.0 * mf.recount_brick(unit)[0]["aspect"], n
        return n

    def for_entry(self, entry):
        """the case at the severity of one entry (LOWERED)"""
        low = LOWERED.get((self.name, entry))
        if not low:
            return self
        sev = {k: v for k, v in {**self.severity, **low}.items() if k != "lengths"}
        return Case(self.name, self.family, low.get("lengths", self.lengths), **sev)

    def brick(self, dims, visc=False):
        """two blocks joined in i inside ONE map (frame): the outside faces are physical boundaries or carry nothing"""
        nx, ny, nz = dims
        eye = np.eye(3, dtype=int)
        return LatticeTopology([LatticeBlock((nx, ny, nz), eye, (0, 0, 0)), LatticeBlock((nx, ny, nz), eye, (nx, 0, 0))],
                               stretch_z=2.0 if (visc and self.family not in ("annulus", "clustered")) else 1.0)

    def brick_mk(self):
        return {k: v for k, v in self.mk().items() if k != "stretch_k"}

    def __repr__(self):
        return self.name


CASES = [Case("annulus", "annulus"), Case("sheared", "sheared"), Case("clustered", "clustered"), Case("pole", "pole"),
         Case("units-annulus-2^-20", "annulus", mf.UNIT_LENGTHS[0]), Case("units-clustered-2^10", "clustered", mf.UNIT_LENGTHS[1]),
         Case("units-default-2^7-1-2^-7", None, mf.UNIT_LENGTHS[2])]
CASE = {c.name: c for c in CASES}
# (mesh, entry) pairs whose severity is lowered because the REFERENCE's conditioning floor exceeds a tenth of the bar at the full one
# (reference_floor; DESIGN §5 has the figures).  On the (2^7, 1, 2^-7) mesh the x coordinates are 1e5 times the k spacing: one ulp of
# a node turns the j- and k-face normals by 1e-11, and the velocity mirrored at a symmetry plane or a wall moves by 8e-11 .. 9e-11 of
# the field maximum in the reference itself.
LOWERED = {("units-default-2^7-1-2^-7", "bc"): dict(lengths=(2.0 ** 4, 1.0, 2.0 ** -4)),
           ("units-default-2^7-1-2^-7", "smoothers"): dict(lengths=(2.0 ** 4, 1.0, 2.0 ** -4))}

EULER = {1: -1, 2: -6, 3: -5, 4: -15, 5: -1, 6: -9}                 # symmetry, far field, Euler wall, extrapolation, supersonic outflow
SUBSONIC = {1: -8, 2: -10, 3: -5, 4: -8, 5: -12, 6: -6}            # subsonic inflow / outflow / bleed
WALL = {1: -6, 2: -6, 3: -1, 4: -6, 5: -3, 6: -6}                  # viscous wall on kMin, symmetry on jMin
EULER_AD = {1: -6, 2: -6, 3: -1, 4: -6, 5: -5, 6: -6}
RANS = FlowParams(equations=RANSEquations)
RANS_UP = FlowParams(equations=RANSEquations, spaceDiscr=upwind)
RANS_DADI = FlowParams(equations=RANSEquations, smoother=DADI, resAveraging=noResAveraging, cfl=1.5, nSubiterations=2, nSubIterTurb=2)


def _dims(big):
    return BIG_DIMS if big else SMALL_DIMS


# ---- every checker call goes through `on`: recount first, on the very keywords and topology the checker gets ----------------------
MAKE_KEYS = ("shape", "lengths", "stretch_k")


@contextlib.contextmanager
def _spy(mk, calls):
    """every block the checker builds -- fine, coarse, each block of a brick -- must arrive at make_block with the case's shape and
    lengths: a keyword filter inside a checker or a topology that dropped them would otherwise run the entry on the cube unnoticed"""
    real, real_c = synth.make_block, checks.make_block

    def make_block(*a, **k):
        assert k.get("shape") is mk.get("shape"), "a checker built a block without the case's shape"
        assert tuple(k.get("lengths", (1.0, 1.0, 1.0))) == tuple(mk.get("lengths", (1.0, 1.0, 1.0))), "... without the case's lengths"
        if k.get("frame") is None and "params" not in k:
            assert k.get("stretch_k", 1.0) == mk.get("stretch_k", 1.0)
        calls.append(1)
        return real(*a, **k)

    synth.make_block = checks.make_block = make_block
    try:
        yield
    finally:
        synth.make_block, checks.make_block = real, real_c


def on(case, checker, engine, where, prm, *args, **kw):
    """checker(engine, where, prm, *args, **kw) on the case's mesh.  where: the block's dims or a topology.  First the family's recount
    (and the unit of length) on a block -- or on every block of the brick, through frame -- built with exactly the make_block keywords
    in kw; then the checker, with a spy on make_block that asserts that its own blocks carry the same shape and lengths."""
    mk = {k: kw[k] for k in MAKE_KEYS if k in kw}
    if hasattr(where, "make_block"):
        case.gate_brick(where, prm, mk)
    else:
        case.gate(tuple(where) if not hasattr(where, "nx") else (where.nx, where.ny, where.nz), prm, mk)
    calls = []
    with _spy(mk, calls):
        out = checker(engine, where, prm, *args, **kw)
    assert calls, "the checker built no block"
    return out


# ---- residual ------------------------------------------------------------------------------------------------------------------
RES_OPTIONS = {
    "euler-scalar": FlowParams(spaceDiscr=dissScalar), "euler-matrix": FlowParams(spaceDiscr=dissMatrix, vis4=0.1),
    "euler-upwind-vanalbada": FlowParams(spaceDiscr=upwind, limiter=vanAlbeda), "euler-upwind-minmod": FlowParams(spaceDiscr=upwind, limiter=minmod),
    "laminar": FlowParams(equations=NSEquations), "rans": RANS, "rans-upwind": RANS_UP, "rans-qcr": RANS.replace(useQCR=True),
}


def _res(key, marches=True, tiled=2):
    def run(engine, case, big):
        prm = RES_OPTIONS[key]
        for dims in _dims(big):
            with dispatch(engine, marches):
                if marches and tiled != 2:
                    engine.set_tuning("viscous_tiled", tiled)
                on(case, checks.check_block_res, engine, dims, prm, seed=3 + dims[0], **case.mk(prm.viscous))
    return run


def _res_others(engine, case, big):
    for dims in _dims(big):
        for prm in (FlowParams(spaceDiscr=dissScalar), RANS_UP):
            mk = case.mk(prm.viscous)
            on(case, checks.check_rk_residual_sequence, engine, dims, prm.replace(equations=NSEquations) if prm.viscous else prm, **mk)
            on(case, checks.check_block_res_vs_blockette, engine, dims, prm, update_intermed=True, **mk)
            on(case, checks.check_block_res_approx, engine, dims, prm, **mk)


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def _geometry(engine, case, big):
    # (the warps relative to the local edge length: a clustered, scaled or collapsed mesh stays one)
    on(case, checks.check_update_geometry, engine, SMALL, FlowParams(), {1: -1, 2: -6, 3: -5, 4: -5, 5: -1, 6: -6}, warp=WARP, **case.mk())
    on(case, checks.check_wall_distance, engine, SMALL, RANS, warp=WARP, **case.mk(True))
    on(case, checks.check_coarse_level_geometry, engine, case.brick((12, 8, 6)), FlowParams(), warp=WARP, **case.brick_mk())
    on(case, checks.check_coordinate_halos_brick, engine, case.brick((10, 9, 8)), FlowParams(), warp=WARP, **case.brick_mk())


# ---- boundaries ----------------------------------------------------------------------------------------------------------------
def _bc(engine, case, big):
    mk, mkv = case.mk(), case.mk(True)
    on(case, checks.check_apply_bc, engine, (10, 9, 8), FlowParams(), EULER, **mk)
    on(case, checks.check_apply_bc, engine, (10, 9, 8), FlowParams(Mach=0.3), SUBSONIC, **mk)
    on(case, checks.check_apply_bc, engine, (10, 9, 8), RANS, {1: -6, 2: -6, 3: -1, 4: -4, 5: -3, 6: -6}, **mkv)
    on(case, checks.check_xhalo_symmetry, engine, (10, 9, 8), FlowParams(), {1: -1, 2: -6, 3: -5, 4: -1, 5: -1, 6: -6}, warp=WARP, **mk)
    on(case, checks.check_wall_stress, engine, SMALL, RANS_UP, WALL, **mkv)


def _res_bc(engine, case, big):
    assert on(case, checks.check_blockette_res_with_bc, engine, case.brick((10, 9, 8), True), RANS_UP, WALL, **case.brick_mk()) > 0


def _pole_bc(kind):
    """the collapsed jMin face of `pole` under polar symmetry (-2), plain symmetry (-1: the collapsed-plane guard of the symmetry
    node halos) and an Euler wall (-5); the guard's condition -- normals of length zero -- recounted on the host"""
    def run(engine, case, big):
        assert case.family == "pole"
        mk = case.mk()
        dims = (10, 9, 8)
        blk = synth.make_block(*dims, FlowParams(), **mk)
        assert mf.zero_length_normals(blk, 3) == dims[0] * dims[2]
        spec = {1: -6, 2: -6, 3: kind, 4: -6, 5: -1, 6: -6}
        with _finite_bocos():
            on(case, checks.check_apply_bc, engine, dims, FlowParams(Mach=0.3), spec, **mk)
            if kind == -1:
                on(case, checks.check_xhalo_symmetry, engine, dims, FlowParams(), spec, warp=WARP, **mk)
                on(case, checks.check_update_geometry, engine, dims, FlowParams(), spec, warp=WARP, **mk)
    return run


@contextlib.contextmanager
def _finite_bocos():
    """make_bocos divides the face normal by its length: on a collapsed face the unit normal is what the reference's boundaryNormals
    leaves there, zero (adjointExtra.F90 boundaryNormals: fact = 1 / max(eps, |ss|) applied to ss = 0)"""
    real = synth.make_bocos

    def make_bocos(blk, prm, spec, **kw):
        with np.errstate(invalid="ignore", divide="ignore"):
            faces, nvisc = real(blk, prm, spec, **kw)
        for f in faces:
            f["norm"] = np.asfortranarray(np.where(np.isfinite(f["norm"]), f["norm"], 0.0))
        return faces, nvisc
    synth.make_bocos = make_bocos
    try:
        yield
    finally:
        synth.make_bocos = real


# ---- smoothers and solves ------------------------------------------------------------------------------------------------------
def _smoothers(engine, case, big):
    mk, topo = case.brick_mk(), case.brick((6, 8, 6))
    for ra in (noResAveraging, alternateResAveraging):
        on(case, checks.check_rk_smoother, engine, topo, FlowParams(resAveraging=ra), **mk)
    on(case, checks.check_dadi_smoother, engine, topo, FlowParams(resAveraging=noResAveraging, cfl=1.5), **mk)
    on(case, checks.check_dadi_smoother, engine, case.brick((6, 8, 6), True), RANS_DADI, **mk)
    on(case, checks.check_sa_solve, engine, case.brick((6, 8, 6), True), RANS.replace(nSubIterTurb=2), **mk)
    on(case, checks.check_smoother_with_bc, engine, (10, 9, 8), RANS_DADI, {1: -6, 2: -6, 3: -1, 4: -1, 5: -3, 6: -6}, **case.mk(True))


def _multigrid(engine, case, big):
    mk, topo = case.brick_mk(), case.brick((6, 8, 6))
    on(case, checks.check_mg_transfer, engine, topo, FlowParams(resAveraging=noResAveraging), **mk)
    on(case, checks.check_mg_cycle, engine, topo, FlowParams(), [0, 1, 0, -1], ncycles=1, brick_spec={1: -6, 2: -6, 3: -1, 4: -6, 5: -5, 6: -6}, **mk)


# ---- matrices ------------------------------------------------------------------------------------------------------------------
def _jac(ad, usePC):
    def run(engine, case, big):
        dims = JAC if usePC else JAC_EXACT
        prm = FlowParams(spaceDiscr=upwind) if (usePC and not ad) else RANS_UP
        on(case, checks.check_ad_jacobian if ad else checks.check_fd_jacobian, engine, dims, prm, WALL if prm.viscous else EULER_AD, usePC=usePC,
           **case.mk(prm.viscous))
    return run


def _nk(engine, case, big):
    from adflow_amd.topology import BrickTopology
    on(case, checks.check_nk_residual, engine, case.brick((12, 8, 6)), RANS_UP, bc_spec=None, **case.brick_mk())
    on(case, checks.check_nk_residual, engine, BrickTopology(1, 1, 1, 12, 8, 6), RANS_UP, bc_spec=WALL, **case.mk(True))


def _ank_T(engine, case, big):
    on(case, ank_checks.check_T_single, engine, JAC, RANS_UP, WALL, True, **case.mk(True))


def _ank_operator(engine, case, big):
    on(case, ank_checks.check_operator, engine, JAC_EXACT, RANS_UP, WALL, True, False, **case.mk(True))


def _ilu(engine, case, big):
    """One ILU(0) setup and apply at pc_checks' bar (the library at most 10 x as far from the longdouble factorisation as a float64
    numpy run of the same algorithm).  `annulus` (ratio 1e4) has pivot blocks with condition numbers up to 9.0e10: this case found that
    L_{c,n} = A_{c,n} D_n^-1 formed as a PRODUCT with the explicit inverse loses a digit there (emulator: 9.4e-11 / 1.34e-10 for
    M^-1 r / M^-T r against 1.58e-11 / 7.2e-12 of the numpy run, ratios 6.0 / 18.6), and k_pc_factor / k_pcc_factor now form it by a
    solve with D_n (pc_right_solve, csrc/pc_block.h): 4.4e-11 / 4.4e-11 on the emulator, 3.3e-11 / 2.8e-11 on the MI355X (numpy there:
    4.3e-11 / 6.9e-11).  DESIGN §5 has the experiment that located the loss in the factorisation and not in the sweeps.
    After the one draw the same factor goes under pc_checks.assert_apply_median (16 vectors per transpose, the median ratio at MARGIN)."""
    assert case.family in ("annulus", "clustered")
    on(case, pc_checks.check_single, engine, JAC, RANS_UP, WALL, median=True, **case.mk(True))


# ---- everything built on the assembled matrix --------------------------------------------------------------------------------------
# The factor entries are held to pc_checks.assert_apply_median: the median over 16 vectors per transpose of e_lib / e_np at MARGIN.  The
# one draw of assert_apply_matches is noise at these condition numbers (e_np varies by 4 to 21 from vector to vector).
MEDIAN = pc_checks.assert_apply_median
FACTOR_MESHES = ("annulus", "clustered", "units-annulus-2^-20", "units-clustered-2^10", "sheared")
MG_CONFIGS = [(3, 2, 2, 1), (2, 1, 0, 0)]          # (levels, nSmooth, fill, fillCoarse)


def _ilu_fill(engine, case, big):
    """ILU(1) and ILU(2) at nState 6, 5 and 1: pattern and level sets against the symbolic yardstick, applications, identity"""
    for jac in (dict(), dict(frozenTurb=True), dict(useTurbOnly=True)):
        on(case, pc_fill_checks.check_single, engine, JAC, RANS_UP, WALL, matches=MEDIAN, **jac, **case.mk(True))


def _ilu_coupled(engine, case, big):
    """the factor over the level on two blocks joined in i inside one map, against the level-wide yardstick, and far from block-local"""
    on(case, pc_coupled_checks.check_wall_topo, engine, case.brick((6, 8, 6), True), RANS_UP, WALL, matches=MEDIAN, **case.brick_mk())


def _pc_mg(engine, case, big):
    """the hierarchy: the coarse sums at their TERMS bar on volumes that span 1e5, the cycle against the numpy cycle"""
    on(case, pc_mg_checks.check_single, engine, JAC, RANS_UP, WALL, MG_CONFIGS, matches=MEDIAN, **case.mk(True))


def _ilu_multi(engine, case, big):
    on(case, multi_checks.check_sweeps_median, engine, JAC, RANS_UP, WALL, **case.mk(True))


def _ank_shifted(engine, case, big):
    """the ILU(0) of J + T, decoupled (nState 5) and coupled (nState 6: turbResScale and turbCFLScale both /= 1, as ank_checks.RANS_COUPLED)"""
    for coupled in (False, True):
        prm = RANS_UP.replace(turbResScale=1.0e3) if coupled else RANS_UP
        on(case, ank_checks.check_shifted_block, engine, JAC, prm, WALL, coupled, matches=MEDIAN, **case.mk(True))


def _jacmult(engine, case, big):
    """jacobianMult, both transposes, against numpy applying the REFERENCE's forward-mode blocks; then its own blocks to rounding"""
    for dims, usePC in ((JAC, True), (JAC_EXACT, False)):
        on(case, jacmult_checks.check_against_reference, engine, dims, RANS_UP, WALL, usePC=usePC, **case.mk(True))


def _jacfree(engine, case, big):
    """jacFreeMult against the reference's blocks, under the default dispatch and with the marches off"""
    for dims, jac in ((JAC, dict(usePC=True)), (JAC_EXACT, dict(usePC=False)), (JAC_EXACT, dict(usePC=False, frozenTurb=True))):
        on(case, jacfree_checks.check_against_reference, engine, dims, RANS_UP, WALL, **jac, **case.mk(True))


ENTRIES = {
    **{f"res-{k}": _res(k) for k in RES_OPTIONS},
    **{f"res-{k}-gather": _res(k, marches=False) for k in ("euler-scalar", "euler-upwind-vanalbada", "laminar", "rans-upwind")},
    **{f"res-{k}-untiled": _res(k, tiled=0) for k in ("laminar", "rans-qcr")},
    "res-sequence-blockette-approx": _res_others,
    "geometry": _geometry, "bc": _bc, "res-bc": _res_bc,
    "pole-polar-symmetry": _pole_bc(-2), "pole-symmetry": _pole_bc(-1), "pole-euler-wall": _pole_bc(-5),
    "smoothers": _smoothers, "multigrid": _multigrid,
    "jac-fd-pc": _jac(False, True), "jac-fd-exact": _jac(False, False), "jac-ad-pc": _jac(True, True), "jac-ad-exact": _jac(True, False),
    "nk": _nk, "ank-T": _ank_T, "ank-operator": _ank_operator, "ilu": _ilu,
    "ilu-fill": _ilu_fill, "ilu-coupled": _ilu_coupled, "pc-mg": _pc_mg, "ilu-multi": _ilu_multi, "ank-shifted": _ank_shifted,
    "jacmult": _jacmult, "jacfree": _jacfree,
}
# the entries the reference cannot run on `pole`: none -- reference_floor finds its outputs finite in every entry
POLE_OUT = ()
# entries whose yardstick is not the oracle but an extended-precision restatement built on the library's own matrix or time step, with a
# bar relative to the float64 run of the same restatement (ank_checks.py, pc_checks.py): there is no reference output to move.  What
# the oracle contributes to them -- the state, the boundary halos and, for `ilu`, the very matrix (forward mode, preconditioner, RANS
# upwind, WALL, (7, 6, 5)) -- has its floor asserted under `jac-ad-pc` and `bc` of the same mesh.  The same holds for every factor entry
# (`ilu-fill`, `ilu-coupled`, `pc-mg`, `ilu-multi`, `ank-shifted`): the matrix they factor is that assembly (on the brick: the same
# routine block by block), covered by `jac-ad-pc` of the same mesh.  `jacmult` and `jacfree` compare with the reference's matrix, which
# reference_floor records from their first call of check_ad_jacobian: they have a floor test of their own, at the assembly's bar.
NO_FLOOR = ("ank-T", "ank-operator", "ilu", "ilu-fill", "ilu-coupled", "pc-mg", "ilu-multi", "ank-shifted")
# the bars of the entries whose checker has one of its own: (global, local or None where the checker applies no local measure) --
# check_fd_jacobian: 1e-9 of the largest entry at delta = 1e-5 (a difference quotient amplifies rounding by 1 / delta), check_ad_jacobian: 1e-10
BARS = {"jac-fd-pc": (1e-9, None), "jac-fd-exact": (1e-9, None), "jac-ad-pc": (1e-10, None), "jac-ad-exact": (1e-10, None),
        "jacmult": (1e-10, None), "jacfree": (1e-10, None)}
ONLY = {"pole-polar-symmetry": ("pole",), "pole-symmetry": ("pole",), "pole-euler-wall": ("pole",),
        "ilu": ("annulus", "clustered", "units-annulus-2^-20", "units-clustered-2^10"),
        "ilu-fill": FACTOR_MESHES, "ilu-coupled": FACTOR_MESHES, "pc-mg": FACTOR_MESHES, "ank-shifted": FACTOR_MESHES,
        "ilu-multi": ("annulus", "clustered")}


def pairs():
    """(case name, entry name) of the tier"""
    out = []
    for c in CASES:
        for e in ENTRIES:
            if e in ONLY and c.name not in ONLY[e]:
                continue
            if c.family == "pole" and e in POLE_OUT:
                continue
            out.append((c.name, e))
    return out


def run(engine, case_name, entry, big):
    with _finite_bocos() if CASE[case_name].family == "pole" else contextlib.nullcontext():
        ENTRIES[entry](engine, CASE[case_name].for_entry(entry), big)


# ---- the reference's own conditioning ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _recording(moved):
    """option_checks.recording with the comparisons switched off -- the REFERENCE's side of every comparison, what the library gives
    plays no part -- plus the matrices of ref.fd_jacobian / ref.ad_jacobian.  moved: every block the checkers build has its nodes
    moved by one ulp (mesh_families.one_ulp_moved)."""
    from oracle import ref
    real = dict(mb=synth.make_block, cmb=checks.make_block, fd=ref.fd_jacobian, ad=ref.ad_jacobian)

    def make_block(*a, **k):
        blk = real["mb"](*a, **k)
        return mf.one_ulp_moved(blk) if moved else blk

    with recording(compare=False) as rec:
        def jacobian(which):
            def run(*a, **k):
                rec.append(np.array(real[which](*a, **k), dtype=np.float64, copy=True))
                raise _Recorded()          # the reference's matrix is all this pair compares: the library's assembly is not run
            return run

        synth.make_block = checks.make_block = make_block
        ref.fd_jacobian, ref.ad_jacobian = jacobian("fd"), jacobian("ad")
        try:
            yield rec
        finally:
            synth.make_block, checks.make_block = real["mb"], real["cmb"]
            ref.fd_jacobian, ref.ad_jacobian = real["fd"], real["ad"]


class _Recorded(Exception):
    pass


def reference_floor(engine, case_name, entry, big):
    """the change of the reference's outputs of one (case, entry) pair when every node moves by one ulp, in the suite's two measures,
    after asserting that they are finite.  `engine` only keeps the checkers running (the emulator); nothing it returns is read."""
    recs = []
    for moved in (False, True):
        with _recording(moved) as rec:
            try:
                run(engine, case_name, entry, big)
            except _Recorded:
                pass
        recs.append(rec)
    assert len(recs[0]) == len(recs[1]) > 0, "the two runs made different numbers of comparisons"
    g = l = 0.0
    for a, b in zip(*recs):
        assert a.shape == b.shape
        assert np.isfinite(a).all(), ("the reference's output is not finite", case_name, entry)
        gg, ll = mf.measures(b, a)
        g, l = max(g, gg), max(l, ll)
    return g, l
