"""Checks of the matrix-free exact products adflow_gpu_jacfree_mult[_dev] (y = dR/dw x by ONE forward-mode evaluation seeded with x:
dRdwMatMult, adjointAPI.F90:1050-1128) and of adflow_gpu_jacfree_solve[_dev] (GMRES on that product: the KSP of solveDirectForRHS on
the shell dRdwT), shared by tests/test_gpu_jacfree.py (real MI355X) and tests/test_hostsim_jacfree.py (the kernel-logic emulator).

Yardstick: numpy applying stencil blocks through the column map of jacmult_checks.LevelOperator -- the reference's own Tapenade
blocks (checks.check_ad_jacobian) on one block, the library's own forward-mode assembled blocks across blocks.  Bar: that of
jacmult_checks.check_against_reference, 1e-10 max|J| nStencil nState max|x|: every block entry may differ by the assembly's
1e-10 max|J|, a result entry sums nStencil nState products.  With the turbulence row (nState 6) the mean-flow rows take max|J| of
the mean-flow rows and the turbulence row its own, as check_ad_jacobian scales its blocks: next to a wall the SA diagonal dwarfs
everything else."""
import ctypes

import numpy as np
import pytest

import ank_turb_checks as ankt
import async_checks
import checks
import jacmult_checks as jm
import option_checks
from device_vectors import dev_call
from adflow_amd import capi
from adflow_amd.params import FlowParams, RANSEquations, dissScalar, dissMatrix, upwind, vanAlbeda, minmod
from adflow_amd.topology import BrickTopology

RANS = FlowParams(equations=RANSEquations, spaceDiscr=upwind, limiter=vanAlbeda)
_KEEP = []            # the reference's flowDoms point into these arrays: alive as long as ref may be called
MK_KEYS = ("stretch_k", "shape", "lengths", "moving", "wall_kmin")


def _split(jac):
    mk = {k: jac.pop(k) for k in MK_KEYS if k in jac}
    return mk, jac


def row_bound(J, st, x):
    """the bar per result entry (n,): J = {nn: blocks (nx, ny, nz, ll, l, s)} or one such array"""
    Js = list(J.values()) if isinstance(J, dict) else [J]
    ns, nst = Js[0].shape[3], np.asarray(st).shape[0]
    f = 1e-10 * nst * ns * float(np.abs(x).max())
    if ns != 6:
        return np.full(x.size, f * max(float(np.abs(B).max()) for B in Js))
    per = np.empty(6)
    per[:5] = max(float(np.abs(B[..., :5, :, :]).max()) for B in Js)
    per[5] = max(float(np.abs(B[..., 5, :, :]).max()) for B in Js)
    return np.tile(f * per, x.size // 6)


def assert_product(what, y, ref, bound):
    err = np.abs(y - ref)
    worst = int(np.argmax(err / bound))
    print(f"{what}: max|y - y_ref| = {err.max():.3e}, largest err / bound = {(err / bound).max():.3e}, max|y| = {np.abs(ref).max():.3e}")
    assert np.abs(ref).max() > 0.0 and np.isfinite(y).all(), what
    assert (err <= bound).all(), (what, worst, err[worst], bound[worst])


# ---- 1. against the reference's blocks --------------------------------------------------------------------------------------------
def check_against_reference(engine, dims, prm, spec, seed=211, approxSA=False, **jac):
    """jacFreeMult against numpy applying the REFERENCE's forward-mode blocks of one block with six physical faces (halo columns
    dropped), under the default dispatch and with the marches switched off.  Returns (operator of the reference's blocks, x)"""
    from oracle import ref
    mk, jac = _split(dict(jac))
    if approxSA:
        blk, r, prm = checks.setup_block_with_bc(engine, dims, prm, spec, seed, **mk)
        _KEEP[:] = [r]
        with ankt.ref_approx_sa():
            Jr = ref.ad_jacobian(blk.nx, blk.ny, blk.nz, jac.get("usePC", True), jac.get("frozenTurb", False), jac.get("useTurbOnly", False),
                                 jac.get("viscPC", False))
        Jfull = ref.ad_jacobian(blk.nx, blk.ny, blk.nz, jac.get("usePC", True), jac.get("frozenTurb", False), jac.get("useTurbOnly", False),
                                jac.get("viscPC", False))
        assert np.abs(Jr - Jfull).max() > 1e-6 * np.abs(Jr).max()           # the switch matters to the matrix
        engine.setupStateResidualMatrix(1, useAD=True, approxSA=True, **jac)
        st = engine.jacobianInfo()[1]
    else:
        _, Jr, st = checks.check_ad_jacobian(engine, dims, prm, spec, seed=seed, **mk, **jac)
    blk = engine.blocks[(1, 1, 1)]
    op = jm.LevelOperator({1: Jr}, {1: (blk.nx, blk.ny, blk.nz)}, st)
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, op.n)
    ref_y, bound = op.apply(x), row_bound(Jr, st, x)
    kw = dict(jac, usePC=jac.get("usePC", True), approxSA=approxSA)
    for marches in (True, False):
        with option_checks.dispatch(engine, marches):
            y = engine.jacFreeMult(x, 1, **kw)
        assert_product(f"{dims} {kw} marches={marches} vs reference blocks", y, ref_y, bound)
    return op, x


# ---- 2. across blocks ---------------------------------------------------------------------------------------------------------------
def check_brick(engine, topo, prm, seed=223, rccl_self=False):
    """against numpy applying the library's own forward-mode assembled blocks through the donor map of the 2-layer pattern: halos with
    donors in other blocks and in the block itself, shared donors, corners, rotated interfaces"""
    blocks, op = jm.brick_operator(engine, topo, prm, seed, useAD=True)
    x = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, op.n)
    ref_y, bound = op.apply(x), row_bound(op.J, op.st, x)
    y = engine.jacFreeMult(x, 1, usePC=True)
    assert_product(f"{len(blocks)} blocks", y, ref_y, bound)
    # the halo seeds matter: the same blocks without the donor map give another result
    assert np.abs(jm.LevelOperator(op.J, op.dims, op.st).apply(x) - y).max() > 1e-6 * np.abs(y).max()
    if rccl_self:
        engine.comm_init_single()
        try:
            engine.set_tuning("comm_self", 1)
            y2 = engine.jacFreeMult(x, 1, usePC=True)
        finally:
            engine.set_tuning("comm_self", 0)
        assert_product(f"{len(blocks)} blocks through pack / ncclSend / ncclRecv to the own rank / unpack", y2, ref_y, bound)
    engine.releaseWorkspace()


# ---- 3. tile-sized block ------------------------------------------------------------------------------------------------------------
def check_tile_sized_block(engine, dims=(70, 24, 40), seed=107):
    """partial waves, several waves per row, several k chunks, marches taken: the exact product against the own assembled exact
    matrix; the work space (the slab of dual arrays and the scratch of the vector) is handed back and laid out again"""
    blk, r, _ = checks.setup_block_with_bc(engine, dims, RANS, jm.WALL, seed, stretch_k=2.0)
    _KEEP[:] = [r]
    engine.setupStateResidualMatrix(1, False, useAD=True)
    op = jm.operator_of(engine, {1: blk})
    assert op.st.shape[0] == 33
    x = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, op.n)
    y = engine.jacFreeMult(x, 1)
    assert_product(f"{dims} exact", y, op.apply(x), row_bound(op.J, op.st, x))
    nbox = (dims[0] + 4) * (dims[1] + 4) * (dims[2] + 4)
    nbytes = engine.releaseWorkspace()
    # the slab holds at least the dual state and the dual residual (2 x nw x 16 B per box cell), the scratch nState doubles per box cell
    assert nbytes >= (2 * 6 * 16 + 6 * 8) * nbox, nbytes
    assert engine.releaseWorkspace() == 0
    assert np.array_equal(engine.jacFreeMult(x, 1), y)
    engine.releaseWorkspace()


# ---- 4. determinism and side effects --------------------------------------------------------------------------------------------------
def check_determinism_and_side_effects(engine, dims=(7, 6, 5), seed=227):
    rm = RANS.replace(limiter=minmod)

    def start():
        blk, r, prm = checks.setup_block_with_bc(engine, dims, rm, jm.WALL, seed, stretch_k=2.0)
        _KEEP[:] = [r]
        return blk, prm
    blk, prm = start()
    engine.setupStateResidualMatrix(1, True, useAD=True)                  # a matrix assembled earlier
    rng = np.random.default_rng(seed + 1)
    x = rng.uniform(-1.0, 1.0, 6 * blk.ncells)
    info0, J0, ym0 = engine.jacobianInfo(), engine.jacobianBlocks(1).copy(), engine.jacobianMult(x, 1)
    engine.download_state(1, 1)
    w0, dw0 = blk["w"].copy(), engine.download_residual(1, 1).copy()
    y = engine.jacFreeMult(x, 1)
    assert np.abs(y).max() > 0.0 and np.array_equal(engine.jacFreeMult(x, 1), y), "two calls with the same x"
    engine.download_state(1, 1)
    assert np.array_equal(blk["w"], w0) and np.array_equal(engine.download_residual(1, 1), dw0)
    info1 = engine.jacobianInfo()
    assert info1[0] == info0[0] and np.array_equal(info1[1], info0[1])
    assert np.array_equal(engine.jacobianBlocks(1), J0) and np.array_equal(engine.jacobianMult(x, 1), ym0)
    assert not np.array_equal(y, ym0)                                     # (the exact operator is not the preconditioner matrix)
    # another state: another product, and the one a fresh setup gives at that state
    wVec = checks.nk_state_vector({1: blk}, prm, np.random.default_rng(seed + 2))
    engine.setW(wVec)
    y2 = engine.jacFreeMult(x, 1)
    assert not np.array_equal(y2, y)
    engine.releaseWorkspace()
    blk, prm = start()
    engine.setW(wVec)
    assert np.array_equal(engine.jacFreeMult(x, 1), y2), "the product of a fresh setup at that state"
    engine.releaseWorkspace()


# ---- 5. device-pointer twin -----------------------------------------------------------------------------------------------------------
def check_dev_twin(engine, dv, dims=(7, 6, 5), seed=233):
    """adflow_gpu_jacfree_mult_dev on device vectors returns bit for bit what the host form returns and does not write x: one
    wall-bounded RANS block at nState 6, 5 and 1"""
    rng = np.random.default_rng(seed)
    rm = RANS.replace(limiter=minmod)
    blk, r, _ = checks.setup_block_with_bc(engine, dims, rm, jm.WALL, seed, stretch_k=2.0)
    _KEEP[:] = [r]
    for ns, kw in ((6, dict()), (5, dict(frozenTurb=True)), (1, dict(useTurbOnly=True)), (6, dict(usePC=True))):
        n = ns * blk.ncells
        x = rng.uniform(-1.0, 1.0, n)
        y = engine.jacFreeMult(x, 1, **kw)
        dx, dy = dv.put(x), dv.put(np.full(n, 7.0))
        dev_call(engine, dv, engine.jacFreeMultDev, dv.ptr(dx), dv.ptr(dy), n, 1, **kw)
        assert np.abs(y).max() > 0.0
        assert np.array_equal(dv.get(dy), y), kw
        assert np.array_equal(dv.get(dx), x), (kw, "x was written")
    engine.releaseWorkspace()


def check_enqueue_only_chain(engine, dv, dims=(7, 6, 5), seed=251, restart=60):
    """three _dev products and one _dev solve in the enqueue-only mode with ONE synchronise at the end, bit-equal to the same chain with
    a synchronise after every call (the pattern of async_checks)"""
    def setup(enqueue):
        blk, r, _ = checks.setup_block_with_bc(engine, dims, RANS, jm.WALL, seed, stretch_k=2.0)
        _KEEP[:] = [r]
        engine.pcSelect(0)
        engine.setupStateResidualMatrix(1, True, useAD=True)
        engine.pcSetup(1)
        engine.releaseWorkspace()                                         # the first product of the chain lays slab and scratch out
        n = 6 * blk.ncells
        rng = np.random.default_rng(seed + 1)
        host = {k: rng.uniform(-1.0, 1.0, n) for k in ("x1", "x2", "x3", "b")}
        d = {k: dv.put(v) for k, v in host.items()}
        d.update({k: dv.put(np.full(n, 7.0)) for k in ("y1", "y2", "y3", "xs")})
        return dict(n=n, host=host, d=d)

    def chain(c, link):
        d, n, p = c["d"], c["n"], dv.ptr
        link(engine.jacFreeMultDev, p(d["x1"]), p(d["y1"]), n, 1)
        link(engine.jacFreeMultDev, p(d["x2"]), p(d["y2"]), n, 1, usePC=True)
        link(engine.jacFreeMultDev, p(d["x3"]), p(d["y3"]), n, 1)
        its, r0, rn = link(engine.jacFreeSolveDev, p(d["b"]), p(d["xs"]), n, 1, restart=restart, maxIts=restart, rtol=1e-6)
        return dict(d, its=its, r0=r0, rn=rn)

    try:
        c, enq, syn = async_checks.both_runs(engine, dv, setup, chain)
        for k, v in c["host"].items():
            assert np.array_equal(enq[k], v), (k, "an input vector was written")
        assert 0 < enq["its"] < restart, enq["its"]
        # every link is the call it stands for: the host forms from the same setup give the same bits
        for xk, yk, kw in (("x1", "y1", dict()), ("x2", "y2", dict(usePC=True)), ("x3", "y3", dict())):
            assert np.array_equal(engine.jacFreeMult(c["host"][xk], 1, **kw), enq[yk]), yk
        assert not np.array_equal(enq["y1"], enq["y3"])
        async_checks.assert_bitwise("jacfree chain", enq, syn)
    finally:
        engine.pcRelease()
        engine.releaseWorkspace()


# ---- 6. the solve ---------------------------------------------------------------------------------------------------------------------
WALL_TOPO = dict(Bi=2, Bj=2, Bk=2, nx=6, ny=5, nz=4, periodic=(False,) * 3)


def check_solve(engine, restart, maxIts, rtol=1e-8, seed=281, **flags):
    """2 x 2 x 2 wall-bounded blocks, RANS Roe: the preconditioner matrix by forward mode and its factor; jacFreeSolve with the exact
    flags; then the assembled exact matrix and gmresSolve with the same factor, restart and tolerance.  The operators differ by
    rounding only: both converge, the iteration counts are equal or differ by one, and the true residual through the numpy operator
    is at most the reported one plus the bar of the product"""
    topo = BrickTopology(**WALL_TOPO)
    blocks, rblocks, bocos, prm = checks.setup_brick_with_bc(engine, topo, RANS, jm.WALL, seed, stretch_k=2.0)
    _KEEP[:] = [rblocks, bocos]
    engine.applyAllBC(1, True)
    engine.pcSelect(0)
    try:
        engine.setupStateResidualMatrix(1, True, useAD=True, **flags)
        engine.pcSetup(1)
        ns = engine.pcInfo()[0]
        n = ns * sum(b.ncells for b in blocks.values())
        b = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, n)
        nb = float(np.linalg.norm(b))
        kw = dict(restart=restart, maxIts=maxIts, rtol=rtol)
        x, its, r0, rn = engine.jacFreeSolve(b, 1, **kw, **flags)
        engine.setupStateResidualMatrix(1, False, useAD=True, **flags)
        op = jm.operator_of(engine, blocks, topo.patterns(2)[0])
        assert op.ns == ns and op.n == n
        xa, itsa, r0a, rna = engine.gmresSolve(b, 1, **kw)
        true = float(np.linalg.norm(b - op.apply(x)))
        slack = float(np.linalg.norm(row_bound(op.J, op.st, x)))
        print(f"jacFreeSolve nState={ns}: {its} iterations (assembled exact matrix: {itsa}; restart {restart}, cap {maxIts}), reported "
              f"||r|| / ||b|| = {rn / nb:.3e} (assembled {rna / nb:.3e}), true through numpy {true / nb:.3e}, bar of the product {slack:.3e}")
        assert 0 < itsa < maxIts and 0 < its < maxIts, (its, itsa, maxIts)
        assert abs(its - itsa) <= 1, (its, itsa)
        assert abs(r0 - nb) <= 1e-12 * nb
        assert rn <= rtol * nb, (rn, rtol * nb)
        assert true <= rn + slack, (true, rn, slack)
        # the solution as guess: nothing to do (at the level the recurrence grants the true residual, as pc_checks does)
        x2, its2, _, _ = engine.jacFreeSolve(b, 1, restart=restart, maxIts=maxIts, rtol=2 * rtol, x0=x, **flags)
        assert its2 == 0 and np.array_equal(x2, x), its2
    finally:
        engine.pcRelease()
        engine.releaseWorkspace()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def check_refusals(engine, dims=(7, 6, 5), seed=229):
    """every refusal with its message, before anything is launched: state, residual, matrix and factor are intact afterwards.  (More
    than one rank in the communicator cannot be had in one process: that refusal is gm_check_ranks', shared with gmres_solve.)"""
    lib = engine.lib
    rm = RANS.replace(limiter=minmod)
    ncell = int(np.prod(dims))
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, 6 * ncell)
    out, ok = np.zeros_like(x), np.zeros_like(x)              # of the refused calls; of the calls that go through
    px, po, pk = x.ctypes.data, out.ctypes.data, ok.ctypes.data
    PC, FROZEN, TURB = capi.JAC_PC, capi.JAC_FROZEN_TURB, capi.JAC_TURB_ONLY

    def refused(match, fns, args):
        for fn in fns:
            assert fn(*args) != 0, match
            assert match in lib.adflow_gpu_last_error().decode(), (match, lib.adflow_gpu_last_error().decode())
    mult = (lib.adflow_gpu_jacfree_mult, lib.adflow_gpu_jacfree_mult_dev)
    solve = (lib.adflow_gpu_jacfree_solve, lib.adflow_gpu_jacfree_solve_dev)
    tail = (30, 30, 1e-6, 0.0, 0, None, None, None)

    # Euler: no turbulence-only operator
    checks.setup_block_with_bc(engine, dims, FlowParams(spaceDiscr=dissScalar), jm.EULER, seed)
    refused("needs the RANS equations", mult, (1, TURB, px, po, ncell))
    # a moving block
    blk, r, _ = checks.setup_block_with_bc(engine, dims, FlowParams(spaceDiscr=dissScalar), jm.EULER, seed, moving=True)
    refused("moving blocks are not linearised", mult, (1, 0, px, po, 5 * ncell))

    blk, r, prm = checks.setup_block_with_bc(engine, dims, rm, jm.WALL, seed, stretch_k=2.0)
    _KEEP[:] = [r]
    engine.pcSelect(0)
    engine.pcRelease()
    refused("no factor", solve, (1, 0, px, po, x.size) + tail)
    engine.setupStateResidualMatrix(1, True, useAD=True)
    engine.pcSetup(1)
    engine.download_state(1, 1)
    w0, dw0, J0 = blk["w"].copy(), engine.download_residual(1, 1).copy(), engine.jacobianBlocks(1).copy()
    z0 = engine.pcApply(x, 1)
    try:
        refused("unknown flags", mult, (1, 64, px, po, x.size))
        refused("TURB_ONLY and FROZEN_TURB exclude each other", mult, (1, TURB | FROZEN, px, po, ncell))
        refused("is not the ground level", mult, (2, 0, px, po, x.size))
        refused("x is NULL", mult, (1, 0, None, po, x.size))
        refused("y is NULL", mult, (1, 0, px, None, x.size))
        refused("same vector", mult, (1, 0, px, px, x.size))
        refused("rows", mult, (1, 0, px, po, x.size + 6))
        refused("rows", mult, (1, FROZEN, px, po, x.size))
        refused("rows", mult, (1, TURB, px, po, x.size))
        # actuator regions, host hooks
        ids = np.asfortranarray(np.array([[3], [3], [3]], np.int32))
        engine.actuator_register([dict(block=np.ones(1, np.int32), cellIDs=ids, force=np.ones(3), heat=1.0, volume=1.0, relaxStart=-1.0,
                                       relaxEnd=-1.0)])
        try:
            refused("actuator regions are not linearised", mult, (1, 0, px, po, x.size))
        finally:
            engine.actuator_register([])
        hook = capi.BC_CALLBACK(lambda level, second: None)
        lib.adflow_gpu_set_bc_callback(ctypes.cast(hook, ctypes.c_void_p))
        try:
            refused("a host boundary-condition hook cannot be linearised", mult, (1, 0, px, po, x.size))
        finally:
            lib.adflow_gpu_set_bc_callback(None)
        lib.adflow_gpu_set_turb_bc_callback(ctypes.cast(hook, ctypes.c_void_p))
        try:
            refused("a host turbulence boundary-condition hook cannot be linearised", mult, (1, 0, px, po, x.size))
        finally:
            lib.adflow_gpu_set_turb_bc_callback(None)
        # a rotational periodicity on the 2-layer pattern where the mean-flow variables are covered; not for the turbulence alone
        R = np.array([[np.cos(0.3), -np.sin(0.3), 0.0], [np.sin(0.3), np.cos(0.3), 0.0], [0.0, 0.0, 1.0]])
        rot = dict(rotMatrix=R, rotCenter=np.zeros(3), translation=np.zeros(3), block=np.array([1], np.int32),
                   indices=np.asfortranarray(np.array([[1, 3, 3]], np.int32)))
        engine.comm_register_periodic(1, 2, [rot])
        try:
            refused("rotational periodicity is not supported", mult, (1, 0, px, po, x.size))
        finally:
            engine.comm_register_periodic(1, 2, [])
        # the solve
        refused("nState", solve, (1, FROZEN, px, po, 5 * ncell) + tail)
        refused("same vector", solve, (1, 0, px, px, x.size) + tail)
        refused("rows", solve, (1, 0, px, po, x.size - 6) + tail)
        refused("unknown flags", solve, (1, 128, px, po, x.size) + tail)
        refused("restart = 0", solve, (1, 0, px, po, x.size, 0, 10, 1e-6, 0.0, 0, None, None, None))
        refused("rtol = -1", solve, (1, 0, px, po, x.size, 10, 10, -1.0, 0.0, 0, None, None, None))
        assert not out.any(), "a refused call wrote its result"
        engine.download_state(1, 1)
        assert np.array_equal(blk["w"], w0) and np.array_equal(engine.download_residual(1, 1), dw0)
        assert np.array_equal(engine.jacobianBlocks(1), J0)
        assert np.array_equal(engine.pcApply(x, 1), z0)
        # what is NOT refused: frozen turbulence runs no turbulence hook, and the turbulence variable alone is not rotated
        lib.adflow_gpu_set_turb_bc_callback(ctypes.cast(hook, ctypes.c_void_p))
        try:
            assert lib.adflow_gpu_jacfree_mult(1, FROZEN, px, pk, 5 * ncell) == 0 and ok.any()
        finally:
            lib.adflow_gpu_set_turb_bc_callback(None)
        engine.comm_register_periodic(1, 2, [rot])
        try:
            assert lib.adflow_gpu_jacfree_mult(1, TURB, px, pk, ncell) == 0
        finally:
            engine.comm_register_periodic(1, 2, [])
    finally:
        engine.pcRelease()
        engine.release_all()
