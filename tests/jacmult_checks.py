"""Checks of adflow_gpu_jacobian_mult (y = J x, y = J^T x with the matrix adflow_gpu_fd_jacobian left on the device) shared by
tests/test_gpu_jacmult.py (real MI355X) and tests/test_hostsim_jacmult.py (the kernel-logic emulator).

The numpy side applies stencil blocks (nx, ny, nz, nState, nState, nStencil) per block of the level through a column map: an owned
cell is its own column, a halo cell is the owned cell it has as donor in the 2-layer pattern, every other halo cell is no column
(adjointUtils.F90:560-700, globalCell >= 0).  Vectors: block, k, j, i, variable fastest."""
import ctypes

import numpy as np

import checks
from device_vectors import dev_call
from adflow_amd import capi
from adflow_amd.params import FlowParams, RANSEquations, dissScalar, upwind, vanAlbeda, minmod

EPS = 2.0 ** -52
WALL = {1: -6, 2: -6, 3: -1, 4: -1, 5: -3, 6: -6}
EULER = {1: -6, 2: -6, 3: -5, 4: -15, 5: -1, 6: -9}
OPEN = {1: -6, 3: -1, 4: -1, 6: -6}          # faces 2 and 5 without subfaces: non-zero blocks on halo columns that have no donor


class LevelOperator:
    """the level's matrix in numpy: J = {nn: blocks}, dims = {nn: (nx, ny, nz)}, st (nStencil, 3), pattern = 2-layer CommPattern or None"""

    def __init__(self, J, dims, st, pattern=None):
        self.J, self.dims, self.st = J, dims, np.asarray(st)
        self.ns = next(iter(J.values())).shape[3]
        self.off, n = {}, 0
        for nn in sorted(dims):
            self.off[nn] = n
            n += int(np.prod(dims[nn]))
        self.ncell = n
        self.colmap = {}
        for nn, (nx, ny, nz) in dims.items():
            m = np.full((nx + 4, ny + 4, nz + 4), -1, np.int64)
            I, J_, K = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
            m[2:nx + 2, 2:ny + 2, 2:nz + 2] = self.off[nn] + (K * ny + J_) * nx + I
            self.colmap[nn] = m
        if pattern is not None and pattern.ncopy:
            db, di = pattern.donorBlock, np.asarray(pattern.donorIndices)
            hb, hi = pattern.haloBlock, np.asarray(pattern.haloIndices)
            for t in range(pattern.ncopy):
                d, h = int(db[t]), int(hb[t])
                nx, ny, nz = dims[d]
                g = self.off[d] + ((di[t, 2] - 2) * ny + (di[t, 1] - 2)) * nx + (di[t, 0] - 2)
                assert 2 <= di[t, 0] <= nx + 1 and 2 <= di[t, 1] <= ny + 1 and 2 <= di[t, 2] <= nz + 1, "donors are owned cells"
                self.colmap[h][hi[t, 0], hi[t, 1], hi[t, 2]] = g

    @property
    def n(self):
        return self.ncell * self.ns

    def apply(self, x, transpose=False, absolute=False):
        X = np.asarray(x).reshape(self.ncell, self.ns)
        if absolute:
            X = np.abs(X)
        Y = np.zeros_like(X)
        for nn, (nx, ny, nz) in self.dims.items():
            I, J_, K = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
            rows = (self.off[nn] + (K * ny + J_) * nx + I).ravel()
            for s in range(self.st.shape[0]):
                d = self.st[s]
                cols = self.colmap[nn][I + 2 - d[0], J_ + 2 - d[1], K + 2 - d[2]].ravel()
                ok = cols >= 0
                B = self.J[nn][..., s].reshape(nx * ny * nz, self.ns, self.ns)[ok]       # (row, ll, l)
                if absolute:
                    B = np.abs(B)
                if transpose:
                    np.add.at(Y, cols[ok], np.einsum("nab,na->nb", B, X[rows[ok]]))
                else:
                    Y[rows[ok]] += np.einsum("nab,nb->na", B, X[cols[ok]])
        return Y.reshape(-1)


def operator_of(engine, blocks, pattern=None):
    ns, st = engine.jacobianInfo()
    J = {nn: engine.jacobianBlocks(nn).copy() for nn in blocks}
    return LevelOperator(J, {nn: (b.nx, b.ny, b.nz) for nn, b in blocks.items()}, st, pattern)


def assert_products_to_rounding(engine, op, seed, what):
    """the product alone: |y - y_np| <= 2 n eps (|B| |x|) entry by entry, n = nStencil nState (the bound of a length-n dot product,
    doubled for the other summation order and FMA contraction).  Returns the device products."""
    rng = np.random.default_rng(seed)
    n = op.st.shape[0] * op.ns
    out = {}
    for tr in (False, True):
        x = rng.uniform(-1.0, 1.0, op.n)
        y = engine.jacobianMult(x, 1, transpose=tr)
        ref, bound = op.apply(x, tr), 2 * n * EPS * op.apply(x, tr, absolute=True)
        err = np.abs(y - ref)
        worst = int(np.argmax(err - bound))
        print(f"{what} transpose={tr}: max|y - y_np| = {err.max():.3e}, largest err / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}, "
              f"max|y| = {np.abs(ref).max():.3e}")
        assert (err <= bound).all(), (what, tr, worst, err[worst], bound[worst])
        assert np.abs(ref).max() > 0.0
        out[tr] = (x, y)
    return out


def check_against_reference(engine, dims, prm, spec, seed=211, **jac):
    """1: the products against numpy applying the REFERENCE's blocks (ref.ad_jacobian, halo columns dropped: one block, empty
    patterns) -- each block entry may differ by the assembly's 1e-10 max|Jr|, a result entry sums nStencil nState products.
    2: against numpy applying the library's own downloaded blocks, to rounding"""
    Jg, Jr, st = checks.check_ad_jacobian(engine, dims, prm, spec, **jac)
    blk = engine.blocks[(1, 1, 1)]
    d = {1: (blk.nx, blk.ny, blk.nz)}
    opr, opg = LevelOperator({1: Jr}, d, st), LevelOperator({1: Jg.copy()}, d, st)
    ns, nst = opr.ns, st.shape[0]
    rng = np.random.default_rng(seed)
    for tr in (False, True):
        x = rng.uniform(-1.0, 1.0, opr.n)
        y = engine.jacobianMult(x, 1, transpose=tr)
        bound = 1e-10 * np.abs(Jr).max() * nst * ns * np.abs(x).max()
        err = np.abs(y - opr.apply(x, tr)).max()
        print(f"{dims} vs reference blocks, transpose={tr}: max|y - y_ref| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (dims, tr, err, bound)
    assert_products_to_rounding(engine, opg, seed + 1, f"{dims} own blocks")
    return opg


def brick_operator(engine, topo, prm, seed=223, useAD=False, **mk):
    """mk: the mesh keywords of checks.setup_brick (make_block / topo.make_block)"""
    blocks, _ = checks.setup_brick(engine, topo, prm, seed, **mk)
    engine.setupStateResidualMatrix(1, True, delta=1e-6, useAD=useAD)
    return blocks, operator_of(engine, blocks, topo.patterns(2)[0])


def check_brick(engine, topo, prm, seed=223, rccl_self=False):
    """3: across blocks (halos with donors in other blocks and in the block itself, shared donors, corners), and 4: the adjoint
    identity |<J x, y> - <x, J^T y>| <= 4 N eps <|J| |x|, |y|>"""
    blocks, op = brick_operator(engine, topo, prm, seed)
    first = assert_products_to_rounding(engine, op, seed + 1, "brick")
    # the halo columns matter: the same blocks without the donor map give another result
    x, y = first[False]
    assert np.abs(LevelOperator(op.J, op.dims, op.st).apply(x) - y).max() > 1e-6 * np.abs(y).max()
    rng = np.random.default_rng(seed + 2)
    x, y = rng.uniform(-1.0, 1.0, op.n), rng.uniform(-1.0, 1.0, op.n)
    lhs = float(np.dot(engine.jacobianMult(x, 1), y))
    rhs = float(np.dot(x, engine.jacobianMult(y, 1, transpose=True)))
    bound = 4 * op.n * EPS * float(np.dot(op.apply(x, absolute=True), np.abs(y)))
    print(f"adjoint identity: |<Jx,y> - <x,JTy>| = {abs(lhs - rhs):.3e} (bound {bound:.3e})")
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    # the accumulation of the reverse exchange runs over donor-sorted lists: two calls agree bit for bit
    for tr in (False, True):
        xx, yy = first[tr]
        assert np.array_equal(engine.jacobianMult(xx, 1, transpose=tr), yy), ("repeatable", tr)
    if rccl_self:
        engine.comm_init_single()
        try:
            engine.set_tuning("comm_self", 1)
            assert_products_to_rounding(engine, op, seed + 1, "brick through pack / ncclSend / ncclRecv to the own rank / unpack")
        finally:
            engine.set_tuning("comm_self", 0)
    return op


def check_dev_twin(engine, dv, topo, dims=(7, 6, 5), seed=233):
    """adflow_gpu_jacobian_mult_dev on device vectors (dv: device_vectors.HostVectors / TorchVectors) returns bit for bit what
    adflow_gpu_jacobian_mult returns from the same x: the same kernels, launch geometry and donor-sorted accumulation.  One
    wall-bounded RANS block at nState 6, 5 and 1, and the blocks of `topo` (halo columns with donors), both transposes"""
    rng = np.random.default_rng(seed)

    def both(what):
        n = engine.jacobianInfo()[0] * sum(b.ncells for (nn, lv, sps), b in engine.blocks.items() if lv == 1)
        for tr in (False, True):
            x = rng.uniform(-1.0, 1.0, n)
            y = engine.jacobianMult(x, 1, transpose=tr)
            dx, dy = dv.put(x), dv.empty(n)
            dev_call(engine, dv, engine.jacobianMultDev, dv.ptr(dx), dv.ptr(dy), n, 1, tr)
            assert np.abs(y).max() > 0.0
            assert np.array_equal(dv.get(dy), y), (what, tr)
            assert np.array_equal(dv.get(dx), x), (what, tr, "x was written")

    rans = FlowParams(equations=RANSEquations, spaceDiscr=upwind, limiter=vanAlbeda)
    for jac in (dict(), dict(frozenTurb=True), dict(useTurbOnly=True)):
        keep = checks.setup_block_with_bc(engine, dims, rans, WALL, seed, stretch_k=2.0)    # (the reference's flowDoms point into keep[1])
        engine.setupStateResidualMatrix(1, True, useAD=True, **jac)
        both(f"{dims} {jac}")
    brick_operator(engine, topo, FlowParams(spaceDiscr=upwind), seed)
    both("brick")
    engine.releaseWorkspace()


def check_refusals_and_side_effects(engine, dims=(7, 6, 5)):
    """6: every error with its message; state and residual untouched; repeatable; the device-pointer form is exercised by
    tools/jac_mult.py"""
    import pytest
    from adflow_amd.synth import make_block
    lib = engine.lib
    prm = FlowParams(spaceDiscr=dissScalar)
    engine.release_all()                                   # no block, no matrix
    x = np.ones(5 * int(np.prod(dims)))
    with pytest.raises(capi.AdflowGpuError, match="no assembled Jacobian"):
        engine.jacobianMult(x, 1)
    blk, _, prm = checks.setup_block_with_bc(engine, dims, prm, EULER, 227)
    engine.setupStateResidualMatrix(1, True, delta=1e-6)
    engine.download_state(1, 1)
    w0, dw0 = blk["w"].copy(), engine.download_residual(1, 1).copy()
    rng = np.random.default_rng(229)
    x = rng.uniform(-1.0, 1.0, x.size)
    y, yt = engine.jacobianMult(x, 1), engine.jacobianMult(x, 1, transpose=True)
    assert np.array_equal(engine.jacobianMult(x, 1), y) and np.array_equal(engine.jacobianMult(x, 1, transpose=True), yt)
    engine.download_state(1, 1)
    assert np.array_equal(blk["w"], w0) and np.array_equal(engine.download_residual(1, 1), dw0)
    out = np.zeros_like(x)
    for args, msg in (((2, 0, x.ctypes.data, out.ctypes.data, x.size), "not the level of the assembly"),
                      ((1, 0, None, out.ctypes.data, x.size), "x is NULL"),
                      ((1, 1, x.ctypes.data, None, x.size), "y is NULL"),
                      ((1, 0, x.ctypes.data, x.ctypes.data, x.size), "same vector"),
                      ((1, 1, x.ctypes.data, out.ctypes.data, x.size + 5), "rows"),
                      ((1, 0, x.ctypes.data, out.ctypes.data, 6 * int(np.prod(dims))), "rows")):
        for fn in (lib.adflow_gpu_jacobian_mult, lib.adflow_gpu_jacobian_mult_dev):
            assert fn(*args) != 0, msg
            assert msg in lib.adflow_gpu_last_error().decode(), (msg, lib.adflow_gpu_last_error().decode())
    # a rotational periodicity on the 2-layer pattern: refused, not ignored (the matrix covers the velocities)
    R = np.array([[np.cos(0.3), -np.sin(0.3), 0.0], [np.sin(0.3), np.cos(0.3), 0.0], [0.0, 0.0, 1.0]])
    rot = dict(rotMatrix=R, rotCenter=np.zeros(3), translation=np.zeros(3), block=np.array([1], np.int32),
               indices=np.asfortranarray(np.array([[1, 3, 3]], np.int32)))
    engine.comm_register_periodic(1, 2, [rot])
    with pytest.raises(capi.AdflowGpuError, match="rotational periodicity is not supported"):
        engine.jacobianMult(x, 1)
    engine.comm_register_periodic(1, 2, [dict(rot, rotMatrix=np.eye(3), translation=np.array([0.0, 0.0, 0.4]))])
    assert np.array_equal(engine.jacobianMult(x, 1), y)               # a pure translation needs nothing
    engine.comm_register_periodic(1, 2, [])
    # a block registered after the assembly has no blocks of the matrix
    engine.register(make_block(4, 3, 3, prm, seed=231), nn=2, level=1)
    with pytest.raises(capi.AdflowGpuError, match="has no assembled blocks"):
        engine.jacobianMult(np.ones(x.size + 5 * 36), 1)
    engine.release_all()
