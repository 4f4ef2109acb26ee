"""Checks of the multigrid preconditioner (adflow_gpu_pc_set_mg, adflow_gpu_pc_mg_info, adflow_gpu_pc_mg_download) shared by
tests/test_gpu_pc_mg.py (real MI355X) and tests/test_hostsim_pc_mg.py (the kernel-logic emulator).

The yardstick is numpy and knows nothing of the library's layout: the fine rows are the stencil blocks the library hands out
(jacmult_checks.operator_of) restricted to the columns inside each structured block, as pc_checks.NumpyILU0 restricts them, plus T from
ankTimeStepBlocks in the ANK cases; the fine cell (i, j, k) of a block belongs to the coarse cell (i // 2, j // 2, k // 2) of the same
block; A_{l+1} = P^T A_l P as explicit sums; per level pc_checks.NumpyILU0 or pc_fill_checks.NumpyILUk on a synthetic operator of the
coarse dimensions; the cycle written from amg.F90:712-759.  All of it runs in float64 and in np.longdouble with the same code.

Bars:
  application      max|z_lib - z_ld| <= pc_checks.MARGIN (10) x the error of the float64 numpy run against longdouble, both transposes
  coarse matrices  level l + 1 of pcMgMatrix against the sums formed from the LIBRARY's level l, entrywise: |diff| <= 32 eps x (sum of the
                   absolute values of the terms) -- 32 is the most terms an entry has (8 diagonals and 24 entries across the 12 faces
                   inside a full aggregate), and a sum of m terms in any order is within (m - 1) eps of that bound
  level 1          equal to the assembled in-block blocks bit for bit without T; with T within 2 eps (|entry| + |T|) per entry: the
                   product that forms the entry of T and its addition are one rounding each, of the term and of the sum, in the
                   library's arithmetic (which may contract them) and in numpy's"""
import contextlib

import numpy as np

import ank_checks as ank
import ank_turb_checks as ankt
import jacmult_checks as jm
import pc_checks as pc
import pc_fill_checks as pcf
import device_vectors  # noqa: F401  (torch before the library, see there)
from adflow_amd import capi

EPS = pc.EPS
TERMS = 32


@contextlib.contextmanager
def mg_of(engine, levels, nsmooth=1, fill_coarse=0, fill=0, slot=0):
    """the setting of the setups inside; both slots are back at one level and fill 0 and slot 0 is selected afterwards"""
    engine.pcSelect(slot)
    engine.pcSetFill(fill)
    engine.pcSetMg(levels, nsmooth, fill_coarse)
    try:
        yield
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcSetFill(0)
            engine.pcSetMg(1, 1, 0)


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------
def in_block(J, st):
    """the blocks (nx, ny, nz, ns, ns, nStencil) with every entry whose column (row - st[s]) lies outside the block set to zero"""
    nx, ny, nz = J.shape[:3]
    out = J.copy()
    I, Jj, K = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    for s in range(st.shape[0]):
        ci, cj, ck = I - st[s, 0], Jj - st[s, 1], K - st[s, 2]
        outside = ~((0 <= ci) & (ci < nx) & (0 <= cj) & (cj < ny) & (0 <= ck) & (ck < nz))
        out[..., s][outside] = 0
    return out


def coarsen(J, st, absolute=False):
    """P^T A P of one block as explicit sums: every fine entry (row, column inside the block) is added to the coarse entry (row // 2,
    column // 2), which is the diagonal when both lie in one aggregate and the entry of the same stencil offset otherwise"""
    nx, ny, nz = J.shape[:3]
    s0 = int(np.where((st == 0).all(axis=1))[0][0])
    C = np.zeros(((nx + 1) // 2, (ny + 1) // 2, (nz + 1) // 2) + J.shape[3:], dtype=J.dtype)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                for s in range(st.shape[0]):
                    ci, cj, ck = i - st[s, 0], j - st[s, 1], k - st[s, 2]
                    if not (0 <= ci < nx and 0 <= cj < ny and 0 <= ck < nz):
                        continue
                    same = (ci // 2, cj // 2, ck // 2) == (i // 2, j // 2, k // 2)
                    B = J[i, j, k, :, :, s]
                    C[i // 2, j // 2, k // 2, :, :, s0 if same else s] += np.abs(B) if absolute else B
    return C


class NumpyMG:
    """the cycle of amg.F90:712-759, block-local, on the numpy operator `op` (its blocks restricted to the in-block columns)"""

    def __init__(self, op, dtype, levels, nsmooth=1, fill=0, fill_coarse=0):
        self.dtype, self.ns, self.nsmooth, self.st = dtype, op.ns, nsmooth, np.asarray(op.st)
        self.n = op.n
        nns = sorted(op.dims)
        J = {nn: in_block(np.array(op.J[nn], dtype=dtype), self.st) for nn in nns}
        self.ops, self.ilu, self.parent = [], [], []
        for l in range(levels):
            if l > 0:
                J = {nn: coarsen(J[nn], self.st) for nn in nns}
            lop = jm.LevelOperator(J, {nn: J[nn].shape[:3] for nn in nns}, self.st)
            self.ops.append(lop)
            f = fill if l == 0 else fill_coarse
            self.ilu.append(pc.NumpyILU0(lop, dtype) if f == 0 else pcf.NumpyILUk(lop, dtype, f))
        for l in range(levels - 1):                       # number of the coarse cell of every fine cell, in the order of the vectors
            F, C = self.ops[l], self.ops[l + 1]
            par = np.zeros(F.ncell, np.int64)
            for nn in nns:
                nx, ny, nz = F.dims[nn]
                cx, cy, cz = C.dims[nn]
                K, Jj, I = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
                par[F.off[nn]:F.off[nn] + nx * ny * nz] = (C.off[nn] + ((K // 2) * cy + Jj // 2) * cx + I // 2).ravel()
            self.parent.append(par)

    def cells(self):
        return tuple(o.ncell for o in self.ops)

    def product(self, l, x, transpose):
        """A_l x or A_l^T x: the in-block columns only (the blocks of the other columns are zero)"""
        op, ns = self.ops[l], self.ns
        X = np.asarray(x, dtype=self.dtype).reshape(op.ncell, ns)
        Y = np.zeros_like(X)
        for nn, (nx, ny, nz) in op.dims.items():
            lo = op.off[nn]
            Xb = X[lo:lo + nx * ny * nz].reshape(nz, ny, nx, ns).transpose(2, 1, 0, 3)
            Yb = np.zeros((nx, ny, nz, ns), dtype=self.dtype)
            for s in range(self.st.shape[0]):
                d = self.st[s]
                row = tuple(slice(max(0, d[a]), (nx, ny, nz)[a] + min(0, d[a])) for a in range(3))
                col = tuple(slice(max(0, -d[a]), (nx, ny, nz)[a] + min(0, -d[a])) for a in range(3))
                B = op.J[nn][..., s][row]
                if transpose:
                    Yb[col] += np.einsum("ijkab,ijka->ijkb", B, Xb[row])
                else:
                    Yb[row] += np.einsum("ijkab,ijkb->ijka", B, Xb[col])
            Y[lo:lo + nx * ny * nz] = Yb.transpose(2, 1, 0, 3).reshape(-1, ns)
        return Y.reshape(-1)

    def smooth(self, l, b, transpose):
        """Richardson from zero, nSmooth iterations, one ILU application each (setupShellPC)"""
        x = self.ilu[l].apply(b, transpose)
        for _ in range(self.nsmooth - 1):
            x = x + self.ilu[l].apply(b - self.product(l, x, transpose), transpose)
        return x

    def cycle(self, r, l, transpose):
        ns, par = self.ns, self.parent[l]
        C = self.ops[l + 1]
        rhs = np.zeros((C.ncell, ns), dtype=self.dtype)
        np.add.at(rhs, par, np.asarray(r, dtype=self.dtype).reshape(-1, ns))
        rhs = rhs.reshape(-1)
        sol = self.smooth(l + 1, rhs, transpose) if l + 2 == len(self.ops) else self.cycle(rhs, l + 1, transpose)
        y = sol.reshape(C.ncell, ns)[par].reshape(-1)
        res = np.asarray(r, dtype=self.dtype) - self.product(l, y, transpose)
        return y + self.smooth(l, res, transpose)

    def apply(self, r, transpose=False):
        if len(self.ops) == 1:
            return self.ilu[0].apply(r, transpose)
        return self.cycle(np.asarray(r, dtype=self.dtype), 0, transpose)

    def pivot_conditions(self):
        return max(i.pivot_conditions() for i in self.ilu)


def yardsticks(op, levels, nsmooth=1, fill=0, fill_coarse=0):
    return tuple(NumpyMG(op, t, levels, nsmooth, fill, fill_coarse) for t in (np.float64, np.longdouble))


# ---- the hierarchy that stands in the selected slot against the yardstick --------------------------------------------------------------
def assert_matrices(engine, op, levels, what, T=None):
    """level 1 against the in-block blocks of `op` (T: the blocks of the pseudo-time term op carries on its diagonal, or None), every
    coarser level against the sums formed from the library's own finer level"""
    st = np.asarray(op.st)
    s0 = int(np.where((st == 0).all(axis=1))[0][0])
    for nn in sorted(op.dims):
        fine = engine.pcMgMatrix(1, nn)
        want = in_block(op.J[nn], st)
        if T is None:
            assert np.array_equal(fine, want), (what, nn, "level 1 is not the assembled in-block blocks bit for bit")
        else:
            bound = np.zeros_like(want)
            bound[..., s0] = 2 * EPS * (np.abs(want[..., s0]) + np.abs(np.transpose(T[nn], (2, 3, 4, 0, 1))))
            off = np.ones(st.shape[0], bool)
            off[s0] = False
            assert np.array_equal(fine[..., off], want[..., off]), (what, nn, "off-diagonal blocks of level 1")
            err = np.abs(fine - want)
            print(f"{what} block {nn}: level 1 with T, largest |diff| / bound = {(err[..., s0] / np.maximum(bound[..., s0], 1e-300)).max():.3f}")
            assert (err <= bound).all(), (what, nn, float(err.max()))
        for l in range(1, levels):
            coarse = engine.pcMgMatrix(l + 1, nn)
            sums, mags = coarsen(fine, st), coarsen(fine, st, absolute=True)
            assert coarse.shape == sums.shape, (coarse.shape, sums.shape)
            err = np.abs(coarse - sums)
            print(f"{what} block {nn}: level {l + 1} {coarse.shape[:3]}, largest |diff| / (eps sum|terms|) = "
                  f"{(err / np.maximum(EPS * mags, 1e-300)).max():.3f} (bar {TERMS}), max|entry| = {np.abs(sums).max():.3e}")
            assert (err <= TERMS * EPS * mags).all(), (what, nn, l + 1)
            assert np.abs(sums).max() > 0.0
            fine = coarse


def assert_hierarchy(engine, op, levels, nsmooth, fill, fill_coarse, seed, what, T=None, cells=None, matches=None):
    """info, matrices and both applications of the hierarchy that stands in the selected slot.  Returns pc_checks' (first, yardsticks).
    matches: the comparison of the applications (default pc_checks.assert_apply_matches, one draw; pc_checks.assert_apply_median: 16)"""
    ys = yardsticks(op, levels, nsmooth, fill, fill_coarse)
    info = engine.pcMgInfo()
    print(f"{what}: pcMgInfo = {info}, pcInfo = {engine.pcInfo()}")
    assert info == (levels, nsmooth, fill_coarse, ys[0].cells()), (info, ys[0].cells())
    if cells is not None:
        assert info[3] == tuple(cells), (info, cells)
    assert engine.pcInfo2()[0] == fill and engine.pcInfo()[0] == op.ns
    assert_matrices(engine, op, levels, what, T)
    return (matches or pc.assert_apply_matches)(engine, op, seed + 1, f"{what} levels={levels} nSmooth={nsmooth} fills=({fill},{fill_coarse})",
                                                ilus=ys)


def check_single(engine, dims, prm, spec, configs, seed=107, cells=None, matches=None, **jac):
    """one block; configs: (levels, nSmooth, fill, fillCoarse) on the same assembly; cells = {levels: cells of every level}; matches: see
    assert_hierarchy"""
    blk, op = pc.single_block(engine, dims, prm, spec, seed, **jac)
    for levels, nsmooth, fill, fc in configs:
        with mg_of(engine, levels, nsmooth, fc, fill):
            engine.pcSetup(1)
            assert_hierarchy(engine, op, levels, nsmooth, fill, fc, seed, f"{dims} nState={op.ns}", cells=cells and cells[levels],
                             matches=matches)
            engine.pcRelease()
    return blk, op


def check_brick(engine, topo, prm, seed=223):
    """blocks with different offsets on every level, 2 levels; the couplings across blocks are absent from the cycle"""
    blocks, op = jm.brick_operator(engine, topo, prm, seed)
    with mg_of(engine, 2):
        engine.pcSetup(1)
        assert_hierarchy(engine, op, 2, 1, 0, 0, seed, f"{len(blocks)} blocks")
        rng = np.random.default_rng(seed + 3)
        nn = sorted(op.dims)[1]
        lo, hi = op.off[nn] * op.ns, (op.off[nn] + int(np.prod(op.dims[nn]))) * op.ns
        for tr in (False, True):
            r = np.zeros(op.n)
            r[lo:hi] = rng.uniform(-1.0, 1.0, hi - lo)
            z = engine.pcApply(r, 1, transpose=tr)
            assert np.abs(z[lo:hi]).max() > 0.0 and not z[:lo].any() and not z[hi:].any(), ("the cycle couples blocks", nn, tr)
        engine.pcRelease()


def check_gmres(engine, dims, seed=281, restart=50, cycles=4):
    """GMRES on the RANS preconditioner matrix with a 2-level hierarchy, both transposes: the iteration count equals that of scipy's
    gmres with the numpy cycle as right preconditioner, the true residual recomputed in numpy is below the tolerance.  The counts at 1, 2
    and 3 levels are printed; no order between them is asserted"""
    rtol = 1e-8
    blk, op = pc.single_block(engine, dims, pc.RANS, jm.WALL, 107, stretch_k=2.0)
    rng = np.random.default_rng(seed)
    rhs = {tr: rng.uniform(-1.0, 1.0, op.n) for tr in (False, True)}
    counts = {}
    for levels in (1, 2, 3):
        with mg_of(engine, levels):
            engine.pcSetup(1)
            for tr in (False, True):
                b = rhs[tr]
                nb = float(np.linalg.norm(b))
                x, its, r0, rn = engine.gmresSolve(b, 1, transpose=tr, restart=restart, maxIts=restart * cycles, rtol=rtol)
                true = float(np.linalg.norm(b - op.apply(x, tr)))
                counts[(levels, tr)] = its
                print(f"gmres {dims} levels={levels} transpose={tr}: {its} iterations, ||b - A x|| / ||b|| = {true / nb:.3e}")
                if levels != 2:
                    continue
                f64 = NumpyMG(op, np.float64, 2)
                k_ref = pc.scipy_gmres_iterations(lambda v: op.apply(v, tr), f64, b, tr, rtol, restart, cycles)
                print(f"    scipy with the numpy cycle: {k_ref}")
                assert its == k_ref, (its, k_ref)
                assert abs(r0 - nb) <= 1e-12 * nb
                assert true <= 2 * rtol * nb, (true, nb)
            engine.pcRelease()
    print(f"gmres {dims}: iterations by (levels, transpose) = {counts}")
    return counts


def check_ank(engine, dims=(7, 6, 5), seed=311):
    """ankPcSetup with 2 levels, flow kind in slot 0 and turbulence in slot 1: T on every level, the application against the yardstick
    on dRdwPre + T"""
    blk, op = pc.single_block(engine, dims, pc.RANS, jm.WALL, seed, frozenTurb=True, stretch_k=2.0)
    engine.timeStep(1)
    engine.ankTimeStep(ank.CFL, ank.TURB_CFL_SCALE, False)
    try:
        for slot, turb in ((0, False), (1, True)):
            if turb:
                engine.ankTimeStep(ank.CFL, ank.TURB_CFL_SCALE, turb=True)
                op = ankt.turb_operator(engine, blk, True)
            Tn = {1: engine.ankTimeStepBlocks(1, turb=turb)}
            ops = ank.shifted(op, Tn)
            st = np.asarray(op.st)
            with mg_of(engine, 2, slot=slot):
                engine.ankPcSetup(1)
                assert_hierarchy(engine, ops, 2, 1, 0, 0, seed + 10 * slot, f"ANK turb={turb} {dims}", T=Tn)
                # the coarse diagonal carries the children's T: it equals the sums with T and not the sums without
                s0 = int(np.where((st == 0).all(axis=1))[0][0])
                lib2 = engine.pcMgMatrix(2, 1)
                with_T = coarsen(in_block(ops.J[1], st), st)
                mags = coarsen(in_block(ops.J[1], st), st, absolute=True)
                without = coarsen(in_block(op.J[1], st), st)
                assert (np.abs(lib2 - with_T) <= (TERMS + 2) * EPS * mags).all()
                assert (np.abs(lib2[..., s0] - without[..., s0]) > (TERMS + 2) * EPS * mags[..., s0]).any(), "T is missing on level 2"
                engine.pcRelease()
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcRelease()
        engine.ankRelease()


def check_ank_solve(engine, dims, prm, spec, cap, seed=347, **mk):
    """ank_checks.check_solve with a 2-level hierarchy: ankSolve converges, its count equals that of scipy's gmres on A = J + T (the
    operator ank_checks forms from the downloaded blocks) with the numpy cycle as right preconditioner"""
    rtol = 1e-4
    blk, Rref, op, Tn, w0 = ank.setup_operator(engine, dims, prm, spec, False, True, seed, **mk)
    ops = ank.shifted(op, Tn)
    try:
        with mg_of(engine, 2):
            engine.ankPcSetup(1)
            b = engine.ankGetR()
            nb = float(np.linalg.norm(b))
            x, its, r0, rn = engine.ankSolve(b, 1, restart=cap, maxIts=cap, rtol=rtol)
            k_ref = pc.scipy_gmres_iterations(lambda v: ops.apply(v), NumpyMG(ops, np.float64, 2), b, False, rtol, cap, cap)
            true = float(np.linalg.norm(b - ops.apply(x)))
            print(f"ankSolve {dims} with 2 levels: {its} iterations (scipy {k_ref}, cap {cap}), ||b - A x|| / ||b|| = {true / nb:.3e}")
            assert 0 < its <= cap and its == k_ref, (its, k_ref, cap)
            assert abs(r0 - nb) <= 1e-12 * nb
            assert true <= 2 * rtol * nb, (true, nb)
    finally:
        engine.pcRelease()
        engine.ankRelease()


def check_slots_and_identity(engine, dims=(7, 6, 5), seed=227):
    blk, op = pc.single_block(engine, dims, pc.RANS, jm.WALL, seed, stretch_k=2.0)
    rng = np.random.default_rng(seed + 1)
    r = rng.uniform(-1.0, 1.0, op.n)
    R = rng.uniform(-1.0, 1.0, (3, op.n))
    try:
        engine.pcSelect(0)
        engine.pcSetup(1)
        assert engine.pcMgInfo() == (1, 1, 0, (op.ncell,))
        z0 = {tr: engine.pcApply(r, 1, transpose=tr) for tr in (False, True)}
        nb0 = engine.pcInfo()[2]
        # pcSetMg(1, ...) followed by a setup is a setup without the call
        engine.pcSetMg(1, 3, 2)
        engine.pcSetup(1)
        assert engine.pcMgInfo() == (1, 1, 0, (op.ncell,)) and engine.pcInfo()[2] == nb0
        for tr in (False, True):
            assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z0[tr]), ("pcSetMg(1, ...) then a setup", tr)
        # a hierarchy in slot 1 leaves the fill-0 factor of slot 0 as it is
        with mg_of(engine, 3, 2, 1, fill=1, slot=1):
            engine.pcSetup(1)
            assert engine.pcMgInfo()[:3] == (3, 2, 1)
            nb1 = engine.pcInfo()[2]
            # everything the cycle needs is counted: the matrices of the three levels, their factors, four vectors per level
            cells = engine.pcMgInfo()[3]
            floor = sum(c * (7 * op.ns ** 2 + 4 * op.ns) * 8 for c in cells) + (13 * cells[0] + 13 * sum(cells[1:])) * op.ns ** 2 * 8
            assert nb1 >= floor, (nb1, floor)
            z1 = engine.pcApply(r, 1)
            assert not np.array_equal(z1, z0[False])
            Z = engine.pcApplyMulti(R, 1)
            for c in range(3):
                assert np.array_equal(Z[c], engine.pcApply(R[c], 1)), ("pcApplyMulti on a hierarchy", c)
            ZT = engine.pcApplyMulti(R, 1, transpose=True)
            for c in range(3):
                assert np.array_equal(ZT[c], engine.pcApply(R[c], 1, transpose=True)), ("pcApplyMulti on a hierarchy, transposed", c)
            assert engine.pcInfo()[2] == nb1                                   # no work space was added for the columns
            engine.pcSelect(0)
            for tr in (False, True):
                assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z0[tr]), ("slot 0 beside a hierarchy in slot 1", tr)
            assert engine.pcInfo()[2] == nb0
            # the hierarchy owns its fine copy: another assembly (frozen turbulence, nState 5) overwrites the assembled blocks, and
            # release_workspace frees none of it
            engine.pcSelect(1)
            engine.setupStateResidualMatrix(1, True, frozenTurb=True, delta=1e-6)
            assert engine.jacobianInfo()[0] == 5
            engine.releaseWorkspace()
            assert np.array_equal(engine.pcApply(r, 1), z1), "after another assembly and release_workspace"
            assert engine.pcRelease() == nb1 and engine.pcRelease() == 0
            with __import__("pytest").raises(capi.AdflowGpuError, match="no factor"):
                engine.pcMgInfo()
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcSetFill(0)
            engine.pcSetMg(1, 1, 0)
            engine.pcRelease()


def check_enqueue_only(engine, dv, dims=(7, 6, 5), seed=293):
    """three chained pcApplyDev calls on a hierarchy (the output of one is the input of the next) under set_async(1) with one
    synchronise at the end: bit-equal to the same chain with a synchronise after every call, the last result within the bar"""
    blk, op = pc.single_block(engine, dims, pc.RANS, jm.WALL, seed, stretch_k=2.0)
    rng = np.random.default_rng(seed + 1)
    r = rng.uniform(-1.0, 1.0, op.n)
    try:
        with mg_of(engine, 3, 2, 1):
            engine.pcSetup(1)
            f64, fld = yardsticks(op, 3, 2, 0, 1)

            def chain(enqueue):
                v = [dv.put(r), dv.empty(op.n), dv.empty(op.n), dv.empty(op.n)]
                dv.sync()
                engine.set_async(enqueue)
                try:
                    for c in range(3):
                        engine.pcApplyDev(dv.ptr(v[c]), dv.ptr(v[c + 1]), op.n, 1, transpose=bool(c % 2))
                        if not enqueue:
                            engine.sync()
                finally:
                    engine.sync()
                    engine.set_async(False)
                return [dv.get(x) for x in v]
            stepped, queued = chain(False), chain(True)
            for c in range(4):
                assert np.array_equal(stepped[c], queued[c]), ("the enqueued chain differs", c)
            assert np.array_equal(queued[0], r)
            # the last link against the yardstick applied to the library's own input of that link
            zl = fld.apply(queued[2], False)
            e_np = float(np.abs(f64.apply(queued[2], False).astype(np.longdouble) - zl).max())
            e_lib = float(np.abs(queued[3].astype(np.longdouble) - zl).max())
            print(f"enqueue-only chain {dims}: last link max|z - z_ld| = {e_lib:.3e}, float64 numpy {e_np:.3e}, ratio {e_lib / max(e_np, 1e-300):.3f}")
            assert e_lib <= pc.MARGIN * e_np and np.abs(zl).max() > 0.0
    finally:
        engine.pcRelease()
        engine.releaseWorkspace()


def check_refusals(engine, dims=(7, 6, 5), seed=229):
    """every refusal of the interface, each leaving the previous factor or hierarchy usable and adflow_gpu_last_error naming the cause"""
    import pytest
    engine.release_all()
    engine.pcSelect(0)
    blk, op = pc.single_block(engine, dims, pc.RANS, jm.WALL, seed, stretch_k=2.0)
    rng = np.random.default_rng(seed + 1)
    r = rng.uniform(-1.0, 1.0, op.n)
    try:
        with pytest.raises(capi.AdflowGpuError, match="no factor"):
            engine.pcMgInfo()
        with mg_of(engine, 2, 2, 1):
            engine.pcSetup(1)
            z = engine.pcApply(r, 1)
            for args, msg in (((0, 1, 0), "1 .no multigrid. to 10 levels"), ((11, 1, 0), "to 10 levels"), ((2, 0, 0), "nSmooth = 0"),
                              ((2, 1, -1), "fillCoarse = -1"), ((2, 1, 3), "fillCoarse = 3")):
                with pytest.raises(capi.AdflowGpuError, match=msg):
                    engine.pcSetMg(*args)
            # a refused setting changes nothing: the hierarchy stands, the next setup builds the same one
            assert engine.pcMgInfo()[:3] == (2, 2, 1) and np.array_equal(engine.pcApply(r, 1), z)
            for args, msg in (((0, 1), "multigrid level 0"), ((3, 1), "multigrid level 3"), ((1, 7), "block 7 is not part")):
                out = np.zeros(1)
                assert engine.lib.adflow_gpu_pc_mg_download(args[0], args[1], out.ctypes.data) != 0
                assert msg in engine.lib.adflow_gpu_last_error().decode(), engine.lib.adflow_gpu_last_error().decode()
            assert engine.lib.adflow_gpu_pc_mg_download(1, 1, None) != 0 and "NULL" in engine.lib.adflow_gpu_last_error().decode()
            engine.pcSetup(1)
            assert engine.pcMgInfo()[:3] == (2, 2, 1) and np.array_equal(engine.pcApply(r, 1), z)
            # 7 x 6 x 5 -> 4 x 3 x 3 -> 2 x 2 x 2 -> 1 x 1 x 1: a fifth level would have the one cell of the fourth
            engine.pcSetMg(4, 1, 0)
            engine.pcSetup(1)
            assert engine.pcMgInfo()[3] == (210, 36, 8, 1)
            z4 = engine.pcApply(r, 1)
            engine.pcSetMg(5, 1, 0)
            with pytest.raises(capi.AdflowGpuError, match=r"multigrid level 5 would have the 1 cells of level 4"):
                engine.pcSetup(1)
            with pytest.raises(capi.AdflowGpuError, match="no factor"):            # as at every failed setup, nothing is kept
                engine.pcApply(r, 1)
            engine.pcSetMg(4, 1, 0)
            engine.pcSetup(1)
            assert np.array_equal(engine.pcApply(r, 1), z4)
            # the entries of a plain factor: info answers, the download refuses
            engine.pcSelect(1)
            engine.pcSetup(1)
            assert engine.pcMgInfo() == (1, 1, 0, (op.ncell,))
            out = np.zeros(1)
            assert engine.lib.adflow_gpu_pc_mg_download(1, 1, out.ctypes.data) != 0
            assert "no hierarchy" in engine.lib.adflow_gpu_last_error().decode()
            engine.pcRelease()
            engine.pcSelect(0)
            # wrong sizes and vectors are refused as for a factor, the hierarchy still applies
            out = np.zeros_like(r)
            for args, msg in (((2, 0, r.ctypes.data, out.ctypes.data, r.size), "not the level of the factor"),
                              ((1, 0, r.ctypes.data, r.ctypes.data, r.size), "same vector"),
                              ((1, 1, r.ctypes.data, out.ctypes.data, r.size - 6), "rows")):
                for fn in (engine.lib.adflow_gpu_pc_apply, engine.lib.adflow_gpu_pc_apply_dev):
                    assert fn(*args) != 0 and msg in engine.lib.adflow_gpu_last_error().decode(), msg
            assert np.array_equal(engine.pcApply(r, 1), z4)
            # a state that is not finite: the message names the multigrid level, block and cell; nothing is kept
            engine.download_state(1, 1)
            w = blk["w"].copy(order="F")
            blk["w"][4, 3, 3, 0] = np.nan
            engine.upload_state(1, 1)
            engine.setupStateResidualMatrix(1, True, delta=1e-6)
            engine.pcSetMg(2, 1, 0)
            with pytest.raises(capi.AdflowGpuError, match=r"pivot block of cell \(\d+,\d+,\d+\) of block 1 on multigrid level [12]"):
                engine.pcSetup(1)
            with pytest.raises(capi.AdflowGpuError, match="no factor"):
                engine.pcMgInfo()
            assert engine.pcRelease() == 0
            blk["w"][...] = w
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcSetFill(0)
            engine.pcSetMg(1, 1, 0)
        engine.release_all()
