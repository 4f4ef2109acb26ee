"""Checks of the block ILU(1) / ILU(2) preconditioner (adflow_gpu_pc_set_fill, adflow_gpu_pc_info2) shared by
tests/test_gpu_pc_fill.py (real MI355X) and tests/test_hostsim_pc_fill.py (the kernel-logic emulator).

The yardstick extends the one of tests/pc_checks.py: a GENERAL symbolic ILU(k) on the block-sparse matrix of the in-block columns in
the natural ordering -- level(i, j) = min over the pivots k of level(i, k) + level(k, j) + 1, entries kept while <= fill -- and then
pc_checks' general IKJ factorisation restricted to that pattern, in float64 and in np.longdouble.  Nothing here knows the offset
stencil of the library or its level sets: the pattern (13 / 23 distinct offsets) and the longest-path level sets the yardstick finds
are compared with what adflow_gpu_pc_info2 reports.  The bar is pc_checks': the library's M^-1 r and M^-T r may be at most MARGIN =
10 x as far from the longdouble result as the float64 numpy run is, in the max-norm, and <M^-1 r, s> = <r, M^-T s>."""
import contextlib

import numpy as np

import ank_checks as ank
import ank_turb_checks as ankt
import jacmult_checks as jm
import pc_checks as pc
from adflow_amd import capi
from adflow_amd.params import FlowParams, dissScalar

ENTRIES = {0: 7, 1: 13, 2: 23}
EULER_JST = FlowParams(spaceDiscr=dissScalar)


@contextlib.contextmanager
def fill_of(engine, fill, slot=0):
    """the fill of the setups inside; both slots are back at fill 0 and slot 0 is selected afterwards, whatever happened"""
    engine.pcSelect(slot)
    engine.pcSetFill(fill)
    try:
        yield
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcSetFill(0)


class NumpyILUk(pc.NumpyILU0):
    """block Jacobi over the blocks of the level, each subdomain: symbolic ILU(fill), then IKJ restricted to that pattern"""

    def __init__(self, op, dtype, fill):
        self.op, self.dtype, self.ns, self.fill = op, dtype, op.ns, fill
        self.sub, self.offsets, self.sets = {}, set(), {}
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
            lev = self._symbolic([set(r) for r in rows], fill)
            zero = np.zeros((self.ns, self.ns), dtype=dtype)
            for i, row in enumerate(rows):
                for c in lev[i]:
                    if c not in row:
                        row[c] = zero.copy()
                    ci, cj, ck = c % nx, c // nx % ny, c // (nx * ny)
                    ii, ij, ik = i % nx, i // nx % ny, i // (nx * ny)
                    self.offsets.add((ci - ii, cj - ij, ck - ik))
            # the level sets of the row dependencies: longest path over the lower entries
            sets = np.zeros(len(rows), np.int64)
            for i in range(len(rows)):
                low = [sets[c] for c in lev[i] if c < i]
                sets[i] = 1 + max(low) if low else 0
            self.sets[nn] = sets
            self.sub[nn] = self._factor(rows)

    @staticmethod
    def _symbolic(pattern, fill):
        """{column: level} of every row of the ILU(fill) factor of a matrix with the rows `pattern` (sets of columns)"""
        lev = []
        for i, cols in enumerate(pattern):
            row = {c: 0 for c in cols}
            done = -1
            while True:
                nxt = [c for c in row if done < c < i]
                if not nxt:
                    break
                k = min(nxt)
                done = k
                for j, lkj in lev[k].items():
                    if j > k:
                        new = row[k] + lkj + 1
                        if new <= fill and new < row.get(j, fill + 1):
                            row[j] = new
            lev.append(row)
        return lev

    def n_sets(self):
        return max(int(s.max()) + 1 for s in self.sets.values())

    def largest_set(self):
        """cells of the largest level set of the level (the sets of all blocks share the launches)"""
        n = self.n_sets()
        return int(sum(np.bincount(s, minlength=n) for s in self.sets.values()).max())


def yardsticks(op, fill):
    return NumpyILUk(op, np.float64, fill), NumpyILUk(op, np.longdouble, fill)


def assert_factor(engine, op, fill, seed, what, ilus=None, expect=None, matches=None):
    """the factor that stands in the selected slot against the yardstick: info, pattern facts, both applications, the identity.
    matches: the comparison of the applications (default pc_checks.assert_apply_matches, one draw; pc_checks.assert_apply_median: 16)"""
    f64, fld = ilus or yardsticks(op, fill)
    info = engine.pcInfo2()
    ns, npl, nb = engine.pcInfo()
    print(f"{what} fill {fill}: pcInfo2 = {info}, yardstick: {len(f64.offsets)} offsets, {f64.n_sets()} level sets, largest "
          f"{f64.largest_set()} cells; {nb} bytes")
    assert info == (fill, ENTRIES[fill], f64.n_sets()), (info, len(f64.offsets), f64.n_sets())
    if expect is not None:
        assert info == expect, (info, expect)
    assert len(f64.offsets) <= ENTRIES[fill]            # a thin block cuts offsets everywhere; none may lie outside the stencil
    assert ns == op.ns and npl == info[2] and nb >= ENTRIES[fill] * ns * ns * 8 * op.ncell, (ns, npl, nb)
    first, _ = (matches or pc.assert_apply_matches)(engine, op, seed + 1, f"{what} fill {fill}", ilus=(f64, fld))
    pc.assert_identity(engine, op, first, seed + 2)
    return first, (f64, fld)


def check_single(engine, dims, prm, spec, seed=107, expect=None, all_offsets=False, matches=None, **jac):
    """one block, fill 1 and 2 on the same assembly; expect = {fill: pcInfo2()}; matches: see assert_factor"""
    blk, op = pc.single_block(engine, dims, prm, spec, seed, **jac)
    out = {}
    for fill in (1, 2):
        with fill_of(engine, fill):
            engine.pcSetup(1)
            out[fill] = assert_factor(engine, op, fill, seed, f"{dims} nState={op.ns}", expect=expect and expect[fill], matches=matches)
            if all_offsets:
                assert len(out[fill][1][0].offsets) == ENTRIES[fill]
            engine.pcRelease()
    return blk, op, out


def check_largest_sets(engine, dims, largest, seed=131):
    """nState = 1 on a block whose level sets span more than one workgroup and a partial wave"""
    blk, op = pc.single_block(engine, dims, pc.RANS, jm.WALL, seed, useTurbOnly=True, stretch_k=2.0)
    assert op.ns == 1
    for fill in (1, 2):
        with fill_of(engine, fill):
            engine.pcSetup(1)
            _, (f64, _) = assert_factor(engine, op, fill, seed, f"{dims} nState=1")
            assert f64.largest_set() == largest[fill], (fill, f64.largest_set())
            engine.pcRelease()


def check_brick(engine, topo, prm, seed=251):
    """blocks of different sizes: level sets of different lengths share one launch, and the couplings across blocks are absent from M"""
    blocks, op = jm.brick_operator(engine, topo, prm, seed)
    for fill in (1, 2):
        with fill_of(engine, fill):
            engine.pcSetup(1)
            assert_factor(engine, op, fill, seed, f"{len(blocks)} blocks")
            rng = np.random.default_rng(seed + 3)
            for nn in sorted(op.dims)[:2]:
                lo, hi = op.off[nn] * op.ns, (op.off[nn] + int(np.prod(op.dims[nn]))) * op.ns
                for tr in (False, True):
                    r = np.zeros(op.n)
                    r[lo:hi] = rng.uniform(-1.0, 1.0, hi - lo)
                    z = engine.pcApply(r, 1, transpose=tr)
                    assert np.abs(z[lo:hi]).max() > 0.0
                    assert not z[:lo].any() and not z[hi:].any(), ("M^-1 couples blocks", nn, tr, fill)
            engine.pcRelease()


def check_dev_twin(engine, dv, topo, seed=257):
    """adflow_gpu_pc_apply_dev on device vectors (dv: device_vectors.HostVectors / TorchVectors) against adflow_gpu_pc_apply at fill 2 on the
    blocks of `topo`, both transposes, bit for bit"""
    from adflow_amd.params import upwind
    blocks, op = jm.brick_operator(engine, topo, FlowParams(spaceDiscr=upwind), seed)
    with fill_of(engine, 2):
        engine.pcSetup(1)
        assert engine.pcInfo2()[:2] == (2, ENTRIES[2])
        pc.assert_apply_dev_twin(engine, dv, op.n, seed + 1, f"{len(blocks)} blocks, fill 2")
        engine.pcRelease()
    engine.releaseWorkspace()


def check_ank(engine, dims=(7, 6, 5), seed=311):
    """ankPcSetup at fill 2 against the yardstick on dRdwPre + T, T as adflow_gpu_ank_download_time_step hands it out; then the
    turbulence factor at fill 2 in slot 1 while slot 0 keeps a fill-0 factor"""
    blk, op = pc.single_block(engine, dims, pc.RANS, jm.WALL, seed, frozenTurb=True, stretch_k=2.0)
    rng = np.random.default_rng(seed)
    x5 = rng.uniform(-1.0, 1.0, op.n)
    engine.timeStep(1)
    engine.ankTimeStep(ank.CFL, ank.TURB_CFL_SCALE, False)
    ops = ank.shifted(op, {1: engine.ankTimeStepBlocks(1, False)})
    try:
        with fill_of(engine, 2):
            engine.ankPcSetup(1)
            assert_factor(engine, ops, 2, seed, f"ANK flow factor {dims}")
            plain = engine.pcApply(x5, 1)
            engine.pcSetup(1)                                               # the same fill without T: another factor
            assert engine.pcInfo2()[0] == 2 and not np.array_equal(engine.pcApply(x5, 1), plain), "T does not reach the factor"
        engine.pcSelect(0)
        engine.ankPcSetup(1)                                                # fill 0 in slot 0
        assert engine.pcInfo2() == (0, 7, sum(dims) - 2)
        z0 = {tr: engine.pcApply(x5, 1, transpose=tr) for tr in (False, True)}
        engine.ankTimeStep(ank.CFL, ank.TURB_CFL_SCALE, turb=True)
        opt = ankt.turb_operator(engine, blk, True)
        opts = ank.shifted(opt, {1: engine.ankTimeStepBlocks(1, turb=True)})
        with fill_of(engine, 2, slot=1):
            engine.ankPcSetup(1)
            assert_factor(engine, opts, 2, seed + 7, f"ANK turbulence factor {dims}, slot 1")
            engine.pcSelect(0)
            assert engine.pcInfo2() == (0, 7, sum(dims) - 2)
            for tr in (False, True):
                assert np.array_equal(engine.pcApply(x5, 1, transpose=tr), z0[tr]), ("slot 0 after the fill-2 setup of slot 1", tr)
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcRelease()
        engine.ankRelease()


def check_gmres(engine, dims, cap, seed=281, scipy_fill_order=False):
    """the comparison of pc_checks.check_gmres_on_pc_matrix at fill 1 and 2: scipy's gmres with the numpy ILU(k) as right
    preconditioner sets the count the cap leaves a factor 2 over; the true residual is recomputed in numpy.  scipy_fill_order: before
    anything is asserted of the library, scipy's own count at fill 2 must not exceed its count at fill 0 on this input"""
    rtol = 1e-8
    blk, op = pc.single_block(engine, dims, pc.RANS, jm.WALL, 107, stretch_k=2.0)
    ilu = {0: pc.NumpyILU0(op, np.float64), 1: NumpyILUk(op, np.float64, 1), 2: NumpyILUk(op, np.float64, 2)}
    rng = np.random.default_rng(seed)
    rhs = {tr: rng.uniform(-1.0, 1.0, op.n) for tr in (False, True)}
    k_ref = {(f, tr): pc.scipy_gmres_iterations(lambda v: op.apply(v, tr), ilu[f], rhs[tr], tr, rtol, cap, cap)
             for f in (0, 1, 2) for tr in (False, True)}
    print(f"scipy's gmres with the numpy ILU(k), {dims}: iterations {k_ref}")
    if scipy_fill_order:
        for tr in (False, True):
            assert k_ref[(2, tr)] <= k_ref[(0, tr)], ("the yardstick itself gains nothing from fill 2 on this input", k_ref)
    its_of = {}
    for fill in (1, 2):
        with fill_of(engine, fill):
            engine.pcSetup(1)
            assert engine.pcInfo2()[:2] == (fill, ENTRIES[fill])
            for tr in (False, True):
                b = rhs[tr]
                x, its, r0, rn = engine.gmresSolve(b, 1, transpose=tr, restart=cap, maxIts=cap, rtol=rtol)
                true = float(np.linalg.norm(b - op.apply(x, tr)))
                nb = float(np.linalg.norm(b))
                print(f"gmres on the PC matrix {dims} fill {fill} transpose={tr}: {its} iterations (scipy {k_ref[(fill, tr)]}, cap {cap}), "
                      f"||b - A x|| / ||b|| = {true / nb:.3e} (reported {rn / nb:.3e})")
                assert 2 * k_ref[(fill, tr)] <= cap, ("the cap leaves no factor 2 over scipy's count", k_ref, cap)
                assert 0 < its <= cap, (its, cap)
                assert abs(r0 - nb) <= 1e-12 * nb
                assert true <= 2 * rtol * nb, (true, nb)
                assert abs(rn - true) <= 1e-3 * rtol * nb + 1e-6 * true
                x2, its2, _, _ = engine.gmresSolve(b, 1, transpose=tr, restart=cap, maxIts=cap, rtol=2 * rtol, x0=x)
                assert its2 == 0 and np.array_equal(x2, x), its2
                its_of[(fill, tr)] = its
            engine.pcRelease()
    return k_ref, its_of


def check_refusals_and_fill0_identity(engine, dims=(7, 6, 5), seed=227):
    import pytest
    engine.release_all()
    engine.pcSelect(0)
    for bad in (-1, 3):
        with pytest.raises(capi.AdflowGpuError, match=r"0, 1 or 2"):
            engine.pcSetFill(bad)
    with pytest.raises(capi.AdflowGpuError, match="no factor"):
        engine.pcInfo2()
    blk, op = pc.single_block(engine, dims, pc.RANS, jm.WALL, seed, stretch_k=2.0)
    rng = np.random.default_rng(seed + 1)
    r = rng.uniform(-1.0, 1.0, op.n)
    try:
        engine.pcSetup(1)                                                   # the default: fill 0
        assert engine.pcInfo2() == (0, 7, sum(dims) - 2) and engine.pcInfo()[1] == sum(dims) - 2
        z0 = {tr: engine.pcApply(r, 1, transpose=tr) for tr in (False, True)}
        x0 = engine.gmresSolve(r, 1, restart=30, maxIts=30, rtol=1e-6)
        # set_fill does not disturb the factor that stands, a refused value changes nothing
        engine.pcSetFill(2)
        with pytest.raises(capi.AdflowGpuError, match=r"0, 1 or 2"):
            engine.pcSetFill(3)
        assert engine.pcInfo2() == (0, 7, sum(dims) - 2)
        for tr in (False, True):
            assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z0[tr]), ("after set_fill", tr)
        engine.pcSetFill(0)
        # a fill-2 factor built and released in the other slot: the fill-0 factor, a new fill-0 setup and the solve are bit-identical
        engine.pcSelect(1)
        with pytest.raises(capi.AdflowGpuError, match="no factor"):
            engine.pcInfo2()
        engine.pcSetFill(2)
        engine.pcSetup(1)
        assert engine.pcInfo2()[:2] == (2, 23)
        z2 = engine.pcApply(r, 1)
        assert not np.array_equal(z2, z0[False])
        nb2 = engine.pcInfo()[2]
        assert nb2 >= 23 * op.ns ** 2 * 8 * op.ncell and engine.pcRelease() == nb2
        engine.pcSelect(0)
        for tr in (False, True):
            assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z0[tr]), ("after a fill-2 factor in slot 1", tr)
        engine.pcSetup(1)
        assert engine.pcInfo2() == (0, 7, sum(dims) - 2)
        for tr in (False, True):
            assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z0[tr]), ("a new fill-0 setup", tr)
        x1 = engine.gmresSolve(r, 1, restart=30, maxIts=30, rtol=1e-6)
        assert x1[1] == x0[1] and np.array_equal(x1[0], x0[0]) and x1[2:] == x0[2:]
        # slot 1 kept its fill: its next setup is a fill-2 factor again, slot 0's is not
        engine.pcSelect(1)
        engine.pcSetup(1)
        assert engine.pcInfo2()[:2] == (2, 23) and np.array_equal(engine.pcApply(r, 1), z2)
        # a state that is not finite: the message names the cell and the fill, nothing is kept
        engine.download_state(1, 1)
        w = blk["w"].copy(order="F")
        blk["w"][4, 3, 3, 0] = np.nan
        engine.upload_state(1, 1)
        engine.setupStateResidualMatrix(1, True, delta=1e-6)
        with pytest.raises(capi.AdflowGpuError, match=r"pivot block of cell \(\d+,\d+,\d+\) of block 1 .*ILU\(2\)"):
            engine.pcSetup(1)
        with pytest.raises(capi.AdflowGpuError, match="no factor"):
            engine.pcInfo2()
        blk["w"][...] = w
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcSetFill(0)
        engine.release_all()
