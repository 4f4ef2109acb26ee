"""Checks of the ILU(0) over the whole level (adflow_gpu_pc_set_coupled(1): one subdomain per process, the couplings across the block
interfaces inside M) shared by tests/test_gpu_pc_coupled.py (real MI355X) and tests/test_hostsim_pc_coupled.py (the kernel-logic
emulator).

The yardstick is pc_checks.NumpyILU0._factor -- the general pattern-restricted IKJ ILU, which knows nothing of the diagonal-only
shortcut -- on ONE row list for the whole level: the rows of engine.jacobianBlocks through jacmult_checks.LevelOperator.colmap (an
owned cell is its own column, a halo cell the owned cell it has as donor in the 2-layer pattern), the six entries with one non-zero
offset and the diagonal, the columns >= 0, natural ordering = block after block in ascending nn, then k, j, i.  Float64 and
longdouble; the bar is pc_checks': the library at most MARGIN x as far from the longdouble run as the float64 run is, the identity
<M^-1 r, s> = <r, M^-T s> within pc_checks.assert_identity."""
import contextlib

import numpy as np
import pytest

import ank_checks as ank
import async_checks as asy
import checks
import jacmult_checks as jm
import pc_checks as pc
from adflow_amd import capi
from adflow_amd.params import FlowParams, dissScalar, upwind
from adflow_amd.topology import BrickTopology, LatticeBlock, LatticeTopology, ell_topology

_KEEP = ank._KEEP           # the reference's flowDoms point into these arrays: alive as long as ref may be called


def ell_half():
    """the four blocks of adflow_amd.topology.ell_topology at half size, with its transforms: 12x8x4, 8x6x4, 8x3x12, 3x8x6 --
    1008 cells, 400 entries across interfaces, 45 level sets, no cell with a duplicate column, no two neighbours that are neighbours"""
    T = [b.T for b in ell_topology().blocks]
    dims = ((12, 8, 4), (8, 6, 4), (8, 3, 12), (3, 8, 6))
    origins = ((0, 0, 0), (12, 7, 0), (0, 0, 4), (12, 0, 4))
    return LatticeTopology([LatticeBlock(d, t, o) for d, t, o in zip(dims, T, origins)])


def level_rows(op, dtype):
    """(rows of the 7-point matrix of the whole level as NumpyILU0._factor takes them, number of entries whose column lies behind a
    block face); asserts that no row has the same column twice"""
    seven = [s for s in range(op.st.shape[0]) if np.count_nonzero(op.st[s]) <= 1 and np.abs(op.st[s]).sum() <= 1]
    assert len(seven) == 7
    rows, ncross = [], 0
    for nn in sorted(op.dims):
        nx, ny, nz = op.dims[nn]
        Jb, cm = op.J[nn], op.colmap[nn]
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    row = {}
                    for s in seven:
                        ci, cj, ck = i - op.st[s, 0], j - op.st[s, 1], k - op.st[s, 2]
                        c = int(cm[ci + 2, cj + 2, ck + 2])
                        if c < 0:
                            continue
                        assert c not in row, ("a row with the same column twice", nn, (i, j, k))
                        row[c] = np.array(Jb[i, j, k, :, :, s], dtype=dtype)
                        ncross += not (0 <= ci < nx and 0 <= cj < ny and 0 <= ck < nz)
                    assert len(rows) in row
                    rows.append(row)
    return rows, ncross


def level_sets(rows):
    """the number of dependency level sets: longest path over the lower neighbours of the whole level"""
    lvl = np.zeros(len(rows), np.int64)
    for c, row in enumerate(rows):
        low = [lvl[n] for n in row if n < c]
        lvl[c] = 1 + max(low) if low else 0
    return int(lvl.max()) + 1


class NumpyLevelILU0(pc.NumpyILU0):
    """pc_checks.NumpyILU0 with one subdomain for the level: the same _factor and apply on one row list"""

    def __init__(self, op, dtype):
        self.op, self.dtype, self.ns = op, dtype, op.ns
        rows, self.ncross = level_rows(op, dtype)
        self.nsets = level_sets(rows)
        self.sub = {min(op.dims): self._factor(rows)}          # (apply: the rows from the first block's offset on = all of them)


def yardsticks(op):
    return NumpyLevelILU0(op, np.float64), NumpyLevelILU0(op, np.longdouble)


@contextlib.contextmanager
def coupled_slots(engine):
    """whatever happens inside, both slots are block-local, fill 0, without hierarchy and empty afterwards"""
    try:
        yield
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcSetCoupled(0)
            engine.pcSetFill(0)
            engine.pcSetMg(1)
            engine.pcRelease()
        engine.ankRelease()
        engine.releaseWorkspace()


def setup_coupled(engine, op, ilus=None, ank_setup=False):
    """the factor over the level in the selected slot; pcCoupledInfo against the numpy counts; returns the yardsticks"""
    ilus = ilus or yardsticks(op)
    engine.pcSetCoupled(1)
    (engine.ankPcSetup if ank_setup else engine.pcSetup)(1)
    info = engine.pcCoupledInfo()
    print(f"coupled factor: pcCoupledInfo = {info}, numpy: {ilus[0].nsets} level sets, {ilus[0].ncross} entries across interfaces")
    assert info == (1, ilus[0].nsets, ilus[0].ncross), (info, ilus[0].nsets, ilus[0].ncross)
    assert engine.pcInfo()[:2] == (op.ns, ilus[0].nsets) and engine.pcInfo2() == (0, 7, ilus[0].nsets)
    return ilus


def assert_coupled_apply(engine, op, seed, what, ilus):
    first, _ = pc.assert_apply_matches(engine, op, seed, what, ilus=ilus)
    pc.assert_identity(engine, op, first, seed + 1)
    return first


def assert_far_from_block_local(engine, op, first, what):
    """the couplings matter: the block-local factor of the same matrix is more than 100 x the bar away"""
    engine.pcSetCoupled(0)
    engine.pcSetup(1)
    assert engine.pcCoupledInfo()[0::2] == (0, 0)
    for tr in (False, True):
        r, z, e_np = first[tr]
        d = float(np.abs(engine.pcApply(r, 1, transpose=tr) - z).max())
        print(f"{what} transpose={tr}: max|z_coupled - z_block| = {d:.3e}, bar {pc.MARGIN * e_np:.3e}")
        assert d > 100.0 * pc.MARGIN * e_np, (what, tr, d, e_np)


def assert_blocks_coupled(engine, op, seed):
    """a right-hand side supported on one block gives a non-zero z on another: the opposite of pc_checks.check_brick"""
    rng = np.random.default_rng(seed)
    nn = sorted(op.dims)[0]
    lo, hi = op.off[nn] * op.ns, (op.off[nn] + int(np.prod(op.dims[nn]))) * op.ns
    for tr in (False, True):
        r = np.zeros(op.n)
        r[lo:hi] = rng.uniform(-1.0, 1.0, hi - lo)
        z = engine.pcApply(r, 1, transpose=tr)
        assert np.abs(z[lo:hi]).max() > 0.0
        assert np.abs(np.concatenate([z[:lo], z[hi:]])).max() > 0.0, ("M^-1 does not couple the blocks", tr)


# ---- 1, 2: bricks and rotated interfaces without boundaries -------------------------------------------------------------------
def check_interfaces(engine, topo, prm, seed, what, nsets=None, ncross=None, many_lower=None):
    with coupled_slots(engine):
        blocks, op = jm.brick_operator(engine, topo, prm, seed)
        ilus = setup_coupled(engine, op)
        if nsets is not None:
            assert ilus[0].nsets == nsets, (ilus[0].nsets, nsets)
        if ncross is not None:
            assert ilus[0].ncross == ncross, (ilus[0].ncross, ncross)
        if many_lower is not None:
            rows = ilus[0].sub[min(op.dims)][0]
            n = sum(1 for c, row in enumerate(rows) if sum(1 for k in row if k < c) > 3)
            assert n == many_lower, ("cells with more than three lower neighbours", n, many_lower)
        first = assert_coupled_apply(engine, op, seed + 1, what, ilus)
        assert_blocks_coupled(engine, op, seed + 3)
        assert_far_from_block_local(engine, op, first, what)
        return op


def check_periodic_brick(engine, topo, nsets=None, many_lower=None):
    check_interfaces(engine, topo, FlowParams(spaceDiscr=dissScalar), 223, f"periodic brick {topo.nx}x{topo.ny}x{topo.nz}", nsets=nsets,
                     many_lower=many_lower)


def check_rotated(engine):
    check_interfaces(engine, ell_half(), FlowParams(spaceDiscr=upwind), 251, "rotated interfaces", nsets=45, ncross=400)


# ---- 3, 4: the benchmark layout in miniature ----------------------------------------------------------------------------------
WALL_TOPO = dict(Bi=2, Bj=2, Bk=2, nx=6, ny=5, nz=4, periodic=(False,) * 3)


MK_KEYS = ("stretch_k", "shape", "lengths")


def wall_brick(engine, seed=107, topo=None, prm=pc.RANS, spec=jm.WALL, **jac):
    """2 x 2 x 2 wall-bounded blocks, RANS Roe preconditioner matrix by forward mode; returns (blocks, prm, operator).
    topo, prm, spec and the mesh keywords among jac (MK_KEYS, handed to checks.setup_brick_with_bc): another wall-bounded brick"""
    mk = {k: jac.pop(k) for k in MK_KEYS if k in jac}
    if topo is None:
        topo = BrickTopology(**WALL_TOPO)
        mk.setdefault("stretch_k", 2.0)
    blocks, rblocks, bocos, prm = checks.setup_brick_with_bc(engine, topo, prm, spec, seed, **mk)
    _KEEP[:] = [rblocks, bocos]
    engine.applyAllBC(1, True)
    engine.setupStateResidualMatrix(1, True, useAD=True, **jac)
    return blocks, prm, jm.operator_of(engine, blocks, topo.patterns(2)[0])


def check_wall_brick_apply(engine, **jac):
    with coupled_slots(engine):
        blocks, prm, op = wall_brick(engine, **jac)
        ilus = setup_coupled(engine, op)
        assert_coupled_apply(engine, op, 109, f"wall-bounded brick {jac}", ilus)


def check_wall_topo(engine, topo, prm, spec, seed=107, matches=None, **mk):
    """the factor over the level on a wall-bounded brick given by the caller (topology, boundary kinds, mesh keywords): the
    applications under `matches` (default pc_checks.assert_apply_matches), the identity, and far from the block-local factor"""
    with coupled_slots(engine):
        blocks, prm, op = wall_brick(engine, seed, topo, prm, spec, **mk)
        ilus = setup_coupled(engine, op)
        assert ilus[0].ncross > 0
        what = f"{len(blocks)} wall-bounded blocks"
        first, _ = (matches or pc.assert_apply_matches)(engine, op, seed + 2, what, ilus=ilus)
        pc.assert_identity(engine, op, first, seed + 3)
        assert_far_from_block_local(engine, op, first, what)


CAP_WALL = 46            # 2 x the 23 iterations scipy's gmres takes with the numpy factor over the level on this matrix (22 transposed)


def check_wall_brick_gmres(engine, cap=CAP_WALL, restart=80, rtol=1e-8, seed=281):
    """gmresSolve with the factor over the level: the iterations of scipy's gmres with the numpy factor over the level by the rule of
    pc_checks.check_gmres_on_pc_matrix (within a cap fixed beforehand that leaves a factor 2 over scipy's count, asserted here as
    well), the true residual in numpy, and fewer iterations than with the block-local factor of the same matrix (36 in numpy)"""
    with coupled_slots(engine):
        blocks, prm, op = wall_brick(engine)
        assert op.ns == 6
        ilus = setup_coupled(engine, op)
        assert_coupled_apply(engine, op, 109, "wall-bounded brick", ilus)
        rng = np.random.default_rng(seed)
        bs = {tr: rng.uniform(-1.0, 1.0, op.n) for tr in (False, True)}
        its_c = {}
        for tr in (False, True):
            b = bs[tr]
            k_ref = pc.scipy_gmres_iterations(lambda v: op.apply(v, tr), ilus[0], b, tr, rtol, restart, cap)
            x, its, r0, rn = engine.gmresSolve(b, 1, transpose=tr, restart=restart, maxIts=cap, rtol=rtol)
            true, nb = float(np.linalg.norm(b - op.apply(x, tr))), float(np.linalg.norm(b))
            print(f"gmres, factor over the level, transpose={tr}: {its} iterations (scipy with the numpy factor {k_ref}), "
                  f"||b - A x|| / ||b|| = {true / nb:.3e} (reported {rn / nb:.3e})")
            assert 2 * k_ref <= cap, ("the cap leaves no factor 2 over scipy's count", k_ref, cap)
            assert 0 < its <= cap, (its, cap)
            assert abs(r0 - nb) <= 1e-12 * nb
            assert true <= 2 * rtol * nb, (true, nb)
            assert abs(rn - true) <= 1e-3 * rtol * nb + 1e-6 * true
            its_c[tr] = its
        engine.pcSetCoupled(0)
        engine.pcSetup(1)
        for tr in (False, True):
            x, its, r0, rn = engine.gmresSolve(bs[tr], 1, transpose=tr, restart=restart, maxIts=restart, rtol=rtol)
            print(f"gmres, block-local factor, transpose={tr}: {its} iterations (factor over the level: {its_c[tr]})")
            assert its_c[tr] < its, ("the couplings save no iteration", tr, its_c[tr], its)


def check_wall_brick_ank(engine, seed=311):
    """adflow_gpu_ank_pc_setup with coupled = 1: the yardstick with T added to the diagonal blocks, as ank_checks.shifted forms it"""
    with coupled_slots(engine):
        blocks, prm, op = wall_brick(engine)
        engine.pcSetCoupled(1)
        engine.pcSetup(1)
        r = np.random.default_rng(seed).uniform(-1.0, 1.0, op.n)
        plain = engine.pcApply(r, 1)
        Tn = ank.assert_T(engine, blocks, prm, True, "wall-bounded brick")
        ops = ank.shifted(op, Tn)
        ilus = setup_coupled(engine, ops, ank_setup=True)
        assert_coupled_apply(engine, ops, seed + 1, "shifted factor over the level", ilus)
        assert not np.array_equal(engine.pcApply(r, 1), plain), "T does not reach the factor"
        engine.pcSetup(1)
        assert np.array_equal(engine.pcApply(r, 1), plain), "pcSetup after the ANK entries"


# ---- 5: equivalence and isolation -----------------------------------------------------------------------------------------------
def check_equivalence_and_isolation(engine, dims=(12, 8, 6), seed=107):
    with coupled_slots(engine):
        # one block without self-interfaces: the same factor either way, bit for bit
        blk, op = pc.single_block(engine, dims, pc.RANS, jm.WALL, seed, stretch_k=2.0)
        rng = np.random.default_rng(seed + 1)
        r = rng.uniform(-1.0, 1.0, op.n)
        engine.pcSelect(0)
        engine.pcSetup(1)
        z0 = {tr: engine.pcApply(r, 1, transpose=tr) for tr in (False, True)}
        engine.pcSelect(1)
        engine.pcSetCoupled(1)
        engine.pcSetup(1)
        assert engine.pcCoupledInfo() == (1, sum(dims) - 2, 0)
        for tr in (False, True):
            assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z0[tr]), ("one block: coupled = 1 is not coupled = 0", tr)
        # the slots are apart: the block-local factor of slot 0 before and after, with the factor over the level in slot 1
        engine.pcSelect(0)
        assert engine.pcCoupledInfo()[0] == 0
        for tr in (False, True):
            assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z0[tr]), ("slot 0 with a coupled factor in slot 1", tr)
        engine.pcSetup(1)
        for tr in (False, True):
            assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z0[tr]), ("slot 0 set up again", tr)
        engine.pcSelect(1)
        assert engine.pcCoupledInfo()[0] == 1
    with coupled_slots(engine):
        # several columns at once on interfaces: the single applications column by column, and the yardstick
        blocks, op = jm.brick_operator(engine, ell_half(), FlowParams(spaceDiscr=upwind), 251)
        ilus = setup_coupled(engine, op)
        nb0 = engine.pcInfo()[2]
        assert nb0 >= (7 * op.ns ** 2 * 8 + 4) * op.ncell
        R = np.random.default_rng(seed + 2).uniform(-1.0, 1.0, (3, op.n))
        for tr in (False, True):
            Z = engine.pcApplyMulti(R, 1, transpose=tr)
            for c in range(3):
                assert np.array_equal(Z[c], engine.pcApply(R[c], 1, transpose=tr)), ("multi against single", tr, c)
                zl = ilus[1].apply(R[c], tr)
                e_np = float(np.abs(ilus[0].apply(R[c], tr).astype(np.longdouble) - zl).max())
                e_lib = float(np.abs(Z[c].astype(np.longdouble) - zl).max())
                print(f"3 columns, transpose={tr}, column {c}: max|z - z_ld| = {e_lib:.3e}, float64 numpy {e_np:.3e}")
                assert e_lib <= pc.MARGIN * e_np, (tr, c, e_lib, e_np)
        # the bytes pc_info reports are the bytes pc_release returns (the work space of the two further columns included)
        nb = engine.pcInfo()[2]
        assert nb == nb0 + 2 * op.n * 8, (nb, nb0)
        assert engine.pcRelease() == nb and engine.pcRelease() == 0
        with pytest.raises(capi.AdflowGpuError, match="no factor"):
            engine.pcCoupledInfo()


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------
def check_refusals(engine, seed=227):
    with coupled_slots(engine):
        blocks, op = jm.brick_operator(engine, BrickTopology(2, 1, 1, 3, 4, 4), FlowParams(spaceDiscr=dissScalar), seed)
        r = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, op.n)
        engine.pcSelect(0)
        engine.pcSetCoupled(1)
        engine.pcSetup(1)
        z = engine.pcApply(r, 1)

        def still_applies():
            engine.pcSelect(0)
            assert engine.pcCoupledInfo()[0] == 1 and np.array_equal(engine.pcApply(r, 1), z)

        with pytest.raises(capi.AdflowGpuError, match="pc_set_coupled: 2"):
            engine.pcSetCoupled(2)
        still_applies()
        engine.pcSelect(1)
        engine.pcSetCoupled(1)
        engine.pcSetup(1)                                    # a factor the refused setups must not keep
        for setting, reset, msg in ((lambda: engine.pcSetFill(1), lambda: engine.pcSetFill(0), "fill 1"),
                                    (lambda: engine.pcSetMg(2), lambda: engine.pcSetMg(1), "multigrid hierarchy of 2 levels")):
            engine.pcSelect(1)
            setting()
            with pytest.raises(capi.AdflowGpuError, match=msg):
                engine.pcSetup(1)
            with pytest.raises(capi.AdflowGpuError, match="no factor"):
                engine.pcApply(r, 1)
            reset()
            still_applies()
        engine.pcSelect(1)
        engine.pcSetup(1)                                    # the settings are back: the slot takes a factor over the level again
        assert np.array_equal(engine.pcApply(r, 1), z)
    with coupled_slots(engine):
        # one block periodic onto itself over two cells: every cell has the same column behind two faces
        blocks, op = jm.brick_operator(engine, BrickTopology(1, 1, 1, 2, 5, 4), FlowParams(spaceDiscr=dissScalar), seed)
        engine.pcSetup(1)                                    # block-local: fine
        engine.pcSetCoupled(1)
        with pytest.raises(capi.AdflowGpuError, match="same column behind two faces"):
            engine.pcSetup(1)
        with pytest.raises(capi.AdflowGpuError, match="no factor"):
            engine.pcInfo()
        engine.pcSetCoupled(0)
        engine.pcSetup(1)
        assert engine.pcCoupledInfo()[0::2] == (0, 0)


# ---- 7: the enqueue-only mode ---------------------------------------------------------------------------------------------------
def check_enqueue_only_chain(engine, dv, seed=251):
    """pc_apply_dev -> jacobian_mult_dev -> pc_apply_dev on the rotated interfaces with the factor over the level under
    adflow_gpu_set_async(1) with one synchronise: bit-equal to the chain with a synchronise after every call, and within the bar"""
    topo = ell_half()

    def setup(enqueue):
        blocks, op = jm.brick_operator(engine, topo, FlowParams(spaceDiscr=upwind), seed)
        engine.pcSelect(0)
        engine.pcSetCoupled(1)
        engine.pcSetup(1)
        r = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, op.n)
        d = dict(r=dv.put(r), z1=dv.put(np.full(op.n, 7.0)), y=dv.put(np.full(op.n, 7.0)), z2=dv.put(np.full(op.n, 7.0)))
        return dict(op=op, r=r, d=d)

    def chain(c, link):
        d, n, p = c["d"], c["op"].n, dv.ptr
        link(engine.pcApplyDev, p(d["r"]), p(d["z1"]), n, 1, False)
        link(engine.jacobianMultDev, p(d["z1"]), p(d["y"]), n, 1, False)
        link(engine.pcApplyDev, p(d["y"]), p(d["z2"]), n, 1, True)
        return dict(d)

    with coupled_slots(engine):
        c, enq, syn = asy.both_runs(engine, dv, setup, chain)
        assert engine.pcCoupledInfo()[0] == 1
        op = c["op"]
        assert np.array_equal(enq["r"], c["r"]), "the right-hand side was written"
        f64, fld = yardsticks(op)
        for out, rhs, tr in (("z1", enq["r"], False), ("z2", enq["y"], True)):
            zl = fld.apply(rhs, tr)
            e_np = float(np.abs(f64.apply(rhs, tr).astype(np.longdouble) - zl).max())
            e_lib = float(np.abs(enq[out].astype(np.longdouble) - zl).max())
            print(f"enqueue-only chain {out}: max|z - z_ld| = {e_lib:.3e}, float64 numpy {e_np:.3e}")
            assert e_lib <= pc.MARGIN * e_np and np.abs(zl).max() > 0.0, (out, e_lib, e_np)
        ref = op.apply(enq["z1"])
        bound = 2 * op.st.shape[0] * op.ns * pc.EPS * op.apply(enq["z1"], absolute=True)
        assert (np.abs(enq["y"] - ref) <= bound).all() and np.abs(ref).max() > 0.0
        asy.assert_bitwise("coupled chain", enq, syn)
