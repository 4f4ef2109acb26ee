"""Checks of the ILU(k) over the whole level on a general block pattern (adflow_gpu_pc_set_level_fill, adflow_gpu_pc_level_info;
csrc/kernels_pc_level.hip) shared by tests/test_gpu_pc_level.py (real MI355X) and tests/test_hostsim_pc_level.py (the kernel-logic
emulator).

The yardstick needs nothing new: the rows of the 7-point matrix of the level from pc_coupled_checks.level_rows (an owned cell is its
own column, a face halo the owned cell it has as donor), completed to the level-of-fill pattern by pc_fill_checks.NumpyILUk._symbolic
(fill entries are zero blocks), factored by pc_checks.NumpyILU0._factor -- the general IKJ ILU restricted to the pattern -- in float64
and in longdouble; the level sets as pc_coupled_checks.level_sets over the completed rows.  The bar is pc_checks': the library at most
MARGIN x as far from the longdouble run as the float64 run is, the identity <M^-1 r, s> = <r, M^-T s> within
pc_checks.assert_identity; and every case holds adflow_gpu_pc_level_info against the numpy counts of the same rows."""
import contextlib

import numpy as np
import pytest

import ank_checks as ank
import async_checks as asy
import jacmult_checks as jm
import pc_checks as pc
import pc_coupled_checks as pcc
import pc_fill_checks as pf
from adflow_amd import capi
from adflow_amd.params import FlowParams, dissScalar, upwind
from adflow_amd.topology import BrickTopology

EULER_JST = FlowParams(spaceDiscr=dissScalar)


class NumpyLevelILUk(pc.NumpyILU0):
    """pc_checks.NumpyILU0 on one row list for the level, completed to the pattern of ILU(fill)"""

    def __init__(self, op, dtype, fill):
        self.op, self.dtype, self.ns, self.fill = op, dtype, op.ns, fill
        rows, self.ncross = pcc.level_rows(op, dtype)
        lev = pf.NumpyILUk._symbolic([set(r) for r in rows], fill)
        zero = np.zeros((self.ns, self.ns), dtype=dtype)
        for row, pattern in zip(rows, lev):
            for c in pattern:
                if c not in row:
                    row[c] = zero.copy()
        self.max_row = max(len(r) for r in rows)
        self.nentries = sum(len(r) for r in rows)
        self.nsets = pcc.level_sets(rows)
        lvl = np.zeros(len(rows), np.int64)
        for c, row in enumerate(rows):
            low = [lvl[n] for n in row if n < c]
            lvl[c] = 1 + max(low) if low else 0
        self.largest_set = int(np.bincount(lvl).max())
        self.off_diagonal_targets = any(m != c and m in rows[c] for c, row in enumerate(rows) for n in row if n < c
                                        for m in rows[n] if m > n)
        self.sub = {min(op.dims): self._factor(rows)}          # (apply: the rows from the first block's offset on = all of them)

    def counts(self):
        """what adflow_gpu_pc_level_info reports without `reused`"""
        return self.fill, self.max_row, self.nentries, self.nsets, self.ncross


def yardsticks(op, fill):
    return NumpyLevelILUk(op, np.float64, fill), NumpyLevelILUk(op, np.longdouble, fill)


@contextlib.contextmanager
def level_slots(engine):
    """whatever happens inside, both slots are back at level fill -1, block-local, fill 0, without hierarchy and empty afterwards"""
    try:
        yield
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcSetLevelFill(-1)
            engine.pcSetCoupled(0)
            engine.pcSetFill(0)
            engine.pcSetMg(1)
            engine.pcRelease()
        engine.ankRelease()
        engine.releaseWorkspace()


def setup_level(engine, op, fill, ilus=None, ank_setup=False, reused=0):
    """the ILU(fill) over the level in the selected slot; every info entry against the numpy counts; returns the yardsticks"""
    ilus = ilus or yardsticks(op, fill)
    engine.pcSetLevelFill(fill)
    (engine.ankPcSetup if ank_setup else engine.pcSetup)(1)
    info, y = engine.pcLevelInfo(), ilus[0]
    print(f"level fill {fill}: pcLevelInfo = {info}, numpy: longest row {y.max_row}, {y.nentries} entries, {y.nsets} level sets (largest "
          f"{y.largest_set} rows), {y.ncross} entries across interfaces")
    assert info == y.counts() + (reused,), (info, y.counts(), reused)
    assert engine.pcInfo()[:2] == (op.ns, y.nsets) and engine.pcInfo2() == (fill, y.max_row, y.nsets)
    assert engine.pcCoupledInfo() == (1, y.nsets, y.ncross)
    return ilus


def assert_level_apply(engine, op, seed, what, ilus, matches=None):
    first, _ = (matches or pc.assert_apply_matches)(engine, op, seed, what, ilus=ilus)
    pc.assert_identity(engine, op, first, seed + 1)
    return first


# ---- 1, 2, 7: bricks and rotated interfaces without boundaries --------------------------------------------------------------------
def check_interfaces(engine, topo, prm, fills, seed, what, two_workgroups=None, matches=None):
    """one assembly, one factor per fill; two_workgroups: the fill at which a level set must be longer than one wave"""
    with level_slots(engine):
        blocks, op = jm.brick_operator(engine, topo, prm, seed)
        for fill in fills:
            ilus = setup_level(engine, op, fill)
            if fill == two_workgroups:
                assert ilus[0].largest_set > 64, ilus[0].largest_set
            assert_level_apply(engine, op, seed + 1 + fill, f"{what}, level fill {fill}", ilus, matches and matches.get(fill))
            pcc.assert_blocks_coupled(engine, op, seed + 3)
            engine.pcRelease()
        return op


def check_periodic_brick(engine, topo, fills, two_workgroups=None, matches=None):
    check_interfaces(engine, topo, EULER_JST, fills, 223, f"periodic brick {topo.nx}x{topo.ny}x{topo.nz}", two_workgroups, matches)


def check_rotated(engine, fills=(1, 2)):
    check_interfaces(engine, pcc.ell_half(), FlowParams(spaceDiscr=upwind), fills, 251, "rotated interfaces")


def check_period_of_three(engine, seed=227):
    """one block periodic onto itself over three cells: two neighbours of a cell are neighbours of each other, so elimination touches
    off-diagonal entries at fill 0 -- coupled = 1 refuses it, the general elimination takes it"""
    topo = BrickTopology(1, 1, 1, 3, 4, 4)
    with level_slots(engine):
        blocks, op = jm.brick_operator(engine, topo, EULER_JST, seed)
        engine.pcSetCoupled(1)
        with pytest.raises(capi.AdflowGpuError, match="neighbours of each other"):
            engine.pcSetup(1)
        engine.pcSetCoupled(0)
        for fill in (0, 1):
            ilus = setup_level(engine, op, fill)
            if fill == 0:
                assert ilus[0].off_diagonal_targets, "the yardstick eliminates on the diagonal only: the case misses its mechanism"
            assert_level_apply(engine, op, seed + 1 + fill, f"period of three cells, level fill {fill}", ilus)


# ---- 3, 4, 5: the benchmark layout in miniature -------------------------------------------------------------------------------------
def check_wall_brick_apply(engine, fill, **jac):
    with level_slots(engine):
        blocks, prm, op = pcc.wall_brick(engine, **jac)
        ilus = setup_level(engine, op, fill)
        assert_level_apply(engine, op, 109, f"wall-bounded brick {jac}, level fill {fill}", ilus)


def check_wall_brick_gmres(engine, fill=2, restart=80, rtol=1e-8, seed=281):
    """nState 6 at fill 2: the applications, then gmresSolve with maxIts = 2 x the iterations scipy's gmres takes with the numpy factor
    (at most 40, cap 80): 0 < its <= 2 k_ref, the true residual in numpy, the reported one as pc_coupled_checks.check_wall_brick_gmres.
    Then the coupled fill-0 factor and the block-local fill-2 factor of the same matrix: where scipy with the numpy factors takes fewer
    iterations with the new factor than with each of the two, so must the library"""
    with level_slots(engine):
        blocks, prm, op = pcc.wall_brick(engine)
        assert op.ns == 6
        ilus = setup_level(engine, op, fill)
        assert_level_apply(engine, op, 109, f"wall-bounded brick, level fill {fill}", ilus)
        rng = np.random.default_rng(seed)
        bs = {tr: rng.uniform(-1.0, 1.0, op.n) for tr in (False, True)}
        others = {"coupled fill 0": pcc.NumpyLevelILU0(op, np.float64), f"block-local fill {fill}": pf.NumpyILUk(op, np.float64, fill)}
        k_ref, k_other, its_l = {}, {}, {}
        for tr in (False, True):
            b = bs[tr]
            k_ref[tr] = pc.scipy_gmres_iterations(lambda v: op.apply(v, tr), ilus[0], b, tr, rtol, restart, 80)
            assert k_ref[tr] <= 40, k_ref
            cap = 2 * k_ref[tr]
            x, its, r0, rn = engine.gmresSolve(b, 1, transpose=tr, restart=restart, maxIts=cap, rtol=rtol)
            true, nb = float(np.linalg.norm(b - op.apply(x, tr))), float(np.linalg.norm(b))
            print(f"gmres, ILU({fill}) over the level, transpose={tr}: {its} iterations (scipy with the numpy factor {k_ref[tr]}), "
                  f"||b - A x|| / ||b|| = {true / nb:.3e} (reported {rn / nb:.3e})")
            assert 0 < its <= cap, (its, cap)
            assert abs(r0 - nb) <= 1e-12 * nb
            assert true <= 2 * rtol * nb, (true, nb)
            assert abs(rn - true) <= 1e-3 * rtol * nb + 1e-6 * true
            its_l[tr] = its
            for name, ilu in others.items():
                k_other[(name, tr)] = pc.scipy_gmres_iterations(lambda v: op.apply(v, tr), ilu, b, tr, rtol, restart, restart)
        print(f"scipy's gmres with the numpy factors: ILU({fill}) over the level {k_ref}, others {k_other}")
        engine.pcSetLevelFill(-1)
        for name, setting in (("coupled fill 0", lambda: engine.pcSetCoupled(1)), (f"block-local fill {fill}", lambda: engine.pcSetFill(fill))):
            engine.pcSetCoupled(0)
            engine.pcSetFill(0)
            setting()
            engine.pcSetup(1)
            for tr in (False, True):
                x, its, r0, rn = engine.gmresSolve(bs[tr], 1, transpose=tr, restart=restart, maxIts=restart, rtol=rtol)
                print(f"gmres, {name}, transpose={tr}: {its} iterations (ILU({fill}) over the level: {its_l[tr]}; scipy {k_other[(name, tr)]} "
                      f"against {k_ref[tr]})")
                if k_ref[tr] < k_other[(name, tr)]:           # the yardstick decides whether the comparison is asserted
                    assert its_l[tr] < its, ("the yardstick gains iterations over this factor, the library does not", name, tr, its_l[tr], its)


def check_wall_brick_ank(engine, fill=1, seed=311):
    """adflow_gpu_ank_pc_setup at level fill 1: the yardstick with T added to the diagonal blocks, as ank_checks.shifted forms it; a
    plain setup afterwards gives the plain result again; both setups keep the tables of the first one"""
    with level_slots(engine):
        blocks, prm, op = pcc.wall_brick(engine)
        ilus = setup_level(engine, op, fill)
        r = np.random.default_rng(seed).uniform(-1.0, 1.0, op.n)
        plain = engine.pcApply(r, 1)
        Tn = ank.assert_T(engine, blocks, prm, True, "wall-bounded brick")
        ops = ank.shifted(op, Tn)
        ilus_t = setup_level(engine, ops, fill, ank_setup=True, reused=1)
        assert_level_apply(engine, ops, seed + 1, f"shifted ILU({fill}) over the level", ilus_t)
        assert not np.array_equal(engine.pcApply(r, 1), plain), "T does not reach the factor"
        setup_level(engine, op, fill, ilus=ilus, reused=1)
        assert np.array_equal(engine.pcApply(r, 1), plain), "pcSetup after the ANK entries"


# ---- 6: one block without self-interfaces ---------------------------------------------------------------------------------------------
def check_single_block(engine, dims=(12, 8, 6), seed=107):
    """the counts are the block-local ones and the applications meet the bar against pc_fill_checks.NumpyILUk of the same fill"""
    nx, ny, nz = dims
    nsets = {0: nx + ny + nz - 2, 1: nx + 2 * ny + 3 * nz - 5, 2: nx + 3 * ny + 7 * nz - 10}
    with level_slots(engine):
        blk, op = pc.single_block(engine, dims, pc.RANS, jm.WALL, seed, stretch_k=2.0)
        for fill in (0, 1, 2):
            engine.pcSetLevelFill(fill)
            engine.pcSetup(1)
            info = engine.pcLevelInfo()
            print(f"one block {dims}, level fill {fill}: pcLevelInfo = {info}")
            assert info[:2] == (fill, pf.ENTRIES[fill]) and info[3:] == (nsets[fill], 0, 0), (info, nsets[fill])
            local = (pc.NumpyILU0(op, np.float64), pc.NumpyILU0(op, np.longdouble)) if fill == 0 else pf.yardsticks(op, fill)
            assert info[2] == sum(len(row) for row in local[0].sub[1][0])
            assert_level_apply(engine, op, seed + 1 + fill, f"one block {dims}, level fill {fill}", local)


def check_single_block_fill3(engine, dims=(7, 6, 5), seed=107):
    """fill 3, which adflow_gpu_pc_set_fill refuses, against the yardstick over the level"""
    with level_slots(engine):
        blk, op = pc.single_block(engine, dims, pc.RANS, jm.WALL, seed, stretch_k=2.0)
        with pytest.raises(capi.AdflowGpuError, match=r"0, 1 or 2"):
            engine.pcSetFill(3)
        ilus = setup_level(engine, op, 3)
        assert_level_apply(engine, op, seed + 1, f"one block {dims}, level fill 3", ilus)


# ---- 8: refusals and isolation ----------------------------------------------------------------------------------------------------------
def check_refusals(engine, seed=227):
    with level_slots(engine):
        blocks, op = jm.brick_operator(engine, BrickTopology(2, 1, 1, 3, 4, 4), EULER_JST, seed)
        r = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, op.n)
        engine.pcSelect(0)
        with pytest.raises(capi.AdflowGpuError, match="no factor"):
            engine.pcLevelInfo()
        engine.pcSetLevelFill(0)
        engine.pcSetup(1)
        z = engine.pcApply(r, 1)

        def still_applies():
            engine.pcSelect(0)
            assert engine.pcLevelInfo()[0] == 0 and np.array_equal(engine.pcApply(r, 1), z)

        for bad in (4, -2):
            with pytest.raises(capi.AdflowGpuError, match=f"pc_set_level_fill: {bad}"):
                engine.pcSetLevelFill(bad)
            still_applies()
        engine.pcSelect(1)
        engine.pcSetLevelFill(0)
        engine.pcSetup(1)                                    # a factor the refused setups must not keep
        for setting, reset, msg in ((lambda: engine.pcSetCoupled(1), lambda: engine.pcSetCoupled(0), "coupled = 1"),
                                    (lambda: engine.pcSetFill(1), lambda: engine.pcSetFill(0), "fill 1"),
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
        # a block-local factor is no factor over the level
        engine.pcSetLevelFill(-1)
        engine.pcSetup(1)
        with pytest.raises(capi.AdflowGpuError, match="no ILU over the level"):
            engine.pcLevelInfo()
    with level_slots(engine):
        # one block periodic onto itself over two cells: every cell has the same column behind two faces
        blocks, op = jm.brick_operator(engine, BrickTopology(1, 1, 1, 2, 5, 4), EULER_JST, seed)
        engine.pcSetup(1)                                    # block-local: fine
        engine.pcSetLevelFill(0)
        with pytest.raises(capi.AdflowGpuError, match="same column behind two faces"):
            engine.pcSetup(1)
        with pytest.raises(capi.AdflowGpuError, match="no factor"):
            engine.pcInfo()


def check_isolation(engine, seed=223):
    """a block-local factor in slot 0 applies bit for bit before, while and after a factor over the level lives in slot 1, and again
    after slot 0 is set up anew"""
    with level_slots(engine):
        blocks, op = jm.brick_operator(engine, BrickTopology(2, 2, 1, 6, 5, 4), EULER_JST, seed)
        r = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, op.n)
        engine.pcSelect(0)
        engine.pcSetup(1)
        z0 = {tr: engine.pcApply(r, 1, transpose=tr) for tr in (False, True)}

        def slot0(when):
            engine.pcSelect(0)
            assert engine.pcCoupledInfo()[0] == 0
            for tr in (False, True):
                assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z0[tr]), (when, tr)

        engine.pcSelect(1)
        engine.pcSetLevelFill(1)
        engine.pcSetup(1)
        z1 = engine.pcApply(r, 1)
        assert engine.pcLevelInfo()[0] == 1 and not np.array_equal(z1, z0[False])
        slot0("with a factor over the level in slot 1")
        engine.pcSetup(1)
        slot0("slot 0 set up again")
        engine.pcSelect(1)
        assert np.array_equal(engine.pcApply(r, 1), z1)
        engine.pcRelease()
        slot0("after the release of slot 1")


# ---- 9: several columns and bytes -------------------------------------------------------------------------------------------------------
def check_multi_and_bytes(engine, fill=1, seed=251):
    with level_slots(engine):
        blocks, op = jm.brick_operator(engine, pcc.ell_half(), FlowParams(spaceDiscr=upwind), seed)
        ilus = setup_level(engine, op, fill)
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
        nb = engine.pcInfo()[2]
        assert nb >= 8 * op.ns ** 2 * ilus[0].nentries, (nb, ilus[0].nentries)
        assert engine.pcRelease() == nb and engine.pcRelease() == 0
        with pytest.raises(capi.AdflowGpuError, match="no factor"):
            engine.pcLevelInfo()


# ---- 10: the tables are built once --------------------------------------------------------------------------------------------------------
def check_table_reuse(engine, seed=223):
    topo = BrickTopology(2, 2, 1, 6, 5, 4)
    with level_slots(engine):
        blocks, op = jm.brick_operator(engine, topo, EULER_JST, seed)
        r = np.random.default_rng(seed + 5).uniform(-1.0, 1.0, op.n)
        setup_level(engine, op, 1)
        z = engine.pcApply(r, 1)
        # other numbers on the same blocks: a denser state everywhere, halos included
        for nn, b in blocks.items():
            engine.download_state(nn, 1)
            b["w"][..., 0] *= 1.25
            engine.upload_state(nn, 1)
        engine.setupStateResidualMatrix(1, True, delta=1e-6)
        op2 = jm.operator_of(engine, blocks, topo.patterns(2)[0])
        assert not np.array_equal(op2.J[min(op2.dims)], op.J[min(op.dims)])
        ilus2 = setup_level(engine, op2, 1, reused=1)
        assert_level_apply(engine, op2, seed + 6, "the new matrix in the tables of the old one", ilus2)
        assert not np.array_equal(engine.pcApply(r, 1), z)
        setup_level(engine, op2, 2, reused=0)              # another fill: other tables
        setup_level(engine, op2, 2, reused=1)


# ---- 11: the enqueue-only mode -------------------------------------------------------------------------------------------------------------
def check_enqueue_only_chain(engine, dv, fill=1, seed=251):
    """a setup, two pc_apply_dev and one gmres_solve_dev on the rotated interfaces under adflow_gpu_set_async(1) with one synchronise:
    bit-equal to the chain with a synchronise after every call, and the applications within the bar"""
    topo = pcc.ell_half()

    def setup(enqueue):
        blocks, op = jm.brick_operator(engine, topo, FlowParams(spaceDiscr=upwind), seed)
        engine.pcSelect(0)
        engine.pcSetLevelFill(fill)
        r = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, op.n)
        d = dict(r=dv.put(r), z1=dv.put(np.full(op.n, 7.0)), z2=dv.put(np.full(op.n, 7.0)), x=dv.put(np.full(op.n, 7.0)))
        return dict(op=op, r=r, d=d)

    def chain(c, link):
        d, n, p = c["d"], c["op"].n, dv.ptr
        link(engine.pcSetup, 1)
        link(engine.pcApplyDev, p(d["r"]), p(d["z1"]), n, 1, False)
        link(engine.pcApplyDev, p(d["z1"]), p(d["z2"]), n, 1, True)
        link(engine.gmresSolveDev, p(d["z2"]), p(d["x"]), n, 1, restart=30, maxIts=30, rtol=1e-8)
        return dict(d)

    with level_slots(engine):
        c, enq, syn = asy.both_runs(engine, dv, setup, chain)
        assert engine.pcLevelInfo()[0] == fill
        op = c["op"]
        assert np.array_equal(enq["r"], c["r"]), "the right-hand side was written"
        f64, fld = yardsticks(op, fill)
        for out, rhs, tr in (("z1", enq["r"], False), ("z2", enq["z1"], True)):
            zl = fld.apply(rhs, tr)
            e_np = float(np.abs(f64.apply(rhs, tr).astype(np.longdouble) - zl).max())
            e_lib = float(np.abs(enq[out].astype(np.longdouble) - zl).max())
            print(f"enqueue-only chain {out}: max|z - z_ld| = {e_lib:.3e}, float64 numpy {e_np:.3e}")
            assert e_lib <= pc.MARGIN * e_np and np.abs(zl).max() > 0.0, (out, e_lib, e_np)
        true = float(np.linalg.norm(enq["z2"] - op.apply(enq["x"])))
        assert true <= 2e-8 * float(np.linalg.norm(enq["z2"])), true
        asy.assert_bitwise("chain with the ILU over the level", enq, syn)
