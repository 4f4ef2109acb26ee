"""Checks of the preconditioner Richardson iterations (adflow_gpu_pc_set_its, adflow_gpu_pc_its_info; csrc/kernels_pc_rich.hip) shared
by tests/test_gpu_pc_its.py (real MI355X) and tests/test_hostsim_pc_its.py (the kernel-logic emulator).

Nothing in the yardstick comes from the code under test.  The matrix is the reference-checked operator the sibling files use
(jacmult_checks.brick_operator, pc_checks.single_block, pc_coupled_checks.wall_brick, ank_checks.shifted for T).  A_full is a numpy
product over pc_coupled_checks.level_rows -- an owned cell is its own column, a first-layer face halo the owned cell it has as donor, a
halo without donor no column --, A_sub the same rows without the entries whose column lies behind a block face.  M is one of the numpy
factors that exist (pc_checks.NumpyILU0, pc_fill_checks.NumpyILUk, pc_coupled_checks.NumpyLevelILU0, pc_level_checks.NumpyLevelILUk,
pc_mg_checks.NumpyMG with the inner iterations added here), factored ONCE per case and wrapped in the recurrences of the header

    S(b; M, A, n):  x = M^-1 b, then n - 1 times x += M^-1 (b - A x)
    local(b) = S(b; M, A_sub, inner);   P(b): y = local(b), then outer - 1 times y += local(b - A_full y)

in float64 and in np.longdouble with the same code.  The bars are pc_checks', unchanged: the library at most MARGIN x as far from the
longdouble run as the float64 numpy run is, both transposes (assert_apply_matches), and <P r, s> = <r, P^T s> on plain factors
(assert_identity)."""
import contextlib

import numpy as np
import pytest

import ank_checks as ank
import async_checks as asy
import jacmult_checks as jm
import multi_checks as mc
import pc_checks as pc
import pc_coupled_checks as pcc
import pc_fill_checks as pf
import pc_level_checks as plc
import pc_mg_checks as pmg
from adflow_amd import capi
from adflow_amd.params import FlowParams, dissScalar, upwind
from adflow_amd.topology import BrickTopology

EULER_JST = FlowParams(spaceDiscr=dissScalar)
BRICK = dict(Bi=2, Bj=1, Bk=1, nx=4, ny=4, nz=4)          # case 2: two periodic blocks, every cell of a block face has a column behind it
F64, LD = np.float64, np.longdouble


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------
class LevelMatrix:
    """A_full x, A_full^T x and the same for A_sub (sub=True) as numpy products over pc_coupled_checks.level_rows"""

    def __init__(self, op, dtype):
        self.dtype, self.ns, self.n = dtype, op.ns, op.n
        rows, self.ncross = pcc.level_rows(op, dtype)
        # the (row, column) pairs whose column lies behind a block face: the loop of level_rows once more, keeping the pairs it counts
        seven = [s for s in range(op.st.shape[0]) if np.count_nonzero(op.st[s]) <= 1 and np.abs(op.st[s]).sum() <= 1]
        cross, r = set(), 0
        for nn in sorted(op.dims):
            nx, ny, nz = op.dims[nn]
            cm = op.colmap[nn]
            for k in range(nz):
                for j in range(ny):
                    for i in range(nx):
                        for s in seven:
                            ci, cj, ck = i - op.st[s, 0], j - op.st[s, 1], k - op.st[s, 2]
                            c = int(cm[ci + 2, cj + 2, ck + 2])
                            if c >= 0 and not (0 <= ci < nx and 0 <= cj < ny and 0 <= ck < nz):
                                cross.add((r, c))
                        r += 1
        assert len(cross) == self.ncross, (len(cross), self.ncross)
        R, C, B, X = [], [], [], []
        for r, row in enumerate(rows):
            for c, blk in row.items():
                R.append(r)
                C.append(c)
                B.append(blk)
                X.append((r, c) in cross)
        self.R, self.C, self.B, self.X = np.array(R), np.array(C), np.stack(B).astype(dtype), np.array(X)

    def apply(self, x, transpose=False, sub=False):
        X = np.asarray(x, dtype=self.dtype).reshape(-1, self.ns)
        keep = ~self.X if sub else np.ones(self.X.size, bool)
        R, C, B = self.R[keep], self.C[keep], self.B[keep]
        Y = np.zeros_like(X)
        if transpose:
            np.add.at(Y, C, np.einsum("nab,na->nb", B, X[R]))
        else:
            np.add.at(Y, R, np.einsum("nab,nb->na", B, X[C]))
        return Y.reshape(-1)


class Rich:
    """P of the header around the numpy factor (or cycle) M; sub: M was built from A_sub; outer_sub: the outer product leaves the
    columns behind block faces out as well (only the guards use it: what a library that forgot them would compute)"""

    def __init__(self, M, A, outer, inner, sub, outer_sub=False):
        self.M, self.A, self.outer, self.inner, self.sub, self.outer_sub, self.dtype = M, A, outer, inner, sub, outer_sub, A.dtype

    def local(self, b, tr):
        x = self.M.apply(b, tr)
        for _ in range(self.inner - 1):
            x = x + self.M.apply(b - self.A.apply(x, tr, sub=self.sub), tr)
        return x

    def apply(self, r, transpose=False):
        b = np.asarray(r, dtype=self.dtype)
        y = self.local(b, transpose)
        for _ in range(self.outer - 1):
            y = y + self.local(b - self.A.apply(y, transpose, sub=self.outer_sub), transpose)
        return y

    def pivot_conditions(self):
        return self.M.pivot_conditions()


class NumpyMGIts(pmg.NumpyMG):
    """pc_mg_checks.NumpyMG whose one ILU application per smoothing iteration on level l is L_l(r) = S(r; M_l, A_l, inner_l), inner_1 =
    inner and inner_l = inner_coarse below level 1; the counts may be changed between applications (the factors do not depend on them)"""
    inner, inner_coarse = 1, 1

    def local(self, l, c, transpose):
        y = self.ilu[l].apply(c, transpose)
        for _ in range((self.inner if l == 0 else self.inner_coarse) - 1):
            y = y + self.ilu[l].apply(c - self.product(l, y, transpose), transpose)
        return y

    def smooth(self, l, b, transpose):
        x = self.local(l, b, transpose)
        for _ in range(self.nsmooth - 1):
            x = x + self.local(l, b - self.product(l, x, transpose), transpose)
        return x


def matrices(op):
    return LevelMatrix(op, F64), LevelMatrix(op, LD)


def pair(ilus, mats, outer, inner, sub, **kw):
    """the float64 and the longdouble yardstick of one setting from the pair of factors and the pair of matrices of the case"""
    return tuple(Rich(M, A, outer, inner, sub, **kw) for M, A in zip(ilus, mats))


def factors(op, kind, fill=0):
    if kind == "local":
        return (pc.NumpyILU0(op, F64), pc.NumpyILU0(op, LD)) if fill == 0 else pf.yardsticks(op, fill)
    if kind == "coupled":
        return pcc.yardsticks(op)
    assert kind == "level"
    return plc.yardsticks(op, fill)


@contextlib.contextmanager
def its_slots(engine):
    """whatever happens inside, both slots are back at (1, 1, 1), level fill -1, block-local, fill 0, without hierarchy and empty"""
    try:
        yield
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcSetIts(1, 1, 1)
            engine.pcSetLevelFill(-1)
            engine.pcSetCoupled(0)
            engine.pcSetFill(0)
            engine.pcSetMg(1)
            engine.pcRelease()
        engine.ankRelease()
        engine.releaseWorkspace()


def setting(engine, kind, fill=0):
    engine.pcSetLevelFill(fill if kind == "level" else -1)
    engine.pcSetCoupled(1 if kind == "coupled" else 0)
    engine.pcSetFill(fill if kind == "local" else 0)


def matrix_bytes(op):
    """the copy (7 blocks of nState^2 doubles per cell), the column table (6 int32 per cell) and the word of every row (one uint32)"""
    return (7 * op.ns ** 2 * 8 + 6 * 4 + 4) * op.ncell


def assert_its_info(engine, op, outer, inner, plain_bytes, hierarchy=False, inner_coarse=1):
    """pcItsInfo and the growth of pcInfo's bytes over the factor without iterations: the copy and its tables when outer > 1 or
    inner > 1 on a plain factor, two work vectors for the outer loop, two for the inner loop of a plain factor"""
    copy = outer > 1 or (inner > 1 and not hierarchy)
    info = engine.pcItsInfo()
    assert info == (outer, inner, inner_coarse, matrix_bytes(op) if copy else 0), (info, matrix_bytes(op))
    if not hierarchy:
        nwork = (2 if outer > 1 else 0) + (2 if inner > 1 else 0)
        grown = engine.pcInfo()[2] - plain_bytes
        assert grown == info[3] + nwork * op.n * 8, (grown, info, nwork)


def assert_both(engine, op, ys, seed, what, identity=True):
    first, _ = pc.assert_apply_matches(engine, op, seed, what, ilus=ys)
    if identity:
        pc.assert_identity(engine, op, first, seed + 1)
    return first


def assert_yardsticks_apart(first_a, ys_a, ys_b, what):
    """the guard of the cases whose mechanism is a difference between two matrices: the two longdouble yardsticks differ, on the
    right-hand sides of the comparison, by more than 100 x the bar"""
    for tr in (False, True):
        r, _, e_np = first_a[tr]
        d = float(np.abs(ys_a[1].apply(r, tr) - ys_b[1].apply(r, tr)).max())
        print(f"{what} transpose={tr}: the yardsticks differ by {d:.3e}, 100 x bar = {100 * pc.MARGIN * e_np:.3e}")
        assert d > 100.0 * pc.MARGIN * e_np, ("the case misses its mechanism", what, tr, d, e_np)


# ---- 1: one block ------------------------------------------------------------------------------------------------------------------
def check_single(engine, dims=(7, 6, 5), seed=107):
    with its_slots(engine):
        blk, op = pc.single_block(engine, dims, EULER_JST, jm.EULER, seed)
        ilus, mats = factors(op, "local"), matrices(op)
        assert mats[0].ncross == 0
        engine.pcSetup(1)
        plain = engine.pcInfo()[2]
        assert engine.pcItsInfo() == (1, 1, 1, 0)
        for q, (outer, inner) in enumerate(((2, 1), (3, 1), (1, 2), (2, 2))):
            engine.pcSetIts(outer, inner, 1)
            engine.pcSetup(1)
            assert_its_info(engine, op, outer, inner, plain)
            assert_both(engine, op, pair(ilus, mats, outer, inner, True), seed + 10 * q, f"{dims} its=({outer},{inner})")


# ---- 2: two periodic blocks, block-local factors -------------------------------------------------------------------------------------
def check_brick(engine, fill, seed=223):
    with its_slots(engine):
        blocks, op = jm.brick_operator(engine, BrickTopology(**BRICK), EULER_JST, seed)
        ilus, mats = factors(op, "local", fill), matrices(op)
        assert mats[0].ncross > 0
        setting(engine, "local", fill)
        engine.pcSetup(1)
        plain = engine.pcInfo()[2]
        first, ys = {}, {}
        for its in ((2, 1), (1, 2)):
            engine.pcSetIts(*its, 1)
            engine.pcSetup(1)
            assert_its_info(engine, op, *its, plain)
            ys[its] = pair(ilus, mats, *its, True)
            first[its] = assert_both(engine, op, ys[its], seed + 1, f"brick fill {fill} its={its}")      # the same r for both
        assert_yardsticks_apart(first[(2, 1)], ys[(2, 1)], ys[(1, 2)], f"brick fill {fill}: outer 2 against inner 2")
        # a right-hand side on one block: outer = 2 reaches the other block through the columns behind the faces, outer = 1 does not
        rng = np.random.default_rng(seed + 3)
        nn = sorted(op.dims)[0]
        lo, hi = op.off[nn] * op.ns, (op.off[nn] + int(np.prod(op.dims[nn]))) * op.ns
        for outer in (2, 1):
            engine.pcSetIts(outer, 1, 1)
            engine.pcSetup(1)
            for tr in (False, True):
                r = np.zeros(op.n)
                r[lo:hi] = rng.uniform(-1.0, 1.0, hi - lo)
                z = engine.pcApply(r, 1, transpose=tr)
                other = np.concatenate([z[:lo], z[hi:]])
                assert np.abs(z[lo:hi]).max() > 0.0
                if outer == 2:
                    assert np.abs(other).max() > 0.0, ("outer = 2 does not couple the blocks", tr)
                else:
                    assert not other.any(), ("outer = 1 couples the blocks", tr)


# ---- 3, 4: the factors over the level ------------------------------------------------------------------------------------------------
def check_rotated(engine, seed=251):
    """the mirror entry across rotated interfaces is not at the opposite direction: the transposed application in particular"""
    with its_slots(engine):
        blocks, op = jm.brick_operator(engine, pcc.ell_half(), FlowParams(spaceDiscr=upwind), seed)
        mats = matrices(op)
        for kind, fill, its in (("coupled", 0, (3, 1)), ("level", 1, (2, 2))):
            setting(engine, kind, fill)
            engine.pcSetIts(*its, 1)
            engine.pcSetup(1)
            assert engine.pcItsInfo() == its + (1, matrix_bytes(op))
            assert_both(engine, op, pair(factors(op, kind, fill), mats, *its, False), seed + 1 + fill, f"rotated interfaces, {kind} its={its}")
            engine.pcRelease()


def check_period_of_three(engine, seed=227):
    """one block periodic onto itself over three cells: two neighbours of a cell are neighbours of each other"""
    with its_slots(engine):
        blocks, op = jm.brick_operator(engine, BrickTopology(1, 1, 1, 3, 4, 4), EULER_JST, seed)
        setting(engine, "level", 0)
        engine.pcSetIts(2, 1, 1)
        engine.pcSetup(1)
        assert engine.pcItsInfo() == (2, 1, 1, matrix_bytes(op))
        assert_both(engine, op, pair(factors(op, "level", 0), matrices(op), 2, 1, False), seed + 1, "period of three cells, its=(2,1)")


def check_level_table_reuse(engine, fill=0, its=(2, 1), seed=223):
    """a setup that keeps the tables of the ILU over the level (reused = 1) redoes the copy: after ankPcSetup on the same pattern T is in
    the products as well as in the factor, and a plain setup afterwards gives the plain bits again"""
    with its_slots(engine):
        prm = EULER_JST
        blocks, op = jm.brick_operator(engine, BrickTopology(**BRICK), prm, seed)
        setting(engine, "level", fill)
        engine.pcSetIts(*its, 1)
        engine.pcSetup(1)
        assert engine.pcLevelInfo()[5] == 0
        r = np.random.default_rng(seed + 9).uniform(-1.0, 1.0, op.n)
        plain = engine.pcApply(r, 1)
        Tn = ank.assert_T(engine, blocks, prm, False, "brick")
        ops = ank.shifted(op, Tn)
        engine.ankPcSetup(1)
        assert engine.pcLevelInfo()[5] == 1 and engine.pcItsInfo() == its + (1, matrix_bytes(op))
        ilus, mats = factors(ops, "level", fill), matrices(ops)
        ys = pair(ilus, mats, *its, False)
        first = assert_both(engine, ops, ys, seed + 1, f"level fill {fill}, tables kept, its={its}")
        assert_yardsticks_apart(first, ys, pair(ilus, matrices(op), *its, False), "tables kept: T in the copy")
        engine.pcSetup(1)
        assert engine.pcLevelInfo()[5] == 1
        assert np.array_equal(engine.pcApply(r, 1), plain), "pcSetup after ankPcSetup on kept tables"
        # other iterations on the same pattern: the tables are built again, with their copy
        engine.pcSetIts(1, 1, 1)
        engine.pcSetup(1)
        assert engine.pcLevelInfo()[5] == 0 and engine.pcItsInfo() == (1, 1, 1, 0)


# ---- 5: the reference's default adjoint preconditioner on one process ----------------------------------------------------------------
CAP_ITS_WALL = 42        # 2 x the 21 iterations scipy's gmres takes on the exact matrix, transposed, with the numpy ILU(2) over the level in
                         # three outer iterations (23 with one: printed, no order asserted); pc_coupled_checks.CAP_WALL is its sibling


def check_wall_brick(engine, fill=2, outer=3, restart=80, rtol=1e-8, seed=281):
    """level fill 2 with outerPreconIts = 3 on the RANS brick: both applications; then the adjoint's order of calls -- the exact matrix
    overwrites the assembly -- and gmresSolve with transpose = 1: 0 < its <= 2 x scipy's count with the numpy preconditioner on the same
    matrix, within the cap fixed beforehand, the true residual recomputed in numpy"""
    with its_slots(engine):
        blocks, prm, op = pcc.wall_brick(engine)
        assert op.ns == 6
        ilus, mats = factors(op, "level", fill), matrices(op)
        setting(engine, "level", fill)
        engine.pcSetIts(outer, 1, 1)
        engine.pcSetup(1)
        ys = pair(ilus, mats, outer, 1, False)
        assert_both(engine, op, ys, 109, f"wall-bounded brick, level fill {fill}, outer {outer}")
        engine.setupStateResidualMatrix(1, False, useAD=True)
        exact = jm.operator_of(engine, blocks, BrickTopology(**pcc.WALL_TOPO).patterns(2)[0])
        assert exact.st.shape[0] == 33
        b = np.random.default_rng(seed).uniform(-1.0, 1.0, op.n)
        k_ref = pc.scipy_gmres_iterations(lambda v: exact.apply(v, True), ys[0], b, True, rtol, restart, restart)
        k_one = pc.scipy_gmres_iterations(lambda v: exact.apply(v, True), ilus[0], b, True, rtol, restart, restart)
        cap = 2 * k_ref
        x, its, r0, rn = engine.gmresSolve(b, 1, transpose=True, restart=restart, maxIts=cap, rtol=rtol)
        true, nb = float(np.linalg.norm(b - exact.apply(x, True))), float(np.linalg.norm(b))
        print(f"gmres on the exact matrix, transposed, ILU({fill}) over the level: {its} iterations at outer {outer} (scipy with the numpy "
              f"preconditioner: {k_ref} at outer {outer}, {k_one} at outer 1; cap {CAP_ITS_WALL}), ||b - A x|| / ||b|| = {true / nb:.3e} "
              f"(reported {rn / nb:.3e})")
        assert cap <= CAP_ITS_WALL, ("scipy's count moved past the cap fixed beforehand", k_ref, CAP_ITS_WALL)
        assert 0 < its <= cap, (its, cap)
        assert abs(r0 - nb) <= 1e-12 * nb
        assert true <= 2 * rtol * nb, (true, nb)
        assert abs(rn - true) <= 1e-3 * rtol * nb + 1e-6 * true


# ---- 6: T in A and in M -----------------------------------------------------------------------------------------------------------------
def check_wall_brick_ank(engine, its=(2, 2), seed=311):
    with its_slots(engine):
        blocks, prm, op = pcc.wall_brick(engine)
        Tn = ank.assert_T(engine, blocks, prm, True, "wall-bounded brick")
        ops = ank.shifted(op, Tn)
        mats = matrices(ops)
        plain_mats = matrices(op)
        for kind in ("local", "coupled"):
            setting(engine, kind)
            engine.pcSetIts(*its, 1)
            engine.ankPcSetup(1)
            ilus = factors(ops, kind)
            ys = pair(ilus, mats, *its, kind == "local")
            first = assert_both(engine, ops, ys, seed + 1, f"ankPcSetup, {kind} its={its}")
            # T is in the copy as well as in the factor: the yardstick whose products lack it is far away
            assert_yardsticks_apart(first, ys, pair(ilus, plain_mats, *its, kind == "local"), f"ankPcSetup, {kind}: T in A")
            engine.pcRelease()


# ---- 7: the hierarchy ----------------------------------------------------------------------------------------------------------------------
def check_hierarchy(engine, brick, seed=107):
    with its_slots(engine):
        if brick:
            blocks, op = jm.brick_operator(engine, BrickTopology(**BRICK), EULER_JST, seed)
        else:
            blk, op = pc.single_block(engine, (12, 8, 6), pc.RANS, jm.WALL, seed, stretch_k=2.0)
        mgs = tuple(NumpyMGIts(op, t, 2, 2, 0, 0) for t in (F64, LD))
        mats = matrices(op)
        what = "brick" if brick else "(12, 8, 6)"
        with pmg.mg_of(engine, 2, 2, 0):
            engine.pcSetup(1)
            plain = engine.pcInfo()[2]
            cells = engine.pcMgInfo()[3]
            for q, (outer, inner, coarse) in enumerate(((2, 2, 2), (1, 1, 2))):
                engine.pcSetIts(outer, inner, coarse)
                engine.pcSetup(1)
                assert_its_info(engine, op, outer, inner, plain, hierarchy=True, inner_coarse=coarse)
                # two vectors on every level that iterates, the copy and two vectors for the outer loop
                grown = sum(2 * c * op.ns * 8 for c, n in zip(cells, (inner, coarse)) if n > 1) + \
                    (matrix_bytes(op) + 2 * op.n * 8 if outer > 1 else 0)
                assert engine.pcInfo()[2] - plain == grown, (engine.pcInfo()[2] - plain, grown)
                for m in mgs:
                    m.inner, m.inner_coarse = inner, coarse
                ys = pair(mgs, mats, outer, 1, False)
                first = assert_both(engine, op, ys, seed + 1 + q, f"hierarchy on {what} its=({outer},{inner},{coarse})", identity=False)
                if brick and outer > 1:
                    # the outer product sees the columns behind the faces although the hierarchy is block-local
                    assert_yardsticks_apart(first, ys, pair(mgs, mats, outer, 1, False, outer_sub=True), "hierarchy on brick: outer product")
            engine.pcRelease()


# ---- 8: several columns ---------------------------------------------------------------------------------------------------------------------
def check_multi(engine, its=(2, 2), seed=223, cap=60):
    with its_slots(engine):
        blocks, op = jm.brick_operator(engine, BrickTopology(**BRICK), EULER_JST, seed)
        ys = pair(factors(op, "local"), matrices(op), *its, True)
        engine.pcSetIts(*its, 1)
        engine.pcSetup(1)
        nb0 = engine.pcInfo()[2]
        rng = np.random.default_rng(seed + 5)
        R = rng.uniform(-1.0, 1.0, (7, op.n))                       # 4 + 3: two groups
        for tr in (False, True):
            Z = engine.pcApplyMulti(R, 1, transpose=tr)
            for c in range(7):
                zl = ys[1].apply(R[c], tr)
                e_np = float(np.abs(ys[0].apply(R[c], tr).astype(LD) - zl).max())
                e_lib = float(np.abs(Z[c].astype(LD) - zl).max())
                print(f"7 columns its={its} transpose={tr} column {c}: max|z - z_ld| = {e_lib:.3e}, float64 numpy {e_np:.3e}")
                assert e_lib <= pc.MARGIN * e_np and np.abs(zl).max() > 0.0, (tr, c, e_lib, e_np)
            assert np.array_equal(engine.pcApplyMulti(R[:1], 1, transpose=tr)[0], engine.pcApply(R[0], 1, transpose=tr)), ("nvec = 1", tr)
        # the work space of the sweeps and the four work vectors of the iterations, each for three more columns
        assert engine.pcInfo()[2] == nb0 + 3 * op.n * 8 + 4 * 3 * op.n * 8, (engine.pcInfo()[2], nb0)
        # (GMRES(60) does not converge on this matrix -- periodic, no boundary -- with or without iterations: the columns run into the
        # cap like their single solves; the wall-bounded block below converges, its columns stop at their own counts)
        B = rng.uniform(-1.0, 1.0, (3, op.n))
        for tr in (False, True):
            mc.assert_columns_match_single_solves(engine, op, B, tr, cap, f"brick its={its}")
        engine.pcRelease()
        blk, op = pc.single_block(engine, (7, 5, 4), pc.RANS, jm.WALL, 107, stretch_k=2.0)
        engine.pcSetup(1)
        B = rng.uniform(-1.0, 1.0, (3, op.n))
        for tr in (False, True):
            _, k, _ = mc.assert_columns_match_single_solves(engine, op, B, tr, cap, f"(7, 5, 4) its={its}")
            assert (np.asarray(k) < cap).all(), ("no column converged below the cap", k)


# ---- 9: the defaults ----------------------------------------------------------------------------------------------------------------------
def check_defaults(engine, seed=223):
    """pcSetIts(1, 1, 1) is no call at all: the same bits, the same bytes, no copy"""
    with its_slots(engine):
        blocks, op = jm.brick_operator(engine, BrickTopology(**BRICK), EULER_JST, seed)
        r = np.random.default_rng(seed + 7).uniform(-1.0, 1.0, op.n)
        for kind, levels in (("local", 1), ("coupled", 1), ("level", 1), ("local", 2)):
            setting(engine, kind)
            with pmg.mg_of(engine, levels, 2, 0):
                engine.pcSetup(1)
                before = {tr: engine.pcApply(r, 1, transpose=tr) for tr in (False, True)}
                nb = engine.pcInfo()[2]
                engine.pcSetIts(1, 1, 1)
                engine.pcSetup(1)
                for tr in (False, True):
                    assert np.array_equal(engine.pcApply(r, 1, transpose=tr), before[tr]), (kind, levels, tr)
                assert engine.pcInfo()[2] == nb and engine.pcItsInfo() == (1, 1, 1, 0), (kind, levels)
                engine.pcRelease()


# ---- 10: slots and persistence ----------------------------------------------------------------------------------------------------------
def check_slots_and_persistence(engine, dims=(7, 5, 4), seed=107):
    with its_slots(engine):
        blk, op = pc.single_block(engine, dims, pc.RANS, jm.WALL, seed, stretch_k=2.0)
        ilus, mats = factors(op, "local"), matrices(op)
        r = np.random.default_rng(271).uniform(-1.0, 1.0, op.n)
        engine.pcSelect(1)
        engine.pcSetup(1)
        plain = {tr: engine.pcApply(r, 1, transpose=tr) for tr in (False, True)}
        nb1 = engine.pcInfo()[2]
        engine.pcSelect(0)
        engine.pcSetIts(3, 1, 1)
        engine.pcSetup(1)
        assert_its_info(engine, op, 3, 1, nb1)
        assert_both(engine, op, pair(ilus, mats, 3, 1, True), seed + 1, f"slot 0 {dims} its=(3,1)")
        z = {tr: engine.pcApply(r, 1, transpose=tr) for tr in (False, True)}
        engine.pcSelect(1)
        assert engine.pcItsInfo() == (1, 1, 1, 0) and engine.pcInfo()[2] == nb1
        for tr in (False, True):
            assert np.array_equal(engine.pcApply(r, 1, transpose=tr), plain[tr]) and not np.array_equal(z[tr], plain[tr]), tr
        engine.pcSetup(1)                                                      # the setting of slot 0 is not the setting of slot 1
        assert engine.pcItsInfo() == (1, 1, 1, 0)
        # the exact matrix overwrites the assembly: the factor applies from its own copy
        engine.setupStateResidualMatrix(1, False, useAD=True)
        assert engine.jacobianInfo()[1].shape[0] == 33
        engine.releaseWorkspace()
        engine.pcSelect(0)
        for tr in (False, True):
            assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z[tr]), ("after the exact assembly and release_workspace", tr)
        nb0 = engine.pcInfo()[2]
        assert engine.pcRelease() == nb0 and engine.pcRelease() == 0
        with pytest.raises(capi.AdflowGpuError, match="no factor"):
            engine.pcItsInfo()
        # the setting outlives the release; a later setup with (1, 1, 1) holds no copy
        engine.setupStateResidualMatrix(1, True, useAD=True)
        engine.pcSetup(1)
        assert engine.pcItsInfo()[:3] == (3, 1, 1) and engine.pcInfo()[2] == nb0
        for tr in (False, True):
            assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z[tr]), ("after a new setup", tr)
        engine.pcSetIts(1, 1, 1)
        assert engine.pcItsInfo()[:3] == (3, 1, 1), "a factor that exists keeps what it was built with"
        engine.pcSetup(1)
        assert engine.pcItsInfo() == (1, 1, 1, 0) and engine.pcInfo()[2] == nb1
        for tr in (False, True):
            assert np.array_equal(engine.pcApply(r, 1, transpose=tr), plain[tr]), ("set back to (1, 1, 1)", tr)


# ---- 11: the enqueue-only mode --------------------------------------------------------------------------------------------------------------
def check_enqueue_only_chain(engine, dv, its=(2, 2), seed=223):
    """pc_apply_dev -> jacobian_mult_dev -> pc_apply_dev under adflow_gpu_set_async(1) with one synchronise: bit-equal to the chain with
    a synchronise after every call, and within the bar"""
    topo = BrickTopology(**BRICK)

    def setup(enqueue):
        blocks, op = jm.brick_operator(engine, topo, EULER_JST, seed)
        engine.pcSelect(0)
        engine.pcSetIts(*its, 1)
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

    with its_slots(engine):
        c, enq, syn = asy.both_runs(engine, dv, setup, chain)
        assert engine.pcItsInfo()[:2] == its
        op = c["op"]
        assert np.array_equal(enq["r"], c["r"]), "the right-hand side was written"
        f64, fld = pair(factors(op, "local"), matrices(op), *its, True)
        for out, rhs, tr in (("z1", enq["r"], False), ("z2", enq["y"], True)):
            zl = fld.apply(rhs, tr)
            e_np = float(np.abs(f64.apply(rhs, tr).astype(LD) - zl).max())
            e_lib = float(np.abs(enq[out].astype(LD) - zl).max())
            print(f"enqueue-only chain {out}: max|z - z_ld| = {e_lib:.3e}, float64 numpy {e_np:.3e}")
            assert e_lib <= pc.MARGIN * e_np and np.abs(zl).max() > 0.0, (out, e_lib, e_np)
        asy.assert_bitwise("chain with iterations", enq, syn)


# ---- 12: refusals -----------------------------------------------------------------------------------------------------------------------------
def check_refusals(engine, seed=227):
    with its_slots(engine):
        engine.pcSelect(0)
        engine.pcRelease()
        with pytest.raises(capi.AdflowGpuError, match="pc_its_info: no factor"):
            engine.pcItsInfo()
        blocks, op = jm.brick_operator(engine, BrickTopology(1, 1, 1, 2, 5, 4), EULER_JST, seed)
        engine.pcSetIts(1, 2, 3)
        for args, msg in (((0, 1, 1), "outer = 0"), ((1, 0, 1), "inner = 0"), ((1, 1, -2), "innerCoarse = -2"), ((-1, 0, 0), "outer = -1")):
            with pytest.raises(capi.AdflowGpuError, match="pc_set_its: " + msg):
                engine.pcSetIts(*args)
        engine.pcSelect(1)
        engine.pcSetup(1)                                    # a factor in the other slot, which no refusal may touch
        r = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, op.n)
        z1 = engine.pcApply(r, 1)
        engine.pcSelect(0)
        # one block periodic onto itself over two cells: every cell has the same column behind two faces.  The refused settings changed
        # nothing: the slot still asks for inner = 2, which needs the matrix of the level
        with pytest.raises(capi.AdflowGpuError, match="same column behind two faces"):
            engine.pcSetup(1)
        with pytest.raises(capi.AdflowGpuError, match="no factor"):
            engine.pcInfo()
        engine.pcSetIts(2, 1, 1)
        with pytest.raises(capi.AdflowGpuError, match="same column behind two faces"):
            engine.pcSetup(1)
        with pytest.raises(capi.AdflowGpuError, match="no factor"):
            engine.pcApply(r, 1)
        engine.pcSetIts(1, 1, 1)
        engine.pcSetup(1)                                    # block-local without iterations: fine, as before
        assert engine.pcItsInfo() == (1, 1, 1, 0)
        engine.pcSelect(1)
        assert np.array_equal(engine.pcApply(r, 1), z1)
