"""Checks of the orderings of the ILU(k) over the whole level (adflow_gpu_pc_set_ordering, _set_ordering_perm, _ordering_info,
_download_ordering; csrc/pc_order.h and the tables of csrc/kernels_pc_level.hip) shared by tests/test_gpu_pc_order.py (real MI355X),
tests/test_hostsim_pc_order.py (the kernel-logic emulator) and tests/test_pc_order_host.py (the host header alone).

The yardstick is independent of the library: the rows of pc_coupled_checks.level_rows relabelled by the permutation, row a =
{inv[c]: block for c in rows[perm[a]]}, completed by pc_fill_checks.NumpyILUk._symbolic, factored by pc_checks.NumpyILU0._factor in
float64 and in longdouble, applied to r[perm] and scattered back.  The bar is pc_checks': the library at most MARGIN x as far from the
longdouble run as the float64 run is, the identity of pc_checks.assert_identity, and pcOrderingInfo / pcLevelInfo equal to the numpy
counts of the relabelled rows.  The RCM permutation is held against `genrcm` below, written from the description in
include/adflow_gpu.h, not from the library's header."""
import contextlib

import numpy as np
import pytest

import ank_checks as ank
import async_checks as asy
import jacmult_checks as jm
import pc_checks as pc
import pc_coupled_checks as pcc
import pc_fill_checks as pf
import pc_its_checks as pi
import pc_level_checks as pl
from adflow_amd import capi
from adflow_amd.params import FlowParams, upwind
from adflow_amd.topology import BrickTopology

NATURAL, RCM, CALLER = 0, 1, 2
RANDOM_SEED = 20261                  # case 2: fixed here; the largest pivot-block condition number of the float64 factor is printed
RANDOM_COND_MAX = 1e10


# ---- George and Liu's GENRCM ---------------------------------------------------------------------------------------------------------
def genrcm(adj):
    """perm[new] = old; adj[c]: the neighbours of cell c without c itself, ascending"""
    n = len(adj)
    numbered = [False] * n
    perm = []

    def structure(root):
        seen, levels = {root}, [[root]]
        while True:
            nxt = []
            for c in levels[-1]:
                for m in adj[c]:
                    if m not in seen and not numbered[m]:
                        seen.add(m)
                        nxt.append(m)
            if not nxt:
                return levels
            levels.append(nxt)

    for start in range(n):
        if numbered[start]:
            continue
        root, levels = start, structure(start)
        size = sum(len(lv) for lv in levels)
        while 1 < len(levels) < size:
            root = min(levels[-1], key=lambda c: len(adj[c]))          # min keeps the first of equal keys
            new = structure(root)
            deeper = len(new) > len(levels)
            levels = new
            if not deeper:
                break
        seq, at = [root], 0
        numbered[root] = True
        while at < len(seq):
            fresh = [m for m in adj[seq[at]] if not numbered[m]]
            for m in fresh:
                numbered[m] = True
            seq += sorted(fresh, key=lambda m: len(adj[m]))            # sorted is stable
            at += 1
        perm += seq[::-1]
    return np.array(perm, dtype=np.int32)


def adjacency_of_rows(rows):
    """the symmetric graph of a row list ({column: block} per row), diagonal left out, neighbours ascending"""
    nb = [set() for _ in rows]
    for r, row in enumerate(rows):
        for c in row:
            if c != r:
                nb[r].add(c)
                nb[c].add(r)
    return [sorted(s) for s in nb]


def brick_graph(Bi, Bj, Bk, nx, ny, nz):
    """(adjacency, global (i, j, k) of every cell) of Bi x Bj x Bk blocks of nx x ny x nz cells without wraps, numbered block after
    block (i fastest over the blocks as inside them), then k, j, i"""
    num, ijk = {}, []
    for bk in range(Bk):
        for bj in range(Bj):
            for bi in range(Bi):
                for k in range(nz):
                    for j in range(ny):
                        for i in range(nx):
                            g = (bi * nx + i, bj * ny + j, bk * nz + k)
                            num[g] = len(ijk)
                            ijk.append(g)
    adj = []
    for (i, j, k) in ijk:
        nbs = [num.get((i + d[0], j + d[1], k + d[2])) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
        adj.append(sorted(m for m in nbs if m is not None))
    return adj, np.array(ijk)


def red_black(ijk):
    """cells sorted by the parity of global i + j + k, stably"""
    return np.argsort(np.asarray(ijk).sum(axis=1) % 2, kind="stable").astype(np.int32)


def scalar_counts(adj, perm, fill):
    """(level sets, largest set, entries, bandwidth) of the scalar symbolic ILU(fill) of a graph in an ordering"""
    perm = np.asarray(perm)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    pattern = [{a} | {int(inv[c]) for c in adj[perm[a]]} for a in range(perm.size)]
    bw = max(abs(c - a) for a, p in enumerate(pattern) for c in p)
    lev = pf.NumpyILUk._symbolic(pattern, fill)
    lvl = np.zeros(perm.size, np.int64)
    for a, row in enumerate(lev):
        low = [lvl[c] for c in row if c < a]
        lvl[a] = 1 + max(low) if low else 0
    return int(lvl.max()) + 1, int(np.bincount(lvl).max()), sum(len(r) for r in lev), bw


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------
class NumpyOrderedILUk(pc.NumpyILU0):
    """pc_level_checks.NumpyLevelILUk on the rows relabelled by perm (perm[new] = old); apply takes and returns the PETSc layout"""

    def __init__(self, op, dtype, fill, perm):
        self.op, self.dtype, self.ns, self.fill = op, dtype, op.ns, fill
        nat, self.ncross = pcc.level_rows(op, dtype)
        self.perm = np.asarray(perm, dtype=np.int64)
        assert sorted(self.perm.tolist()) == list(range(len(nat)))
        inv = np.empty_like(self.perm)
        inv[self.perm] = np.arange(self.perm.size)
        rows = [{int(inv[c]): blk for c, blk in nat[self.perm[a]].items()} for a in range(len(nat))]
        self.bandwidth = max(abs(c - a) for a, row in enumerate(rows) for c in row)
        lev = pf.NumpyILUk._symbolic([set(r) for r in rows], fill)
        zero = np.zeros((self.ns, self.ns), dtype=dtype)
        for row, pattern in zip(rows, lev):
            for c in pattern:
                if c not in row:
                    row[c] = zero.copy()
        self.max_row = max(len(r) for r in rows)
        self.nentries = sum(len(r) for r in rows)
        lvl = np.zeros(len(rows), np.int64)
        for c, row in enumerate(rows):
            low = [lvl[n] for n in row if n < c]
            lvl[c] = 1 + max(low) if low else 0
        self.nsets = int(lvl.max()) + 1
        self.largest_set = int(np.bincount(lvl).max())
        self.all_lower = int(sum(1 for c, row in enumerate(rows) if len(row) > 1 and all(n <= c for n in row)))
        self.row_lengths = (min(len(r) for r in rows), self.max_row)
        self.sub = {min(op.dims): self._factor(rows)}

    def apply(self, r, transpose=False):
        ns, p = self.ns, self.perm
        y = super().apply(np.asarray(r).reshape(-1, ns)[p].reshape(-1), transpose)
        z = np.empty_like(y)
        z.reshape(-1, ns)[p] = y.reshape(-1, ns)
        return z

    def counts(self):
        """what adflow_gpu_pc_level_info reports without `reused`"""
        return self.fill, self.max_row, self.nentries, self.nsets, self.ncross


def yardsticks(op, fill, perm):
    return NumpyOrderedILUk(op, np.float64, fill, perm), NumpyOrderedILUk(op, np.longdouble, fill, perm)


def rcm_of(op):
    """the Python GENRCM on the graph of the level's rows"""
    return genrcm(adjacency_of_rows(pcc.level_rows(op, np.float64)[0]))


@contextlib.contextmanager
def order_slots(engine):
    """pc_level_checks.level_slots, and both slots back at the natural ordering without a stored permutation and without iterations"""
    try:
        yield
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcSetOrdering(NATURAL)
            engine.pcDropOrderingPerm()
            engine.pcSetIts(1, 1, 1)
            engine.pcSetLevelFill(-1)
            engine.pcSetCoupled(0)
            engine.pcSetFill(0)
            engine.pcSetMg(1)
            engine.pcRelease()
        engine.ankRelease()
        engine.releaseWorkspace()


def setup_ordered(engine, op, fill, kind, perm=None, ilus=None, ank_setup=False, reused=0, hand_over=True):
    """the ILU(fill) over the level in the selected slot in the ordering `kind`; perm: the caller's permutation (kind 2; handed over
    unless hand_over is False) or the expected one (kind 1: default the Python GENRCM); the downloaded ordering and every info entry
    against the numpy counts of the relabelled rows; returns the yardsticks"""
    if kind == RCM and perm is None:
        perm = ilus[0].perm if ilus else rcm_of(op)
    if kind == NATURAL:
        perm = np.arange(op.n // op.ns)
    engine.pcSetLevelFill(fill)
    engine.pcSetOrdering(kind, perm if kind == CALLER and hand_over else None)
    (engine.ankPcSetup if ank_setup else engine.pcSetup)(1)
    got = engine.pcOrdering()
    assert got.dtype == np.int32 and np.array_equal(got, perm), ("the ordering of the factor", kind, int((got != perm).sum()))
    ilus = ilus or yardsticks(op, fill, perm)
    y, info, oinfo = ilus[0], engine.pcLevelInfo(), engine.pcOrderingInfo()
    print(f"ordering {kind}, level fill {fill}: pcLevelInfo = {info}, pcOrderingInfo = {oinfo}; numpy: rows of {y.row_lengths} entries, "
          f"{y.nentries} entries, {y.nsets} level sets (largest {y.largest_set} rows), bandwidth {y.bandwidth}, {y.all_lower} rows whose "
          f"off-diagonal entries are all lower")
    assert info == y.counts() + (reused,), (info, y.counts(), reused)
    assert oinfo == (kind, y.bandwidth, y.nsets, y.nentries), (oinfo, y.bandwidth, y.nsets, y.nentries)
    assert engine.pcInfo()[:2] == (op.ns, y.nsets) and engine.pcInfo2() == (fill, y.max_row, y.nsets)
    return ilus


def assert_ordered_apply(engine, op, seed, what, ilus):
    first, _ = pc.assert_apply_matches(engine, op, seed, what, ilus=ilus)
    pc.assert_identity(engine, op, first, seed + 1)
    return first


# ---- 1, 4, 5: RCM on periodic bricks, rotated interfaces, a period of three cells ----------------------------------------------------
def check_rcm(engine, topo, prm, fills, seed, what):
    with order_slots(engine):
        blocks, op = jm.brick_operator(engine, topo, prm, seed)
        perm = rcm_of(op)
        assert not np.array_equal(perm, np.arange(perm.size)), "RCM gives the natural ordering: the case misses its mechanism"
        for fill in fills:
            ilus = setup_ordered(engine, op, fill, RCM, perm)
            assert_ordered_apply(engine, op, seed + 1 + fill, f"{what}, RCM, level fill {fill}", ilus)
            engine.pcRelease()


def check_rcm_periodic_brick(engine, fills=(0, 1, 2)):
    """2 x 2 x 1 periodic blocks of 6 x 5 x 4.  Measured: the bar is met at every fill (ratios 0.09 to 1.4 on the MI355X), but at fill 1
    and 2 the ILU of this matrix in the RCM ordering is unstable -- max|z| of 1e10 and 1e23 for |r| <= 1, and at fill 2 the float64
    numpy run itself is further from the longdouble run than max|z| -- so the ratio carries little there; the counts and the
    permutation are exact at every fill, and the other RCM cases meet the bar at fill 1 and 2 with max|z| of order 1"""
    check_rcm(engine, BrickTopology(2, 2, 1, 6, 5, 4), pl.EULER_JST, fills, 223, "periodic brick 2x2x1 of 6x5x4")


def check_rcm_rotated(engine, fills=(1, 2)):
    check_rcm(engine, pcc.ell_half(), FlowParams(spaceDiscr=upwind), fills, 251, "rotated interfaces")


def check_rcm_period_of_three(engine):
    check_rcm(engine, BrickTopology(1, 1, 1, 3, 4, 4), pl.EULER_JST, (1,), 227, "period of three cells")


# ---- 2: a caller's random permutation ----------------------------------------------------------------------------------------------------
def check_random_permutation(engine, fills=(1, 2), seed=227):
    """lower entries at any distance, rows of very different lengths in one slice, merge keys in no geometric order"""
    with order_slots(engine):
        blocks, op = jm.brick_operator(engine, BrickTopology(2, 1, 1, 3, 4, 4), pl.EULER_JST, seed)
        perm = np.random.default_rng(RANDOM_SEED).permutation(op.n // op.ns).astype(np.int32)
        for fill in fills:
            ilus = yardsticks(op, fill, perm)
            cond = ilus[0].pivot_conditions()
            print(f"random permutation (seed {RANDOM_SEED}), level fill {fill}: largest pivot-block condition number of the float64 numpy "
                  f"factor {cond:.3e}, rows of {ilus[0].row_lengths} entries")
            assert cond < RANDOM_COND_MAX, (cond, "choose another RANDOM_SEED")
            assert ilus[0].row_lengths[1] >= 2 * ilus[0].row_lengths[0], ilus[0].row_lengths
            setup_ordered(engine, op, fill, CALLER, perm, ilus=ilus)
            assert_ordered_apply(engine, op, seed + 1 + fill, f"random permutation, level fill {fill}", ilus)
            engine.pcRelease()


# ---- 3: red-black through kind 2 -----------------------------------------------------------------------------------------------------------
def check_red_black(engine, dims=(12, 8, 6), seed=107):
    """one wall-bounded RANS block at fill 0: two level sets, so several workgroups in one launch and rows whose off-diagonal entries
    are all lower"""
    with order_slots(engine):
        blk, op = pc.single_block(engine, dims, pc.RANS, jm.WALL, seed, stretch_k=2.0)
        assert op.ns == 6
        ijk = np.array([(i, j, k) for k in range(dims[2]) for j in range(dims[1]) for i in range(dims[0])])
        perm = red_black(ijk)
        ilus = setup_ordered(engine, op, 0, CALLER, perm)
        assert ilus[0].nsets == 2 and engine.pcOrderingInfo()[2] == 2, ilus[0].nsets
        assert ilus[0].largest_set > 64 and ilus[0].all_lower > 64, (ilus[0].largest_set, ilus[0].all_lower)
        assert_ordered_apply(engine, op, seed + 1, f"red-black, one block {dims}, level fill 0", ilus)


# ---- 6: the benchmark layout in miniature, GMRES ---------------------------------------------------------------------------------------------
def check_wall_brick_gmres(engine, fill=2, restart=80, rtol=1e-8, seed=281):
    """nState 6, RCM at fill 2: gmresSolve in both directions with maxIts = 2 x the count scipy's GMRES takes with the numpy RCM factor
    (itself at most 60), the true residual as pc_level_checks.check_wall_brick_gmres; then the natural ordering of the same matrix side
    by side: where scipy with the numpy factors takes fewer (more) iterations with RCM, so must the library"""
    with order_slots(engine):
        blocks, prm, op = pcc.wall_brick(engine)
        assert op.ns == 6
        ilus = setup_ordered(engine, op, fill, RCM)
        assert_ordered_apply(engine, op, 109, f"wall-bounded brick, RCM, level fill {fill}", ilus)
        rng = np.random.default_rng(seed)
        bs = {tr: rng.uniform(-1.0, 1.0, op.n) for tr in (False, True)}
        natural = pl.NumpyLevelILUk(op, np.float64, fill)
        k_rcm, k_nat, its_rcm = {}, {}, {}
        for tr in (False, True):
            b = bs[tr]
            k_rcm[tr] = pc.scipy_gmres_iterations(lambda v: op.apply(v, tr), ilus[0], b, tr, rtol, restart, restart)
            k_nat[tr] = pc.scipy_gmres_iterations(lambda v: op.apply(v, tr), natural, b, tr, rtol, restart, restart)
            assert k_rcm[tr] <= 60, k_rcm
            cap = 2 * k_rcm[tr]
            x, its, r0, rn = engine.gmresSolve(b, 1, transpose=tr, restart=restart, maxIts=cap, rtol=rtol)
            true, nb = float(np.linalg.norm(b - op.apply(x, tr))), float(np.linalg.norm(b))
            print(f"gmres, RCM ILU({fill}) over the level, transpose={tr}: {its} iterations (scipy with the numpy factor {k_rcm[tr]}), "
                  f"||b - A x|| / ||b|| = {true / nb:.3e} (reported {rn / nb:.3e})")
            assert 0 < its <= cap, (its, cap)
            assert abs(r0 - nb) <= 1e-12 * nb
            assert true <= 2 * rtol * nb, (true, nb)
            assert abs(rn - true) <= 1e-3 * rtol * nb + 1e-6 * true
            its_rcm[tr] = its
        engine.pcSetOrdering(NATURAL)
        engine.pcSetup(1)
        assert engine.pcOrderingInfo()[0] == NATURAL and engine.pcLevelInfo()[5] == 0
        print(f"level sets: natural {natural.nsets} (largest {natural.largest_set}), RCM {ilus[0].nsets} (largest {ilus[0].largest_set}); "
              f"entries {natural.nentries} / {ilus[0].nentries}")
        for tr in (False, True):
            x, its, r0, rn = engine.gmresSolve(bs[tr], 1, transpose=tr, restart=restart, maxIts=restart, rtol=rtol)
            print(f"gmres at fill {fill}, transpose={tr}: natural {its} iterations, RCM {its_rcm[tr]} (scipy with the numpy factors: "
                  f"natural {k_nat[tr]}, RCM {k_rcm[tr]})")
            if k_rcm[tr] < k_nat[tr]:                            # the yardstick decides whether a comparison is asserted
                assert its_rcm[tr] < its, ("the yardstick gains iterations with RCM, the library does not", tr, its_rcm[tr], its)
            elif k_rcm[tr] > k_nat[tr]:
                assert its_rcm[tr] > its, ("the yardstick loses iterations with RCM, the library does not", tr, its_rcm[tr], its)


# ---- 7: ankPcSetup ------------------------------------------------------------------------------------------------------------------------------
def check_wall_brick_ank(engine, fill=1, seed=311):
    """T reaches the RCM factor; a plain setup afterwards gives the plain result again; both setups keep the tables"""
    with order_slots(engine):
        blocks, prm, op = pcc.wall_brick(engine)
        ilus = setup_ordered(engine, op, fill, RCM)
        perm = ilus[0].perm
        r = np.random.default_rng(seed).uniform(-1.0, 1.0, op.n)
        plain = engine.pcApply(r, 1)
        Tn = ank.assert_T(engine, blocks, prm, True, "wall-bounded brick")
        ops = ank.shifted(op, Tn)
        ilus_t = setup_ordered(engine, ops, fill, RCM, perm, ank_setup=True, reused=1)
        assert_ordered_apply(engine, ops, seed + 1, f"shifted RCM ILU({fill}) over the level", ilus_t)
        assert not np.array_equal(engine.pcApply(r, 1), plain), "T does not reach the factor"
        setup_ordered(engine, op, fill, RCM, perm, ilus=ilus, reused=1)
        assert np.array_equal(engine.pcApply(r, 1), plain), "pcSetup after the ANK entries"


# ---- 8: bit identity -------------------------------------------------------------------------------------------------------------------------------
def check_bit_identity(engine, fill=1, seed=223):
    """pcSetOrdering(0) against a slot that never saw the call; the identity through kind 2 against kind 0"""
    with order_slots(engine):
        blocks, op = jm.brick_operator(engine, BrickTopology(2, 2, 1, 6, 5, 4), pl.EULER_JST, seed)
        r = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, op.n)
        n = op.n // op.ns
        engine.pcSelect(1)                                   # this slot never sees an ordering call before its setup
        engine.pcSetLevelFill(fill)
        engine.pcSetup(1)
        z1 = {tr: engine.pcApply(r, 1, transpose=tr) for tr in (False, True)}
        info1, level1 = engine.pcInfo(), engine.pcLevelInfo()
        engine.pcSelect(0)
        engine.pcSetLevelFill(fill)
        engine.pcSetOrdering(RCM)
        engine.pcSetOrdering(NATURAL)
        engine.pcSetup(1)
        assert engine.pcInfo() == info1 and engine.pcLevelInfo() == level1, (engine.pcInfo(), info1)
        assert engine.pcOrderingInfo()[0] == NATURAL and np.array_equal(engine.pcOrdering(), np.arange(n))
        for tr in (False, True):
            assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z1[tr]), ("pcSetOrdering(0)", tr)
        engine.pcSetOrdering(CALLER, np.arange(n, dtype=np.int32))
        engine.pcSetup(1)
        assert engine.pcOrderingInfo()[0] == CALLER and engine.pcLevelInfo()[:5] == level1[:5] and engine.pcLevelInfo()[5] == 0
        assert engine.pcInfo() == info1
        for tr in (False, True):
            assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z1[tr]), ("the identity through kind 2", tr)


# ---- 9: refusals and isolation -------------------------------------------------------------------------------------------------------------------
def check_refusals(engine, seed=227):
    with order_slots(engine):
        blocks, op = jm.brick_operator(engine, BrickTopology(2, 1, 1, 3, 4, 4), pl.EULER_JST, seed)
        n = op.n // op.ns
        r = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, op.n)
        good = np.random.default_rng(seed + 2).permutation(n).astype(np.int32)
        engine.pcSelect(0)
        with pytest.raises(capi.AdflowGpuError, match="no factor"):
            engine.pcOrderingInfo()
        with pytest.raises(capi.AdflowGpuError, match="no factor"):
            engine.pcOrdering()
        engine.pcSetLevelFill(1)
        engine.pcSetOrdering(CALLER, good)
        engine.pcSetup(1)
        z = engine.pcApply(r, 1)

        def slot0_applies():
            engine.pcSelect(0)
            assert engine.pcOrderingInfo()[0] == CALLER and np.array_equal(engine.pcOrdering(), good)
            assert np.array_equal(engine.pcApply(r, 1), z)

        # the setters: the message names the value or the first offending index; kind and permutation stay
        for bad in (3, -1):
            with pytest.raises(capi.AdflowGpuError, match=f"pc_set_ordering: {bad}"):
                engine.pcSetOrdering(bad)
        dup, out = good.copy(), good.copy()
        dup[7] = dup[2]
        out[5] = n
        low = good.copy()
        low[4] = -1
        for perm, msg in ((dup, rf"perm\[7\] = {dup[7]} occurs twice"), (out, rf"perm\[5\] = {n} lies outside"),
                          (low, r"perm\[4\] = -1 lies outside")):
            with pytest.raises(capi.AdflowGpuError, match=msg):
                engine.pcSetOrdering(CALLER, perm)
        assert engine.lib.adflow_gpu_pc_set_ordering_perm(good.ctypes.data, 0) != 0
        assert "n = 0" in engine.lib.adflow_gpu_last_error().decode()
        slot0_applies()
        engine.pcSetup(1)                                    # the refused calls changed neither the kind nor the permutation nor the tables
        assert engine.pcLevelInfo()[5] == 1
        slot0_applies()
        # the setups of slot 1
        engine.pcSelect(1)
        engine.pcSetLevelFill(1)
        engine.pcSetup(1)                                    # a factor the refused setups must not keep

        def refused(msg):
            engine.pcSelect(1)
            with pytest.raises(capi.AdflowGpuError, match=msg):
                engine.pcSetup(1)
            with pytest.raises(capi.AdflowGpuError, match="no factor"):
                engine.pcApply(r, 1)
            with pytest.raises(capi.AdflowGpuError, match="no factor"):
                engine.pcOrderingInfo()
            slot0_applies()
            engine.pcSelect(1)

        engine.pcSetOrdering(CALLER)
        refused("holds no permutation")
        engine.pcSetOrdering(CALLER, good[:n // 2].argsort().argsort().astype(np.int32))
        refused(f"has {n // 2} entries")
        engine.pcDropOrderingPerm()
        refused("holds no permutation")
        for kind in (RCM, CALLER):
            engine.pcSetOrdering(kind, good if kind == CALLER else None)
            engine.pcSetLevelFill(-1)
            for setting, reset in ((lambda: None, lambda: None), (lambda: engine.pcSetFill(1), lambda: engine.pcSetFill(0)),
                                   (lambda: engine.pcSetCoupled(1), lambda: engine.pcSetCoupled(0)),
                                   (lambda: engine.pcSetMg(2), lambda: engine.pcSetMg(1))):
                setting()
                refused(f"ordering {kind}")
                reset()
            engine.pcSetLevelFill(1)
        engine.pcSetup(1)                                    # the settings fit again: the slot takes an ordered factor
        assert np.array_equal(engine.pcApply(r, 1), z)
        # a block-local factor reports the natural ordering and no bandwidth
        engine.pcSetOrdering(NATURAL)
        engine.pcSetLevelFill(-1)
        engine.pcSetup(1)
        assert engine.pcOrderingInfo()[:2] == (NATURAL, -1) and np.array_equal(engine.pcOrdering(), np.arange(n))
        slot0_applies()


def check_isolation(engine, seed=223):
    """a block-local factor in slot 0 applies bit for bit before, while and after an RCM factor lives in slot 1"""
    with order_slots(engine):
        blocks, op = jm.brick_operator(engine, BrickTopology(2, 2, 1, 6, 5, 4), pl.EULER_JST, seed)
        r = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, op.n)
        engine.pcSelect(0)
        engine.pcSetup(1)
        z0 = {tr: engine.pcApply(r, 1, transpose=tr) for tr in (False, True)}

        def slot0(when):
            engine.pcSelect(0)
            assert engine.pcCoupledInfo()[0] == 0 and engine.pcOrderingInfo()[:2] == (NATURAL, -1)
            for tr in (False, True):
                assert np.array_equal(engine.pcApply(r, 1, transpose=tr), z0[tr]), (when, tr)

        engine.pcSelect(1)
        engine.pcSetLevelFill(1)
        engine.pcSetOrdering(RCM)
        engine.pcSetup(1)
        z1 = engine.pcApply(r, 1)
        assert engine.pcOrderingInfo()[0] == RCM and not np.array_equal(z1, z0[False])
        slot0("with an RCM factor in slot 1")
        engine.pcSetup(1)
        slot0("slot 0 set up again")
        engine.pcSelect(1)
        assert np.array_equal(engine.pcApply(r, 1), z1)
        engine.pcRelease()
        slot0("after the release of slot 1")


# ---- 10: table reuse ----------------------------------------------------------------------------------------------------------------------------------
def check_table_reuse(engine, fill=1, seed=227):
    with order_slots(engine):
        blocks, op = jm.brick_operator(engine, BrickTopology(2, 1, 1, 3, 4, 4), pl.EULER_JST, seed)
        n = op.n // op.ns
        r = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, op.n)
        rcm = rcm_of(op)
        p1 = np.random.default_rng(seed + 2).permutation(n).astype(np.int32)
        p2 = np.random.default_rng(seed + 3).permutation(n).astype(np.int32)
        y_rcm, y1, y2 = (yardsticks(op, fill, p) for p in (rcm, p1, p2))
        setup_ordered(engine, op, fill, RCM, rcm, ilus=y_rcm)
        z_rcm = engine.pcApply(r, 1)
        setup_ordered(engine, op, fill, RCM, rcm, ilus=y_rcm, reused=1)                     # the same ordering
        assert np.array_equal(engine.pcApply(r, 1), z_rcm)
        setup_ordered(engine, op, fill, CALLER, p1, ilus=y1, reused=0)                      # a change of kind
        z1 = engine.pcApply(r, 1)
        setup_ordered(engine, op, fill, CALLER, p1, ilus=y1, reused=1, hand_over=False)     # the same permutation, not handed over again
        assert np.array_equal(engine.pcApply(r, 1), z1)
        setup_ordered(engine, op, fill, CALLER, p2, ilus=y2, reused=0)                      # a new permutation
        assert_ordered_apply(engine, op, seed + 4, "the second permutation", y2)
        setup_ordered(engine, op, fill, CALLER, p2, ilus=y2, reused=0)                      # handed over again: the library cannot know it is the same
        setup_ordered(engine, op, fill, NATURAL, reused=0, ilus=yardsticks(op, fill, np.arange(n)))
        setup_ordered(engine, op, fill, RCM, rcm, ilus=y_rcm, reused=0)
        assert np.array_equal(engine.pcApply(r, 1), z_rcm)


# ---- 11: several columns, iterations, bytes ---------------------------------------------------------------------------------------------------------------
def check_multi_its_and_bytes(engine, fill=1, seed=251):
    with order_slots(engine):
        blocks, op = jm.brick_operator(engine, pcc.ell_half(), FlowParams(spaceDiscr=upwind), seed)
        ilus = setup_ordered(engine, op, fill, RCM)
        R = np.random.default_rng(seed + 2).uniform(-1.0, 1.0, (3, op.n))

        def columns(ys, what):
            for tr in (False, True):
                Z = engine.pcApplyMulti(R, 1, transpose=tr)
                for c in range(3):
                    assert np.array_equal(Z[c], engine.pcApply(R[c], 1, transpose=tr)), (what, "multi against single", tr, c)
                    zl = ys[1].apply(R[c], tr)
                    e_np = float(np.abs(ys[0].apply(R[c], tr).astype(np.longdouble) - zl).max())
                    e_lib = float(np.abs(Z[c].astype(np.longdouble) - zl).max())
                    print(f"{what}: 3 columns, transpose={tr}, column {c}: max|z - z_ld| = {e_lib:.3e}, float64 numpy {e_np:.3e}")
                    assert e_lib <= pc.MARGIN * e_np, (what, tr, c, e_lib, e_np)

        columns(ilus, "RCM factor")
        plain_bytes = engine.pcInfo()[2]
        engine.pcSetIts(3, 1, 1)
        engine.pcSetup(1)
        assert engine.pcItsInfo()[:3] == (3, 1, 1) and engine.pcOrderingInfo()[0] == RCM
        assert np.array_equal(engine.pcOrdering(), ilus[0].perm)
        columns(pi.pair(ilus, pi.matrices(op), 3, 1, False), "RCM factor in 3 outer iterations")
        nb = engine.pcInfo()[2]
        assert nb > plain_bytes >= 8 * op.ns ** 2 * ilus[0].nentries, (nb, plain_bytes, ilus[0].nentries)
        assert engine.pcRelease() == nb and engine.pcRelease() == 0
        with pytest.raises(capi.AdflowGpuError, match="no factor"):
            engine.pcOrderingInfo()


# ---- 12: the enqueue-only mode ---------------------------------------------------------------------------------------------------------------------------------
def check_enqueue_only_chain(engine, dv, fill=1, seed=251):
    """setup, two applications and a gmres solve with the RCM factor under adflow_gpu_set_async(1) with one synchronise: within the bar,
    and bit-equal to the chain with a synchronise after every call"""
    topo = pcc.ell_half()

    def setup(enqueue):
        blocks, op = jm.brick_operator(engine, topo, FlowParams(spaceDiscr=upwind), seed)
        engine.pcSelect(0)
        engine.pcSetLevelFill(fill)
        engine.pcSetOrdering(RCM)
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

    with order_slots(engine):
        c, enq, syn = asy.both_runs(engine, dv, setup, chain)
        op = c["op"]
        perm = rcm_of(op)
        assert engine.pcOrderingInfo()[0] == RCM and np.array_equal(engine.pcOrdering(), perm)
        assert np.array_equal(enq["r"], c["r"]), "the right-hand side was written"
        f64, fld = yardsticks(op, fill, perm)
        for out, rhs, tr in (("z1", enq["r"], False), ("z2", enq["z1"], True)):
            zl = fld.apply(rhs, tr)
            e_np = float(np.abs(f64.apply(rhs, tr).astype(np.longdouble) - zl).max())
            e_lib = float(np.abs(enq[out].astype(np.longdouble) - zl).max())
            print(f"enqueue-only chain {out}: max|z - z_ld| = {e_lib:.3e}, float64 numpy {e_np:.3e}")
            assert e_lib <= pc.MARGIN * e_np and np.abs(zl).max() > 0.0, (out, e_lib, e_np)
        true = float(np.linalg.norm(enq["z2"] - op.apply(enq["x"])))
        assert true <= 2e-8 * float(np.linalg.norm(enq["z2"])), true
        asy.assert_bitwise("chain with the RCM ILU over the level", enq, syn)
