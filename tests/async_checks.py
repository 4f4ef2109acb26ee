"""Checks of the enqueue-only mode (adflow_gpu_set_async(1): every hot-path entry returns once its work is enqueued on the library's
stream, one adflow_gpu_sync where the host needs a value), shared by tests/test_gpu_async.py (real MI355X) and
tests/test_hostsim_async.py (the kernel-logic emulator, where every queue is synchronous: the twin proves the test logic and the
host-side state handling).

Every case runs a CHAIN of calls with nothing between them -- no synchronise from the test, no torch operation on the chain's
vectors -- and makes two comparisons:
 1. against the reference, with the yardstick and the bar the synchronous test of the same entry uses (checks.TOL with its local
    measure; the numpy operators and ILU yardsticks of jacmult_checks, pc_checks, pc_fill_checks, ank_checks, ank_turb_checks).
    No tolerance is introduced here.
 2. against the same chain from the same start with a synchronise after every call, bit for bit.  The two runs launch the same
    kernels in the same order; the only sums formed with atomicAdd (sumsq2 of get_r_vec, res_norms, the halo norm) are not part of
    any chain.  This leg tells which link went wrong.
Every link of a chain gets input of its own (state vectors perturbed by 1e-3 relative with different seeds, different right-hand
sides), and the REFERENCE results of consecutive links are asserted to differ by more than SEPARATION x the bar: a result taken
from the wrong call's data is then far outside it."""
import contextlib

import numpy as np
import pytest

import ank_checks as ank
import ank_turb_checks as ankt
import checks
import jacmult_checks as jm
import pc_checks as pc
import pc_fill_checks as pcf
from adflow_amd import capi
from adflow_amd.params import (FlowParams, NSEquations, RANSEquations, DADI, dissMatrix, upwind, vanAlbeda, firstOrder, secondOrder,
                               noResAveraging, alwaysResAveraging)
from util import TOL, rel_err, owned

EPS = 2.0 ** -52
SEPARATION = 1e3
RANS = pc.RANS                                                          # Roe, van Albada
RANS2 = pc.RANS.replace(orderTurb=secondOrder)                          # ADFLOW_RES_TURB_FIRST_ORDER changes the result
LAMINAR_MATRIX = FlowParams(equations=NSEquations, spaceDiscr=dissMatrix, vis4=0.1, muSuthDim=1.0)
_KEEP = ank._KEEP           # the reference's flowDoms point into these arrays: alive as long as ref may be called


@contextlib.contextmanager
def enqueue_only(engine):
    """the enqueue-only mode for the calls inside; whatever happens, the queue is drained and the mode is off afterwards"""
    engine.set_async(True)
    try:
        yield
    finally:
        try:
            engine.sync()
        finally:
            engine.set_async(False)


class Link:
    """one pass over a chain: link(fn, *args) is one call of it.  enqueue = False: the comparison run, a synchronise after every call
    (the mode is off there, so every entry also synchronises by itself)"""

    def __init__(self, engine, enqueue):
        self.engine, self.enqueue = engine, enqueue

    def __call__(self, fn, *args, **kw):
        out = fn(*args, **kw)
        if not self.enqueue:
            self.engine.sync()
        return out

    def refused(self, match, fn, *args, **kw):
        """a call the library must refuse: its error comes back, nothing else happens"""
        with pytest.raises(capi.AdflowGpuError, match=match):
            fn(*args, **kw)
        if not self.enqueue:
            self.engine.sync()


def _host(dv, v):
    if isinstance(v, np.ndarray):
        return v.copy()
    if hasattr(v, "data_ptr"):
        return dv.get(v)
    return v


def both_runs(engine, dv, setup, chain, after=None):
    """setup(enqueue) -> ctx: the start of a run (blocks registered, device vectors made: every torch operation happens here);
    chain(ctx, link) -> {name: device vector | host value}: the calls, each through link(); after(ctx) -> {name: host array}: what is
    read from the device once the queue is drained.  Runs it from one setup with a synchronise after every call, then from a new
    setup enqueue-only with ONE dv.sync() before and ONE engine.sync() after.  Returns (ctx of the enqueue-only run, its results,
    the results of the synchronised run)."""
    out = {}
    for enqueue in (False, True):       # the enqueue-only run last: the reference stays bound to ITS blocks for the yardsticks
        ctx = setup(enqueue)
        dv.sync()
        if enqueue:
            with enqueue_only(engine):
                vecs = chain(ctx, Link(engine, True))
        else:
            vecs = chain(ctx, Link(engine, False))
        engine.sync()
        res = {k: _host(dv, v) for k, v in vecs.items()}
        if after is not None:
            res.update(after(ctx))
        out[enqueue] = (ctx, res)
    return out[True][0], out[True][1], out[False][1]


def assert_bitwise(what, enq, syn, skip=()):
    """leg 2: every result of the enqueue-only run is bit for bit the result of the synchronised run"""
    assert set(enq) == set(syn), (set(enq) ^ set(syn))
    for k in enq:
        if k in skip:
            continue
        a, b = enq[k], syn[k]
        same = np.array_equal(a, b, equal_nan=True) if isinstance(a, np.ndarray) else a == b
        if not same and isinstance(a, np.ndarray):
            d = np.abs(a - b)
            print(f"{what}: link result '{k}' differs from the synchronised run in {int((a != b).sum())} of {a.size} entries, max {np.nanmax(d):.3e} "
                  f"of {np.nanmax(np.abs(b)):.3e}")
        assert same, (what, "enqueue-only against a synchronise after every call", k)
    print(f"{what}: {len(enq) - len(skip)} results bit-equal to the run with a synchronise after every call")


def assert_links_distinct(what, refs, bars):
    """the distinct-input condition, on the reference side alone: consecutive reference results (vectors of one length) differ by
    more than SEPARATION x the larger of their bars (absolute, max-norm)"""
    for m in range(len(refs) - 1):
        d = float(np.abs(np.asarray(refs[m], dtype=np.float64) - np.asarray(refs[m + 1], dtype=np.float64)).max())
        bar = max(bars[m], bars[m + 1])
        assert d > SEPARATION * bar, (what, "the reference results of links", m, m + 1, "are too close to tell a mix-up", d, bar)


@contextlib.contextmanager
def tuning(engine, keys):
    """keys = {name: (value inside, value afterwards)}"""
    try:
        for k, (v, _) in keys.items():
            engine.set_tuning(k, v)
        yield
    finally:
        for k, (_, v) in keys.items():
            engine.set_tuning(k, v)


# ---- 1. residual chain (and 8: refused calls inside it) --------------------------------------------------------------------------
def check_residual_chain(engine, dv, topo, prm, bc_spec=None, seed=21, nlinks=3, tune=None, rccl_self=False, refusals=False, **mk):
    """nlinks x adflow_gpu_nk_residual_dev(w_i -> r_i) back to back, one synchronise: every r_i against check_nk_residual's reference
    for w_i at its bar, and against the synchronised run.  tune: tuning keys for both runs; rccl_self: every interface a message to
    the own rank (comm_self; a communicator of one rank).  refusals: calls the library refuses sit between the links of the
    enqueue-only run -- and only there: the results are those of the chain without them (what this can see: the queue stays usable and
    no refused call leaves work or state behind; the mode has no getter, a leak of it would not change these bits)."""
    first = {}
    if rccl_self:
        engine.comm_init_single()
        tune = dict(tune or {}, comm_self=(1, 0))

    def setup(enqueue):
        blocks, rblocks, p = checks.nk_setup(engine, topo, prm, seed, bc_spec, **mk)
        _KEEP[:] = [rblocks]
        ws = [checks.nk_state_vector(blocks, p, np.random.default_rng(seed + 1 + 977 * m)) for m in range(nlinks)]
        if enqueue:
            first["refs"] = [checks.nk_reference(rblocks, p, w, bc_spec) for w in ws]
            for l in range(p.nw):
                cols = [r.reshape(-1, p.nw)[:, l] for r in first["refs"]]
                assert_links_distinct(f"residual chain, variable {l}", cols, [TOL * np.abs(c).max() for c in cols])
        return dict(p=p, ws=ws, n=ws[0].size, d_w=[dv.put(w) for w in ws], d_r=[dv.put(np.full(ws[0].size, 7.0)) for _ in ws])

    def chain(c, link):
        n = c["n"]
        for m, (w, r) in enumerate(zip(c["d_w"], c["d_r"])):
            link(engine.FormFunction_mf_dev, dv.ptr(w), dv.ptr(r), n)
            if refusals and link.enqueue:
                link.refused("DOF", engine.FormFunction_mf_dev, dv.ptr(w), dv.ptr(r), n + c["p"].nw)
                link.refused("no factor", engine.pcApplyDev, dv.ptr(w), dv.ptr(r), n)
                if m == 0:      # fails inside the cycle, which forces the mode on (once: a second identical call would be captured)
                    link.refused("not -1, 0 or 1", engine.executeMGCycle, [2])
                link.refused("no base state", engine.ankMultDev, dv.ptr(w), dv.ptr(r), n)
        out = {f"r{m}": r for m, r in enumerate(c["d_r"])}
        out.update({f"w{m}": w for m, w in enumerate(c["d_w"])})
        return out

    with tuning(engine, tune or {}):
        c, enq, syn = both_runs(engine, dv, setup, chain)
    what = f"residual chain {len(engine.blocks)} block(s) {(topo.nx, topo.ny, topo.nz)} eq={prm.equations} sd={prm.spaceDiscr} tune={tune} refusals={refusals}"
    worst = 0.0
    for m in range(nlinks):
        assert np.array_equal(enq[f"w{m}"], c["ws"][m]), (what, m, "the state vector was written")
        worst = max(worst, checks.assert_rvec(enq[f"r{m}"], first["refs"][m], c["p"].nw, what=f"{what}, link {m}"))
    print(f"{what}: largest error against the reference {worst:.3e} (bar {TOL:.0e})")
    assert_bitwise(what, enq, syn)


# ---- 1b. the split evaluation ------------------------------------------------------------------------------------------------------
WALL_BRICK = {1: -6, 2: -6, 3: -1, 4: -6, 5: -3, 6: -6}


def _vector_to_dws(blocks, prm, vec, ns):
    """{nn: dw of the owned cells} from a level vector of ank_get_r (block, k, j, i, variable fastest)"""
    out, off = {}, 0
    for nn in sorted(blocks):
        n = blocks[nn].ncells * ns
        out[nn] = _dw_of_vector(blocks[nn], prm, vec[off:off + n])
        off += n
    return out


def check_split_chain(engine, dv, topo, seed=19, nlinks=3):
    """the evaluation split around the exchange (tuning split_eval = 2, gf_cus = 2: the interior tiles of the SA march and of the fused
    viscous march on the side queue) chained: nlinks x [ank_set_w_dev(w_i), block_res(CLOSURES | HALO | FLOW | TURB), ank_get_r_dev(r_i)]
    on a non-periodic brick with boundary subfaces.  The next link's state write waits behind the join of the side queue, or reads
    and writes under kernels that still run there.  That this configuration TAKES the split is asserted first: with tuning
    test_fault = 2 the same call fails behind the fork of the split evaluation, and only there.  Each dw against the reference's
    whole blocketteRes for w_i (checks.assert_dw, the bar of check_blockette_res_with_bc) and bit for bit against the synchronised run."""
    from oracle import ref
    C = capi.ANK_COUPLED
    first = {}

    def evaluate():
        engine.blocketteRes(1, updateIntermed=False, flowRes=True, turbRes=True, halo=True, closures=True)

    def setup(enqueue):
        blocks, rblocks, bocos, prm = checks.setup_brick_with_bc(engine, topo, RANS, WALL_BRICK, seed, stretch_k=2.0)
        _KEEP[:] = [rblocks, bocos]
        w0 = ank.owned_vector(blocks, "w", prm.nw)
        ws = [w0 * (1.0 + 1e-3 * np.random.default_rng(seed + 1 + 977 * m).uniform(-1.0, 1.0, w0.size)) for m in range(nlinks)]
        # the split is taken: the fault behind its fork is reported (and the side queue joined on that exit)
        try:
            engine.set_tuning("test_fault", 2)
            with pytest.raises(capi.AdflowGpuError, match="split evaluation fails behind its fork"):
                evaluate()
        finally:
            engine.set_tuning("test_fault", 0)
        engine.sync()
        if enqueue:
            refs = []
            for w in ws:
                off = 0
                for nn in sorted(rblocks):
                    r = rblocks[nn]
                    n = r.ncells * prm.nw
                    r.owned("w")[...] = np.transpose(w[off:off + n].reshape(r.nz, r.ny, r.nx, prm.nw), (2, 1, 0, 3))
                    off += n
                    ref.call_level("setPointers", 1, nn)
                    ref.call("computePressureSimple", 0)
                    ref.call("computeLamViscosity", 0)
                    ref.call("computeEddyViscosity", 0)
                    ref.call("bcTurbTreatment")
                    ref.call("applyAllTurbBCThisBlock", 1)
                    ref.call("applyAllBC_block", 1)
                ref.call_level("whalo2", 1, 1, prm.nw)
                dws = {}
                for nn in sorted(rblocks):
                    ref.call_level("setPointers", 1, nn)
                    ref.blockette_res_core(False, True, True)
                    dws[nn] = rblocks[nn]["dw"].copy(order="F")
                refs.append(dws)
            first["refs"] = refs
            for nn in sorted(blocks):
                for l in range(prm.nw):
                    cols = [owned(blocks[nn], d[nn][..., l]) for d in refs]
                    assert_links_distinct(f"split chain, block {nn}, variable {l}", cols, [TOL * np.abs(c).max() for c in cols])
        n = w0.size
        return dict(blocks=blocks, prm=prm, n=n, ws=ws, d_w=[dv.put(w) for w in ws], d_r=[dv.put(np.full(n, 7.0)) for _ in ws])

    def chain(c, link):
        n = c["n"]
        for w, r in zip(c["d_w"], c["d_r"]):
            link(engine.ankSetWDev, dv.ptr(w), n, C)
            link(evaluate)
            link(engine.ankGetRDev, dv.ptr(r), n, C)
        out = {f"r{m}": r for m, r in enumerate(c["d_r"])}
        out.update({f"w{m}": w for m, w in enumerate(c["d_w"])})
        return out

    with tuning(engine, {"split_eval": (2, 1), "gf_cus": (2, 0)}):
        c, enq, syn = both_runs(engine, dv, setup, chain)
    blocks, prm = c["blocks"], c["prm"]
    what = f"split-evaluation chain, {len(blocks)} blocks {(topo.nx, topo.ny, topo.nz)}"
    worst = 0.0
    for m in range(nlinks):
        assert np.array_equal(enq[f"w{m}"], c["ws"][m]), (what, m, "the state vector was written")
        dws = _vector_to_dws(blocks, prm, enq[f"r{m}"], prm.nw)
        for nn in sorted(blocks):
            checks.assert_dw(blocks[nn], dws[nn], first["refs"][m][nn], prm.nw, what=f"{what}: link {m}, block {nn}")
            worst = max([worst] + [rel_err(owned(blocks[nn], dws[nn][..., l]), owned(blocks[nn], first["refs"][m][nn][..., l]))
                                   for l in range(prm.nw)])
    print(f"{what}: largest error against the reference {worst:.3e} (bar {TOL:.0e})")
    assert_bitwise(what, enq, syn)


# ---- 3. smoothers and the multigrid cycle ----------------------------------------------------------------------------------------
def _snapshot(blocks):
    if not isinstance(blocks, dict):
        blocks = {1: blocks}
    return {f"{n}({nn})": b[n].copy() for nn, b in blocks.items() for n in ("w", "p", "rlv", "rev") if n in b.a}


def check_sweeps_chain(engine, check, *args, **kw):
    """check = one of checks.check_rk_smoother / check_dadi_smoother / check_smoother_with_bc / check_mg_cycle: its sweeps (cycles)
    enqueue-only with one comparison against the reference at the end (their own assert_state / assert_dw), then the same from a new
    setup with every entry synchronising itself: the state (and dw) downloaded at the end bit for bit"""
    snaps = []
    for chain in (lambda: enqueue_only(engine), contextlib.nullcontext):
        got = check(engine, *args, chain=chain, **kw)
        snap = _snapshot(got[0] if isinstance(got, tuple) else got)
        if isinstance(got, tuple):
            snap.update({f"dw({nn})": dw for nn, dw in got[1].items()})
        snaps.append(snap)
    assert_bitwise(f"{check.__name__} {args[:1]}", snaps[0], snaps[1])


# ---- 4. assembled-matrix chain ----------------------------------------------------------------------------------------------------
def check_matrix_chain(engine, dv, topo=None, prm=None, dims=None, seed=251):
    """fd_jacobian by finite differences, at once pc_setup at fill 0 (slot 0) and fill 2 (slot 1), pc_apply_dev(r1 -> z1),
    pc_apply_dev(r2 -> z2, transpose, slot 1), jacobian_mult_dev(x1 -> y1), (y1 -> y2, transpose), (x2 -> y3), pc_apply_dev(y3 -> z3):
    one synchronise.  topo: the blocks of a brick (donor halos), else one wall-bounded RANS block `dims` with nState 6.
    Against jm.LevelOperator on the downloaded blocks (2 n eps |B| |x| entry by entry) and the numpy ILU yardsticks (MARGIN)."""
    def setup(enqueue):
        if topo is not None:
            blocks, rblocks = checks.setup_brick(engine, topo, prm, seed)
            pattern = topo.patterns(2)[0]
        else:
            blk, r, _ = checks.setup_block_with_bc(engine, dims, RANS, jm.WALL, seed, stretch_k=2.0)
            blocks, rblocks, pattern = {1: blk}, {1: r}, None
        _KEEP[:] = [rblocks]
        ns = 5 if topo is not None else blocks[1].nw
        n = ns * sum(b.ncells for b in blocks.values())
        rng = np.random.default_rng(seed + 1)
        host = {k: rng.uniform(-1.0, 1.0, n) for k in ("r1", "r2", "x1", "x2")}
        d = {k: dv.put(v) for k, v in host.items()}
        d.update({k: dv.put(np.full(n, 7.0)) for k in ("z1", "z2", "y1", "y2", "y3", "z3")})
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcSetFill(0)
        return dict(blocks=blocks, pattern=pattern, n=n, host=host, d=d)

    def chain(c, link):
        d, n, p = c["d"], c["n"], dv.ptr
        link(engine.setupStateResidualMatrix, 1, True, delta=1e-6)
        link(engine.pcSelect, 0)
        link(engine.pcSetup, 1)
        link(engine.pcSelect, 1)
        link(engine.pcSetFill, 2)
        link(engine.pcSetup, 1)
        link(engine.pcSelect, 0)
        link(engine.pcApplyDev, p(d["r1"]), p(d["z1"]), n, 1, False)
        link(engine.pcSelect, 1)
        link(engine.pcApplyDev, p(d["r2"]), p(d["z2"]), n, 1, True)
        link(engine.jacobianMultDev, p(d["x1"]), p(d["y1"]), n, 1, False)
        link(engine.jacobianMultDev, p(d["y1"]), p(d["y2"]), n, 1, True)
        link(engine.jacobianMultDev, p(d["x2"]), p(d["y3"]), n, 1, False)
        link(engine.pcSelect, 0)
        link(engine.pcApplyDev, p(d["y3"]), p(d["z3"]), n, 1, False)
        return dict(d)

    def after(c):
        return {f"J({nn})": engine.jacobianBlocks(nn).copy() for nn in c["blocks"]}

    try:
        c, enq, syn = both_runs(engine, dv, setup, chain, after)
        what = f"matrix chain {len(c['blocks'])} block(s)"
        for k, v in c["host"].items():
            assert np.array_equal(enq[k], v), (what, k, "an input vector was written")
        op = jm.operator_of(engine, c["blocks"], c["pattern"])
        assert op.n == c["n"] and engine.pcInfo2()[0] == 0
        engine.pcSelect(1)
        assert engine.pcInfo2()[:2] == (2, pcf.ENTRIES[2])
        engine.pcSelect(0)
        refs, bars = [], []
        # the factors: at most MARGIN x as far from the longdouble result as the float64 numpy run is
        ilu = {0: (pc.NumpyILU0(op, np.float64), pc.NumpyILU0(op, np.longdouble)), 2: pcf.yardsticks(op, 2)}
        for out, rhs, fill, tr in (("z1", enq["r1"], 0, False), ("z2", enq["r2"], 2, True), ("z3", enq["y3"], 0, False)):
            f64, fld = ilu[fill]
            zl = fld.apply(rhs, tr)
            e_np = float(np.abs(f64.apply(rhs, tr).astype(np.longdouble) - zl).max())
            e_lib = float(np.abs(enq[out].astype(np.longdouble) - zl).max())
            print(f"{what} {out} (fill {fill}, transpose={tr}): max|z - z_ld| = {e_lib:.3e}, float64 numpy {e_np:.3e} (bar {pc.MARGIN:.0f} x), "
                  f"max|z| = {float(np.abs(zl).max()):.3e}")
            assert e_lib <= pc.MARGIN * e_np, (what, out, e_lib, e_np)
            refs.append((out, np.asarray(zl, dtype=np.float64), pc.MARGIN * e_np))
        # the products: 2 n eps (|B| |x|) entry by entry
        nst = op.st.shape[0] * op.ns
        for out, x, tr in (("y1", enq["x1"], False), ("y2", enq["y1"], True), ("y3", enq["x2"], False)):
            ref, bound = op.apply(x, tr), 2 * nst * EPS * op.apply(x, tr, absolute=True)
            err = np.abs(enq[out] - ref)
            print(f"{what} {out} transpose={tr}: max|y - y_np| = {err.max():.3e}, largest err / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}, "
                  f"max|y| = {np.abs(ref).max():.3e}")
            assert (err <= bound).all() and np.abs(ref).max() > 0.0, (what, out)
            refs.append((out, ref, float(bound.max())))
        order = {k: m for m, k in enumerate(("z1", "z2", "y1", "y2", "y3", "z3"))}
        refs.sort(key=lambda t: order[t[0]])
        assert_links_distinct(what, [r for _, r, _ in refs], [b for _, _, b in refs])
        assert_bitwise(what, enq, syn)
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcSetFill(0)
            engine.pcRelease()
        engine.releaseWorkspace()


# ---- 7. caller's host arrays ------------------------------------------------------------------------------------------------------
def wall_distance_start(engine, dims, seed=83):
    """check_wall_distance's general case on a RANS block, up to the reference's d2Wall; nothing of it handed to the engine yet"""
    from adflow_amd.synth import make_block
    checks.new_level(engine)
    prm = FlowParams(equations=RANSEquations).replace(currentLevel=1, groundLevel=1)
    blk = make_block(*dims, prm, seed=seed, stretch_k=2.0)
    engine.set_options(prm)
    engine.register(blk, nn=1, level=1)
    return checks.wall_distance_case(blk, prm, np.random.default_rng(seed), dims)


def _enqueue_evaluations(engine, n):
    for _ in range(n):
        engine.blocketteRes(1, True, True, True)


def check_update_wall_distances_consumes_xsurf(engine, dv, dims, n_evals=3):
    """enqueue-only, with residual evaluations of the block already in the queue: update_wall_distances(xSurf in pinned memory), and
    the caller overwrites xSurf with NaN as soon as the call returns -- as the reference refills it every warp.  d2Wall against
    check_wall_distance's reference."""
    blk, ind, uv, xSurf, r = wall_distance_start(engine, dims)
    engine.registerWallAssociation(ind, uv)
    engine.upload_coordinates(1, 1)
    mine = dv.pinned(xSurf)
    dv.sync()
    with enqueue_only(engine):
        _enqueue_evaluations(engine, n_evals)
        engine.updateWallDistancesQuickly(mine, 1)
        mine[...] = np.nan
    e = checks.assert_wall_distance(engine, r, ind)
    print(f"update_wall_distances, xSurf overwritten at return, {dims}: d2Wall error {e:.3e} (bar {TOL:.0e})")


def check_wall_distance_register_consumes_its_arrays(engine, dv, dims, n_evals=3):
    """the same for the two arrays of wall_distance_register: surfNodeIndices zeroed (no association anywhere) and uv set to NaN as
    soon as the call returns"""
    blk, ind, uv, xSurf, r = wall_distance_start(engine, dims)
    my_ind, my_uv = dv.pinned(ind), dv.pinned(uv)
    assert my_ind.dtype == np.int32 and my_ind.flags["F_CONTIGUOUS"] and my_uv.flags["F_CONTIGUOUS"]
    dv.sync()
    with enqueue_only(engine):
        _enqueue_evaluations(engine, n_evals)
        engine.registerWallAssociation(my_ind, my_uv)
        my_ind[...] = 0
        my_uv[...] = np.nan
    engine.upload_coordinates(1, 1)
    engine.updateWallDistancesQuickly(xSurf, 1)
    e = checks.assert_wall_distance(engine, r, ind)
    print(f"wall_distance_register, both arrays overwritten at return, {dims}: d2Wall error {e:.3e} (bar {TOL:.0e})")


# ---- 2. mixed hot-path chain on one level ---------------------------------------------------------------------------------------
def _dw_of_vector(blk, prm, vec):
    """dw of the owned cells from the vector ank_get_r hands out (dw / volRef, turbulence x turbResScale), for checks.assert_dw"""
    ns = vec.size // blk.ncells
    res = np.transpose(vec.reshape(blk.nz, blk.ny, blk.nx, ns), (2, 1, 0, 3)) * blk.owned("volRef")[..., None]
    if ns > 5:
        res[..., 5] /= prm.turbResScale
    dw = np.zeros(blk["w"].shape[:3] + (ns,), order="F")
    owned(blk, dw)[...] = res
    return dw


def check_hot_path_chain(engine, dv, dims, seed=107):
    """time_step, block_res (closures, halo, flow, turbulence) at the block's state A, ank_set_w_dev of a second state B, block_res with
    DISS_APPROX | VISC_APPROX | TURB_FIRST_ORDER (the guards), block_res plain again; dw taken into a device vector of its own by
    ank_get_r_dev after each evaluation.  Each against the reference's blockResCore for that state and those flags (the references of
    check_block_res / check_block_res_approx) with checks.assert_dw; the third bit for bit what a fresh engine gives for state B (the
    pattern of check_assembly_leaves_no_trace, nothing synchronised in between)."""
    from oracle import ref
    C = capi.ANK_COUPLED
    first = {}

    def start():
        blk, r, prm = checks.setup_block_with_bc(engine, dims, RANS2, jm.WALL, seed, stretch_k=2.0)
        _KEEP[:] = [r]
        return blk, r, prm

    def setup(enqueue):
        blk, r, prm = start()
        wA = ank.owned_vector({1: blk}, "w", blk.nw)
        wB = wA * (1.0 + 1e-3 * np.random.default_rng(seed + 1).uniform(-1.0, 1.0, wA.size))
        if enqueue:
            R = ank.RefResidual(r, prm, blk.nw, False)
            refs = []
            for w, approx in ((wA, False), (wB, True), (wB, False)):
                R.prepare(w)
                if not refs:
                    R.freeze_sensor()                                      # referenceShockSensor at state A
                if approx:
                    ref.load().ref_set_int(b"orderTurb", firstOrder)
                try:
                    ref.block_res_core(True, True, True, diss_approx=approx, visc_approx=approx)
                finally:
                    ref.load().ref_set_int(b"orderTurb", prm.orderTurb)
                refs.append(r["dw"].copy(order="F"))
            first["refs"] = refs
            # (links 1 and 2 share state B by design and blockResCore's Roe flux does not read dissApprox: they differ in the viscous
            # and the turbulence entries only, so the condition is taken over the variables together, each scaled by its maximum)
            scaled = [np.stack([owned(blk, d[..., l]) / np.abs(owned(blk, refs[0][..., l])).max() for l in range(blk.nw)]) for d in refs]
            assert_links_distinct("hot-path chain", scaled, [TOL * np.abs(c).max() for c in scaled])
        n = wA.size
        return dict(blk=blk, prm=prm, n=n, wB=wB, d_wB=dv.put(wB), d_r=[dv.put(np.full(n, 7.0)) for _ in range(3)])

    def evaluate(**fl):
        engine.blocketteRes(1, updateIntermed=True, flowRes=True, turbRes=True, halo=True, closures=True, **fl)

    def chain(c, link):
        n, d_r = c["n"], c["d_r"]
        link(engine.timeStep, 1)
        link(engine.referenceShockSensor, 1)
        link(evaluate)
        link(engine.ankGetRDev, dv.ptr(d_r[0]), n, C)
        link(engine.ankSetWDev, dv.ptr(c["d_wB"]), n, C)
        link(evaluate, dissApprox=True, viscApprox=True, turbFirstOrder=True)
        link(engine.ankGetRDev, dv.ptr(d_r[1]), n, C)
        link(evaluate)
        link(engine.ankGetRDev, dv.ptr(d_r[2]), n, C)
        return {f"r{m}": v for m, v in enumerate(d_r)}

    c, enq, syn = both_runs(engine, dv, setup, chain)
    blk, prm = c["blk"], c["prm"]
    what = f"hot-path chain {dims}"
    for m, name in enumerate(("state A", "state B, approximate + first-order turbulence", "state B")):
        checks.assert_dw(blk, _dw_of_vector(blk, prm, enq[f"r{m}"]), first["refs"][m], blk.nw, what=f"{what}: {name}")
        e = max(rel_err(owned(blk, _dw_of_vector(blk, prm, enq[f"r{m}"])[..., l]), owned(blk, first["refs"][m][..., l])) for l in range(blk.nw))
        print(f"{what}: {name}: largest error against the reference {e:.3e} (bar {TOL:.0e})")
    assert not np.array_equal(enq["r1"], enq["r2"]), "the flags do not reach the evaluation"
    assert_bitwise(what, enq, syn)
    # a fresh engine state: B written, two plain evaluations (the first stands where the chain had the approximate one: an
    # evaluation's whalo2 re-forms the owned energy from the pressure whatever its flags are)
    start()
    engine.ankSetW(c["wB"], coupled=True)
    evaluate()
    evaluate()
    fresh = engine.ankGetR(coupled=True)
    assert np.array_equal(enq["r2"], fresh), (what, "the plain evaluation after the flagged one against a fresh engine",
                                             float(np.abs(enq["r2"] - fresh).max()))
    print(f"{what}: the third evaluation is bit-equal to a fresh engine's")


# ---- 6. mesh-warp chain ------------------------------------------------------------------------------------------------------------
def check_mesh_warp_chain(engine, dims, seed=81):
    """upload_coordinates, xhalo, exchange_coor, update_geometry, update_wall_distances, block_res enqueue-only after the owned nodes
    moved: x, vol, sI, sJ, sK against the reference's xhalo_block / volume_block / metric_block (checks._assert_geometry, the bar of
    check_update_geometry), d2Wall against updateWallDistancesQuickly (checks.assert_wall_distance), dw against blockResCore on the
    warped block (checks.assert_dw, the bar of check_block_res); all of them bit for bit against the synchronised run."""
    from oracle import ref
    from adflow_amd.synth import make_block, make_bocos
    from adflow_amd.topology import CommPattern
    first = {}
    names = {"x": capi.ARR_X, "vol": capi.ARR_VOL, "sI": capi.ARR_SI, "sJ": capi.ARR_SJ, "sK": capi.ARR_SK, "d2Wall": capi.ARR_D2WALL}

    def setup(enqueue):
        checks.new_level(engine)
        prm = RANS.replace(currentLevel=1, groundLevel=1)
        blk = make_block(*dims, prm, seed=seed, stretch_k=2.0)
        faces, nvisc = make_bocos(blk, prm, jm.WALL, seed=seed + 1)
        engine.set_options(prm)
        engine.register(blk, nn=1, level=1)
        engine.bc_register(faces, nvisc, nn=1, level=1)
        empty = CommPattern()
        for L in (0, 1, 2):
            engine.comm_register(1, L, empty)
        rng = np.random.default_rng(seed)
        nsurf = 57
        ind = np.asfortranarray(rng.integers(1, nsurf + 1, size=(4, blk.nx, blk.ny, blk.nz), dtype=np.int32))
        ind[0][rng.uniform(size=ind.shape[1:]) < 0.1] = 0
        uv = np.asfortranarray(rng.uniform(0.0, 1.0, size=(2, blk.nx, blk.ny, blk.nz)))
        xSurf = rng.uniform(-0.2, 1.2, size=3 * nsurf)
        engine.registerWallAssociation(ind, uv)
        checks._warp_owned_nodes({1: blk}, seed)
        if enqueue:
            r = blk.copy()
            rfaces = [dict(f, norm=f["norm"].copy(order="F")) for f in faces]
            ref.alloc_doms(1, 1)
            ref.bind_block(r, prm)
            ref.set_bocos(rfaces, nvisc)
            ref.call("xhalo_block")
            ref.call("volume_block")
            ref.call("metric_block")
            ref.call("boundaryNormals")
            r["d2Wall"][...] = -1.0
            ref.update_wall_distances(ind, uv, xSurf)
            ref.block_res_core(True, True, True)
            first.update(r=r, ind=ind)
            _KEEP[:] = [r, rfaces]
        return dict(blk=blk, xSurf=xSurf)

    def chain(c, link):
        link(engine.upload_coordinates, 1, 1)
        link(engine.xhalo, 1)
        link(engine.exchangeCoor, 1)
        link(engine.update_geometry, 1)
        link(engine.updateWallDistancesQuickly, c["xSurf"], 1)
        link(engine.blocketteRes, 1, True, True, True)
        return {}

    def after(c):
        out = {n: engine.download_array(which, np.zeros_like(c["blk"][n]), 1, 1) for n, which in names.items()}
        out["dw"] = engine.download_residual(1, 1).copy(order="F")
        return out

    c, enq, syn = both_runs(engine, _NoVectors(), setup, chain, after)
    blk, r = c["blk"], first["r"]
    what = f"mesh-warp chain {dims}"
    checks._assert_geometry(engine, {1: blk}, {1: r}, what)
    e_wd = checks.assert_wall_distance(engine, r, first["ind"])
    checks.assert_dw(blk, enq["dw"], r["dw"], blk.nw, what=f"{what}: dw")
    e_dw = max(rel_err(owned(blk, enq["dw"][..., l]), owned(blk, r["dw"][..., l])) for l in range(blk.nw))
    e_geo = max(rel_err(enq[n][1:-1, 1:-1, 1:-1] if n == "vol" else enq[n], r[n][1:-1, 1:-1, 1:-1] if n == "vol" else r[n])
                for n in ("x", "vol", "sI", "sJ", "sK"))
    print(f"{what}: largest error against the reference: geometry {e_geo:.3e}, d2Wall {e_wd:.3e}, dw {e_dw:.3e} (bar {TOL:.0e})")
    assert_bitwise(what, enq, syn)


class _NoVectors:
    """a chain without device vectors of the test's own"""

    def sync(self):
        pass


# ---- 5. the ANK step, flow and turbulence --------------------------------------------------------------------------------------------
def _scramble_dtl(engine, blk):
    """dtl on the device made useless: a T formed from it is far from the formula's"""
    bad = np.full((blk.ie, blk.je, blk.ke), 1.0e30, order="F")
    engine.upload_array(capi.ARR_DTL, bad, 1, 1)


def check_ank_flow_chain(engine, dv, dims, cap, seed=331):
    """the flow update in the order of INTEGRATION.md: time_step, ank_time_step, fd_jacobian(PC | FROZEN_TURB | USE_AD), ank_pc_setup,
    reference_shock_sensor, ank_set_base_dev, ank_get_r_dev, ank_mult_dev with v1, with v = 0 (y exactly zero, ank_last_h 0), with v2,
    ank_solve_dev, ank_physicality_check_dev, ank_set_w_dev, ank_unsteady_res_dev without and with its norm.  One wall-bounded RANS
    block with the scalar dissipation (ank_checks' scheme for this flavour), decoupled (nState 5), the approximate flavour.  Yardsticks: ank_checks' for each call on its own."""
    rtol, omega = 1e-4, 0.7
    F = engine._ankFlags(dissApprox=True, viscApprox=True)
    first = {}

    def setup(enqueue):
        blk, r, prm = checks.setup_block_with_bc(engine, dims, ank.RANS_JST, jm.WALL, seed, stretch_k=2.0)
        _KEEP[:] = [r]
        for s in (1, 0):
            engine.pcSelect(s)
        w0 = ank.state_vector(engine, {1: blk}, 5)
        n = w0.size
        rng = np.random.default_rng(seed + 1)
        host = dict(w0=w0, v1=rng.uniform(-1.0, 1.0, n), v0=np.zeros(n), v2=rng.uniform(-1.0, 1.0, n),
                    wls=w0 * (1.0 + 1e-3 * rng.uniform(-1.0, 1.0, n)))
        # T from the formula needs the dtl and the state ank_time_step reads: from a time step of the same state up front, in BOTH runs
        # (they start from the same device state); then dtl is scrambled on the device, so that the chain's own time_step has to run in
        # front of its ank_time_step
        engine.timeStep(1)
        Tn = ank.numpy_T(engine, {1: blk}, prm, False)
        _scramble_dtl(engine, blk)
        if enqueue:
            first["Tn"] = Tn
            R = ank.RefResidual(r, prm, 5, True)
            R.r0 = R(w0, freeze=True)
            first["R"] = R
        d = {k: dv.put(v) for k, v in host.items()}
        d.update({k: dv.put(np.full(n, 7.0)) for k in ("b", "y1", "y0", "y2", "x", "u1", "u2")})
        return dict(blk=blk, prm=prm, n=n, host=host, d=d)

    def chain(c, link):
        d, n, p = c["d"], c["n"], dv.ptr
        out = dict(d)
        link(engine.timeStep, 1)
        link(engine.ankTimeStep, ank.CFL, ank.TURB_CFL_SCALE, False)
        link(engine.setupStateResidualMatrix, 1, True, frozenTurb=True, useAD=True)
        link(engine.ankPcSetup, 1)
        link(engine.referenceShockSensor, 1)
        link(engine.ankSetBaseDev, p(d["w0"]), n, F)
        link(engine.ankGetRDev, p(d["b"]), n, 0)
        link(engine.ankMultDev, p(d["v1"]), p(d["y1"]), n)
        link(engine.ankMultDev, p(d["v0"]), p(d["y0"]), n)
        out["h0"] = link(engine.ankLastH)
        link(engine.ankMultDev, p(d["v2"]), p(d["y2"]), n)
        out["h2"] = link(engine.ankLastH)
        out["solve"] = link(engine.ankSolveDev, p(d["b"]), p(d["x"]), n, 1, restart=cap, maxIts=cap, rtol=rtol)
        out["lambda"] = link(engine.ankPhysicalityCheckDev, p(d["w0"]), p(d["x"]), n, 0)
        link(engine.ankSetWDev, p(d["wls"]), n, 0)
        out["nrm1"] = link(engine.ankUnsteadyResDev, p(d["x"]), omega, p(d["u1"]), n, 0, norm=False)
        link(engine.ankSetWDev, p(d["wls"]), n, 0)
        out["nrm2"] = link(engine.ankUnsteadyResDev, p(d["x"]), omega, p(d["u2"]), n, 0, norm=True)
        return out

    def after(c):
        return {"T": engine.ankTimeStepBlocks(1, False), "dw": engine.download_residual(1, 1).copy(order="F"),
                "J": engine.jacobianBlocks(1).copy()}

    try:
        c, enq, syn = both_runs(engine, dv, setup, chain, after)
        blk, prm, w0, Tn, R = c["blk"], c["prm"], c["host"]["w0"], first["Tn"], first["R"]
        what = f"ANK flow chain {dims}"
        for k, v in c["host"].items():
            assert np.array_equal(enq[k], v), (what, k, "an input vector was written")
        ank.assert_T_block(enq["T"], Tn[1], what)
        op = jm.operator_of(engine, {1: blk})
        assert op.ns == 5
        ops = ank.shifted(op, Tn)
        pc.assert_apply_matches(engine, ops, seed + 2, f"{what}: shifted factor")
        b = enq["b"]
        e_b = float(np.abs(b - R.r0).max() / np.abs(R.r0).max())
        print(f"{what}: base residual against the reference {e_b:.3e} (bar 1e-09)")
        assert e_b <= 1e-9
        quotient = lambda h, v: (R(w0 + h * v) - R.r0) / h
        h1, h2 = ank.ds_step(w0, enq["v1"]), ank.ds_step(w0, enq["v2"])       # (ank_last_h keeps the last product's only)
        y1r, bar1, _ = ank.assert_product(f"{what}: product 1", enq["y1"], enq["v1"], h1, op, Tn, blk, quotient)
        y2r, bar2, _ = ank.assert_product(f"{what}: product 3", enq["y2"], enq["v2"], h2, op, Tn, blk, quotient)
        assert abs(enq["h2"] - h2) <= 1e-12 * abs(h2), (enq["h2"], h2)
        assert not enq["y0"].any() and enq["h0"] == 0.0, (what, "v = 0", enq["h0"])
        assert_links_distinct(what, [y1r, np.zeros_like(y1r), y2r], [bar1, 0.0, bar2])
        its, r0n, rn = enq["solve"]
        ank.assert_solve(f"{what}: solve", its, r0n, b, enq["x"], ops, cap, rtol)
        lam_np, x_np, _ = ank.numpy_physicality(w0, enq["x"], 5, False, 1.0, 0.2, 0.99, 1.0, 0.01)
        assert abs(enq["lambda"] - lam_np) <= 4 * EPS * abs(lam_np), (enq["lambda"], lam_np)
        assert enq["nrm1"] is None and np.array_equal(enq["u1"], enq["u2"]), (what, "the line-search residual with and without its norm")
        ankt.assert_unsteady(f"{what}: line-search residual", enq["u2"], enq["nrm2"], enq["dw"], blk, prm, Tn, enq["x"], omega, "flow")
        assert_bitwise(what, enq, syn)
    finally:
        engine.pcRelease()
        engine.ankRelease()
        engine.releaseWorkspace()


def check_ank_turb_chain(engine, dv, dims, cap, seed=409):
    """the turbulence update with ADFLOW_ANK_TURB in slot 1 while slot 0 keeps the flow factor, ank_select_base switching between the
    two bases inside the chain: the flow front (time steps, flow assembly, shifted flow factor in slot 0, flow base), then turbulence
    time step, assembly (TURB_ONLY | APPROX_SA | USE_AD), ank_pc_setup in slot 1, turbulence base, ank_get_r_dev, a turbulence product,
    the turbulence state back, select flow: a flow product, select turbulence: solve, step limiter (entries clipped in place), state
    write, line-search residual without and with its norm.  Yardsticks: ank_turb_checks' for each call on its own; the flow factor
    and the flow product against ank_checks' on the flow matrix assembled again afterwards at the same state."""
    rtol, omega = 1e-4, 0.7
    T = capi.ANK_TURB
    FT = engine._ankFlags(turb=True, approxSA=True)
    FF = engine._ankFlags(dissApprox=True, viscApprox=True)
    first = {}

    def setup(enqueue):
        blk, r, prm = ankt.setup(engine, dims, seed, ank.RANS_JST)
        for s in (1, 0):
            engine.pcSelect(s)
        engine.download_state(1, 1)
        start = {name: blk[name].copy() for name in ("w", "p", "rlv", "rev")}
        w5, wt = ank.owned_vector({1: blk}, "w", 5), ankt.turb_vector({1: blk})
        n5, n1 = w5.size, wt.size
        rng = np.random.default_rng(seed + 1)
        dwt = -1e-3 * rng.uniform(0.1, 1.0, n1) * wt
        dwt[5], dwt[n1 - 7], dwt[n1 // 2] = 200.0 * wt[5], 1e4 * wt[n1 - 7], 3.0 * wt[n1 // 2]      # clipped, clipped, limits
        host = dict(w5=w5, wt=wt, v5=rng.uniform(-1.0, 1.0, n5), vt=rng.uniform(-1.0, 1.0, n1), dwt0=dwt,
                    wtls=wt * (1.0 + 1e-3 * rng.uniform(-1.0, 1.0, n1)))
        engine.timeStep(1)                                                 # (as in check_ank_flow_chain)
        Tn, Tt = ank.numpy_T(engine, {1: blk}, prm, False), ankt.numpy_T_turb(engine, {1: blk}, prm)
        _scramble_dtl(engine, blk)
        if enqueue:
            first["Tn"], first["Tt"] = Tn, Tt
            Rt = ankt.RefTurbResidual(r, prm)
            with ankt.ref_approx_sa(True):
                Rt.r0 = Rt(wt)
            first["Rt"] = Rt
        d = {k: dv.put(v) for k, v in host.items()}
        d["dwt"] = dv.put(dwt)
        d.update({k: dv.put(np.full(n5, 7.0)) for k in ("b5", "y5")})
        d.update({k: dv.put(np.full(n1, 7.0)) for k in ("bt", "yt", "xt", "u1", "u2")})
        return dict(blk=blk, r=r, prm=prm, n5=n5, n1=n1, host=host, d=d, start=start)

    def chain(c, link):
        d, n5, n1, p = c["d"], c["n5"], c["n1"], dv.ptr
        out = dict(d)
        link(engine.timeStep, 1)
        link(engine.ankTimeStep, ank.CFL, ank.TURB_CFL_SCALE, False)
        link(engine.setupStateResidualMatrix, 1, True, frozenTurb=True, useAD=True)
        link(engine.pcSelect, 0)
        link(engine.ankPcSetup, 1)
        link(engine.referenceShockSensor, 1)
        link(engine.ankSetBaseDev, p(d["w5"]), n5, FF)
        link(engine.ankGetRDev, p(d["b5"]), n5, 0)
        link(engine.ankTimeStep, ank.CFL, ank.TURB_CFL_SCALE, False, 1, True)
        link(engine.setupStateResidualMatrix, 1, True, useTurbOnly=True, useAD=True, approxSA=True)
        link(engine.pcSelect, 1)
        link(engine.ankPcSetup, 1)
        link(engine.ankSetWDev, p(d["w5"]), n5, 0)                         # pressure and laminar viscosity of the flow state
        link(engine.ankSetBaseDev, p(d["wt"]), n1, FT)
        link(engine.ankGetRDev, p(d["bt"]), n1, T)
        link(engine.ankMultDev, p(d["vt"]), p(d["yt"]), n1)
        out["ht"] = link(engine.ankLastH)
        link(engine.ankSetWDev, p(d["wt"]), n1, T)                         # (the product left nuTilde perturbed)
        link(engine.ankSelectBase, False)
        link(engine.ankMultDev, p(d["v5"]), p(d["y5"]), n5)
        link.refused("factor was set up for nState = 1", engine.ankSolveDev, p(d["b5"]), p(d["y5"]), n5, 1)     # slot 1 is the turbulence factor
        link(engine.ankSetWDev, p(d["w5"]), n5, 0)
        link(engine.ankSelectBase, True)
        out["solve"] = link(engine.ankSolveDev, p(d["bt"]), p(d["xt"]), n1, 1, restart=cap, maxIts=cap, rtol=rtol)
        out["lambda"] = link(engine.ankPhysicalityCheckDev, p(d["wt"]), p(d["dwt"]), n1, T)
        link(engine.ankSetWDev, p(d["wtls"]), n1, T)
        out["nrm1"] = link(engine.ankUnsteadyResDev, p(d["xt"]), omega, p(d["u1"]), n1, FT, norm=False)
        link(engine.ankSetWDev, p(d["wtls"]), n1, T)
        out["nrm2"] = link(engine.ankUnsteadyResDev, p(d["xt"]), omega, p(d["u2"]), n1, FT, norm=True)
        return out

    def after(c):
        return {"T": engine.ankTimeStepBlocks(1, False), "Tt": engine.ankTimeStepBlocks(1, turb=True),
                "dw": engine.download_residual(1, 1).copy(order="F"), "Jt": engine.jacobianBlocks(1).copy()}

    try:
        c, enq, syn = both_runs(engine, dv, setup, chain, after)
        blk, prm, wt, w5 = c["blk"], c["prm"], c["host"]["wt"], c["host"]["w5"]
        Tn, Tt, Rt = first["Tn"], first["Tt"], first["Rt"]
        what = f"ANK turbulence chain {dims}"
        for k, v in c["host"].items():
            assert np.array_equal(enq[k], v), (what, k, "an input vector was written")
        ankt.assert_T_turb_block(enq["Tt"], Tt[1], blk, what)
        ank.assert_T_block(enq["T"], Tn[1], what)
        opt = jm.operator_of(engine, {1: blk})
        assert opt.ns == 1
        opts = ank.shifted(opt, Tt)
        engine.pcSelect(1)
        pc.assert_apply_matches(engine, opts, seed + 2, f"{what}: shifted turbulence factor, slot 1")
        bt = enq["bt"]
        e_b = float(np.abs(bt - Rt.r0).max() / np.abs(Rt.r0).max())
        print(f"{what}: base residual against the reference {e_b:.3e} (bar 1e-09)")
        assert e_b <= 1e-9

        def quotient(h, v):
            with ankt.ref_approx_sa(True):
                return (Rt(wt + h * v) - Rt.r0) / h
        ht = ank.ds_step(wt, enq["vt"])
        ank.assert_product(f"{what}: turbulence product", enq["yt"], enq["vt"], enq["ht"], opt, Tt, blk, quotient)
        assert abs(enq["ht"] - ht) <= 1e-12 * abs(ht), (enq["ht"], ht)
        its, r0n, rn = enq["solve"]
        ank.assert_solve(f"{what}: solve", its, r0n, bt, enq["xt"], opts, cap, rtol)
        lam_np, dwt_np, clip = ankt.numpy_physicality_turb(wt, c["host"]["dwt0"], 1.0, 0.99, 1.0, 0.01)
        assert enq["lambda"] == lam_np and 0.0 < lam_np < 1.0 and clip.sum() == 2, (enq["lambda"], lam_np, clip.sum())
        assert np.array_equal(enq["dwt"], dwt_np), (what, "the clipped update")
        assert enq["nrm1"] is None and np.array_equal(enq["u1"], enq["u2"]), (what, "the line-search residual with and without its norm")
        ankt.assert_unsteady(f"{what}: line-search residual", enq["u2"], enq["nrm2"], enq["dw"], blk, prm, Tt, enq["xt"], omega, "turb")
        assert_bitwise(what, enq, syn)
        # slot 0 kept the flow factor, and the flow product taken between the turbulence calls: against the flow matrix of the same
        # state, assembled again now (the turbulence assembly replaced it on the device)
        for name, a in c["start"].items():
            blk[name][...] = a
        engine.upload_state(1, 1)
        engine.setupStateResidualMatrix(1, True, frozenTurb=True, useAD=True)
        op5 = jm.operator_of(engine, {1: blk})
        assert op5.ns == 5
        engine.pcSelect(0)
        pc.assert_apply_matches(engine, ank.shifted(op5, Tn), seed + 3, f"{what}: shifted flow factor, slot 0, after the turbulence calls")
        R5 = ank.RefResidual(c["r"], prm, 5, True)
        R5.r0 = R5(w5, freeze=True)
        e_b = float(np.abs(enq["b5"] - R5.r0).max() / np.abs(R5.r0).max())
        assert e_b <= 1e-9, e_b
        ank.assert_product(f"{what}: flow product after ank_select_base", enq["y5"], enq["v5"], ank.ds_step(w5, enq["v5"]), op5, Tn, blk,
                           lambda h, v: (R5(w5 + h * v) - R5.r0) / h)
    finally:
        for s in (1, 0):
            engine.pcSelect(s)
            engine.pcRelease()
        engine.ankRelease()
        engine.releaseWorkspace()
