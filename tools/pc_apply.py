#!/usr/bin/env python
"""The block ILU(fill) preconditioner alone (adflow_gpu_pc_setup / adflow_gpu_pc_apply_dev), timed with HIP events: the RANS Roe
preconditioner matrix (7-point, forward-mode assembly) on one 160 x 128 x 64 wall-bounded block.  Prints ms for the setup, ms for
z = M^-1 r and z = M^-T r, ms for y = J x with the same matrix in the same run (one launch over the 7-point bytes: the yardstick),
the byte floor (7, 13 or 23 nState^2 x 8 B per owned cell), TB/s and launches per application; then GMRES on the preconditioner
matrix itself: iterations and ms to reduce the residual by --rtol (default 1e-8).
--nvec N adds, in the same process: Z = M^-1 R and M^-T R for N columns through adflow_gpu_pc_apply_multi_dev (one call) against N
calls of adflow_gpu_pc_apply_dev, with the time per launch and the GB/s on the factor of the multi call, and the wall time of GMRES
for N right-hand sides through adflow_gpu_gmres_solve_multi_dev against N calls of adflow_gpu_gmres_solve_dev.
--mg L [--nsmooth N --fill-coarse F] makes the setup a multigrid hierarchy of L levels (adflow_gpu_pc_set_mg: the cycle of amg.F90,
N Richardson iterations of the ILU smoother per level, fill F below the first level): the same lines, with the cells of every level,
the bytes the hierarchy holds and the launches of one cycle; floor_bytes is then one pass over the matrix and the factor of every
level per smoothing iteration.  Without --mg nothing changes.
--brick Bi Bj Bk builds the matrix on Bi x Bj x Bk blocks of nx x ny x nz with wall / symmetry / farfield on the outside of the brick and
1-to-1 interfaces inside (the benchmark's layout); --coupled (fill 0, no --mg) then runs every line twice in the same process, with
one ILU subdomain per block (adflow_gpu_pc_set_coupled(0)) and with one for the level (1): setup, both applications with launches,
level sets, microseconds per launch and GB/s on the factor bytes, and GMRES.
--level-fill F (0 .. 3, also with --brick) runs the same lines three times in the same process: the block-local factor of fill F
(F <= 2), the coupled fill-0 factor, and the ILU(F) over the whole level (adflow_gpu_pc_set_level_fill: longest row, entries of the
pattern, level sets, whether the timed setup kept the tables; GB/s on the bytes of the pattern's blocks).
--outer-its N --inner-its N [--inner-its-coarse N] (adflow_gpu_pc_set_its: the Richardson iterations of setupStandardKSP around the
factor; each takes one count or a comma-separated list, and every combination runs on the same assembly in the same process) prints
the same lines, with the launches of one application counted from the recurrences, plus -- when outer > 1 -- the ms of one residual
pass t = b - A x over the owned copy of the 7-point matrix (with the update y += z that follows it), taken as the difference to the
same factor at outer = 1 set up in the same run, beside the y = J x line of the same matrix.
--ordering natural|rcm|redblack|FILE (with --level-fill; adflow_gpu_pc_set_ordering) runs the ILU over the level alone, in that
ordering: redblack (cells sorted by the parity of global i + j + k, stably) and FILE (one 0-based cell number of the PETSc layout per
line, perm[new] = old) go through the caller's permutation.  The setup line then carries the ordering, level sets, entries, bandwidth
and bytes, and the wall ms of the FIRST setup (ordering, symbolic factorisation, tables, allocation, numbers) beside the timed one,
which keeps the tables.
usage: pc_apply.py [--fill 0|1|2] [--mg L [--nsmooth N] [--fill-coarse F]] [--rtol 1e-8] [--nvec N] [--brick Bi Bj Bk] [--coupled]
       [--level-fill F [--ordering natural|rcm|redblack|FILE]] [--outer-its N[,N..]] [--inner-its N[,N..]] [--inner-its-coarse N]
       [n] [nx ny nz]      (n timed applications of each kind, default 10)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adflow_amd.engine import Engine  # noqa: E402
from adflow_amd.params import FlowParams, RANSEquations, upwind, vanAlbeda  # noqa: E402
from adflow_amd.synth import make_block, make_bocos  # noqa: E402
from adflow_amd.topology import BrickTopology, CommPattern, apply_local_copies_fast  # noqa: E402

WALL = {1: -6, 2: -6, 3: -1, 4: -1, 5: -3, 6: -6}
ITS = [1, 1, 1]           # the iterations the slot is set to (--outer-its, --inner-its, --inner-its-coarse)


def main():
    import torch
    argv, fill, rtol, nvec = list(sys.argv[1:]), 0, 1e-8, 0
    mg, nsmooth, fillc, level_fill, ordering = 1, 1, 0, None, None
    outers, inners, inner_coarse = [1], [1], 1
    brick, both = None, "--coupled" in argv
    if both:
        argv.remove("--coupled")
    if "--brick" in argv:
        at = argv.index("--brick")
        brick = tuple(int(a) for a in argv[at + 1:at + 4])
        del argv[at:at + 4]
    for opt in ("--fill", "--rtol", "--nvec", "--mg", "--nsmooth", "--fill-coarse", "--level-fill", "--outer-its", "--inner-its",
                "--inner-its-coarse", "--ordering"):
        if opt in argv:
            at = argv.index(opt)
            if opt == "--fill":
                fill = int(argv[at + 1])
            elif opt == "--nvec":
                nvec = int(argv[at + 1])
            elif opt == "--mg":
                mg = int(argv[at + 1])
            elif opt == "--nsmooth":
                nsmooth = int(argv[at + 1])
            elif opt == "--fill-coarse":
                fillc = int(argv[at + 1])
            elif opt == "--level-fill":
                level_fill = int(argv[at + 1])
            elif opt == "--ordering":
                ordering = argv[at + 1]
            elif opt == "--outer-its":
                outers = [int(a) for a in argv[at + 1].split(",")]
            elif opt == "--inner-its":
                inners = [int(a) for a in argv[at + 1].split(",")]
            elif opt == "--inner-its-coarse":
                inner_coarse = int(argv[at + 1])
            else:
                rtol = float(argv[at + 1])
            del argv[at:at + 2]
    n_it = int(argv[0]) if len(argv) > 0 else 10
    dims = tuple(int(a) for a in argv[1:4]) if len(argv) > 3 else (160, 128, 64)
    eng = Engine(0)
    prm = FlowParams(equations=RANSEquations, spaceDiscr=upwind, limiter=vanAlbeda).replace(currentLevel=1, groundLevel=1)
    eng.release_all()
    eng.set_options(prm)
    if ordering is not None and level_fill is None:
        sys.exit("--ordering: an ordering of the ILU over the level; give --level-fill")
    if brick:
        cells = register_brick(eng, BrickTopology(*brick, *dims, periodic=(False,) * 3), prm)
    else:
        blk = make_block(*dims, prm, seed=7, stretch_k=2.0)
        faces, nvisc = make_bocos(blk, prm, WALL, seed=8)
        eng.register(blk)
        eng.bc_register(faces, nvisc)
        for L in (1, 2):
            eng.comm_register(1, L, CommPattern())
        cells = blk.nx * blk.ny * blk.nz
    eng.applyAllBC(1, True)
    eng.setupStateResidualMatrix(1, True, useAD=True)
    eng.releaseWorkspace()
    ns, st = eng.jacobianInfo()
    n = ns * cells
    for its in [(o, i, inner_coarse) for o in outers for i in inners]:
        if its != (1, 1, 1) or len(outers) * len(inners) > 1:      # (a library without the entry point still serves the defaults)
            eng.pcSetIts(*its)
        ITS[:] = its
        if level_fill is not None:
            if fill or mg > 1 or both:
                sys.exit("--level-fill: runs the block-local factor of that fill and the coupled fill-0 factor itself; no --fill, --mg, --coupled")
            if ordering is not None:
                kind, perm = ordering_of(ordering, brick or (1, 1, 1), dims, cells)
                eng.pcSetLevelFill(level_fill)
                eng.pcSetOrdering(kind, perm)
                one_factor(eng, torch, dims, brick, ns, cells, n, n_it, level_fill, 1, rtol, 0, None, level_fill, ordering)
                eng.pcSetOrdering(0)
                eng.pcSetLevelFill(-1)
                continue
            if level_fill <= 2:
                eng.pcSetFill(level_fill)
                one_factor(eng, torch, dims, brick, ns, cells, n, n_it, level_fill, 1, rtol, 0, 0)
                eng.pcSetFill(0)
            eng.pcSetCoupled(1)
            one_factor(eng, torch, dims, brick, ns, cells, n, n_it, 0, 1, rtol, 0, 1)
            eng.pcSetCoupled(0)
            eng.pcSetLevelFill(level_fill)
            one_factor(eng, torch, dims, brick, ns, cells, n, n_it, level_fill, 1, rtol, 0, None, level_fill)
            eng.pcSetLevelFill(-1)
        elif both:
            if fill or mg > 1:
                sys.exit("--coupled: the factor over the level takes fill 0 and no hierarchy")
            for coupled in (0, 1):
                eng.pcSetCoupled(coupled)
                one_factor(eng, torch, dims, brick, ns, cells, n, n_it, 0, 1, rtol, 0, coupled)
            eng.pcSetCoupled(0)
        else:
            if fill:                                          # (a library without the entry point still serves fill 0)
                eng.pcSetFill(fill)
            if mg > 1:
                eng.pcSetMg(mg, nsmooth, fillc)
            one_factor(eng, torch, dims, brick, ns, cells, n, n_it, fill, mg, rtol, nvec, None)
    eng.releaseWorkspace()
    eng.close()


def ordering_of(name, brick, dims, cells):
    """(kind, permutation or None) of --ordering for adflow_gpu_pc_set_ordering"""
    import numpy as np
    if name in ("natural", "rcm"):
        return ("natural", "rcm").index(name), None
    if name == "redblack":
        # the PETSc layout: block after block (i fastest over the blocks), then k, j, i
        Bi, Bj, Bk = brick
        nx, ny, nz = dims
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        par = np.concatenate([((i + bi * nx) + (j + bj * ny) + (k + bk * nz)).reshape(-1) % 2
                              for bk in range(Bk) for bj in range(Bj) for bi in range(Bi)])
        return 2, np.argsort(par, kind="stable").astype(np.int32)
    perm = np.loadtxt(name, dtype=np.int64, ndmin=1)
    if perm.size != cells:
        sys.exit(f"--ordering {name}: {perm.size} entries, the level has {cells} cells")
    return 2, perm.astype(np.int32)


def register_brick(eng, topo, prm):
    """the blocks of a wall-bounded brick with their boundary subfaces and both patterns on the engine; returns the owned cells"""
    from adflow_amd.synth import set_porosities
    lid = topo.local_ids()
    blocks = {lid[g]: make_block(topo.nx, topo.ny, topo.nz, prm, seed=7 + 17 * g, wall_kmin=False, stretch_k=2.0)
              for g in range(topo.nblocks)}
    bocos = {}
    for g in range(topo.nblocks):
        spec = topo.boundary_spec(g, WALL)
        if spec:
            bocos[lid[g]] = make_bocos(blocks[lid[g]], prm, spec, seed=8 + 31 * g)
        set_porosities(blocks[lid[g]], bocos[lid[g]][0] if lid[g] in bocos else [])
    pats = {L: topo.patterns(L)[0] for L in (1, 2)}
    apply_local_copies_fast(blocks, pats[2])
    for nn, b in blocks.items():
        eng.register(b, nn=nn, level=1)
        if nn in bocos:
            eng.bc_register(*bocos[nn], nn=nn, level=1)
    for L in (1, 2):
        eng.comm_register(1, L, pats[L])
    return sum(b.nx * b.ny * b.nz for b in blocks.values())


def one_factor(eng, torch, dims, brick, ns, cells, n, n_it, fill, mg, rtol, nvec, coupled, level_fill=None, ordering=None):
    """setup, applications and GMRES with the settings of the selected slot as they stand; coupled: None, or the subdomain setting
    the lines name (then with the level sets, the microseconds per launch and the GB/s on the factor bytes); level_fill: None, or the
    fill of the ILU over the level the slot is set to (the same extra figures, the floor from the entries of its pattern)"""
    tag = {} if coupled is None else {"coupled": coupled}
    if level_fill is not None:
        tag["level_fill"] = level_fill
    if brick:
        tag["brick"] = list(brick)
    outer, inner, inner_coarse = ITS
    if ITS != [1, 1, 1]:
        tag["its"] = list(ITS)
    base = None
    if outer > 1:
        # the same factor without the outer loop, in the same run: what the residual pass is the difference to
        eng.pcSetIts(1, inner, inner_coarse)
        eng.pcSetup(1)
        base = {tr: time_apply(eng, torch, n, n_it, tr) for tr in (False, True)}
        eng.pcSetIts(outer, inner, inner_coarse)
    floor = {0: 7, 1: 13, 2: 23}.get(fill, 7) * ns * ns * 8 * cells
    if ordering is not None:
        import time
        tag["ordering"] = ordering
        eng.sync()
        t0 = time.perf_counter()
    eng.pcSetup(1)                                        # warm-up (allocations, tables)
    eng.sync()
    if ordering is not None:
        kind, bandwidth, _, _ = eng.pcOrderingInfo()
        tag.update(ordering_kind=kind, bandwidth=bandwidth, first_setup_wall_ms=round(1e3 * (time.perf_counter() - t0), 1))
    eng.event_record(1)
    eng.pcSetup(1)
    eng.event_record(2)
    eng.sync()
    _, planes, nbytes = eng.pcInfo()
    if level_fill is not None:
        _, max_row, n_entries, _, n_cross, reused = eng.pcLevelInfo()
        floor = n_entries * ns * ns * 8
        tag.update(longest_row=max_row, pattern_entries=n_entries, entries_per_cell=round(n_entries / cells, 2), cross_entries=n_cross,
                   timed_setup_reused_tables=reused)
    print(json.dumps({"what": "pc_setup (tables, allocation, factorisation)", "dims": list(dims), "nState": ns, "ms": round(eng.event_elapsed_ms(1, 2), 3),
                      "fill": fill, "hyperplanes_or_level_sets": planes, "factor_bytes": nbytes, **tag}), flush=True)
    if mg > 1:
        planes, floor = cycle_cost(eng, dims, ns, fill, planes)
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 0.5
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    ms_of = {}
    eng.set_async(True)
    try:
        for what, fn, launches in (("J x", lambda: eng.jacobianMultDev(x.data_ptr(), y.data_ptr(), n, 1, False), 2),
                                   ("M^-1 r", lambda: eng.pcApplyDev(x.data_ptr(), y.data_ptr(), n, 1, False), its_launches(2 * planes, mg)),
                                   ("M^-T r", lambda: eng.pcApplyDev(x.data_ptr(), y.data_ptr(), n, 1, True), its_launches(2 * planes, mg))):
            for _ in range(3):
                fn()
            eng.event_record(1)
            for _ in range(n_it):
                fn()
            eng.event_record(2)
            eng.sync()
            ms = eng.event_elapsed_ms(1, 2) / n_it
            ms_of[what] = ms
            more = dict(tag)
            if (coupled is not None or level_fill is not None) and what != "J x":
                more.update(level_sets=planes, us_per_launch=round(1e3 * ms / launches, 2),
                            GB_per_s_on_the_factor=round(floor / (ms * 1e-3) / 1e9, 1))
            print(json.dumps({"what": what, "ms": round(ms, 4), "floor_bytes": floor, "TB_per_s": round(floor / (ms * 1e-3) / 1e12, 3),
                              "launches": int(launches), "ratio_to_J_x": round(ms / ms_of["J x"], 2),
                              "checksum": float(y.abs().sum().item()), **more}), flush=True)
    finally:
        eng.set_async(False)
    if base:
        pass7 = 7 * ns * ns * 8 * cells
        for tr, what in ((False, "M^-1 r"), (True, "M^-T r")):
            ms = (ms_of[what] - outer * base[tr]) / (outer - 1)
            print(json.dumps({"what": "residual pass t = b - A^T x" if tr else "residual pass t = b - A x", "how": "with y += z; (ms at outer - "
                              "outer x ms at outer 1) / (outer - 1), same factor, same run", "ms": round(ms, 4), "ms_at_outer_1": round(base[tr], 4),
                              "floor_bytes": pass7, "TB_per_s": round(pass7 / (ms * 1e-3) / 1e12, 3) if ms > 0 else None,
                              "ratio_to_J_x": round(ms / ms_of["J x"], 2), **tag}), flush=True)
    b = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 0.5
    for tr in (False, True):
        for timed in (False, True):
            torch.cuda.synchronize()
            eng.event_record(1)
            its, r0, rn = eng.gmresSolveDev(b.data_ptr(), y.data_ptr(), n, 1, tr, restart=30, maxIts=60, rtol=rtol)
            eng.event_record(2)
            eng.sync()
        print(json.dumps({"what": f"gmres on the PC matrix, rtol {rtol:g}", "fill": fill, "transpose": tr, "iterations": its, "ms": round(eng.event_elapsed_ms(1, 2), 3),
                          "rnorm0": r0, "true_rnorm": rn, **tag}), flush=True)
    if nvec > 1:
        multi_columns(eng, torch, gen, n, nvec, n_it, fill, planes, floor, rtol)
    eng.pcRelease()


def time_apply(eng, torch, n, n_it, transpose):
    """ms of one application of the factor that stands, enqueue-only, as one_factor times it"""
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 0.5
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    eng.set_async(True)
    try:
        for _ in range(3):
            eng.pcApplyDev(x.data_ptr(), y.data_ptr(), n, 1, transpose)
        eng.event_record(1)
        for _ in range(n_it):
            eng.pcApplyDev(x.data_ptr(), y.data_ptr(), n, 1, transpose)
        eng.event_record(2)
        eng.sync()
    finally:
        eng.set_async(False)
    return eng.event_elapsed_ms(1, 2) / n_it


def its_launches(one, mg):
    """launches of one application from those of one sweep pair or cycle: inner x (sweeps) + (inner - 1) x (residual, update) on a plain
    factor, that outer times, and (outer - 1) x (residual, update); the inner iterations of a hierarchy are not counted here"""
    outer, inner, _ = ITS
    local = one if mg > 1 else inner * one + 2 * (inner - 1)
    return outer * local + 2 * (outer - 1)


def cycle_cost(eng, dims, ns, fill, planes1):
    """half the launches of one cycle (the callers print 2 x) and its byte floor, from the sizes adflow_gpu_pc_mg_info reports: per
    level nSmooth ILU applications (two sweeps over the level sets each) and nSmooth passes over the 7-point matrix (the fused
    prolongation / residual or the residual of a Richardson iteration; none for the first iteration of the last level); per level but
    the last the restriction, the fused pass and y += x, and a residual and x += d per further Richardson iteration"""
    levels, nsmooth, fillc, cells = eng.pcMgInfo()
    ent = {0: 7, 1: 13, 2: 23}
    sets = {0: lambda a, b, c: a + b + c - 2, 1: lambda a, b, c: a + 2 * b + 3 * c - 5, 2: lambda a, b, c: a + 3 * b + 7 * c - 10}
    launches, floor, d = 0, 0, list(dims)
    for l in range(levels):
        f = fill if l == 0 else fillc
        npl = planes1 if l == 0 else sets[f](*d)
        last = l == levels - 1
        launches += 2 * npl * nsmooth + (0 if last else 3) + 2 * (nsmooth - 1)
        floor += cells[l] * ns * ns * 8 * (ent[f] * nsmooth + 7 * (nsmooth - (1 if last else 0)))
        d = [(a + 1) // 2 for a in d]
    print(json.dumps({"what": "hierarchy", "levels": levels, "nSmooth": nsmooth, "fillCoarse": fillc, "cells": list(cells),
                      "launches_per_cycle": launches, "floor_bytes_per_cycle": floor}), flush=True)
    return launches / 2, floor


def multi_columns(eng, torch, gen, n, nvec, n_it, fill, planes, floor, rtol):
    """nvec columns through the multi entries against nvec calls of the single entries, same process, same factor"""
    X = torch.rand(nvec * n, dtype=torch.float64, device="cuda", generator=gen) - 0.5
    Y = torch.empty_like(X)
    torch.cuda.synchronize()
    # a call serves the columns in groups of at most 4; a fill-2 factor column by column
    groups = nvec if fill == 2 else (nvec + 3) // 4

    def timed(fn, reps):
        for _ in range(2):
            fn()
        eng.event_record(1)
        for _ in range(reps):
            fn()
        eng.event_record(2)
        eng.sync()
        return eng.event_elapsed_ms(1, 2) / reps

    eng.set_async(True)
    try:
        for tr in (False, True):
            def single():
                for c in range(nvec):
                    eng.pcApplyDev(X.data_ptr() + 8 * c * n, Y.data_ptr() + 8 * c * n, n, 1, tr)
            ms_s = timed(single, n_it)
            sum_s = float(Y.abs().sum().item())
            ms_m = timed(lambda: eng.pcApplyMultiDev(X.data_ptr(), n, Y.data_ptr(), n, nvec, n, 1, tr), n_it)
            launches = 2 * planes * groups
            print(json.dumps({"what": "M^-T R" if tr else "M^-1 R", "fill": fill, "nvec": nvec, "ms_multi": round(ms_m, 4),
                              "ms_nvec_single_calls": round(ms_s, 4), "multi_over_single": round(ms_m / ms_s, 3), "launches": launches,
                              "us_per_launch": round(1e3 * ms_m / launches, 2),
                              "GB_per_s_on_the_factor": round(groups * floor / (ms_m * 1e-3) / 1e9, 1),
                              "checksum": float(Y.abs().sum().item()), "checksum_single_calls": sum_s}), flush=True)
    finally:
        eng.set_async(False)
    gmres_columns(eng, torch, X, Y, n, nvec, fill, rtol)


def gmres_columns(eng, torch, B, X, n, nvec, what, rtol):
    """wall time of GMRES for nvec right-hand sides: one lock-step call against nvec single solves"""
    kw = dict(restart=30, maxIts=60, rtol=rtol)
    for tr in (False, True):
        for _ in range(2):                                # the second run is the timed one
            torch.cuda.synchronize()
            eng.event_record(1)
            its_s = [eng.gmresSolveDev(B.data_ptr() + 8 * c * n, X.data_ptr() + 8 * c * n, n, 1, tr, **kw)[0] for c in range(nvec)]
            eng.event_record(2)
            eng.sync()
            ms_s = eng.event_elapsed_ms(1, 2)
            eng.event_record(1)
            its_m = eng.gmresSolveMultiDev(B.data_ptr(), n, X.data_ptr(), n, nvec, n, 1, tr, **kw)[0]
            eng.event_record(2)
            eng.sync()
            ms_m = eng.event_elapsed_ms(1, 2)
        print(json.dumps({"what": f"gmres, {nvec} right-hand sides, rtol {rtol:g}", "case": what, "transpose": tr, "ms_multi": round(ms_m, 3),
                          "ms_nvec_single_solves": round(ms_s, 3), "multi_over_single": round(ms_m / ms_s, 3),
                          "iterations_multi": [int(i) for i in its_m], "iterations_single": its_s}), flush=True)


if __name__ == "__main__":
    main()
