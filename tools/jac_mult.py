#!/usr/bin/env python
"""The products with the assembled matrix alone (adflow_gpu_jacobian_mult_dev: y = J x, y = J^T x on device vectors), timed with HIP
events: the RANS Roe preconditioner matrix (7-point, forward-mode assembly) on one 160 x 128 x 64 wall-bounded block and the exact
dR/dw (33-point) on a 96 x 64 x 48 block.  Prints ms per product, the bytes of the byte floor (nStencil nState^2 x 8 B per owned
cell: one pass over the matrix), TB/s and the fraction of the measured copy ceiling (profiles/r06_fin6_calibration.json).
--nvec N adds, on the 160 x 128 x 64 block and in the same process: Y = J X and J^T X for N columns through
adflow_gpu_jacobian_mult_multi_dev (one call) against N calls of adflow_gpu_jacobian_mult_dev, with the GB/s on the matrix of the multi
call, and the wall time of GMRES (block ILU(0)) for N right-hand sides through adflow_gpu_gmres_solve_multi_dev against N single solves.
--free times, in one process on one 160 x 128 x 64 RANS Roe block (or --dims NX NY NZ), one product of each of the three operators a
Krylov solver for the exact dR/dw can run on: adflow_gpu_jacfree_mult_dev with the exact flags (one forward-mode evaluation, no
matrix), adflow_gpu_ank_mult_dev (a finite difference of two residuals) and adflow_gpu_jacobian_mult_dev on the assembled exact
33-point matrix, with the bytes each one keeps on the device.  --free --no-matrix leaves the assembled matrix out (a mesh on which
it does not fit).
--blocks N puts N such blocks on the level (8: the size of the benchmark mesh).
usage: jac_mult.py [--nvec N] [--free [--no-matrix] [--blocks N] [--dims NX NY NZ]] [n]   (n timed products of each kind, default 20)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adflow_amd import capi  # noqa: E402
from adflow_amd.engine import Engine  # noqa: E402
from adflow_amd.params import FlowParams, RANSEquations, upwind, vanAlbeda  # noqa: E402
from adflow_amd.synth import make_block, make_bocos  # noqa: E402
from adflow_amd.topology import CommPattern  # noqa: E402

WALL = {1: -6, 2: -6, 3: -1, 4: -1, 5: -3, 6: -6}


def case(eng, torch, dims, usePC, n_it, ceiling, nvec=0):
    prm = FlowParams(equations=RANSEquations, spaceDiscr=upwind, limiter=vanAlbeda).replace(currentLevel=1, groundLevel=1)
    blk = make_block(*dims, prm, seed=7, stretch_k=2.0)
    faces, nvisc = make_bocos(blk, prm, WALL, seed=8)
    eng.release_all()
    eng.set_options(prm)
    eng.register(blk)
    eng.bc_register(faces, nvisc)
    for L in (1, 2):
        eng.comm_register(1, L, CommPattern())
    eng.applyAllBC(1, True)
    eng.setupStateResidualMatrix(1, usePC, useAD=True)
    ns, st = eng.jacobianInfo()
    cells = blk.nx * blk.ny * blk.nz
    n = ns * cells
    floor = st.shape[0] * ns * ns * 8 * cells
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 0.5
    y = torch.empty_like(x)
    torch.cuda.synchronize()
    eng.set_async(True)
    try:
        for tr in (False, True):
            for _ in range(3):
                eng.jacobianMultDev(x.data_ptr(), y.data_ptr(), n, 1, tr)
            eng.event_record(1)
            for _ in range(n_it):
                eng.jacobianMultDev(x.data_ptr(), y.data_ptr(), n, 1, tr)
            eng.event_record(2)
            eng.sync()
            ms = eng.event_elapsed_ms(1, 2) / n_it
            tbs = floor / (ms * 1e-3) / 1e12
            print(json.dumps({"matrix": "PC 7-point" if usePC else "dRdw 33-point", "dims": list(dims), "nState": ns, "nStencil": int(st.shape[0]),
                              "product": "J^T x" if tr else "J x", "ms": round(ms, 4), "floor_bytes": floor, "TB_per_s": round(tbs, 3),
                              "of_copy_ceiling": round(tbs / ceiling, 3), "checksum": float(y.abs().sum().item())}), flush=True)
    finally:
        eng.set_async(False)
    if nvec > 1:
        multi_columns(eng, torch, gen, n, nvec, n_it, floor)
    eng.releaseWorkspace()


def multi_columns(eng, torch, gen, n, nvec, n_it, floor):
    """nvec columns through the multi entries against nvec calls of the single entries, same process, same matrix"""
    from pc_apply import gmres_columns
    X = torch.rand(nvec * n, dtype=torch.float64, device="cuda", generator=gen) - 0.5
    Y = torch.empty_like(X)
    torch.cuda.synchronize()
    groups = (nvec + 3) // 4                              # a call reads the matrix once per group of at most 4 columns

    def timed(fn):
        for _ in range(3):
            fn()
        eng.event_record(1)
        for _ in range(n_it):
            fn()
        eng.event_record(2)
        eng.sync()
        return eng.event_elapsed_ms(1, 2) / n_it

    eng.set_async(True)
    try:
        for tr in (False, True):
            def single():
                for c in range(nvec):
                    eng.jacobianMultDev(X.data_ptr() + 8 * c * n, Y.data_ptr() + 8 * c * n, n, 1, tr)
            ms_s = timed(single)
            sum_s = float(Y.abs().sum().item())
            ms_m = timed(lambda: eng.jacobianMultMultiDev(X.data_ptr(), n, Y.data_ptr(), n, nvec, n, 1, tr))
            print(json.dumps({"product": "J^T X" if tr else "J X", "nvec": nvec, "ms_multi": round(ms_m, 4), "ms_nvec_single_calls": round(ms_s, 4),
                              "multi_over_single": round(ms_m / ms_s, 3),
                              "GB_per_s_on_the_matrix": round(groups * floor / (ms_m * 1e-3) / 1e9, 1),
                              "checksum": float(Y.abs().sum().item()), "checksum_single_calls": sum_s}), flush=True)
    finally:
        eng.set_async(False)
    eng.pcSetup(1)
    gmres_columns(eng, torch, X, Y, n, nvec, "PC 7-point matrix, fill 0", 1e-8)
    eng.pcRelease()


def free_case(eng, torch, dims, n_it, with_matrix=True, nblocks=1):
    """the matrix-free exact product against the finite-difference operator of ANK and the assembled exact matrix; nblocks: that many
    wall-bounded blocks of `dims` side by side on the level (the size of the benchmark mesh with 8)"""
    prm = FlowParams(equations=RANSEquations, spaceDiscr=upwind, limiter=vanAlbeda).replace(currentLevel=1, groundLevel=1)
    blk = make_block(*dims, prm, seed=7, stretch_k=2.0)
    blocks = [blk] + [blk.copy() for _ in range(nblocks - 1)]
    bocos = [make_bocos(b, prm, WALL, seed=8) for b in blocks]
    eng.release_all()
    eng.set_options(prm)
    for nn, (b, (faces, nvisc)) in enumerate(zip(blocks, bocos), start=1):
        eng.register(b, nn=nn)
        eng.bc_register(faces, nvisc, nn=nn)
    for L in (1, 2):
        eng.comm_register(1, L, CommPattern())
    eng.applyAllBC(1, True)
    cells = nblocks * blk.nx * blk.ny * blk.nz
    n = blk.nw * cells
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 0.5
    y = torch.empty_like(x)
    torch.cuda.synchronize()

    def timed(fn):
        eng.set_async(True)
        try:
            for _ in range(3):
                fn()
            eng.event_record(1)
            for _ in range(n_it):
                fn()
            eng.event_record(2)
            eng.sync()
        finally:
            eng.set_async(False)
        return eng.event_elapsed_ms(1, 2) / n_it

    def report(what, ms, kept, **more):
        print(json.dumps(dict({"operator": what, "dims": list(dims), "blocks": nblocks, "cells": cells, "ms": round(ms, 4), "bytes_kept": int(kept),
                               "checksum": float(y.abs().sum().item())}, **more)), flush=True)

    eng.releaseWorkspace()
    ms = timed(lambda: eng.jacFreeMultDev(x.data_ptr(), y.data_ptr(), n, 1))
    y_free = y.clone()
    report("adflow_gpu_jacfree_mult_dev, exact flags (slab of dual arrays + scratch of the vector)", ms, eng.releaseWorkspace())
    # the finite-difference operator of the coupled ANK step: (R(w + h v) - r0) / h + T v
    eng.timeStep(1)
    eng.ankTimeStep(5.0, 2.5, coupled=True)
    eng.download_state(1, 1)
    w6 = np.tile(np.ascontiguousarray(np.transpose(blk.owned("w"), (2, 1, 0, 3))).reshape(-1), nblocks)
    eng.ankSetBase(w6, coupled=True)
    ms = timed(lambda: eng.ankMultDev(x.data_ptr(), y.data_ptr(), n))
    report("adflow_gpu_ank_mult_dev, coupled (base state, base residual, T)", ms, eng.ankRelease())
    for nn in range(1, nblocks + 1):                      # (the ANK product leaves the perturbed state on the device)
        eng.upload_state(nn, 1)
    eng.applyAllBC(1, True)
    if with_matrix:
        eng.event_record(1)
        eng.setupStateResidualMatrix(1, False, useAD=True)
        eng.event_record(2)
        eng.sync()
        ms_asm = eng.event_elapsed_ms(1, 2)
        ns, st = eng.jacobianInfo()
        nbox = nblocks * (blk.nx + 4) * (blk.ny + 4) * (blk.nz + 4)
        eng.releaseWorkspace()
        ms = timed(lambda: eng.jacobianMultDev(x.data_ptr(), y.data_ptr(), n, 1, False))
        floor = st.shape[0] * ns * ns * 8 * cells
        rel = float(((y - y_free).abs().max() / y.abs().max()).item())
        report("adflow_gpu_jacobian_mult_dev, assembled exact 33-point matrix (blocks over the box + scratch of two vectors)", ms,
               st.shape[0] * ns * ns * 8 * nbox + eng.releaseWorkspace(), matrix_bytes_owned_rows=floor,
               TB_per_s_on_the_matrix=round(floor / (ms * 1e-3) / 1e12, 3), assembly_ms=round(ms_asm, 1),
               max_difference_to_the_matrix_free_product_rel=rel)
    eng.releaseWorkspace()


def main():
    import torch
    argv, nvec = list(sys.argv[1:]), 0
    if "--free" in argv:
        argv.remove("--free")
        dims, with_matrix, nblocks = (160, 128, 64), True, 1
        if "--blocks" in argv:
            at = argv.index("--blocks")
            nblocks = int(argv[at + 1])
            del argv[at:at + 2]
        if "--no-matrix" in argv:
            argv.remove("--no-matrix")
            with_matrix = False
        if "--dims" in argv:
            at = argv.index("--dims")
            dims = tuple(int(a) for a in argv[at + 1:at + 4])
            del argv[at:at + 4]
        eng = Engine(0)
        free_case(eng, torch, dims, int(argv[0]) if argv else 20, with_matrix, nblocks)
        eng.close()
        return
    if "--nvec" in argv:
        at = argv.index("--nvec")
        nvec = int(argv[at + 1])
        del argv[at:at + 2]
    sys.argv[1:] = argv
    n_it = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    with open(os.path.join(ROOT, "profiles", "r06_fin6_calibration.json")) as f:
        ceiling = json.load(f)["copy16u8_1gib_gbs"] / 1e3
    eng = Engine(0)
    case(eng, torch, (160, 128, 64), True, n_it, ceiling, nvec)
    case(eng, torch, (96, 64, 48), False, n_it, ceiling)
    eng.close()


if __name__ == "__main__":
    main()
