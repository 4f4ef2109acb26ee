#!/usr/bin/env python
"""The linear solve of the approximate Newton-Krylov step (adflow_gpu_ank_*), timed with HIP events on one wall-bounded RANS Roe
block (default 160 x 128 x 64), decoupled (nState = 5), approximate residual flavour.  Prints ms per application of the matrix-free
operator y = (R(w + h v) - r0) / h + T v next to ms per adflow_gpu_nk_residual_dev evaluation of the same build (the operator's
excess is three vector passes and a sum), ms per shifted setup (adflow_gpu_ank_pc_setup) next to adflow_gpu_pc_setup on the same
matrix, and ms per 10-iteration solve.
usage: ank_step.py [--turb] [n] [nx ny nz]   (n timed applications of each kind, default 10)
--turb: the turbulence update of the decoupled step instead (ADFLOW_ANK_TURB, approxSA and first-order turbulence advection as
ANKTurbSolveKSP sets them): ms per ank_mult_dev(turb) next to adflow_gpu_block_res with HALO | TURB, per ank_pc_setup at nState = 1,
per 10-iteration ank_solve_dev(turb), and per ank_unsteady_res_dev of the three kinds (flow decoupled, coupled, turbulence)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adflow_amd.engine import Engine  # noqa: E402
from adflow_amd.params import FlowParams, RANSEquations, upwind, vanAlbeda  # noqa: E402
from adflow_amd.synth import make_block, make_bocos  # noqa: E402
from adflow_amd.topology import CommPattern  # noqa: E402

WALL = {1: -6, 2: -6, 3: -1, 4: -1, 5: -3, 6: -6}


def timed(eng, fn, n_it, warm=3):
    for _ in range(warm):
        fn()
    eng.event_record(1)
    for _ in range(n_it):
        fn()
    eng.event_record(2)
    eng.sync()
    return eng.event_elapsed_ms(1, 2) / n_it


def turb_mode(eng, blk, dims, n_it):
    import numpy as np
    import torch
    from adflow_amd import capi
    cells = blk.nx * blk.ny * blk.nz
    T, SA = capi.ANK_TURB, capi.RES_APPROX_SA | capi.RES_TURB_FIRST_ORDER
    eng.setupStateResidualMatrix(1, True, useTurbOnly=True, useAD=True, approxSA=True)
    eng.releaseWorkspace()
    eng.timeStep(1)
    eng.ankTimeStep(5.0, 2.5, turb=True)
    eng.pcSelect(1)
    for what, fn in (("adflow_gpu_pc_setup", eng.pcSetup), ("adflow_gpu_ank_pc_setup (shifted)", eng.ankPcSetup)):
        fn(1)
        eng.sync()
        eng.event_record(1)
        fn(1)
        eng.event_record(2)
        eng.sync()
        print(json.dumps({"what": what, "dims": list(dims), "nState": 1, "ms": round(eng.event_elapsed_ms(1, 2), 3),
                          "hyperplanes": eng.pcInfo()[1]}), flush=True)
    eng.download_state(1, 1)
    w6 = np.ascontiguousarray(np.transpose(blk.owned("w"), (2, 1, 0, 3))).reshape(-1)
    eng.ankSetBase(w6, coupled=True)                      # pressure and viscosities from the closures of the state write
    wt = np.ascontiguousarray(w6.reshape(-1, blk.nw)[:, 5])
    eng.ankSetBase(wt, turb=True, approxSA=True, turbFirstOrder=True)
    bt = torch.from_numpy(eng.ankGetR(turb=True)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(5)
    v = torch.rand(cells, dtype=torch.float64, device="cuda", generator=gen) - 0.5
    y = torch.empty_like(v)
    torch.cuda.synchronize()
    eng.set_async(True)
    try:
        res_flags = capi.RES_HALO | capi.RES_TURB
        ms_res = timed(eng, lambda: eng._chk(eng.lib.adflow_gpu_block_res(1, res_flags)), n_it)
        print(json.dumps({"what": "adflow_gpu_block_res(HALO | TURB)", "ms": round(ms_res, 4)}), flush=True)
        ms_op = timed(eng, lambda: eng.ankMultDev(v.data_ptr(), y.data_ptr(), cells), n_it)
        # beside the residual: the sums read w0, v; the state write reads w0, v, rho, rlv and writes nuTilde, rev; the quotient reads
        # dw, volRef, r0, T, v and writes y
        print(json.dumps({"what": "adflow_gpu_ank_mult_dev(turb)", "ms": round(ms_op, 4), "ratio_to_block_res": round(ms_op / ms_res, 3),
                          "vector_bytes": (2 + 6 + 6) * cells * 8}), flush=True)
    finally:
        eng.set_async(False)
    for _ in range(2):
        torch.cuda.synchronize()
        eng.event_record(1)
        its, r0, rn = eng.ankSolveDev(bt.data_ptr(), y.data_ptr(), cells, 1, restart=10, maxIts=10, rtol=1e-12)
        eng.event_record(2)
        eng.sync()
    print(json.dumps({"what": "ank_solve(turb), 10 iterations", "iterations": its, "ms": round(eng.event_elapsed_ms(1, 2), 3), "rnorm0": r0,
                      "true_rnorm": rn, "h": eng.ankLastH()}), flush=True)
    eng.ankSetW(wt, turb=True)
    eng.pcRelease()
    eng.pcSelect(0)
    # the line-search residual of the three kinds, with the norm (synchronous) and without it
    eng.ankTimeStep(5.0, 2.5, coupled=True)
    for kind, ns, flags in (("coupled", blk.nw, capi.ANK_COUPLED | SA), ("flow decoupled", 5, 0), ("turbulence", 1, T | SA)):
        if kind == "flow decoupled":
            eng.ankTimeStep(5.0)
        n = ns * cells
        dW = (torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 1e-6
        r = torch.empty_like(dW)
        torch.cuda.synchronize()
        for norm in (True, False):
            ms = timed(eng, lambda: eng.ankUnsteadyResDev(dW.data_ptr(), 0.5, r.data_ptr(), n, flags, norm=norm), n_it)
            print(json.dumps({"what": f"adflow_gpu_ank_unsteady_res_dev, {kind}", "norm": norm, "ms": round(ms, 4),
                              "pass_bytes": (3 * ns + 1 + (1 if ns == 1 else 5)) * cells * 8}), flush=True)
    eng.ankRelease()
    eng.releaseWorkspace()
    eng.close()


def main():
    import numpy as np
    import torch
    turb = "--turb" in sys.argv
    if turb:
        sys.argv.remove("--turb")
    n_it = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    dims = tuple(int(a) for a in sys.argv[2:5]) if len(sys.argv) > 4 else (160, 128, 64)
    eng = Engine(0)
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
    if turb:
        return turb_mode(eng, blk, dims, n_it)
    eng.setupStateResidualMatrix(1, True, frozenTurb=True, useAD=True)
    eng.releaseWorkspace()
    cells = blk.nx * blk.ny * blk.nz
    n5, n6 = 5 * cells, blk.nw * cells
    eng.timeStep(1)
    eng.ankTimeStep(5.0)
    for what, fn in (("adflow_gpu_pc_setup", eng.pcSetup), ("adflow_gpu_ank_pc_setup (shifted)", eng.ankPcSetup)):
        fn(1)                                             # warm-up (allocations, tables)
        eng.sync()
        eng.event_record(1)
        fn(1)
        eng.event_record(2)
        eng.sync()
        print(json.dumps({"what": what, "dims": list(dims), "nState": 5, "ms": round(eng.event_elapsed_ms(1, 2), 3),
                          "hyperplanes": eng.pcInfo()[1]}), flush=True)
    eng.download_state(1, 1)
    w6 = np.ascontiguousarray(np.transpose(blk.owned("w"), (2, 1, 0, 3))).reshape(-1)
    w5 = np.ascontiguousarray(w6.reshape(-1, blk.nw)[:, :5]).reshape(-1)
    eng.referenceShockSensor(1)
    eng.ankSetBase(w5, dissApprox=True, viscApprox=True, useBlockettes=True)
    b5 = torch.from_numpy(eng.ankGetR()).cuda()
    gen = torch.Generator(device="cuda").manual_seed(5)
    v = torch.rand(n5, dtype=torch.float64, device="cuda", generator=gen) - 0.5
    y = torch.empty_like(v)
    wd = torch.from_numpy(w6).cuda()
    rd = torch.empty_like(wd)
    torch.cuda.synchronize()
    eng.set_async(True)
    ms_of = {}
    try:
        for what, fn in (("adflow_gpu_nk_residual_dev", lambda: eng._chk(eng.lib.adflow_gpu_nk_residual_dev(wd.data_ptr(), rd.data_ptr(), n6))),
                         ("adflow_gpu_ank_mult_dev", lambda: eng.ankMultDev(v.data_ptr(), y.data_ptr(), n5))):
            for _ in range(3):
                fn()
            eng.event_record(1)
            for _ in range(n_it):
                fn()
            eng.event_record(2)
            eng.sync()
            ms_of[what] = eng.event_elapsed_ms(1, 2) / n_it
            print(json.dumps({"what": what, "ms": round(ms_of[what], 4),
                              "ratio_to_nk_residual": round(ms_of[what] / ms_of["adflow_gpu_nk_residual_dev"], 3)}), flush=True)
    finally:
        eng.set_async(False)
    # the excess over one residual evaluation: the sums read w0, v; the state write reads w0, v; the quotient reads v, r0, T and writes y
    extra = (2 + 2 + 3) * n5 * 8 + 5 * cells * 8
    print(json.dumps({"what": "operator minus residual", "ms": round(ms_of["adflow_gpu_ank_mult_dev"] - ms_of["adflow_gpu_nk_residual_dev"], 4),
                      "vector_bytes": extra}), flush=True)
    for timed in (False, True):
        torch.cuda.synchronize()
        eng.event_record(1)
        its, r0, rn = eng.ankSolveDev(b5.data_ptr(), y.data_ptr(), n5, 1, restart=10, maxIts=10, rtol=1e-12)
        eng.event_record(2)
        eng.sync()
    print(json.dumps({"what": "ank_solve, 10 iterations", "iterations": its, "ms": round(eng.event_elapsed_ms(1, 2), 3), "rnorm0": r0,
                      "true_rnorm": rn, "h": eng.ankLastH()}), flush=True)
    eng.pcRelease()
    eng.ankRelease()
    eng.releaseWorkspace()
    eng.close()


if __name__ == "__main__":
    main()
