#!/usr/bin/env python
"""Flow integration on the mesh of tools/wall_forces.py (a 2 x 2 x 2 brick of 160 x 128 x 64 blocks, RANS, Roe upwind, viscous wall on
the floor of the brick) with a subsonic inflow on the iMin face of the brick and a subsonic outflow on its iMax face, after one
evaluation of the whole blocketteRes:
  (a) adflow_gpu_flow_integrate_dev beside adflow_gpu_wall_integrate_dev;
  (b) adflow_gpu_flow_integrate_fwd_dev, one forward product, beside adflow_gpu_wall_integrate_fwd_dev;
  (c) adflow_gpu_flow_integrate_bwd_dev, one transposed sweep at nRhs = 1, beside adflow_gpu_wall_integrate_bwd_dev.
All between two HIP events in enqueue-only mode, after one warm-up call each.  Prints one JSON line with median, min and max.
usage: flow_int.py [n] [nx ny nz]   (n repetitions of the integrations and products, default 10; the sweeps run 3 times)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library: one HIP runtime in the process)
from adflow_amd.engine import Engine  # noqa: E402
from adflow_amd.params import FlowParams, RANSEquations, upwind, vanAlbeda  # noqa: E402
from adflow_amd.synth import make_block, make_bocos, set_porosities  # noqa: E402
from adflow_amd.topology import BrickTopology  # noqa: E402

DUCT_BRICK = {1: -8, 2: -10, 3: -1, 4: -6, 5: -3, 6: -6}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = max(3, int(args[0])) if args else 10
    dims = tuple(int(a) for a in args[1:4]) if len(args) > 3 else (160, 128, 64)
    eng = Engine(0)
    prm = FlowParams(equations=RANSEquations, spaceDiscr=upwind, limiter=vanAlbeda).replace(currentLevel=1, groundLevel=1)
    eng.release_all()
    eng.set_options(prm)
    topo = BrickTopology(2, 2, 2, *dims, periodic=(False, False, False))
    lid = topo.local_ids()
    keep, ncells, nflow = [], 0, {-8: 0, -10: 0}
    for g in range(topo.nblocks):
        cg = topo.coords(g)
        blk = make_block(*dims, prm, seed=20260925 + g, stretch_k=3.0 if cg[2] == 0 else 1.0, wall_kmin=False)
        blk["d2Wall"] += float(cg[2])
        spec = topo.boundary_spec(g, DUCT_BRICK)
        faces, nvisc = make_bocos(blk, prm, spec, seed=31 * g + 1) if spec else ([], 0)
        set_porosities(blk, faces)
        eng.register(blk, nn=lid[g], level=1)
        if faces:
            eng.bc_register(faces, nvisc, nn=lid[g], level=1)
        keep.append((blk, faces))
        ncells += blk.ncells
        for f in faces:                 # owned face cells of the in- and outflow subfaces: the cells of the block's face
            if f["bcType"] in (-8, -10):
                nflow[f["bcType"]] += (dims[1] * dims[2], dims[0] * dims[2], dims[0] * dims[1])[(f["faceID"] - 1) // 2]
    for L in (1, 2):
        eng.comm_register(1, L, topo.patterns(L)[0])
    eng.blocketteRes(1, False, True, True, halo=True, closures=True)
    wpar = eng.wallPar(prm.Mach)
    fpar = eng.flowPar(prm.rhoInfDim, prm.RGasDim)
    nvec = 6 * ncells
    rng = np.random.default_rng(1)
    d_x = torch.from_numpy(rng.uniform(-1.0, 1.0, nvec)).cuda()
    d_w = torch.zeros(nvec, dtype=torch.float64, device="cuda")
    d_out = torch.zeros(64, dtype=torch.float64, device="cuda")
    d_dot = torch.zeros(64, dtype=torch.float64, device="cuda")
    obw, obf = np.zeros((1, 1, 64)), np.zeros((1, 1, 64))
    obw[0, 0, :12] = rng.uniform(-1.0, 1.0, 12)
    obf[0, 0, 18:32] = rng.uniform(-1.0, 1.0, 14)
    torch.cuda.synchronize()

    def timed(fn, reps):
        def once():
            eng.event_record(1)
            fn()
            eng.event_record(2)
            eng.sync()
            return eng.event_elapsed_ms(1, 2)
        eng.set_async(True)
        try:
            once()
            return [once() for _ in range(reps)]
        finally:
            eng.sync()
            eng.set_async(False)

    p = lambda t: t.data_ptr()
    res = {"what": "flow integration beside the wall integration: value (a), forward product (b), transposed sweep (c)",
           "dims": list(dims), "blocks": topo.nblocks, "cells": ncells, "inflow_faces": nflow[-8], "outflow_faces": nflow[-10]}

    def put(name, ms, digits):
        res[name + "_ms_median"], res[name + "_ms_min"], res[name + "_ms_max"] = (round(statistics.median(ms), digits), round(min(ms), digits),
                                                                                 round(max(ms), digits))
    put("flow", timed(lambda: eng.flowIntegrateDev(fpar, p(d_out)), n), 4)
    massflow = float(d_out.cpu().numpy()[18])
    put("wall", timed(lambda: eng.wallIntegrateDev(wpar, p(d_out)), n), 4)
    put("flow_fwd", timed(lambda: eng.flowIntegrateFwdDev(p(d_x), nvec, fpar, p(d_out), p(d_dot)), n), 4)
    dot = d_dot.cpu().numpy().copy()
    put("wall_fwd", timed(lambda: eng.wallIntegrateFwdDev(p(d_x), nvec, wpar, p(d_out), p(d_dot)), n), 4)
    put("flow_bwd", timed(lambda: eng.flowIntegrateBwdDev(obf, p(d_w), nvec, nvec, fpar), 3), 2)
    res["massFlow"] = massflow
    res["outBar_dot_fwd"], res["bwd_dot_x"] = float((obf[0, 0] * dot).sum()), float(d_w.cpu().numpy() @ d_x.cpu().numpy())
    put("wall_bwd", timed(lambda: eng.wallIntegrateBwdDev(obw, p(d_w), nvec, nvec, wpar), 3), 2)
    eng.releaseWorkspace()
    print(json.dumps(res), flush=True)
    eng.release_all()
    eng.close()


if __name__ == "__main__":
    main()
