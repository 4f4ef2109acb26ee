#!/usr/bin/env python
"""Surface integration on the device against the route a host had before it, on the benchmark's wall-bounded mesh (a 2 x 2 x 2 brick
of 160 x 128 x 64 blocks, RANS, Roe upwind, viscous wall on the floor of the brick), after one evaluation of the whole blocketteRes:
  (a) adflow_gpu_wall_integrate_dev in enqueue-only mode between two HIP events;
  (b) adflow_gpu_download_state of every block plus adflow_gpu_download_wall_stress of every viscous subface (host clock: the copies
      are synchronous), after which the host would still run the Fortran loop.
Prints one JSON line with the median of each over n repetitions after warm-up, the bytes (b) moves and the bytes (a) reads per face.
usage: wall_forces.py [n] [nx ny nz]   (n >= 20 repetitions, default 20; block size, default 160 128 64)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (before the library: one HIP runtime in the process)
from adflow_amd.engine import Engine  # noqa: E402
from adflow_amd.params import FlowParams, RANSEquations, upwind, vanAlbeda  # noqa: E402
from adflow_amd.synth import make_block, make_bocos, set_porosities  # noqa: E402
from adflow_amd.topology import BrickTopology  # noqa: E402

WALL_BRICK = {1: -6, 2: -6, 3: -1, 4: -6, 5: -3, 6: -6}
# doubles the face kernel reads per owned face of a viscous wall under RANS: p 2, velocity 3, density 2, face normal 3, four nodes 12,
# unit normal 3, stress 6, rlv 2, d2Wall 1 (plus one byte of blanking where set); it writes 7 (Fp, Fv, area)
READ_DOUBLES, WRITE_DOUBLES = 34, 7


def owned_shape(f, blk):
    amax = blk.jl if f["faceID"] <= 2 else blk.il
    bmax = blk.kl if f["faceID"] <= 4 else blk.jl
    return (min(f["icEnd"], amax) - max(f["icBeg"], 2) + 1, min(f["jcEnd"], bmax) - max(f["jcBeg"], 2) + 1)


def main():
    n = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 20
    dims = tuple(int(a) for a in sys.argv[2:5]) if len(sys.argv) > 4 else (160, 128, 64)
    eng = Engine(0)
    prm = FlowParams(equations=RANSEquations, spaceDiscr=upwind, limiter=vanAlbeda).replace(currentLevel=1, groundLevel=1)
    eng.release_all()
    eng.set_options(prm)
    topo = BrickTopology(2, 2, 2, *dims, periodic=(False, False, False))
    lid = topo.local_ids()
    walls, keep, state_bytes, nfaces = [], [], 0, 0
    for g in range(topo.nblocks):
        cg = topo.coords(g)
        blk = make_block(*dims, prm, seed=20260925 + g, stretch_k=3.0 if cg[2] == 0 else 1.0, wall_kmin=False)
        blk["d2Wall"] += float(cg[2])
        spec = topo.boundary_spec(g, WALL_BRICK)
        faces, nvisc = make_bocos(blk, prm, spec, seed=31 * g + 1) if spec else ([], 0)
        set_porosities(blk, faces)
        eng.register(blk, nn=lid[g], level=1)
        if faces:
            eng.bc_register(faces, nvisc, nn=lid[g], level=1)
        for m in range(nvisc):
            shp = owned_shape(faces[m], blk)
            walls.append((lid[g], m + 1, shp))
            nfaces += shp[0] * shp[1]
        keep.append((blk, faces))
        state_bytes += sum(blk[k].nbytes for k in ("w", "p", "gamma", "rlv", "rev"))
    for L in (1, 2):
        eng.comm_register(1, L, topo.patterns(L)[0])
    eng.blocketteRes(1, False, True, True, halo=True, closures=True)
    par = eng.wallPar(prm.Mach)
    d_out = torch.zeros(64, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    first = eng.wallIntegrate(par)                    # allocates the buffers; the values for the record

    def route_a():
        eng.event_record(1)
        eng.wallIntegrateDev(par, d_out.data_ptr())
        eng.event_record(2)
        eng.sync()
        return eng.event_elapsed_ms(1, 2)

    def route_b():
        t0 = time.perf_counter()
        for nn in sorted(lid.values()):
            eng.download_state(nn, 1)
        for nn, mm, shp in walls:
            eng.wall_stress(shp, mm, nn=nn)
        return (time.perf_counter() - t0) * 1e3

    eng.set_async(True)
    try:
        for _ in range(3):
            route_a()
        a = [route_a() for _ in range(n)]
    finally:
        eng.sync()
        eng.set_async(False)
    assert (d_out.cpu().numpy() == first[0]).all(), "the enqueue-only form disagrees with the host form"
    for _ in range(2):
        route_b()
    b = [route_b() for _ in range(n)]
    stress_bytes = 9 * 8 * nfaces
    print(json.dumps({"what": "wall integration on the device (a) against state + wall stress download (b)", "dims": list(dims),
                      "blocks": topo.nblocks, "wall_faces": nfaces, "repetitions": n,
                      "a_ms_median": round(statistics.median(a), 4), "a_ms_min": round(min(a), 4), "a_ms_max": round(max(a), 4),
                      "b_ms_median": round(statistics.median(b), 2), "b_ms_min": round(min(b), 2), "b_ms_max": round(max(b), 2),
                      "b_bytes": state_bytes + stress_bytes, "a_read_bytes_per_face": 8 * READ_DOUBLES,
                      "a_write_bytes_per_face": 8 * WRITE_DOUBLES, "Fp": [float(v) for v in first[0, 0:3]],
                      "Fv": [float(v) for v in first[0, 3:6]], "yplusMax": float(first[0, 17])}), flush=True)
    eng.release_all()
    eng.close()


if __name__ == "__main__":
    main()
