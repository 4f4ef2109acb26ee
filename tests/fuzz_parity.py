"""Randomised parity sweep: block sizes, options and entry points drawn at random, every case checked against the reference's
own Fortran (oracle/_ref) at the 1e-10 bar of tests/util.py.  Test infrastructure, not a test module: run it by hand,

    python tests/fuzz_parity.py --cases 200 --seed 7             # kernel-logic emulator (CPU only)
    python tests/fuzz_parity.py --cases 200 --seed 7 --gpu       # the HIP library on cuda:0

It prints one line per case and stops at the first failure with the arguments that reproduce it.  The sizes are chosen around the
tile edges of the marching kernels (60 / 62 produced columns of 64 lanes, 4 rows, k chunks of 32 / 22 planes)."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import checks  # noqa: E402
from adflow_amd.params import (FlowParams, EulerEquations, NSEquations, RANSEquations, dissScalar, dissMatrix, upwind,  # noqa: E402
                               noLimiter, vanAlbeda, minmod, firstOrder, secondOrder, DADI, RungeKutta, noResAveraging,
                               alternateResAveraging)
from adflow_amd.topology import BrickTopology  # noqa: E402

# BCType: -1 symm, -3 adiabatic wall, -4 isothermal wall, -5 Euler wall, -6 farfield, -7 supersonic inflow, -9 supersonic outflow,
# -15 extrap
EULER_BC = [-1, -5, -6, -7, -9, -15]
VISC_BC = [-1, -3, -4, -6, -7, -9, -15]

EDGE_NX = [1, 2, 3, 5, 58, 59, 60, 61, 62, 63, 64, 65, 119, 120, 121, 124, 125]
EDGE_NY = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14]
EDGE_NZ = [1, 2, 3, 5, 20, 21, 22, 23, 31, 32, 33, 34, 43, 44, 45]


def draw_case(rng, huge=False):
    eq = int(rng.choice([EulerEquations, NSEquations, RANSEquations], p=[0.25, 0.25, 0.5]))
    sd = int(rng.choice([dissScalar, dissMatrix, upwind], p=[0.3, 0.2, 0.5]))
    big = rng.random() < 0.35
    nx = int(rng.choice(EDGE_NX)) if big else int(rng.integers(1, 14))
    ny = int(rng.choice(EDGE_NY))
    nz = int(rng.choice(EDGE_NZ)) if (big and nx < 70) else int(rng.integers(1, 12))
    kw = dict(equations=eq, spaceDiscr=sd)
    if sd == upwind:
        kw["limiter"] = int(rng.choice([noLimiter, vanAlbeda, minmod]))
        kw["kappaCoef"] = float(rng.choice([1.0 / 3.0, -1.0, 0.0, 0.5]))
    else:
        kw["vis2"] = float(rng.choice([0.25, 0.0, 0.5]))
        kw["vis4"] = float(rng.choice([0.0156, 0.1, 0.03]))
        kw["dirScaling"] = bool(rng.random() < 0.8)
        kw["adis"] = float(rng.choice([0.67, 1.0, 0.5]))
    if eq == RANSEquations:
        kw["useQCR"] = bool(rng.random() < 0.3)
        kw["orderTurb"] = int(rng.choice([firstOrder, secondOrder]))
        kw["useRotationSA"] = bool(rng.random() < 0.2)
        kw["useft2SA"] = bool(rng.random() < 0.7)
    if eq != EulerEquations and rng.random() < 0.4:
        kw["muSuthDim"] = 1.0          # viscous-dominated
    if huge:     # GPU runs: several i tiles, many j tiles, three or more k chunks
        nx, ny, nz = int(rng.integers(100, 201)), int(rng.integers(5, 41)), int(rng.integers(40, 101))
    mk = dict(seed=int(rng.integers(1, 10 ** 6)))
    if rng.random() < 0.5:
        mk["stretch_k"] = float(rng.choice([1.5, 2.0, 3.0]))
    if rng.random() < 0.3:
        mk["holes"] = 0.05
    if rng.random() < 0.15:
        mk["left_handed"] = True
    entry = str(rng.choice(["block_res", "blockette", "blockette_intermed", "approx", "bc", "rk", "dadi", "sa_solve", "nk", "full_bc", "ad",
                            "mg", "lattice"],
                           p=[0.18, 0.07, 0.07, 0.07, 0.11, 0.07, 0.07, 0.05, 0.05, 0.09, 0.05, 0.07, 0.05]))
    if huge:
        entry = str(rng.choice(["block_res", "blockette", "blockette_intermed"]))
    if eq != EulerEquations and entry in ("block_res", "blockette", "blockette_intermed", "approx"):
        # meshes far from the origin, clustered to wall spacings down to 1.65e-5 of the block: where a kernel that subtracts
        # absolute coordinates loses what the reference's node differences keep.  (A stream of its own, seeded by the case: the
        # other draws of a case stay what they were.)
        far = np.random.default_rng(mk["seed"])
        o = float(far.choice([0.0, 300.0, 3000.0]))
        if o != 0.0:
            mk["origin"] = (o, -2.0 * o, 0.5 * o)
        if far.random() < 0.5:
            mk["stretch_k"] = float(far.choice([5.0, 8.0, 11.0]))
    if entry == "bc":
        kinds = EULER_BC if eq == EulerEquations else VISC_BC
        mk["spec"] = {f: int(rng.choice(kinds)) for f in range(1, 7)}
        mk["secondHalo"] = bool(rng.random() < 0.6)
        mk.pop("left_handed", None)
    if entry == "full_bc":
        # round 4: the whole blocketteRes on a brick whose ends are physical boundaries (closures, BCs, whalo2, core, wall stress)
        kinds = [-1, -5, -6, -15] if eq == EulerEquations else [-1, -3, -4, -6, -15]
        wide = rng.random() < 0.25
        mk = dict(seed=mk["seed"], topo=(int(rng.integers(1, 3)), int(rng.integers(1, 3)), int(rng.integers(1, 3)),
                                       int(rng.choice([61, 70, 125])) if wide else int(rng.integers(3, 14)), int(rng.integers(3, 9)),
                                       int(rng.integers(3, 8))),
                  spec={f: int(rng.choice(kinds)) for f in range(1, 7)}, floor_p=bool(eq != RANSEquations and rng.random() < 0.2),     # (RANS with floored pressures: the reference itself yields NaN)
                  split_eval=(2 if rng.random() < 0.3 else None))
        if rng.random() < 0.5:
            mk["stretch_k"] = 2.0
        if "dirScaling" in kw:
            kw["dirScaling"] = True     # (blocketteResCore, the reference of this entry, scales the dissipation unconditionally)
    if entry == "ad":
        # round 4: forward-mode assembly against the reference's Tapenade routines (no extrapolation faces under the exact
        # linearisation: DESIGN 5)
        usePC = bool(rng.random() < 0.6)
        kinds = ([-1, -5, -6] if eq == EulerEquations else [-1, -3, -4, -6]) + ([-15, -9] if usePC else [])
        mk = dict(seed=mk["seed"], spec={f: int(rng.choice(kinds)) for f in range(1, 7)}, usePC=usePC,
                  frozenTurb=bool(eq == RANSEquations and rng.random() < 0.2))
        nx, ny, nz = int(rng.integers(3, 9)), int(rng.integers(3, 7)), int(rng.integers(3, 6))
        if eq != EulerEquations:
            mk["stretch_k"] = 2.0
    if entry == "mg":
        # round 5: multigrid cycles on blocks of ANY cell count (odd counts coarsen irregularly: half-weight cells), 2 or 3 levels,
        # periodic bricks or one block with six boundary subfaces of which some are cut in two (the cut survives the coarsening)
        nlev = int(rng.integers(2, 4))
        lo = 4 if nlev == 2 else 8
        dims3 = (int(rng.integers(lo, 22)), int(rng.integers(lo, 16)), int(rng.integers(lo, 12)))
        withbc = bool(rng.random() < 0.5)
        kinds = [-1, -5, -6] if eq == EulerEquations else [-1, -6]      # (viscous: the wall is put on kMin below, where d2Wall points)
        mk = dict(seed=mk["seed"], nlev=nlev, dims3=dims3, nb=(1 if withbc else int(rng.integers(1, 3))),
                  spec=({f: int(rng.choice(kinds)) for f in range(1, 7)} if withbc else None),
                  split=({int(rng.choice([3, 5])): int(rng.choice(kinds))} if withbc and rng.random() < 0.5 else None),
                  dadi=bool(rng.random() < 0.4))
        kw["resAveraging"] = int(rng.choice([noResAveraging, alternateResAveraging]))
        # (what this entry must NOT draw: cycles that blow up in the reference itself and then amplify rounding -- measured: the
        # unlimited fully-upwind scheme between four inviscid walls drives wall pressures to the floor of bcEulerWall within one sweep;
        # RANS + SA cycles on 20-cell blocks reach NaN in the second cycle)
        if kw.get("limiter") == noLimiter:
            kw["limiter"] = vanAlbeda
        # (and: a smoother sweep on the noisy synthetic state can leave p3 >= 2 p2 at an inviscid wall; the linear extrapolation of
        # bcEulerWall then floors the halo pressure at exactly 0, the Roe average between that halo and its cell has a^2 ~ 1e-17 and
        # 1 / a turns rounding into O(1) -- in the reference as much as here.  Constant extrapolation keeps the walls in the draw)
        kw["eulerWallBCTreatment"] = 1
        if eq == RANSEquations:
            kw["equations"] = NSEquations
            for k_ in ("useQCR", "orderTurb", "useRotationSA", "useft2SA"):
                kw.pop(k_, None)
        if "vis2" in kw:
            kw["vis2"] = max(kw["vis2"], 0.25)
        if eq != EulerEquations:
            mk["stretch_k"] = 2.0
    if entry == "lattice":
        # round 5: the four-block mesh with rotated / reversed / left-handed index systems, one consumer of the lists at random
        mk = dict(seed=mk["seed"], what=str(rng.choice(["whalo", "loopback", "coor", "res_bc", "rk", "dadi", "mg_bc", "nk"])),
                  scale=1, layers=int(rng.integers(1, 3)), split_eval=(2 if rng.random() < 0.5 else None))
        if eq != EulerEquations:
            mk["stretch_z"] = 2.0
    if entry in ("rk", "dadi", "sa_solve", "nk"):
        # periodic bricks of 1 - 2 blocks; even cell counts are not needed on a single grid.  One case in four with i lines of more
        # than one wavefront (the cyclic-reduction kernels of round 4)
        wide = rng.random() < 0.25 and entry != "nk"
        mk = dict(seed=mk["seed"], topo=(int(rng.integers(1, 3)), int(rng.integers(1, 3)), 1,
                                       int(rng.choice([65, 70, 129, 190, 250])) if wide else int(rng.integers(3, 20)),
                                       int(rng.integers(3, 10)), int(rng.integers(3, 9))))
        if entry == "sa_solve":
            kw["equations"] = RANSEquations
            kw["nSubIterTurb"] = int(rng.integers(1, 3))
        if entry in ("rk", "dadi"):
            kw["resAveraging"] = int(rng.choice([noResAveraging, alternateResAveraging]))
    return (nx, ny, nz), kw, mk, entry


def draw_jac_case(rng):
    """--jac (late round 5): the two assemblies of setupStateResidualMatrix only -- forward mode and finite differences, mostly the
    preconditioner matrix on the upwind scheme (the marching kernels k_pc_march / k_sa_march, plain and dual), blocks of one to three
    tiles per direction with partial tiles, random boundary kinds, frozenTurb / useTurbOnly"""
    eq = int(rng.choice([EulerEquations, NSEquations, RANSEquations], p=[0.1, 0.3, 0.6]))
    sd = int(rng.choice([dissScalar, dissMatrix, upwind], p=[0.1, 0.1, 0.8]))
    kw = dict(equations=eq, spaceDiscr=sd)
    if sd == upwind:
        kw["limiter"] = int(rng.choice([noLimiter, vanAlbeda, minmod]))
    else:
        kw["vis4"] = float(rng.choice([0.0156, 0.1]))
    if eq == RANSEquations:
        kw["orderTurb"] = int(rng.choice([firstOrder, secondOrder]))
        kw["useft2SA"] = bool(rng.random() < 0.7)
    if eq != EulerEquations and rng.random() < 0.3:
        kw["muSuthDim"] = 1.0          # viscous-dominated
    entry = "ad" if rng.random() < 0.5 else "pc"
    usePC = bool(rng.random() < 0.85)
    kinds = ([-1, -5, -6] if eq == EulerEquations else [-1, -3, -4, -6]) + ([-15, -9] if usePC else [])
    turb = float(rng.random())
    mk = dict(seed=int(rng.integers(1, 10 ** 6)), spec={f: int(rng.choice(kinds)) for f in range(1, 7)}, usePC=usePC,
              frozenTurb=bool(eq == RANSEquations and turb < 0.2), useTurbOnly=bool(eq == RANSEquations and usePC and 0.2 <= turb < 0.35))
    wide = rng.random() < 0.2
    nx = int(rng.choice([58, 60, 61, 64, 121])) if wide else int(rng.integers(3, 12))
    ny = int(rng.integers(3, 11))
    nz = int(rng.integers(3, 8)) if wide else int(rng.choice([3, 4, 5, 6, 7, 20, 33]))
    if eq != EulerEquations:
        mk["stretch_k"] = 2.0
    return (nx, ny, nz), kw, mk, entry


# the reference's Runge-Kutta stage sets next to the default five-stage one (inputParamRoutines.F90:3576-3635): {nRKStages: (etaRK, cdisRK)}
STAGE_SETS = {1: ([1.0], [1.0]), 2: ([0.2222, 1.0], [1.0, 1.0]), 3: ([0.2846, 0.6067, 1.0], [1.0, 1.0, 1.0]),
              4: ([0.33333333, 0.26666667, 0.55555555, 1.0], [1.0, 0.5, 0.0, 0.0]),
              6: ([0.0722, 0.1421, 0.2268, 0.3425, 0.5349, 1.0], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0])}


def draw_options(orng, kw, mk, entry):
    """options that every earlier draw left at their defaults: the gas model, the free stream, the stage set, the explicit turbulence
    relaxation.  A stream of its own (the cases of a seed keep their sizes, schemes and entries), and each option only where the entry
    reads it and the reference stays finite: no free-stream change under the multigrid cycles and the lattice (their draws are
    tuned to states that survive a cycle), the supersonic free stream only where no smoother sweep follows."""
    out = {}
    eq = kw["equations"]
    if entry in ("mg", "lattice"):
        return out
    if orng.random() < 0.4:
        out["gammaConstant"] = float(orng.choice([1.3, 1.5]))
        if mk.get("floor_p"):
            out.pop("gammaConstant")          # (check_blockette_res_with_bc floors with the factor 0.4 = gamma - 1 of the default gas)
    if eq != EulerEquations and orng.random() < 0.4:
        out["prandtl"] = float(orng.choice([0.9, 0.6]))
        out["prandtlTurb"] = float(orng.choice([0.6, 0.8]))
    if orng.random() < 0.4:
        quiet = entry in ("rk", "dadi", "sa_solve")
        out["Mach"] = float(orng.choice([0.3, 0.6] if quiet else [0.3, 1.3, 2.0]))
        out["alphaDeg"] = float(orng.choice([-7.0, 0.0, 12.0]))
    if entry == "rk" and orng.random() < 0.6:
        n = int(orng.choice(sorted(STAGE_SETS)))
        out.update(nRKStages=n, etaRK=list(STAGE_SETS[n][0]), cdisRK=list(STAGE_SETS[n][1]))
    if entry in ("sa_solve", "dadi") and eq == RANSEquations and orng.random() < 0.5:
        out.update(turbRelax=1, alfaTurb=float(orng.choice([0.6, 0.9])))
    return out


def run_case(engine, dims, kw, mk, entry):
    prm = FlowParams(**kw)
    mk = dict(mk)
    seed = mk.pop("seed")
    if entry == "approx":
        mk.pop("left_handed", None)
        checks.check_block_res_approx(engine, dims, prm, seed=seed, **mk)
    elif entry == "bc":
        spec, second = mk.pop("spec"), mk.pop("secondHalo")
        checks.check_apply_bc(engine, (max(dims[0], 2), max(dims[1], 2), max(dims[2], 1)), prm, spec, secondHalo=second, seed=seed, **mk)
    elif entry == "full_bc":
        t = mk.pop("topo")
        if prm.equations == RANSEquations and not any(v in (-3, -4) for v in mk["spec"].values()):
            mk["spec"][5] = -3          # SA wants a wall distance that means something
        checks.check_blockette_res_with_bc(engine, BrickTopology(*t, periodic=(False, False, False)), prm, mk.pop("spec"), seed=seed,
                                           allow_degenerate=mk.get("floor_p", False), **mk)
    elif entry == "ad":
        checks.check_ad_jacobian(engine, dims, prm, mk.pop("spec"), usePC=mk.pop("usePC"), frozenTurb=mk.pop("frozenTurb"), seed=seed, **mk)
    elif entry == "pc":
        checks.check_fd_jacobian(engine, dims, prm, mk.pop("spec"), usePC=mk.pop("usePC"), frozenTurb=mk.pop("frozenTurb"), seed=seed, **mk)
    elif entry == "mg":
        nlev, d3 = mk.pop("nlev"), mk.pop("dims3")
        cyc = [0, 1, 0, -1] if nlev == 2 else [0, 1, 0, 1, 0, -1, 0, 1, 0, -1, 0, -1]
        p2 = prm.replace(smoother=DADI, cfl=1.5, resAveraging=noResAveraging) if mk.pop("dadi") else prm.replace(smoother=RungeKutta)
        if p2.equations == RANSEquations:
            p2 = p2.replace(smoother=DADI, cfl=1.5, resAveraging=noResAveraging, nSubiterations=2, nSubIterTurb=2)
        spec, split, nb = mk.pop("spec"), mk.pop("split"), mk.pop("nb")
        if spec and p2.equations != EulerEquations:
            spec[5] = -3
            if split and 5 in split:
                split = {3: split[5]}
        checks.check_mg_cycle(engine, BrickTopology(nb, 1, 1, *d3), p2, cyc, ncycles=1, nlevels=nlev, bc_spec=spec, bc_split=split, seed=seed,
                              allow_degenerate=True, **mk)
    elif entry == "lattice":
        from adflow_amd.topology import ell_topology
        what, layers, se = mk.pop("what"), mk.pop("layers"), mk.pop("split_eval")
        topo = ell_topology(mk.pop("scale"), stretch_z=mk.pop("stretch_z", 1.0))
        walls = {1: -6, 2: -6, 3: -1, 4: -6, 5: (-3 if prm.equations != EulerEquations else -5), 6: -6}
        if what == "whalo":
            checks.check_halo_exchange(engine, topo, prm, layers, seed=seed)
        elif what == "loopback":
            checks.check_halo_loopback(engine, topo, int(2 + seed % 3), prm, layers, seed=seed)
        elif what == "coor":
            checks.check_coordinate_halos_brick(engine, topo, prm, seed=seed)
        elif what == "res_bc":
            checks.check_blockette_res_with_bc(engine, topo, prm.replace(dirScaling=True), walls, seed=seed, split_eval=se)
        elif what == "rk":
            checks.check_rk_smoother(engine, topo, prm.replace(smoother=RungeKutta), seed=seed)
        elif what == "dadi":
            checks.check_dadi_smoother(engine, topo, prm.replace(smoother=DADI, cfl=1.5, resAveraging=noResAveraging), seed=seed)
        elif what == "mg_bc":
            p2 = prm.replace(smoother=RungeKutta)
            if p2.equations == RANSEquations:
                p2 = p2.replace(smoother=DADI, cfl=1.5, resAveraging=noResAveraging, nSubiterations=2, nSubIterTurb=2)
            checks.check_mg_cycle(engine, topo, p2, [0, 1, 0, -1], ncycles=1, brick_spec=walls, seed=seed)
        else:
            checks.check_nk_residual(engine, topo, prm, seed=seed)
    elif entry in ("rk", "dadi", "sa_solve", "nk"):
        topo = BrickTopology(*mk.pop("topo"))
        if entry == "rk":
            checks.check_rk_smoother(engine, topo, prm.replace(smoother=RungeKutta), seed=seed)
        elif entry == "dadi":
            checks.check_dadi_smoother(engine, topo, prm.replace(smoother=DADI, cfl=1.5), seed=seed)
        elif entry == "sa_solve":
            checks.check_sa_solve(engine, topo, prm, seed=seed)
        else:
            checks.check_nk_residual(engine, topo, prm, seed=seed)
    elif entry == "block_res" or not kw.get("dirScaling", True):
        # (blocketteResCore scales the dissipation unconditionally: the dirScaling = F case has blockResCore as its reference)
        checks.check_block_res(engine, dims, prm, seed=seed, **mk)
    else:
        checks.check_block_res_vs_blockette(engine, dims, prm, update_intermed=(entry == "blockette_intermed"), seed=seed, **mk)


# tuning keys that select between kernels: key, the non-default settings drawn
KERNEL_KEYS = [("roe_march", [0]), ("inviscid_march", [0, 1]), ("viscous_tiled", [0]), ("sa_march", [0]), ("euler_march", [0]),
               ("dadi_pcr", [0]), ("dadi_upd", [0]), ("ra_pcr", [0]), ("rvec_joint", [0]), ("metric_from_x", [0, 1, 4])]
KERNEL_DEFAULTS = {"roe_march": 1, "inviscid_march": 2, "viscous_tiled": 2, "sa_march": 1, "euler_march": 1, "dadi_pcr": 1, "dadi_upd": 1,
                   "ra_pcr": 1, "rvec_joint": 1, "metric_from_x": 5}


ALL_DEFAULTS = {"split_eval": 1, "pc_fused": 1, "jac_snap": 1, **KERNEL_DEFAULTS}

# entries whose mesh a family may replace: the ones that build single blocks or periodic bricks with make_block's keywords (the
# lattice has its own map; the multigrid cycles and the smoother sweeps are tuned to states that survive on the cube)
FAMILY_ENTRIES = ("block_res", "blockette", "blockette_intermed", "approx", "bc", "nk", "full_bc", "ad")


def draw_family(frng, mk, entry):
    """the mesh family (tests/mesh_families.py) and the unit of length of a case, from a stream of its own: {} or the keywords shape /
    lengths of make_block.  `pole` only under the residual entries: the entries with boundary subfaces build them with make_bocos,
    whose unit normals of a collapsed face (0 / 0) need the definition that mesh_checks._finite_bocos gives them."""
    import mesh_families as mf
    out = {}
    if entry not in FAMILY_ENTRIES or mk.get("left_handed"):
        return out
    names = ["annulus", "sheared", "clustered"] + (["pole"] if entry in ("block_res", "blockette", "blockette_intermed") else [])
    name = str(frng.choice(names + ["cube"]))
    if name != "cube":
        out["shape"] = mf.family(name)
        # the far-origin draw's clustering (exp(11 z), halo nodes at z = 2 on a one-cell block) is made for the cube: under a map with a
        # growth law of its own it overflows; the family keeps the mild clustering only
        if mk.get("stretch_k", 1.0) > 3.0 or name in ("annulus", "clustered"):
            out["stretch_k"] = 2.0 if name in ("sheared", "pole") else 1.0
    k = int(frng.integers(0, len(mf.UNIT_LENGTHS) + 2))
    if k < len(mf.UNIT_LENGTHS):
        out["lengths"] = mf.UNIT_LENGTHS[k]
    return out


def cases_of(cases, seed, big=False, jac=False, families=False):
    """the cases of a sweep, in order: (n, dims, options, make_block keywords, entry, tuning keys)"""
    rng = np.random.default_rng(seed)
    for n in range(cases):
        dims, kw, mk, entry = draw_jac_case(rng) if jac else draw_case(rng, big)
        # round 5: the tuning keys of the new code paths at random (results never depend on them)
        # (four draws of keys that round 6 removed stay, so that earlier seeds replay as they were)
        rng.choice([0, 1, 2]); rng.integers(0, 2); rng.choice([4, 8]); rng.integers(0, 2)
        tune = {"pc_fused": n % 2, "jac_snap": (n // 2) % 2}      # (pc_fused, jac_snap without a draw: earlier seeds replay as they were)
        # round 6: the kernel-selection keys too -- in one case of three, one or two of the marching kernels are switched off, so that the
        # kernels behind them (gather forms, the per-face march under the Roe march) meet every scheme / boundary / size the sweep draws
        # (their own stream of random numbers: the cases of a seed stay what they were)
        trng = np.random.default_rng([seed, n, 6])
        if trng.random() < 1.0 / 3.0:
            for _ in range(int(trng.integers(1, 3))):
                k_, vals = KERNEL_KEYS[int(trng.integers(0, len(KERNEL_KEYS)))]
                tune[k_] = int(trng.choice(vals))
        # the options no earlier draw moved (draw_options), again from a stream of their own
        kw = {**kw, **draw_options(np.random.default_rng([seed, n, 7]), kw, mk, entry)}
        if families:
            # the mesh family and the unit of length: a stream seeded by the case's own seed, as the far-origin draw's is
            mk = {**mk, **draw_family(np.random.default_rng([int(mk["seed"]), 8]), mk, entry)}
        yield n, dims, kw, mk, entry, tune


def describe(dims, kw, mk, entry, tune):
    """a case as one line of text (tests/golden/fuzz_sweep_cases.json holds the lines of the 300 cases of test_random_parity_sweep)"""
    return repr((tuple(int(d) for d in dims), entry, sorted(kw.items()), sorted((k, str(v)) for k, v in mk.items()),
                 sorted({**ALL_DEFAULTS, **tune}.items())))


def sweep(engine, cases, seed, only=-1, quiet=False, big=False, jac=False, families=False):
    """Run `cases` random cases; returns (number run, description of the first failure or None).
    families: the mesh family and the lengths drawn too (draw_family); without it the cases are what they always were."""
    for n, dims, kw, mk, entry, tune in cases_of(cases, seed, big, jac, families):
        if only >= 0 and n != only:
            continue
        try:
            for k_, v_ in tune.items():
                engine.set_tuning(k_, v_)
            run_case(engine, dims, kw, mk, entry)
            if not quiet:
                print(f"[{n:4d}] ok   {dims} {entry} {kw} {mk} {tune}", flush=True)
        except AssertionError as ex:
            return n + 1, f"case {n} (seed {seed}): {dims} {entry} {kw} {mk} {tune}: {ex}"
        finally:
            for k_, v_ in ALL_DEFAULTS.items():
                engine.set_tuning(k_, v_)
    return cases, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--gpu", action="store_true", help="the HIP library on cuda:0 instead of the emulator")
    ap.add_argument("--only", type=int, default=-1, help="run this case index only")
    ap.add_argument("--big", action="store_true", help="blocks of 100-200 x 5-40 x 40-100 cells (residual entry points only; for --gpu)")
    ap.add_argument("--jac", action="store_true", help="the Jacobian assemblies only (draw_jac_case)")
    ap.add_argument("--families", action="store_true", help="draw the mesh family and the unit of length too (tests/mesh_families.py)")
    a = ap.parse_args()
    from adflow_amd.engine import Engine
    if a.gpu:
        eng = Engine(0)
    else:
        from hostsim.build import build
        eng = Engine(0, _lib_path=build())
    t0 = time.time()
    n, failure = sweep(eng, a.cases, a.seed, a.only, big=a.big, jac=a.jac, families=a.families)
    if failure:
        print("FAIL", failure)
        print(f"reproduce: python tests/fuzz_parity.py --seed {a.seed} --cases {a.cases} --only {n - 1}" + (" --gpu" if a.gpu else "")
              + (" --big" if a.big else "") + (" --jac" if a.jac else "")
              + (" --families" if a.families else ""))
    print(f"{n} cases, {1 if failure else 0} failures, {time.time() - t0:.0f} s")
    nfail = 1 if failure else 0
    eng.close()
    return 1 if nfail else 0


if __name__ == "__main__":
    sys.exit(main())
