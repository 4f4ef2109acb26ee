"""Pins the kernel dispatch: for a table of configurations one evaluation runs on the emulator (tests/hostsim) with its launch trace
switched on, and the ordered list of kernels launched must equal the list recorded in tests/dispatch_plan_table.json.

The table was recorded at the commit BEFORE the dispatch moved into plan_flow (adflow_amd/csrc/flow_plan.h), with the same trace hook
in the emulator.  A change of the dispatch has to change that table in the open:

    python tests/test_dispatch_plan.py --record tests/dispatch_plan_table.json

A name is the kernel as spelled at its launch site, template arguments included (`(k_roe_march<LIM, false, true, true>)`): renaming a
kernel or a template parameter changes the table too.  Runs of a repeated sub-sequence are folded: [[names...], count]."""
import ctypes
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))

import checks  # noqa: E402
from adflow_amd.params import (FlowParams, EulerEquations, NSEquations, RANSEquations, dissScalar, dissMatrix, upwind, vanAlbeda,  # noqa: E402
                               firstOrder, RungeKutta)
from adflow_amd.synth import make_block  # noqa: E402
from adflow_amd.topology import BrickTopology  # noqa: E402
from oracle import ref  # noqa: E402

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")
TABLE = os.path.join(HERE, "dispatch_plan_table.json")
EQ = {"euler": EulerEquations, "ns": NSEquations, "rans": RANSEquations}
SD = {"scalar": dict(spaceDiscr=dissScalar), "matrix": dict(spaceDiscr=dissMatrix, vis4=0.1),
      "upwind": dict(spaceDiscr=upwind, limiter=vanAlbeda), "upwind1": dict(spaceDiscr=upwind, limiter=firstOrder)}
WALLS = {1: -6, 2: -6, 3: -1, 4: -6, 5: -3, 6: -6}
EULER_WALLS = {1: -6, 2: -6, 3: -1, 4: -6, 5: -5, 6: -6}
DIMS = (7, 6, 5)


def prm_of(eq, sd, **kw):
    return FlowParams(equations=EQ[eq], **SD[sd], **kw)


def block_res(e, eq, sd, intermed=False, approx=None, moving=False):
    """blocketteRes core on one block; approx = (dissApprox, viscApprox, upwindFirstOrder)"""
    prm = prm_of(eq, sd)
    mk = dict(stretch_k=2.0) if eq != "euler" else {}
    if moving:
        mk["moving"] = True
    if approx:
        checks.check_block_res_approx(e, DIMS, prm, diss_approx=approx[0], visc_approx=approx[1], blockettes=approx[2], seed=5, **mk)
    elif intermed or moving:
        checks.check_block_res(e, DIMS, prm, seed=5, **mk)
    else:
        checks.check_block_res_vs_blockette(e, DIMS, prm.replace(dirScaling=True), seed=5, **mk)


def rk_stages(e, eq, sd):
    checks.check_rk_residual_sequence(e, DIMS, prm_of(eq, sd), **(dict(stretch_k=2.0) if eq != "euler" else {}))


def coarse(e, eq, sd):
    prm = prm_of(eq, sd, smoother=RungeKutta)
    checks.check_mg_cycle(e, BrickTopology(1, 1, 1, 8, 8, 4), prm, [0, 1, 0, -1], ncycles=1)


def rvec(e, eq, sd):
    checks.check_nk_residual(e, BrickTopology(1, 1, 1, *DIMS), prm_of(eq, sd), bc_spec=WALLS if eq != "euler" else EULER_WALLS, stretch_k=2.0)


def split(e, eq, sd):
    checks.check_blockette_res_with_bc(e, BrickTopology(2, 1, 1, 6, 5, 4, periodic=(True, False, False)), prm_of(eq, sd), WALLS, seed=7,
                                       split_eval=2, stretch_k=2.0)


def jac(e, eq, sd, ad=True, pc=False, viscPC=False):
    prm = prm_of(eq, sd)
    spec = WALLS if eq != "euler" else EULER_WALLS
    mk = dict(stretch_k=2.0) if eq != "euler" else {}
    if ad:
        checks.check_ad_jacobian(e, (4, 3, 3), prm, spec, usePC=pc, viscPC=viscPC, **mk)
    else:
        checks.check_fd_jacobian(e, (4, 3, 3), prm, spec, usePC=pc, viscPC=viscPC, **mk)


CASES = {}
for _eq in EQ:
    for _sd in SD:
        CASES[f"fine-{_eq}-{_sd}"] = (block_res, (_eq, _sd), {}, {})
CASES["intermed-euler-scalar"] = (block_res, ("euler", "scalar"), dict(intermed=True), {})
CASES["intermed-rans-upwind"] = (block_res, ("rans", "upwind"), dict(intermed=True), {})
CASES["coarse-euler-scalar"] = (coarse, ("euler", "scalar"), {}, {})
CASES["coarse-ns-upwind"] = (coarse, ("ns", "upwind"), {}, {})
for _eq, _sd in (("euler", "scalar"), ("euler", "upwind"), ("ns", "matrix"), ("ns", "upwind")):
    CASES[f"rk-{_eq}-{_sd}"] = (rk_stages, (_eq, _sd), {}, {})
for _sd in ("scalar", "matrix", "upwind"):
    CASES[f"approx-rans-{_sd}-diss+visc"] = (block_res, ("rans", _sd), dict(approx=(True, True, False)), {})
    CASES[f"approx-rans-{_sd}-diss"] = (block_res, ("rans", _sd), dict(approx=(True, False, False)), {})
CASES["approx-rans-upwind-diss+visc+first"] = (block_res, ("rans", "upwind"), dict(approx=(True, True, True)), {})
CASES["approx-rans-upwind-diss+first"] = (block_res, ("rans", "upwind"), dict(approx=(True, False, True)), {})
CASES["approx-euler-scalar-diss"] = (block_res, ("euler", "scalar"), dict(approx=(True, False, False)), {})
CASES["rvec-rans-upwind"] = (rvec, ("rans", "upwind"), {}, {})
CASES["rvec-rans-upwind-rvec_joint0"] = (rvec, ("rans", "upwind"), {}, dict(rvec_joint=0))
CASES["rvec-rans-scalar"] = (rvec, ("rans", "scalar"), {}, {})
for _eq, _sd in (("euler", "scalar"), ("euler", "upwind"), ("rans", "upwind"), ("rans", "matrix")):
    CASES[f"moving-{_eq}-{_sd}"] = (block_res, (_eq, _sd), dict(moving=True), {})
CASES["split-rans-upwind"] = (split, ("rans", "upwind"), {}, {})
CASES["split-ns-matrix"] = (split, ("ns", "matrix"), {}, {})
CASES["split-rans-scalar"] = (split, ("rans", "scalar"), {}, {})
for _sd in ("upwind", "scalar", "matrix"):
    CASES[f"ad-exact-rans-{_sd}"] = (jac, ("rans", _sd), dict(ad=True, pc=False), {})
    CASES[f"ad-pc-rans-{_sd}"] = (jac, ("rans", _sd), dict(ad=True, pc=True), {})
CASES["ad-pc-viscpc-rans-upwind"] = (jac, ("rans", "upwind"), dict(ad=True, pc=True, viscPC=True), {})
CASES["ad-pc-viscpc-ns-matrix"] = (jac, ("ns", "matrix"), dict(ad=True, pc=True, viscPC=True), {})
CASES["ad-exact-euler-upwind"] = (jac, ("euler", "upwind"), dict(ad=True, pc=False), {})
CASES["fd-pc-rans-upwind"] = (jac, ("rans", "upwind"), dict(ad=False, pc=True), {})
CASES["fd-pc-rans-scalar"] = (jac, ("rans", "scalar"), dict(ad=False, pc=True), {})
CASES["fd-pc-viscpc-rans-upwind"] = (jac, ("rans", "upwind"), dict(ad=False, pc=True, viscPC=True), {})
# every kernel-selection key on the configurations it affects
CASES["roe_march0-rans-upwind"] = (block_res, ("rans", "upwind"), {}, dict(roe_march=0))
CASES["roe_march0-ad-exact-rans-upwind"] = (jac, ("rans", "upwind"), dict(ad=True, pc=False), dict(roe_march=0))
CASES["roe_march0-fd-pc-rans-upwind"] = (jac, ("rans", "upwind"), dict(ad=False, pc=True), dict(roe_march=0))
CASES["inviscid_march0-rans-upwind"] = (block_res, ("rans", "upwind"), {}, dict(inviscid_march=0))
CASES["inviscid_march0-ns-matrix"] = (block_res, ("ns", "matrix"), {}, dict(inviscid_march=0))
CASES["inviscid_march0-approx-rans-upwind"] = (block_res, ("rans", "upwind"), dict(approx=(True, True, True)), dict(inviscid_march=0))
CASES["inviscid_march1-rans-scalar"] = (block_res, ("rans", "scalar"), {}, dict(inviscid_march=1))
CASES["inviscid_march1-ad-exact-rans-scalar"] = (jac, ("rans", "scalar"), dict(ad=True, pc=False), dict(inviscid_march=1))
CASES["viscous_tiled0-rans-upwind"] = (block_res, ("rans", "upwind"), {}, dict(viscous_tiled=0))
CASES["viscous_tiled0-approx-rans-upwind"] = (block_res, ("rans", "upwind"), dict(approx=(True, True, True)), dict(viscous_tiled=0))
CASES["viscous_tiled0-ad-exact-ns-upwind"] = (jac, ("ns", "upwind"), dict(ad=True, pc=False), dict(viscous_tiled=0))
CASES["viscous_tiled0-split-rans-upwind"] = (split, ("rans", "upwind"), {}, dict(viscous_tiled=0))
CASES["sa_march0-rans-upwind"] = (block_res, ("rans", "upwind"), {}, dict(sa_march=0))
CASES["sa_march0-split-rans-upwind"] = (split, ("rans", "upwind"), {}, dict(sa_march=0))
CASES["sa_march0-ad-pc-rans-upwind"] = (jac, ("rans", "upwind"), dict(ad=True, pc=True), dict(sa_march=0))
CASES["sa_march0-fd-pc-rans-upwind"] = (jac, ("rans", "upwind"), dict(ad=False, pc=True), dict(sa_march=0))
CASES["euler_march0-euler-scalar"] = (block_res, ("euler", "scalar"), {}, dict(euler_march=0))
CASES["euler_march0-rk-euler-scalar"] = (rk_stages, ("euler", "scalar"), {}, dict(euler_march=0))
CASES["pc_fused0-fd-pc-rans-upwind"] = (jac, ("rans", "upwind"), dict(ad=False, pc=True), dict(pc_fused=0))
CASES["pc_fused0-ad-pc-rans-upwind"] = (jac, ("rans", "upwind"), dict(ad=True, pc=True), dict(pc_fused=0))
CASES["pc_fused0-ad-exact-rans-upwind"] = (jac, ("rans", "upwind"), dict(ad=True, pc=False), dict(pc_fused=0))
CASES["pc_fused0-ad-exact-ns-matrix"] = (jac, ("ns", "matrix"), dict(ad=True, pc=False), dict(pc_fused=0))
CASES["pc_fused0-approx-rans-matrix"] = (block_res, ("rans", "matrix"), dict(approx=(True, True, False)), dict(pc_fused=0))
CASES["jac_snap0-fd-pc-rans-upwind"] = (jac, ("rans", "upwind"), dict(ad=False, pc=True), dict(jac_snap=0))

DEFAULTS = {"roe_march": 1, "inviscid_march": 2, "viscous_tiled": 2, "sa_march": 1, "euler_march": 1, "pc_fused": 1, "rvec_joint": 1,
            "jac_snap": 1, "split_eval": 1}


def fold(seq):
    """[a, b, a, b, a, b, c] -> [[[a, b], 3], c]: the longest run of the shortest repeated sub-sequence at every position"""
    out, i, n = [], 0, len(seq)
    while i < n:
        best = (1, 1)
        for p in range(1, min(48, (n - i) // 2) + 1):
            r = 1
            while seq[i + r * p:i + (r + 1) * p] == seq[i:i + p]:
                r += 1
            if r > 1 and r * p > best[0] * best[1]:
                best = (p, r)
        p, r = best
        out.append([seq[i:i + p], r] if r > 1 else seq[i])
        i += p * r
    return out


def unfold(folded):
    out = []
    for x in folded:
        out += x[0] * x[1] if isinstance(x, list) else [x]
    return out


def trace_of(engine, name):
    from hostsim.build import LIB
    lib = ctypes.CDLL(LIB)
    lib.hostsim_trace_read.restype = ctypes.c_long
    lib.hostsim_trace_read.argtypes = [ctypes.c_char_p, ctypes.c_long]
    fn, args, kw, tune = CASES[name]
    for k, v in tune.items():
        engine.set_tuning(k, v)
    lib.hostsim_trace_start(1)
    try:
        fn(engine, *args, **kw)
        n = lib.hostsim_trace_read(None, 0)
        buf = ctypes.create_string_buffer(n)
        assert lib.hostsim_trace_read(buf, n) == n
    finally:
        lib.hostsim_trace_start(0)
        for k, v in DEFAULTS.items():
            engine.set_tuning(k, v)
    return [line.rsplit(" ", 2)[0] for line in buf.value.decode().splitlines()]


@pytest.mark.parametrize("name", sorted(CASES))
def test_dispatch(hostsim_engine, name):
    expected = unfold(json.load(open(TABLE))[name])
    got = trace_of(hostsim_engine, name)
    assert got == expected, next((i, g, x) for i, (g, x) in enumerate(zip(got + [None], expected + [None])) if g != x)


def test_fold_roundtrip():
    s = list("xababab") + ["c"] * 5 + list("abcabcd")
    assert unfold(fold(s)) == s and len(fold(s)) < len(s)


if __name__ == "__main__":
    assert sys.argv[1] == "--record"
    from adflow_amd.engine import Engine
    from hostsim.build import build
    eng = Engine(0, _lib_path=build())
    table = {}
    for nm in sorted(CASES):
        table[nm] = fold(trace_of(eng, nm))
        print(nm, len(unfold(table[nm])), flush=True)
    with open(sys.argv[2], "w") as f:
        f.write("{\n" + ",\n".join(f' {json.dumps(k)}: {json.dumps(v)}' for k, v in sorted(table.items())) + "\n}\n")
    eng.close()
