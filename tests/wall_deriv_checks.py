"""TEST INFRASTRUCTURE.  Derivatives of the surface integration with respect to the state: adflow_gpu_wall_integrate_fwd (the funcsDot
of master_d for the wall subfaces, one forward-mode pass) and adflow_gpu_wall_integrate_bwd (the wbar of master_b, a coloured sweep
of the same pass), csrc/kernels_wallint.hip compiled for dual numbers.

Yardstick.  surfaceIntegrations is one of the modules the oracle stubs, so there is no wallIntegrationFace_d to call: the yardstick is
the REFERENCE CHAIN DIFFERENTIATED NUMERICALLY.  Every block is bound to the oracle; computePressureSimple / computeLamViscosity /
computeEddyViscosity with halos, applyAllBC_block, timeStep_block, initres_flow and residual_block with rkStage = 0 run at the states
w +- h v and w +- (h / 2) v (interface halos filled from their donors in numpy first); p, w, rlv and the stored tau of the reference go
through the numpy face_terms of wall_force_checks; the derivative of every face term is the Richardson combination (4 D(h/2) - D(h)) / 3
of the two central differences.  v is random, every component scaled by the mean magnitude of that state variable; h = H below.

Bar.  For every case and entry the distance between the Richardson values of (h, h/2) and of (h/2, h/4) is the yardstick's own noise.
It is measured relative to M_e = sum over the faces |d t_i|, the magnitude sum of the per-face derivatives, so that cancellation between
faces cannot flatter it.  measure_floor() prints the ratio per case; the largest over all cases of this file and all entries, measured
on the CPU, is FLOOR, and the one bar of every comparison with the yardstick is BAR = 10 FLOOR (the factor covers the dependence of
that noise on the step).  Every comparison asserts M_e > 0 for the force entries, so a zero result cannot pass.

tests/test_gpu_wall_deriv.py runs the checkers on the MI355X, tests/test_hostsim_wall_deriv.py on the emulator."""
import numpy as np

import device_vectors  # noqa: F401  (torch before the library: see its docstring)
import async_checks
import checks
import wall_force_checks as wf
from adflow_amd import capi, synth
from adflow_amd.topology import BrickTopology, LatticeBlock, LatticeTopology, apply_local_copies_fast
from util import TOL

H = 2.0 ** -13                  # the step of the yardstick, relative to the scale of each state variable: the one of 2^-9, 2^-11,
                                # 2^-13, 2^-15 with the least noise (1.1e-7, 4.5e-10, 1.5e-10, 1.8e-9: truncation left, rounding right)
FLOOR = 1.523669424422693e-10   # the largest |R(h, h/2) - R(h/2, h/4)| / M_e over the cases below and all entries (measure_floor)
BAR = 10.0 * FLOOR
ALLWALL = {1: -6, 2: -6, 3: -6, 4: -6, 5: -3, 6: -6}


class DCase(wf.Case):
    """wall_force_checks.Case with, optionally, blocks joined by 1-to-1 interfaces (a topology), and the reference chain at a
    perturbed state"""

    def __init__(self, prm, topo=None, spec=None, seed=57, fam=None, blank=None, **mk):
        super().__init__(prm)
        self.topo, self.pats = topo, None
        self.faminfo, self.blankinfo = fam or {}, blank or {}
        if topo is not None:
            blocks = checks.make_brick(topo, self.prm, seed, wall_kmin=False, **mk)
            lid = topo.local_ids()
            for g in range(topo.nblocks):
                nn = lid[g]
                faces, nvisc = synth.make_bocos(blocks[nn], self.prm, topo.boundary_spec(g, spec), seed=seed + 31 * g + 1)
                synth.set_porosities(blocks[nn], faces)
                self.blks[nn], self.bocos[nn] = blocks[nn], (faces, nvisc)
            self.pats = {L: topo.patterns(L)[0] for L in (1, 2)}
            apply_local_copies_fast(self.blks, self.pats[2])
            self._finish()

    def add(self, nn, dims, spec, split=(), seed=57, fam=None, blank=None, **mk):
        blk = checks._make_block(*dims, self.prm, seed=seed, **mk)
        self.blks[nn] = blk
        self.bocos[nn] = synth.make_bocos(blk, self.prm, spec, seed=seed + 1, split=split)
        self.faminfo.update({(nn, m): f for m, f in (fam or {}).items()})
        self.blankinfo.update({(nn, m): b for m, b in (blank or {}).items()})
        return self._finish()

    def _finish(self):
        for nn, (faces, _) in self.bocos.items():
            self.fam[nn] = [int(self.faminfo.get((nn, m + 1), 0)) for m in range(len(faces))]
            self.blank[nn] = [self.blankinfo.get((nn, m + 1)) for m in range(len(faces))]
        self.inputs = self.ref_inputs(None)
        return self

    @property
    def nw(self):
        return self.prm.nw

    def ncells(self):
        return sum(b.ncells for b in self.blks.values())

    def scatter(self, v, l0, ns):
        """a vector in the PETSc layout (block, k, j, i, ns variables from l0 fastest) -> {nn: (nx, ny, nz, nw)}"""
        out, off = {}, 0
        for nn in sorted(self.blks):
            b = self.blks[nn]
            n = b.ncells * ns
            d = np.zeros((b.nx, b.ny, b.nz, self.nw))
            d[..., l0:l0 + ns] = np.transpose(v[off:off + n].reshape(b.nz, b.ny, b.nx, ns), (2, 1, 0, 3))
            out[nn] = d
            off += n
        return out

    def ref_inputs(self, dw):
        """the reference chain on every block at w + dw (dw: {nn: owned (nx, ny, nz, nw)} or None): face_inputs of every wall subface"""
        from oracle import ref
        copies = {nn: b.copy() for nn, b in self.blks.items()}
        if dw is not None:
            for nn, r in copies.items():
                r.owned("w")[...] += dw[nn]
        if self.pats is not None:
            apply_local_copies_fast(copies, self.pats[2], names=("w",))
        inputs = {}
        for nn in sorted(copies):
            r = copies[nn]
            faces, nvisc = self.bocos[nn]
            ref.bind_block(r, self.prm)
            ref.set_bocos(faces, nvisc)
            ref.call("computePressureSimple", 1)
            if self.prm.viscous:
                ref.call("computeLamViscosity", 1)
            if self.prm.eddyModel:
                ref.call("computeEddyViscosity", 1)
            ref.call("applyAllBC_block", 1)
            ref.load().ref_set_int(b"rkStage", 0)
            ref.call("timeStep_block", 0)
            ref.call("initres_flow")
            ref.call("residual_block")
            for m, f in enumerate(faces):
                if f["bcType"] in wf.WALL_TYPES:
                    tau = ref.wall_stress(m + 1)[0] if m < nvisc else None
                    inputs[(nn, m + 1)] = wf.face_inputs(self.blks[nn], r, f, tau)
        return inputs

    def terms(self, par, dw):
        inp = self.ref_inputs(dw)
        return {key: wf.face_terms(d, self.prm, par, self.blank[key[0]][key[1] - 1])[0] for key, d in inp.items()}

    def run(self, engine, evaluate=True):
        super().run(engine, evaluate=False)
        if self.pats is not None:
            for L in (1, 2):
                engine.comm_register(1, L, self.pats[L])
        if evaluate:
            engine.applyAllBC(1, True)
            engine.timeStep(1, False)
            engine.residual(1, 0)


def state_range(case, frozenTurb=False, useTurbOnly=False):
    if useTurbOnly:
        return 5, 1
    return 0, (5 if frozenTurb or case.nw == 5 else case.nw)


def direction(case, seed, l0, ns):
    """a random direction, every component scaled by the mean magnitude of its state variable"""
    rng = np.random.default_rng(seed)
    scale = np.array([np.mean([np.abs(b.owned("w")[..., l]).mean() for b in case.blks.values()]) for l in range(l0, l0 + ns)])
    return rng.uniform(-1.0, 1.0, (case.ncells(), ns)) * scale, scale


def richardson(case, par, v, l0, ns, h):
    """{key: {e: per-face derivative}} of the face terms in the direction v, from the steps h and h / 2"""
    def central(step):
        dw = case.scatter(step * v.reshape(-1), l0, ns)
        tp = case.terms(par, dw)
        tm = case.terms(par, {nn: -d for nn, d in dw.items()})
        return {key: {e: (tp[key][e] - tm[key][e]) / (2.0 * step) for e in wf.SUMS} for key in tp}
    d1, d2 = central(h), central(0.5 * h)
    return {key: {e: (4.0 * d2[key][e] - d1[key][e]) / 3.0 for e in wf.SUMS} for key in d1}


def group_sums(case, faces, groups):
    """(S, M) (nG, 64): the sum of the per-face derivatives and the sum of their magnitudes over the subfaces of every group"""
    glist = [None] if groups is None else groups
    S, M = np.zeros((len(glist), 64)), np.zeros((len(glist), 64))
    for g, fams in enumerate(glist):
        for key in case.walls():
            if fams is not None and case.fam[key[0]][key[1] - 1] not in fams:
                continue
            for e in wf.SUMS:
                S[g, e] += faces[key][e].sum()
                M[g, e] += np.abs(faces[key][e]).sum()
    return S, M


_yard = {}


def yardstick(name, case, par, groups, seed, frozenTurb=False, useTurbOnly=False):
    """(v (n,), S, M) of the named case: computed once, shared, never changed"""
    key = (name, seed, frozenTurb, useTurbOnly, None if groups is None else tuple(map(tuple, groups)))
    if key not in _yard:
        l0, ns = state_range(case, frozenTurb, useTurbOnly)
        v, _ = direction(case, seed, l0, ns)
        S, M = group_sums(case, richardson(case, par, v, l0, ns, H), groups)
        _yard[key] = (v.reshape(-1), S, M)
    return _yard[key]


def noise_of(case, par, seed=11, frozenTurb=False, useTurbOnly=False):
    """the largest |S(h, h/2) - S(h/2, h/4)| / M_e over the entries (one group of every wall)"""
    l0, ns = state_range(case, frozenTurb, useTurbOnly)
    v, _ = direction(case, seed, l0, ns)
    S1, M1 = group_sums(case, richardson(case, par, v, l0, ns, H), None)
    S2, _ = group_sums(case, richardson(case, par, v, l0, ns, 0.5 * H), None)
    ok = M1[0] > 0
    r = np.zeros(64)
    r[ok] = np.abs(S1[0] - S2[0])[ok] / M1[0][ok]
    return float(r.max()), int(np.argmax(r))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
RANS, NS, EULER = wf.RANS, wf.NS, wf.EULER
CAV = dict(computeCavitation=True, cavitationnumber=0.6, cavSensorOffset=0.01, cavSensorSharpness=10.0, cavExponent=2, cpmin_rho=20.0,
           cpmin_family=-1.0)


def par_of(case):
    """every computed sum entry alive: cavitation and the KS sum on, a reference point and an axis off the origin"""
    return wf.default_par(case.prm, pointRef=(0.3, -0.2, 0.1), momentAxis=((0.1, 0.2, -0.3), (0.9, 0.1, 0.4)),
                          velDirFreeStream=(0.8, 0.36, -0.48), sepSensorOffset=0.1, sepSensorSharpness=3.0, **CAV)


def _one(prm, dims, spec, **kw):
    return lambda: DCase(prm).add(1, dims, spec, **kw)


def _blank():
    ib = np.ones((3, 5), np.int8, order="F")
    ib[1, 2], ib[0, 0], ib[2, 4] = 0, -1, 0
    return ib


CASES = {}
for _fid in range(1, 7):
    CASES[f"rans-face{_fid}"] = _one(RANS, (6, 5, 4), wf.spec_with(_fid, -3), stretch_k=2.0)
CASES.update({
    "ns-isothermal": _one(NS, (6, 5, 4), wf.spec_with(5, -4), stretch_k=2.0),
    "euler": _one(EULER, (6, 5, 4), {1: -5, 2: -6, 3: -6, 4: -6, 5: -5, 6: -6}),
    "euler-constant": _one(EULER.replace(eulerWallBCTreatment=1), (6, 5, 4), wf.spec_with(5, -5)),
    "euler-normal-momentum": _one(EULER.replace(eulerWallBCTreatment=4), (6, 5, 4), wf.spec_with(5, -5)),
    "rans-linear-pressure": _one(RANS.replace(viscWallBCTreatment=2), (6, 5, 4), wf.spec_with(5, -3), stretch_k=2.0),
    "two-blocks": lambda: DCase(RANS, BrickTopology(Bi=2, Bj=1, Bk=1, nx=6, ny=5, nz=4, periodic=(False,) * 3), ALLWALL, stretch_k=2.0,
                                fam={(1, 1): 3, (2, 1): 7}),
    "rotated": lambda: DCase(RANS, LatticeTopology([LatticeBlock((6, 5, 4), np.eye(3, dtype=int), (0, 0, 0)),
                                                    LatticeBlock((5, 6, 4), np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]]), (11, 0, 0))],
                                                   stretch_z=2.0), ALLWALL, fam={(1, 1): 3, (2, 1): 7}),
    "edge": _one(RANS, (6, 5, 4), {1: -6, 2: -6, 3: -3, 4: -6, 5: -3, 6: -6}, stretch_k=2.0, fam={1: 3, 2: 7}),
    "split-blanked": _one(RANS, (6, 5, 4), wf.spec_with(5, -3), split={5: -3}, stretch_k=2.0, fam={1: 3, 2: 7}, blank={1: _blank()}),
    "thin": _one(RANS, (6, 5, 2), wf.spec_with(5, -3), stretch_k=2.0),
    # wall treatments that reach past the first interior cell, on the transposed side: the halo's pressure from the second interior
    # layer (linear extrapolation), and -- two walls along an edge -- from two cells away in the plane of the other wall; the Euler
    # wall (no stress) with the linear and the normal-momentum pressure, the second reading its in-plane neighbours
    "thin-linear": _one(RANS.replace(viscWallBCTreatment=2), (6, 5, 2), wf.spec_with(5, -3), stretch_k=2.0),
    "edge-linear": _one(RANS.replace(viscWallBCTreatment=2), (6, 5, 4), {1: -6, 2: -6, 3: -3, 4: -6, 5: -3, 6: -6}, stretch_k=2.0,
                        fam={1: 3, 2: 7}),
    "euler-edge-normal-momentum": _one(EULER.replace(eulerWallBCTreatment=4), (6, 5, 4), {1: -5, 2: -6, 3: -6, 4: -6, 5: -5, 6: -6}),
})
FORWARD = [f"rans-face{f}" for f in range(1, 7)] + ["ns-isothermal", "euler", "euler-constant", "euler-normal-momentum", "rans-linear-pressure"]
TRANSPOSE = ["two-blocks", "rotated", "edge", "split-blanked", "thin", "rans-linear-pressure", "thin-linear", "edge-linear", "euler",
             "euler-normal-momentum", "euler-edge-normal-momentum"]
COLOURING = ["thin", "two-blocks", "thin-linear", "edge-linear", "euler-edge-normal-momentum"]
FLAGGED = [("rans-face5", dict(frozenTurb=True))]
GROUPS = [[3], [7], [3, 7]]


def case_of(name):
    return wf.cached(("deriv", name), CASES[name])


def groups_of(case):
    return GROUPS if any(any(f) for f in case.fam.values()) else None


def measure_floor():
    """prints the noise of the yardstick per case and returns (the largest, its case): FLOOR of this file is that number"""
    worst, where = 0.0, None
    for name in dict.fromkeys(FORWARD + TRANSPOSE):
        case = case_of(name)
        r, e = noise_of(case, par_of(case))
        print(f"{name}: largest |R(h, h/2) - R(h/2, h/4)| / M_e = {r:.3e} (entry {e})")
        if r > worst:
            worst, where = r, name
    for name, kw in FLAGGED:
        case = case_of(name)
        r, e = noise_of(case, par_of(case), **kw)
        print(f"{name} {kw}: {r:.3e} (entry {e})")
        worst = max(worst, r)
    print(f"floor {worst!r} ({where}); FLOOR = {FLOOR!r}, BAR = {BAR!r}")
    return worst, where


# ---- 1. forward against the reference -----------------------------------------------------------------------------------------------
def force_entries(case):
    """the entries whose derivative must be alive: the pressure force, and the viscous force where a wall of the case is viscous"""
    visc = any(d["viscous"] for d in case.inputs.values())
    return list(range(wf.E_FP, wf.E_FP + 3)) + (list(range(wf.E_FV, wf.E_FV + 3)) if visc else [])


def assert_alive(what, M, case, groups):
    for g in range(M.shape[0]):
        if groups is not None and not any(case.fam[k[0]][k[1] - 1] in groups[g] for k in case.walls()):
            continue
        assert all(M[g, e] > 0.0 for e in force_entries(case)), (what, g, "trivial derivative of a force")


def check_forward(engine, name, **flags):
    case = case_of(name)
    par, groups = par_of(case), groups_of(case)
    v, S, M = yardstick(name, case, par, groups, 11, **flags)
    case.run(engine)
    base = engine.wallIntegrate(par, groups)
    out, dot = engine.wallIntegrateFwd(v, par, groups, **flags)
    assert_alive(name, M, case, groups)
    for g in range(S.shape[0]):
        for e in range(64):
            if e not in wf.SUMS:
                assert dot[g, e] == 0.0, (name, g, e, "an entry without a derivative")
        for e in wf.SUMS:
            err, bar = abs(dot[g, e] - S[g, e]), BAR * M[g, e]
            assert err <= bar, (name, flags, g, e, err, bar, dot[g, e], S[g, e])
    worst = max(abs(dot[g, e] - S[g, e]) / M[g, e] for g in range(S.shape[0]) for e in wf.SUMS if M[g, e] > 0)
    print(f"{name} {flags}: largest |outDot - S_ref| / M_e = {worst:.3e}, bar {BAR:.1e}")
    # the value parts are the integration of the same state
    _, scl, _ = case.yardstick(par, groups)
    for g in range(out.shape[0]):
        for e in wf.SUMS:
            assert abs(out[g, e] - base[g, e]) <= TOL * scl[g, e], (name, "out against wallIntegrate", g, e)
        assert abs(out[g, wf.E_YPLUS] - base[g, wf.E_YPLUS]) <= TOL * abs(base[g, wf.E_YPLUS])
        assert abs(out[g, wf.E_CPMIN] - base[g, wf.E_CPMIN]) <= TOL * max(scl[g, wf.E_CPMIN], abs(base[g, wf.E_CPMIN]))
    engine.releaseWorkspace()


# ---- 2. transpose against the reference, 4. identity -----------------------------------------------------------------------------------
def weights(case, groups, nRhs, seed=5):
    rng = np.random.default_rng(seed)
    nG = 1 if groups is None else len(groups)
    ob = np.zeros((nRhs, nG, 64))
    ob[:, :, wf.SUMS] = rng.uniform(-1.0, 1.0, (nRhs, nG, len(wf.SUMS)))
    return ob


def check_transpose(engine, name, **flags):
    case = case_of(name)
    par, groups = par_of(case), groups_of(case)
    v, S, M = yardstick(name, case, par, groups, 13, **flags)
    assert_alive(name, M, case, groups)
    case.run(engine)
    ob = weights(case, groups, 1)
    wbar = engine.wallIntegrateBwd(ob, v.size, par, groups, **flags)
    assert wbar.shape == (1, v.size) and np.isfinite(wbar).all()
    lhs, rhs, bar = float(wbar[0] @ v), float((ob[0] * S).sum()), BAR * float((np.abs(ob[0]) * M).sum())
    print(f"{name} {flags}: bwd(outBar) . v = {lhs:.9e}, outBar . FD_ref(v) = {rhs:.9e}, |difference| / bar = {abs(lhs - rhs) / bar:.3e}")
    assert bar > 0.0 and abs(lhs - rhs) <= bar, (name, flags, lhs, rhs, bar)
    # the identity with the single exchange-seeded pass, to rounding of the magnitude sums
    _, dot = engine.wallIntegrateFwd(v, par, groups, values=False, **flags)
    a, mag = float((ob[0] * dot).sum()), float((np.abs(ob[0]) * np.abs(dot)).sum()) + float(np.abs(wbar[0]) @ np.abs(v))
    assert abs(a - lhs) <= 1e-12 * mag, (name, flags, "outBar . fwd(v) against bwd(outBar) . v", a, lhs, mag)
    engine.releaseWorkspace()


def check_turb_only(engine, name="rans-face5"):
    """ADFLOW_JAC_TURB_ONLY: the turbulence variable reaches a wall face only through the eddy viscosity of its stress, rev(halo) +
    rev(first cell), and the wall boundary condition makes the halo's the negative of the cell's: every face term of the reference has
    the derivative zero (the yardstick's M_e is zero, so no relative bar exists), and the dual pass gives exact zeros because the two
    derivative parts cancel exactly"""
    case = case_of(name)
    par = par_of(case)
    v, S, M = yardstick(name, case, par, None, 11, useTurbOnly=True)
    assert not S.any() and not M.any() and np.abs(v).min() > 0.0
    case.run(engine)
    out, dot = engine.wallIntegrateFwd(v, par, useTurbOnly=True)
    assert not dot.any() and np.abs(out[0, wf.E_FV:wf.E_FV + 3]).min() > 0.0
    wbar = engine.wallIntegrateBwd(weights(case, None, 1), v.size, par, useTurbOnly=True)
    assert wbar.shape == (1, case.ncells()) and not wbar.any()
    engine.releaseWorkspace()


# ---- 3. the colouring ---------------------------------------------------------------------------------------------------------------------
def check_colouring(engine, name):
    """the matrix column by column from fwd(e_j), row by row from bwd of unit weights"""
    case = case_of(name)
    par, groups = par_of(case), groups_of(case)
    case.run(engine)
    n = case.nw * case.ncells()
    nG = 1 if groups is None else len(groups)
    A = np.zeros((nG, 64, n))
    x = np.zeros(n)
    for j in range(n):
        x[j] = 1.0
        A[:, :, j] = engine.wallIntegrateFwd(x, par, groups, values=False)[1]
        x[j] = 0.0
    rows = [(g, e) for g in range(nG) for e in wf.SUMS]
    viscous = any(d["viscous"] for d in case.inputs.values())
    worst = 0.0
    for r0 in range(0, len(rows), capi.MAX_NVEC):
        part = rows[r0:r0 + capi.MAX_NVEC]
        ob = np.zeros((len(part), nG, 64))
        for r, (g, e) in enumerate(part):
            ob[r, g, e] = 1.0
        B = engine.wallIntegrateBwd(ob, n, par, groups)
        for r, (g, e) in enumerate(part):
            scale = np.abs(A[g, e]).max()
            # (only the viscous force and moment of a case without a viscous wall may be empty)
            assert scale > 0.0 or (wf.E_FV <= e < wf.E_FV + 3 or wf.E_MV <= e < wf.E_MV + 3) and not viscous, (name, g, e, "an empty row")
            err = np.abs(B[r] - A[g, e]).max()
            assert err <= 1e-12 * scale, (name, g, e, err, scale, int(np.argmax(np.abs(B[r] - A[g, e]))))
            worst = max(worst, err / scale if scale > 0 else 0.0)
    print(f"{name}: {n} columns, {len(rows)} rows, largest |bwd row - fwd columns| / max|row| = {worst:.3e}")
    engine.releaseWorkspace()


# ---- 5. several weight sets -----------------------------------------------------------------------------------------------------------------
def check_multi(engine, name="two-blocks"):
    case = case_of(name)
    par, groups = par_of(case), groups_of(case)
    case.run(engine)
    n = case.nw * case.ncells()
    ob = weights(case, groups, 3, seed=9)
    ld = n + 7
    wb = engine.wallIntegrateBwd(ob, n, par, groups, ld=ld, fill=7.0)
    assert wb.shape == (3, ld) and (wb[:, n:] == 7.0).all(), "the padding was written"
    for r in range(3):
        one = engine.wallIntegrateBwd(ob[r], n, par, groups)
        assert np.abs(one).max() > 0 and np.array_equal(one[0], wb[r, :n]), (r, "three sets at once against one at a time")
    engine.releaseWorkspace()


# ---- 6. nothing moves -----------------------------------------------------------------------------------------------------------------------
def _snapshot(engine, case, par, groups):
    out = wf._state(engine, case)
    for (nn, mm), d in case.inputs.items():
        if d["viscous"]:
            out[("tau", nn, mm)] = [a.copy() for a in engine.wall_stress(d["p1"].shape, mm, nn=nn)]
    out["int"] = [engine.wallIntegrate(par, groups)]
    for (nn, mm), d in case.inputs.items():
        out[("F", nn, mm)] = [a.copy() for a in engine.wallForces(d["p1"].shape, mm, nn=nn)]
    return out


def check_nothing_moves(engine, dv, name="two-blocks"):
    case = case_of(name)
    par, groups = par_of(case), groups_of(case)
    case.run(engine)
    n = case.nw * case.ncells()
    v = direction(case, 17, 0, case.nw)[0].reshape(-1)
    ob = weights(case, groups, 2, seed=21)
    before = _snapshot(engine, case, par, groups)
    out, dot = engine.wallIntegrateFwd(v, par, groups)
    wbar = engine.wallIntegrateBwd(ob, n, par, groups)
    after = _snapshot(engine, case, par, groups)
    for k in before:
        for a, b in zip(before[k], after[k]):
            assert np.array_equal(a, b), (k, "changed by the derivative entries")
    out2, dot2 = engine.wallIntegrateFwd(v, par, groups)
    assert np.array_equal(dot, dot2) and np.array_equal(out, out2) and np.abs(dot).max() > 0, "two forward calls"
    assert np.array_equal(wbar, engine.wallIntegrateBwd(ob, n, par, groups)) and np.abs(wbar).max() > 0, "two transposed calls"
    # the _dev forms, enqueue-only, chained with an evaluation, one synchronise at the end, against the synchronous chain
    nG = len(groups)

    def setup(enqueue):
        case.run(engine)
        d = dict(x=dv.put(v), out=dv.put(np.full(nG * 64, 7.0)), dot=dv.put(np.full(nG * 64, 7.0)), wbar=dv.put(np.full(2 * n, 7.0)),
                 int=dv.put(np.full(nG * 64, 7.0)), dot0=dv.put(np.full(nG * 64, 7.0)), wpad=dv.put(np.full(2 * (n + 5), 7.0)))
        return dict(d=d)

    def chain(c, link):
        d, p = c["d"], dv.ptr
        link(engine.blocketteRes, 1, True, True, case.nw > 5)
        link(engine.wallIntegrateFwdDev, p(d["x"]), n, par, p(d["out"]), p(d["dot"]), groups)
        link(engine.wallIntegrateBwdDev, ob, p(d["wbar"]), n, n, par, groups)
        link(engine.wallIntegrateDev, par, p(d["int"]), groups)
        link(engine.wallIntegrateFwdDev, p(d["x"]), n, par, 0, p(d["dot0"]), groups)              # no value parts asked for
        link(engine.wallIntegrateBwdDev, ob, p(d["wpad"]), n, n + 5, par, groups)                 # device columns with a padding
        return dict(d)
    c, enq, syn = async_checks.both_runs(engine, dv, setup, chain)
    async_checks.assert_bitwise("derivatives of the integration, chained", enq, syn)
    assert np.array_equal(enq["dot"].reshape(nG, 64), dot) and np.array_equal(enq["wbar"].reshape(2, n), wbar), "the _dev forms against the host forms"
    assert np.array_equal(enq["x"], v), "x was written"
    assert np.array_equal(enq["dot0"], enq["dot"]), "outDot without out"
    wpad = enq["wpad"].reshape(2, n + 5)
    assert np.array_equal(wpad[:, :n], wbar) and (wpad[:, n:] == 7.0).all(), "device columns ld > n: the result, and the padding untouched"
    engine.releaseWorkspace()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def check_refusals(engine):
    case = case_of("rans-face5")
    par = par_of(case)
    case.run(engine)
    lib = engine.lib
    n = case.nw * case.ncells()
    x, dot, out = np.ones(n), np.zeros(64), np.zeros(64)
    ob, wbar = np.zeros(64), np.zeros(2 * n + 8)
    ob[0] = 1.0
    msg = lambda: lib.adflow_gpu_last_error().decode()
    base = engine.wallIntegrate(par)

    def fwd(flags=0, x_=x, n_=n, dot_=dot):
        return lib.adflow_gpu_wall_integrate_fwd(1, flags, None if x_ is None else x_.ctypes.data, n_, par.ctypes.data, 0, None, 0,
                                                 out.ctypes.data, None if dot_ is None else dot_.ctypes.data)

    def bwd(flags=0, ob_=ob, nRhs=1, wbar_=wbar, n_=n, ld=n):
        return lib.adflow_gpu_wall_integrate_bwd(1, flags, par.ctypes.data, 0, None, 0, None if ob_ is None else ob_.ctypes.data, nRhs,
                                                 None if wbar_ is None else wbar_.ctypes.data, n_, ld)

    def refused(word, rc):
        assert rc != 0 and word in msg(), (word, rc, msg())
    refused("rows", fwd(n_=n - 6))
    refused("rows", bwd(n_=n + 6, ld=n + 6))
    refused("rows", fwd(flags=capi.JAC_FROZEN_TURB))
    refused("x is NULL", fwd(x_=None))
    refused("outDot is NULL", fwd(dot_=None))
    refused("outBar is NULL", bwd(ob_=None))
    refused("wbar is NULL", bwd(wbar_=None))
    for f in (capi.JAC_PC, capi.JAC_VISC_PC, capi.JAC_APPROX_SA):
        refused("approximations of the fluxes", fwd(flags=f))
        refused("approximations of the fluxes", bwd(flags=f))
    for e in (wf.E_YPLUS, wf.E_CPMIN):
        bad = ob.copy()
        bad[e] = 0.5
        refused("has no derivative", bwd(ob_=bad))
    refused("nRhs", bwd(nRhs=0))
    refused("nRhs", bwd(nRhs=capi.MAX_NVEC + 1))
    refused("ld >= n", bwd(nRhs=2, ld=n - 1))
    assert not dot.any() and not wbar.any(), "a refused call wrote its result"
    # the level is usable: the same calls go through, and the integration is what it was
    assert fwd() == 0 and dot.any() and bwd() == 0 and wbar[:n].any(), msg()
    assert np.array_equal(engine.wallIntegrate(par), base)
    assert engine.releaseWorkspace() > 0 and engine.releaseWorkspace() == 0
    # a level with boundary subfaces but no wall: zeros, no error
    far = wf.cached(("deriv", "no-wall"), lambda: DCase(RANS).add(1, (6, 5, 4), dict(wf.FAR), stretch_k=2.0))
    far.run(engine)
    out2, dot2 = engine.wallIntegrateFwd(x, par)
    assert not dot2.any() and not out2[0, :63].any() and out2[0, wf.E_CPMIN] == 10000.0
    wb = engine.wallIntegrateBwd(ob, n, par)
    assert wb.shape == (1, n) and not wb.any()
    engine.releaseWorkspace()
