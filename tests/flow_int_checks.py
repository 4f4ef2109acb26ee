"""TEST INFRASTRUCTURE.  Flow integration on the device (adflow_gpu_flow_integrate and its _fwd / _bwd derivatives, the flow kernels of
csrc/kernels_wallint.hip) against a yardstick written here in numpy from the formulas of surfaceIntegrations::flowIntegrationFace
(surfaceIntegrations.F90:894-1200) with computePtot / computeTtot of flowUtils -- surfaceIntegrations is one of the modules the oracle
stubs -- and fed the REFERENCE's own fields: every block is bound to the oracle as wall_deriv_checks.DCase binds it (closures,
applyAllBC_block, timeStep_block, initres_flow, residual_block); p, w, gamma, sI / sJ / sK, sFaceI / J / K and x come from the bound
block.  The yardstick never reads the library's output.

Bars of the values, those of wall_force_checks.  Every sum S = sum t_i: |S - S_ref| <= TOL sum scale_i, TOL = 1e-10 of tests/util.py.
scale_i is the term with every difference replaced by the sum of the magnitudes; through a root or a power (the speed, the speed of
sound, Ptot, viLocal) and through a quotient it adds the magnitude of the analytic derivative times the magnitudes of the inputs.  Both
rules are carried by the class Mag below: every quantity is a pair (value, magnitude) and every operation of the formulas propagates
both.  Every comparison asserts sum scale_i > 0, and |S_ref| > 0 for the mass flow, so that zeros cannot pass.

Derivatives: the same reference chain differentiated numerically as in wall_deriv_checks -- central differences at h and h / 2,
Richardson-combined, per face.  The states have a non-dimensional Ptot >= 1.02 on every integrated face (asserted from the reference's
fields), so that the clip min(1, 1 / Ptot) and the root at zero stay out of the stencil.  On SupersonicOutflow faces the dual boundary
conditions of the library leave the halo unlinearised, as BCExtra_d.F90 does: there the yardstick HOLDS THE HALO AT ITS BASE VALUE and
perturbs the interior cell only.  FLOOR is the largest |R(h, h/2) - R(h/2, h/4)| / M_e (M_e = sum over the faces |d t_i|) over all
cases and entries at the least noisy step of 2^-9 .. 2^-15, measured on the CPU by measure_floor(); BAR = 10 FLOOR, the margin of
wall_deriv_checks for the same reason (the dependence of that noise on the step).

tests/test_gpu_flow_int.py runs the checkers on the MI355X, tests/test_hostsim_flow_int.py on the emulator."""
import numpy as np

import device_vectors  # noqa: F401  (torch before the library: see its docstring)
import async_checks
import checks
import wall_force_checks as wf
import wall_deriv_checks as wd
from adflow_amd import capi
from adflow_amd.engine import Engine
from adflow_amd.topology import BrickTopology
from util import TOL

FLOW_TYPES, INFLOW_TYPES = (-7, -8, -9, -10), (-7, -8)
# entries of a group's output (0-based; localValues(e + 1) of constants.F90:454-500)
E_FP, E_MASSFLOW, E_MASSPTOT, E_MASSTTOT, E_MASSPS, E_MP, E_FM, E_MM, E_MASSMN, E_MASSA, E_MASSRHO, E_AREA = 0, 18, 19, 20, 21, 22, 25, 28, 31, 35, 36, 37
E_MASSV, E_MASSN, E_AREAPTOT, E_AREAPS, E_COF, E_MASSVI = 38, 41, 47, 48, 50, 59
SUMS = [0, 1, 2] + list(range(18, 32)) + [35, 36, 37] + list(range(38, 44)) + [47, 48] + list(range(50, 59)) + [59]
assert len(SUMS) == 38

H = 2.0 ** -11                  # the step of the yardstick, relative to the scale of each state variable: the one of 2^-9, 2^-11,
                                # 2^-13, 2^-15 with the least noise (4.6e-10, 5.4e-12, 1.5e-11, 8.6e-11: truncation left, rounding right)
FLOOR = 5.352089902075258e-12   # the largest |R(h, h/2) - R(h/2, h/4)| / M_e over the cases below and all entries (measure_floor)
BAR = 10.0 * FLOOR


class Mag:
    """(value, magnitude): the magnitude of a sum or difference is the sum of the magnitudes, of a product the product; a quotient, a
    root and a power add |f'| times the magnitude of the argument"""

    __array_ufunc__ = None                  # (numpy scalars and arrays on the left defer to the operators below)

    def __init__(self, v, s=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.s = np.abs(self.v) if s is None else np.asarray(s, dtype=np.float64)

    @staticmethod
    def of(a):
        return a if isinstance(a, Mag) else Mag(a)

    def __add__(self, o):
        o = Mag.of(o)
        return Mag(self.v + o.v, self.s + o.s)

    __radd__ = __add__

    def __sub__(self, o):
        o = Mag.of(o)
        return Mag(self.v - o.v, self.s + o.s)

    def __rsub__(self, o):
        return Mag.of(o) - self

    def __neg__(self):
        return Mag(-self.v, self.s)

    def __mul__(self, o):
        o = Mag.of(o)
        return Mag(self.v * o.v, self.s * o.s)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Mag.of(o)                       # a / b: |a| / |b| where b carries no cancellation, times |b|_mag / |b| where it does
        return Mag(self.v / o.v, self.s * o.s / (o.v * o.v))

    def __rtruediv__(self, o):
        return Mag.of(o) / self

    def sqrt(self):
        r = np.sqrt(self.v)
        return Mag(r, r + np.where(r > 0, self.s / (2.0 * np.where(r > 0, r, 1.0)), 0.0))

    def pow(self, y):
        r = self.v ** y
        return Mag(r, np.abs(r) + np.abs(y * self.v ** (y - 1.0)) * self.s)

    def min1(self):
        """min(1, x)"""
        return Mag(np.where(self.v < 1.0, self.v, 1.0), np.where(self.v < 1.0, self.s, 1.0))


def flow_inputs(blk, r, f):
    """what flowIntegrationFace reads on the owned faces of subface f through setBCPointers: wall_force_checks.face_inputs (pp1, pp2,
    ww1, ww2, ssi, the four nodes of xx) plus gamma1, gamma2 and sFace"""
    d = wf.face_inputs(blk, r, f, None)
    fid = f["faceID"]
    a0, a1, b0, b1 = wf.owned_range(blk, f)
    sa, sb = slice(a0, a1 + 1), slice(b0, b1 + 1)
    lo = fid in (1, 3, 5)
    nl = (blk.il, blk.jl, blk.kl)[(fid - 1) // 2]
    halo, inner, node = (1, 2, 1) if lo else (nl + 1, nl, nl)
    d["g1"], d["g2"] = wf._plane(r["gamma"], fid, halo, sa, sb), wf._plane(r["gamma"], fid, inner, sa, sb)
    name = ("sFaceI", "sFaceJ", "sFaceK")[(fid - 1) // 2]
    d["sF"] = wf._plane(r[name], fid, node, slice(a0 - 1, a1), slice(b0 - 1, b1)) if name in r.a else np.zeros(d["p1"].shape)
    d["fact"] = 1.0 if lo else -1.0            # the opposite of the wall forces
    d["bcType"] = f["bcType"]
    for k in ("p1", "p2", "w1", "w2", "g1", "g2", "ss", "sF"):
        d[k] = np.array(d[k], copy=True)
    return d


def flow_terms(d, prm, par, iblank=None):
    """the terms of every owned face of one subface as Mag: ({e: Mag over the faces} for e in SUMS, Ptot)"""
    pRef, rhoRef, TRef, uRef, timeRef = prm.pInfDim, par[capi.FLOWINT_RHOREF], prm.TRef, prm.uRef, prm.timeRef
    refPoint = prm.LRef * par[capi.FLOWINT_POINTREF:capi.FLOWINT_POINTREF + 3]
    internal = -1.0 if par[capi.FLOWINT_INTERNALFLOW] != 0.0 else 1.0
    inflow = -1.0 if d["bcType"] in INFLOW_TYPES else 1.0
    fact = d["fact"]
    shp = d["p1"].shape
    ib = np.ones(shp, np.int64) if iblank is None else np.asarray(iblank, np.int64).reshape(shp, order="F")
    blk = np.maximum(ib, 0).astype(np.float64)
    w1, w2 = d["w1"], d["w2"]
    mean = lambda a, b: 0.5 * (Mag(a) + Mag(b))
    vm = [mean(w1[..., 1 + c], w2[..., 1 + c]) for c in range(3)]
    rhom, pm, gammam = mean(w1[..., 0], w2[..., 0]), mean(d["p1"], d["p2"]), mean(d["g1"], d["g2"])
    ss = [Mag(d["ss"][..., c]) for c in range(3)]
    sF = Mag(d["sF"])
    vnm = vm[0] * ss[0] + vm[1] * ss[1] + vm[2] * ss[2] - sF
    v2 = vm[0] * vm[0] + vm[1] * vm[1] + vm[2] * vm[2]
    vmag = v2.sqrt() - sF
    am = (gammam * pm / rhom).sqrt()
    MNm = vmag / am
    cellArea = Mag(np.sqrt(d["ss"][..., 0] ** 2 + d["ss"][..., 1] ** 2 + d["ss"][..., 2] ** 2))
    govgm1 = prm.gammaInf / (prm.gammaInf - 1.0)
    kin = 0.5 * v2
    x = 1.0 + rhom * kin / (govgm1 * pm)
    Ptot = pm * x.pow(govgm1)
    Ttot = pm / (rhom * prm.RGas) * x
    mRe = np.sqrt(pRef * rhoRef)
    mfl = rhom * vnm * (blk * fact * mRe)
    t = {E_MASSFLOW: mfl, E_AREA: cellArea * blk}
    pmd = pm * pRef
    t[E_MASSPTOT] = Ptot * mfl * pRef
    t[E_MASSTTOT] = Ttot * mfl * TRef
    t[E_MASSRHO] = rhom * mfl * rhoRef
    t[E_MASSA] = am * mfl * uRef
    t[E_MASSPS] = pmd * mfl
    t[E_MASSMN] = MNm * mfl
    t[E_AREAPTOT] = Ptot * pRef * cellArea * blk
    t[E_AREAPS] = pmd * cellArea * blk
    for c in range(3):
        t[E_MASSV + c] = (vm[c] * uRef - sF * ss[c] / cellArea) * mfl
        t[E_MASSN + c] = ss[c] / cellArea * mfl
    viConst = 2.0 * govgm1 * par[capi.FLOWINT_RGASDIM]
    pratio = (1.0 / Ptot).min1()
    t[E_MASSVI] = (viConst * (1.0 - pratio.pow(1.0 / govgm1)) * Ttot * TRef).sqrt() * mfl
    n0, n1, n2, n3 = d["nodes"]
    xco = [0.25 * (Mag(n0[..., c]) + Mag(n1[..., c]) + Mag(n2[..., c]) + Mag(n3[..., c])) for c in range(3)]
    xc = [xco[c] - refPoint[c] for c in range(3)]
    pf = -(pmd - prm.pInf * pRef) * (fact * blk)
    fp = [pf * ss[c] for c in range(3)]
    mfl2 = mfl * (fact / timeRef * internal * inflow) * blk / cellArea
    fm = [mfl2 * ss[c] * vm[c] for c in range(3)]
    mp, mm = wf._cross(xc, fp), wf._cross(xc, fm)
    for c in range(3):
        t[E_FP + c], t[E_FM + c], t[E_MP + c], t[E_MM + c] = fp[c], fm[c], mp[c], mm[c]
        for e in range(3):
            t[E_COF + 3 * c + e] = xco[e] * fp[c] + xco[e] * fm[c]
    assert sorted(t) == SUMS
    return t, Ptot.v


class FCase(wd.DCase):
    """wall_deriv_checks.DCase whose `inputs` are those of the in- and outflow subfaces; the wall subfaces go to wall_inputs"""

    def ref_inputs(self, dw, hold=True):
        from oracle import ref
        from adflow_amd.topology import apply_local_copies_fast
        copies = {nn: b.copy() for nn, b in self.blks.items()}
        if dw is not None:
            for nn, r in copies.items():
                r.owned("w")[...] += dw[nn]
        if self.pats is not None:
            apply_local_copies_fast(copies, self.pats[2], names=("w",))
        inputs, walls = {}, {}
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
                if f["bcType"] in FLOW_TYPES:
                    d = flow_inputs(self.blks[nn], r, f)
                    if dw is not None and hold and f["bcType"] == -9:
                        # the halo of a supersonic outflow face is not linearised (BCExtra_d.F90): held at its base value
                        base = self.inputs[(nn, m + 1)]
                        d["w1"], d["p1"], d["g1"] = base["w1"], base["p1"], base["g1"]
                    inputs[(nn, m + 1)] = d
                elif dw is None and f["bcType"] in wf.WALL_TYPES:
                    tau = ref.wall_stress(m + 1)[0] if m < nvisc else None
                    walls[(nn, m + 1)] = wf.face_inputs(self.blks[nn], r, f, tau)
        if dw is None:
            self.wall_inputs = walls
        return inputs

    def terms(self, par, dw):
        inp = self.ref_inputs(dw)
        out = {}
        for key, d in inp.items():
            t, _ = flow_terms(d, self.prm, par, self.blank[key[0]][key[1] - 1])
            out[key] = {e: t[e].v for e in SUMS}
        return out

    def yardstick(self, par, groups=None):
        """(values (nG, 64), scales (nG, 64)); groups as Engine.flowIntegrate"""
        glist = [None] if groups is None else groups
        val, scl = np.zeros((len(glist), 64)), np.zeros((len(glist), 64))
        for key in self.walls():
            t, ptot = flow_terms(self.inputs[key], self.prm, par, self.blank[key[0]][key[1] - 1])
            assert ptot.min() >= 1.02, ("Ptot on an integrated face", key, ptot.min())
            for g, fams in enumerate(glist):
                if fams is not None and self.fam[key[0]][key[1] - 1] not in fams:
                    continue
                for e in SUMS:
                    val[g, e] += t[e].v.sum()
                    scl[g, e] += t[e].s.sum()
        return val, scl

    def wall_yardstick(self, par, groups=None):
        c = wf.Case(self.prm)
        c.blks, c.bocos, c.inputs, c.fam, c.blank = self.blks, self.bocos, self.wall_inputs, self.fam, self.blank
        return c.yardstick(par, groups)[:2]


def par_of(case, **kw):
    kw.setdefault("pointRef", (0.3, -0.2, 0.1))
    return Engine.flowPar(case.prm.rhoInfDim, case.prm.RGasDim, **kw)


def compare_sums(out, val, scl, what="", empty=(), show=False):
    assert out.shape == val.shape
    worst = 0.0
    for g in range(out.shape[0]):
        for e in range(64):
            if e not in SUMS:
                assert out[g, e] == 0.0, (what, g, e, "a slot the flow integration leaves zero")
        if g in empty:
            assert not out[g].any() and not val[g].any(), (what, g, "a group without a subface")
            continue
        assert abs(val[g, E_MASSFLOW]) > 0.0, (what, g, "zero mass flow in the reference")
        for e in SUMS:
            err, bar = abs(out[g, e] - val[g, e]), TOL * scl[g, e]
            assert scl[g, e] > 0.0, (what, g, e, "an empty scale")
            worst = max(worst, err / scl[g, e])
            if show:
                print(f"{what} group {g} entry {e}: |S - S_ref| = {err:.3e}, bar {bar:.3e}, S_ref = {val[g, e]:.6e}")
            assert err <= bar, (what, g, e, err, bar, out[g, e], val[g, e])
    print(f"{what}: largest |S - S_ref| / sum scale_i = {worst:.3e}, bar {TOL:.1e}")


def check(engine, case, par=None, groups=None, what="", run=True, empty=()):
    par = par_of(case) if par is None else par
    if run:
        case.run(engine)
    out = engine.flowIntegrate(par, groups)
    val, scl = case.yardstick(par, groups)
    compare_sums(out, val, scl, what, empty=empty)
    return out, val, scl


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
EULER, RANS = wf.EULER, wf.RANS
SUPER = EULER.replace(Mach=2.0)
WALLS = {1: -5, 2: -5, 3: -5, 4: -5, 5: -5, 6: -5}


def through(d, lo=-8, hi=-10, base=WALLS):
    """inflow on the min face of direction d, outflow on the opposite max face, walls elsewhere"""
    sp = dict(base)
    sp[2 * d + 1], sp[2 * d + 2] = lo, hi
    return sp


def _blank():
    ib = np.ones((5, 4), np.int8, order="F")
    ib[1, 2], ib[0, 0], ib[2, 3], ib[4, 1] = 0, -1, 0, 0
    return ib


def _one(prm, dims, spec, **kw):
    return lambda: FCase(prm).add(1, dims, spec, **kw)


RANS_SPEC = {1: -8, 2: -10, 3: -5, 4: -5, 5: -3, 6: -5}
CASES = {
    "euler-i": _one(EULER, (6, 5, 4), through(0)),
    "euler-j": _one(EULER, (6, 5, 4), through(1)),
    "euler-k": _one(EULER, (6, 5, 4), through(2)),
    "supersonic": _one(SUPER, (6, 5, 4), through(0, -7, -9)),
    "rans": _one(RANS, (6, 5, 4), RANS_SPEC, stretch_k=2.0),
    "280": _one(EULER, (3, 20, 14), through(0)),
    # the inflow face in two subfaces of different families (subfaces 1, 2), the outflow face subface 3, a blanked subface
    "split": _one(EULER, (6, 5, 4), through(0), split={1: -8}, fam={1: 1, 2: 2, 3: 3}),
    "blanked": _one(EULER, (6, 5, 4), through(0), blank={1: _blank()}),
    "moving": _one(EULER, (6, 5, 4), through(0), moving=True),
    "brick": lambda: FCase(EULER, BrickTopology(Bi=2, Bj=2, Bk=2, nx=6, ny=5, nz=4, periodic=(False,) * 3), through(0)),
}
FORWARD = ["euler-i", "euler-j", "euler-k", "supersonic", "rans", "split", "blanked"]
TRANSPOSE = ["euler-j", "supersonic", "rans", "split", "blanked", "brick"]
COLOURING = ["euler-i", "euler-k", "supersonic", "rans"]
FLAGGED = [("rans", dict(frozenTurb=True))]
GROUPS = [[1, 2], [2], [9]]


def case_of(name):
    return wf.cached(("flow", name), CASES[name])


def groups_of(case):
    return GROUPS if any(any(f) for f in case.fam.values()) else None


def _types(case):
    return sorted({case.inputs[k]["bcType"] for k in case.inputs})


# ---- values -----------------------------------------------------------------------------------------------------------------------------
def check_direction(engine, d):
    case = case_of("euler-" + "ijk"[d])
    assert sorted((k[1], v["fact"], v["bcType"]) for k, v in case.inputs.items()) == [(2 * d + 1, 1.0, -8), (2 * d + 2, -1.0, -10)]
    out, val, scl = check(engine, case, what=f"subsonic in- and outflow along {'ijk'[d]}")
    # each face alone
    engine.bcSetFamilies([1 if m + 1 == 2 * d + 1 else (2 if m + 1 == 2 * d + 2 else 0) for m in range(6)], None)
    one = engine.flowIntegrate(par_of(case), [[1], [2]])
    for e in SUMS:
        assert abs(one[0, e] + one[1, e] - out[0, e]) <= TOL * scl[0, e], (e, "the two faces against both")


def check_supersonic(engine):
    case = case_of("supersonic")
    assert _types(case) == [-9, -7]
    check(engine, case, what="supersonic in- and outflow at Mach 2")


def check_rans(engine):
    case = case_of("rans")
    assert case.nw == 6 and _types(case) == [-10, -8]
    check(engine, case, what="RANS, nw = 6")


def check_sizes(engine):
    case = case_of("280")
    assert all(d["p1"].shape == (20, 14) for d in case.inputs.values())      # 280 faces: two workgroups of 256 per subface
    check(engine, case, what="20 x 14 faces")


def check_split_and_groups(engine):
    case = case_of("split")
    assert sorted(case.inputs) == [(1, 1), (1, 2), (1, 3)] and [case.inputs[(1, m)]["bcType"] for m in (1, 2, 3)] == [-8, -8, -10]
    out, val, scl = check(engine, case, groups=GROUPS, what="inflow face in two subfaces, three groups", empty=(2,))
    whole = case_of("euler-i")
    par = par_of(case)
    vw, sw = whole.yardstick(par)
    allg = engine.flowIntegrate(par, [[1, 2, 3]])
    compare_sums(allg, vw, sw, "the split face against the unsplit reference")
    none = engine.flowIntegrate(par, None)
    assert np.array_equal(none, allg), "nGroups = 0 against the group of every family"
    only1 = engine.flowIntegrate(par, [[1]])
    for e in SUMS:
        assert abs(only1[0, e] + out[1, e] - out[0, e]) <= TOL * scl[0, e], ("the two parts against both", e)


def check_blanking(engine):
    case, plain = case_of("blanked"), case_of("euler-i")
    ib = case.blank[1][0]
    assert (ib == 0).sum() >= 3 and (ib == -1).sum() == 1 and (ib == 1).sum() > 5
    out, val, _ = check(engine, case, what="blanking with zeros and a -1")
    v0, _ = plain.yardstick(par_of(plain))
    assert abs(val[0, E_AREA] - v0[0, E_AREA]) > 1e-3 * v0[0, E_AREA] and abs(val[0, E_MASSFLOW] - v0[0, E_MASSFLOW]) > 0


def check_internal_flow(engine):
    case = case_of("euler-j")
    off, _, scl = check(engine, case, what="external flow")
    on, val, _ = check(engine, case, par=par_of(case, internalFlow=True), run=False, what="internal flow")
    flip = set(range(E_FM, E_FM + 3)) | set(range(E_MM, E_MM + 3))
    for e in SUMS:
        if e in flip:
            assert on[0, e] == -off[0, e] and on[0, e] != 0.0, (e, "FMom and MMom flip sign")
        elif not (E_COF <= e < E_COF + 9):
            assert on[0, e] == off[0, e], (e, "nothing else moves")
    # (the centre-of-force sums hold pressure plus momentum part: they move by twice the momentum part, held by the yardstick above)


def check_moving(engine):
    case = case_of("moving")
    assert all(np.abs(d["sF"]).min() > 0 for d in case.inputs.values())
    out, val, _ = check(engine, case, what="a moving block, sFace nonzero")
    rest = case_of("euler-i").yardstick(par_of(case))[0]
    assert abs(val[0, E_MASSFLOW] - rest[0, E_MASSFLOW]) > 1e-6 * abs(rest[0, E_MASSFLOW])


def check_brick(engine):
    case = case_of("brick")
    assert len(case.blks) == 8 and sum(d["bcType"] == -8 for d in case.inputs.values()) == 4
    check(engine, case, what="2 x 2 x 2 blocks, the inflow face over four of them")


def _snapshot(engine, case):
    out = wf._state(engine, case)
    wpar = wf.default_par(case.prm)
    out["wall"] = [engine.wallIntegrate(wpar)]
    for (nn, mm), d in case.wall_inputs.items():
        out[("F", nn, mm)] = [a.copy() for a in engine.wallForces(d["p1"].shape, mm, nn=nn)]
    return out


def check_determinism_and_async(engine, dv):
    case = case_of("split")
    case.run(engine)
    par = par_of(case)
    before = _snapshot(engine, case)
    a = engine.flowIntegrate(par, GROUPS)
    b = engine.flowIntegrate(par, GROUPS)
    assert np.array_equal(a, b) and a[0, E_MASSFLOW] != 0.0, "two calls in a row"
    d_out = dv.put(np.full(3 * 64, 7.0))
    dv.sync()
    engine.set_async(True)
    try:
        engine.flowIntegrateDev(par, dv.ptr(d_out), GROUPS)
        engine.flowIntegrateDev(par, dv.ptr(d_out), GROUPS)
    finally:
        engine.sync()
        engine.set_async(False)
    assert np.array_equal(a, dv.get(d_out).reshape(3, 64)), "enqueue-only device form against the synchronous host form"
    after = _snapshot(engine, case)
    for k in before:
        for x, y in zip(before[k], after[k]):
            assert np.array_equal(x, y), (k, "changed by the flow integration")
    val, scl = case.yardstick(par, GROUPS)
    compare_sums(a, val, scl, "determinism case", empty=(2,))


def check_wall_plus_flow(engine):
    """integrateSurfaces on a mesh with both kinds of faces: the two vectors added"""
    case = case_of("rans")
    assert len(case.wall_inputs) == 4 and len(case.inputs) == 2
    case.run(engine)
    par, wpar = par_of(case), wf.default_par(case.prm, pointRef=(0.3, -0.2, 0.1))
    both = engine.wallIntegrate(wpar) + engine.flowIntegrate(par)
    vf, sf = case.yardstick(par)
    vw, sw = case.wall_yardstick(wpar)
    val, scl = vf + vw, sf + sw
    val[0, wf.E_CPMIN] = vw[0, wf.E_CPMIN]
    for e in sorted(set(SUMS) | set(wf.SUMS)):
        assert scl[0, e] > 0.0 or e in (wf.E_CAV, wf.E_CPMIN_KS), e
        assert abs(both[0, e] - val[0, e]) <= TOL * scl[0, e], ("integrateSurfaces", e, both[0, e], val[0, e])
    shared = [E_FP + c for c in range(3)] + list(range(E_COF, E_COF + 9))
    assert all(abs(vf[0, e]) > 0 and abs(vw[0, e]) > 0 for e in shared), "iFp and iCoForce* receive both parts"
    assert abs(both[0, wf.E_YPLUS] - vw[0, wf.E_YPLUS]) <= TOL * abs(vw[0, wf.E_YPLUS]) and vw[0, wf.E_YPLUS] > 0


def check_errors(engine):
    case = case_of("euler-i")
    par = par_of(case)
    lib = engine.lib
    n = case.nw * case.ncells()
    out, dot, x, wbar, ob = np.zeros((4, 64)), np.zeros(64), np.ones(n), np.zeros(2 * n + 8), np.zeros(64)
    ob[E_MASSFLOW] = 1.0
    msg = lambda: lib.adflow_gpu_last_error().decode()
    P = lambda a: None if a is None else a.ctypes.data

    def val(par_=par, nG=0, fl=None, ld=0):
        return lib.adflow_gpu_flow_integrate(1, P(par_), nG, P(fl), ld, P(out))

    def fwd(flags=0, x_=x, n_=n, dot_=dot, nG=0, fl=None, ld=0):
        return lib.adflow_gpu_flow_integrate_fwd(1, flags, P(x_), n_, P(par), nG, P(fl), ld, P(out), P(dot_))

    def bwd(flags=0, ob_=ob, nRhs=1, wbar_=wbar, n_=n, ld=n, nG=0, fl=None, ldf=0):
        return lib.adflow_gpu_flow_integrate_bwd(1, flags, P(par), nG, P(fl), ldf, P(ob_), nRhs, P(wbar_), n_, ld)

    def refused(word, call, **kw):
        engine.releaseWorkspace()
        rc = call(**kw)
        assert rc != 0 and word in msg(), (word, kw, rc, msg())
        assert engine.releaseWorkspace() == 0, ("a refused call left buffers behind", word, kw)

    # a level without registered boundary subfaces
    checks.new_level(engine)
    engine.set_options(case.prm)
    engine.register(case.blks[1], nn=1, level=1)
    for call in (val, fwd, bwd):
        refused("no registered boundary subfaces", call)
    case.run(engine)
    fl = np.asfortranarray(np.array([[3, 0, 0], [1, 0, 0]], np.int32))
    for call in (val, fwd, bwd):
        refused("nGroups", call, nG=-1)
        refused("ldFam - 1", call, nG=2, fl=fl, **{"ldf" if call is bwd else "ld": 3})
    bad = par.copy()
    bad[capi.FLOWINT_RHOREF] = 0.0
    refused("rhoRef", val, par_=bad)
    for f in (capi.JAC_PC, capi.JAC_VISC_PC, capi.JAC_APPROX_SA):
        refused("approximations of the fluxes", fwd, flags=f)
        refused("approximations of the fluxes", bwd, flags=f)
    refused("rows", fwd, n_=n - 5)
    refused("rows", bwd, n_=n + 5, ld=n + 5)
    refused("x is NULL", fwd, x_=None)
    refused("outDot is NULL", fwd, dot_=None)
    refused("outBar is NULL", bwd, ob_=None)
    refused("wbar is NULL", bwd, wbar_=None)
    refused("nRhs", bwd, nRhs=0)
    refused("nRhs", bwd, nRhs=capi.MAX_NVEC + 1)
    refused("ld >= n", bwd, nRhs=2, ld=n - 1)
    assert not out.any() and not dot.any() and not wbar.any(), "a refused call wrote its result"
    # the level is usable, and what the entries allocated is what adflow_gpu_release_workspace frees and counts
    check(engine, case, run=False, what="a valid call after the refused ones")
    assert fwd() == 0 and dot.any() and bwd() == 0 and wbar[:n].any(), msg()
    assert engine.releaseWorkspace() > 0 and engine.releaseWorkspace() == 0
    check(engine, case, run=False, what="the buffers come back with the next call")
    # halos exchanged with another rank: _bwd refuses before its record exists.  Rank 0's half of a brick over two ranks, its pattern
    # with sends and receives registered (the refusal comes before any exchange)
    topo = BrickTopology(Bi=2, Bj=1, Bk=1, nx=6, ny=5, nz=4, owner=lambda g: g, periodic=(False,) * 3)
    from adflow_amd import synth
    faces2 = synth.make_bocos(case.blks[1], case.prm, topo.boundary_spec(0, through(0)), seed=58)
    assert [f["bcType"] for f in faces2[0] if f["faceID"] == 1] == [-8] and not any(f["faceID"] == 2 for f in faces2[0])
    checks.new_level(engine)
    engine.set_options(case.prm)
    engine.register(case.blks[1], nn=1, level=1)
    engine.bc_register(*faces2, nn=1, level=1)
    for lay in (1, 2):
        pat = topo.patterns(lay)[0]
        assert pat.sendProc.size > 0 and pat.recvProc.size > 0
        engine.comm_register(1, lay, pat)
    wbar[:] = 0.0
    refused("other ranks", bwd)
    assert not wbar.any(), "the refused call wrote its result"
    # a level with boundary subfaces but no in- or outflow subface: zeros, no error
    far = wf.cached(("flow", "no-flow"), lambda: FCase(EULER).add(1, (6, 5, 4), dict(wf.FAR)))
    far.run(engine)
    assert not engine.flowIntegrate(par).any()
    out2, dot2 = engine.flowIntegrateFwd(x, par)
    assert not out2.any() and not dot2.any()
    wb = engine.flowIntegrateBwd(ob, n, par)
    assert wb.shape == (1, n) and not wb.any()
    engine.releaseWorkspace()


def check_moving_is_refused_by_the_derivatives(engine):
    case = case_of("moving")
    case.run(engine)
    engine.releaseWorkspace()
    x = np.ones(case.nw * case.ncells())
    try:
        engine.flowIntegrateFwd(x, par_of(case))
    except capi.AdflowGpuError as err:
        assert "moving" in str(err)
        assert engine.releaseWorkspace() == 0, "the refusal left buffers behind"
    else:
        raise AssertionError("a moving block is not linearised: the derivative entries refuse it")


# ---- derivatives ------------------------------------------------------------------------------------------------------------------------
def richardson(case, par, v, l0, ns, h):
    def central(step):
        dw = case.scatter(step * v.reshape(-1), l0, ns)
        tp = case.terms(par, dw)
        tm = case.terms(par, {nn: -d for nn, d in dw.items()})
        return {key: {e: (tp[key][e] - tm[key][e]) / (2.0 * step) for e in SUMS} for key in tp}
    d1, d2 = central(h), central(0.5 * h)
    return {key: {e: (4.0 * d2[key][e] - d1[key][e]) / 3.0 for e in SUMS} for key in d1}


def group_sums(case, faces, groups):
    glist = [None] if groups is None else groups
    S, M = np.zeros((len(glist), 64)), np.zeros((len(glist), 64))
    for g, fams in enumerate(glist):
        for key in case.walls():
            if fams is not None and case.fam[key[0]][key[1] - 1] not in fams:
                continue
            for e in SUMS:
                S[g, e] += faces[key][e].sum()
                M[g, e] += np.abs(faces[key][e]).sum()
    return S, M


_yard = {}


def yardstick(name, case, par, groups, seed, frozenTurb=False, useTurbOnly=False):
    key = (name, seed, frozenTurb, useTurbOnly, None if groups is None else tuple(map(tuple, groups)))
    if key not in _yard:
        l0, ns = wd.state_range(case, frozenTurb, useTurbOnly)
        v, _ = wd.direction(case, seed, l0, ns)
        S, M = group_sums(case, richardson(case, par, v, l0, ns, H), groups)
        _yard[key] = (v.reshape(-1), S, M)
    return _yard[key]


def noise_of(case, par, h=H, seed=11, **flags):
    l0, ns = wd.state_range(case, **flags)
    v, _ = wd.direction(case, seed, l0, ns)
    S1, M1 = group_sums(case, richardson(case, par, v, l0, ns, h), None)
    S2, _ = group_sums(case, richardson(case, par, v, l0, ns, 0.5 * h), None)
    ok = M1[0] > 0
    r = np.zeros(64)
    r[ok] = np.abs(S1[0] - S2[0])[ok] / M1[0][ok]
    return float(r.max()), int(np.argmax(r))


def measure_floor(steps=(H,)):
    """prints the noise of the yardstick per case and step and returns (the largest at the step H, its case)"""
    result = None
    for h in steps:
        worst, where = 0.0, None
        runs = [(name, {}) for name in dict.fromkeys(FORWARD + TRANSPOSE)] + FLAGGED
        for name, kw in runs:
            case = case_of(name)
            r, e = noise_of(case, par_of(case), h=h, **kw)
            print(f"h = 2^{int(np.log2(h))} {name} {kw}: largest |R(h, h/2) - R(h/2, h/4)| / M_e = {r:.3e} (entry {e})")
            if r > worst:
                worst, where = r, name
        print(f"h = 2^{int(np.log2(h))}: floor {worst!r} ({where}); FLOOR = {FLOOR!r}, BAR = {BAR!r}")
        if h == H:
            result = (worst, where)
    return result


def assert_alive(what, M, case, groups):
    for g in range(M.shape[0]):
        if groups is not None and not any(case.fam[k[0]][k[1] - 1] in groups[g] for k in case.walls()):
            continue
        assert all(M[g, e] > 0.0 for e in SUMS if e != E_AREA), (what, g, "a trivial derivative")
        assert M[g, E_AREA] == 0.0


def check_forward(engine, name, **flags):
    case = case_of(name)
    par, groups = par_of(case), groups_of(case)
    case.yardstick(par, groups)                                  # (asserts Ptot >= 1.02 on every integrated face)
    v, S, M = yardstick(name, case, par, groups, 11, **flags)
    assert_alive(name, M, case, groups)
    case.run(engine)
    base = engine.flowIntegrate(par, groups)
    out, dot = engine.flowIntegrateFwd(v, par, groups, **flags)
    worst = 0.0
    for g in range(S.shape[0]):
        for e in range(64):
            if e not in SUMS:
                assert dot[g, e] == 0.0, (name, g, e, "an entry without a derivative")
        for e in SUMS:
            err, bar = abs(dot[g, e] - S[g, e]), BAR * M[g, e]
            if M[g, e] > 0:
                worst = max(worst, err / M[g, e])
            assert err <= bar, (name, flags, g, e, err, bar, dot[g, e], S[g, e])
    print(f"{name} {flags}: largest |outDot - S_ref| / M_e = {worst:.3e}, bar {BAR:.1e}")
    assert np.array_equal(out, base), (name, "the value parts of the forward pass against flowIntegrate, to the bit")
    engine.releaseWorkspace()


def weights(case, groups, nRhs, seed=5):
    rng = np.random.default_rng(seed)
    nG = 1 if groups is None else len(groups)
    ob = np.zeros((nRhs, nG, 64))
    ob[:, :, SUMS] = rng.uniform(-1.0, 1.0, (nRhs, nG, len(SUMS)))
    return ob


def check_transpose(engine, name, **flags):
    case = case_of(name)
    par, groups = par_of(case), groups_of(case)
    v, S, M = yardstick(name, case, par, groups, 13, **flags)
    assert_alive(name, M, case, groups)
    case.run(engine)
    ob = weights(case, groups, 1)
    wbar = engine.flowIntegrateBwd(ob, v.size, par, groups, **flags)
    assert wbar.shape == (1, v.size) and np.isfinite(wbar).all()
    lhs, rhs, bar = float(wbar[0] @ v), float((ob[0] * S).sum()), BAR * float((np.abs(ob[0]) * M).sum())
    print(f"{name} {flags}: bwd(outBar) . v = {lhs:.9e}, outBar . FD_ref(v) = {rhs:.9e}, |difference| / bar = {abs(lhs - rhs) / bar:.3e}")
    assert bar > 0.0 and abs(lhs - rhs) <= bar, (name, flags, lhs, rhs, bar)
    _, dot = engine.flowIntegrateFwd(v, par, groups, values=False, **flags)
    a, mag = float((ob[0] * dot).sum()), float((np.abs(ob[0]) * np.abs(dot)).sum()) + float(np.abs(wbar[0]) @ np.abs(v))
    assert abs(a - lhs) <= 1e-12 * mag, (name, flags, "outBar . fwd(v) against bwd(outBar) . v", a, lhs, mag)
    assert np.array_equal(wbar, engine.flowIntegrateBwd(ob, v.size, par, groups, **flags)), "two transposed calls"
    engine.releaseWorkspace()


def check_turb_only(engine, name="rans"):
    """ADFLOW_JAC_TURB_ONLY: no term of flowIntegrationFace reads the turbulence variable or the eddy viscosity, so every derivative
    is exactly zero in the reference (M_e = 0, no relative bar exists) and the dual pass, which seeds nothing the terms read, gives
    exact zeros"""
    case = case_of(name)
    par = par_of(case)
    v, S, M = yardstick(name, case, par, None, 11, useTurbOnly=True)
    assert not S.any() and not M.any() and np.abs(v).min() > 0.0
    case.run(engine)
    out, dot = engine.flowIntegrateFwd(v, par, useTurbOnly=True)
    assert not dot.any() and out[0, E_MASSFLOW] != 0.0
    wbar = engine.flowIntegrateBwd(weights(case, None, 1), v.size, par, useTurbOnly=True)
    assert wbar.shape == (1, case.ncells()) and not wbar.any()
    engine.releaseWorkspace()


def check_colouring(engine, name):
    """the matrix column by column from fwd(e_j), row by row from bwd of unit weights: the 5 x 5 x 4 box of the coloured sweep holds
    every cell a term of a flow face depends on"""
    case = case_of(name)
    par, groups = par_of(case), groups_of(case)
    case.run(engine)
    n = case.nw * case.ncells()
    nG = 1 if groups is None else len(groups)
    A = np.zeros((nG, 64, n))
    x = np.zeros(n)
    for j in range(n):
        x[j] = 1.0
        A[:, :, j] = engine.flowIntegrateFwd(x, par, groups, values=False)[1]
        x[j] = 0.0
    rows = [(g, e) for g in range(nG) for e in SUMS]
    worst = 0.0
    for r0 in range(0, len(rows), capi.MAX_NVEC):
        part = rows[r0:r0 + capi.MAX_NVEC]
        ob = np.zeros((len(part), nG, 64))
        for r, (g, e) in enumerate(part):
            ob[r, g, e] = 1.0
        B = engine.flowIntegrateBwd(ob, n, par, groups)
        for r, (g, e) in enumerate(part):
            scale = np.abs(A[g, e]).max()
            assert scale > 0.0 or e == E_AREA, (name, g, e, "an empty row")
            err = np.abs(B[r] - A[g, e]).max()
            assert err <= 1e-12 * scale, (name, g, e, err, scale, int(np.argmax(np.abs(B[r] - A[g, e]))))
            worst = max(worst, err / scale if scale > 0 else 0.0)
    print(f"{name}: {n} columns, {len(rows)} rows, largest |bwd row - fwd columns| / max|row| = {worst:.3e}")
    engine.releaseWorkspace()


def check_multi(engine, name="split"):
    case = case_of(name)
    par, groups = par_of(case), groups_of(case)
    case.run(engine)
    n = case.nw * case.ncells()
    ob = weights(case, groups, 4, seed=9)
    ld = n + 7
    wb = engine.flowIntegrateBwd(ob, n, par, groups, ld=ld, fill=7.0)
    assert wb.shape == (4, ld) and (wb[:, n:] == 7.0).all(), "the padding was written"
    one = engine.flowIntegrateBwd(ob[0], n, par, groups)
    assert np.abs(one).max() > 0 and np.array_equal(one[0], wb[0, :n]), "column 0 of four sets against the single sweep"
    engine.releaseWorkspace()


def check_chained(engine, dv, name="split"):
    """the _dev forms, enqueue-only, chained with an evaluation, one synchronise at the end, against the synchronous chain and the
    host forms; state, residual and the wall entries' arrays unchanged"""
    case = case_of(name)
    par, groups = par_of(case), groups_of(case)
    case.run(engine)
    n = case.nw * case.ncells()
    nG = len(groups)
    v = wd.direction(case, 17, 0, case.nw)[0].reshape(-1)
    ob = weights(case, groups, 2, seed=21)
    before = _snapshot(engine, case)
    out, dot = engine.flowIntegrateFwd(v, par, groups)
    wbar = engine.flowIntegrateBwd(ob, n, par, groups)
    after = _snapshot(engine, case)
    for k in before:
        for a, b in zip(before[k], after[k]):
            assert np.array_equal(a, b), (k, "changed by the derivative entries")

    def setup(enqueue):
        case.run(engine)
        return dict(d=dict(x=dv.put(v), out=dv.put(np.full(nG * 64, 7.0)), dot=dv.put(np.full(nG * 64, 7.0)),
                           wbar=dv.put(np.full(2 * n, 7.0)), int=dv.put(np.full(nG * 64, 7.0))))

    def chain(c, link):
        d, p = c["d"], dv.ptr
        link(engine.blocketteRes, 1, True, True, case.nw > 5)
        link(engine.flowIntegrateFwdDev, p(d["x"]), n, par, p(d["out"]), p(d["dot"]), groups)
        link(engine.flowIntegrateBwdDev, ob, p(d["wbar"]), n, n, par, groups)
        link(engine.flowIntegrateDev, par, p(d["int"]), groups)
        return dict(d)
    c, enq, syn = async_checks.both_runs(engine, dv, setup, chain)
    async_checks.assert_bitwise("flow integration and its derivatives, chained", enq, syn)
    assert np.array_equal(enq["dot"].reshape(nG, 64), dot) and np.array_equal(enq["wbar"].reshape(2, n), wbar), "the _dev forms against the host forms"
    assert np.array_equal(enq["out"], enq["int"]) and np.array_equal(enq["out"].reshape(nG, 64), out)
    engine.releaseWorkspace()
