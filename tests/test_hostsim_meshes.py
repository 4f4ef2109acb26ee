"""CPU-only: the mesh families of tests/mesh_families.py -- the shape hook of adflow_amd.synth leaves the default map bit for bit
what it was, the recounts hold on every family and fail on the cube, the reference's own conditioning floor is far below the bars
on every (mesh, entry) pair the GPU tier uses, and the emulator twins of tests/test_gpu_meshes.py."""
import hashlib
import json
import os

import numpy as np
import pytest

import mesh_checks as mc
import mesh_families as mf
from adflow_amd.params import FlowParams, RANSEquations
from adflow_amd.synth import make_block, make_coarse_block, make_nodes
from oracle import ref
from util import TOL, LOCAL_TOL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
needs_ref = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")


# ---- the hook itself -----------------------------------------------------------------------------------------------------------
def _h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def _hb(b):
    return {n: _h(b[n]) for n in ("x", "sI", "sJ", "sK", "vol", "d2Wall", "w")}


def test_shape_none_is_the_default_map_bit_for_bit():
    """tests/golden/synth_default_map.json: hashes of the arrays of make_nodes / make_block / make_coarse_block recorded before
    the hook existed -- a few sizes, with and without frame (the four blocks of ell_topology and their coarse levels)"""
    from adflow_amd.topology import ell_topology
    gold = json.load(open(os.path.join(GOLDEN, "synth_default_map.json")))
    rans = FlowParams(equations=RANSEquations)
    got = {}
    far = dict(stretch_k=2.0, lengths=(2.0, 0.5, 1.5), origin=(3.0, -1.0, 0.25), amp=0.03)
    for dims in ((5, 4, 3), (12, 8, 6), (9, 7, 5)):
        got["nodes %s" % (dims,)] = _h(make_nodes(*dims))
        got["block %s" % (dims,)] = _hb(make_block(*dims, FlowParams(), seed=3))
        b = make_block(*dims, rans, seed=4, **far)
        got["block rans %s" % (dims,)] = _hb(b)
        got["coarse %s" % (dims,)] = _hb(make_coarse_block(b, rans, seed=5, **far))
    topo = ell_topology(stretch_z=2.0)
    for g in range(topo.nblocks):
        b = topo.make_block(g, rans, seed=6 + g)
        got["ell block %d" % g] = _hb(b)
        if all(n % 2 == 0 for n in topo.dims(g)):
            got["ell coarse %d" % g] = _hb(make_coarse_block(b, rans, seed=9))
    assert got == gold


def test_cube_as_a_shape_is_the_default_map():
    """the hook evaluates a shape on the very parameters the default map gets: the cube written as a shape gives the same nodes"""
    for dims in ((5, 4, 3), (12, 8, 6)):
        for kw in ({}, dict(stretch_k=2.0, lengths=(2.0, 0.5, 1.5), origin=(3.0, -1.0, 0.25))):
            a, b = make_nodes(*dims, **kw), make_nodes(*dims, shape=mf.Cube(), **kw)
            assert np.abs(a - b).max() <= 4e-16 * np.abs(a).max()


@pytest.mark.parametrize("name", sorted(mf.FAMILIES))
def test_shared_nodes_of_a_brick_and_its_coarse_level_are_bit_identical(name):
    """through frame: two blocks joined in i evaluate ONE map; the nodes of the interface, and the halo nodes inside the neighbour,
    are the same bits on both sides -- on the fine level, on the coarse level, and between the levels (coarse node = fine node)"""
    case = mc.CASE[name]
    topo = case.brick((6, 8, 6))
    fine = [topo.make_block(g, FlowParams(), seed=g, **case.brick_mk()) for g in range(2)]
    coarse = [make_coarse_block(b, FlowParams(), seed=7, **case.brick_mk()) for b in fine]
    for lev, n in ((fine, 6), (coarse, 3)):
        a, b = lev[0]["x"], lev[1]["x"]
        assert np.array_equal(a[n:n + 3], b[0:3])            # nodes il - 1, il, ie of the first block = nodes 0, 1, 2 of the second
    for f, c in zip(fine, coarse):
        assert c.shape is f.shape
        assert np.array_equal(c["x"][1:-1, 1:-1, 1:-1], f["x"][1:-1:2, 1:-1:2, 1:-1:2])


# ---- the recounts --------------------------------------------------------------------------------------------------------------
ALL_DIMS = mc.BIG_DIMS + [(12, 8, 6), (10, 9, 8), (6, 8, 6), mc.JAC, mc.JAC_EXACT]


@pytest.mark.parametrize("name", sorted(mf.FAMILIES))
def test_recount_holds_on_the_family_and_fails_on_the_default_map(name):
    for dims in ALL_DIMS:
        for sk in (1.0, 2.0):
            n = mf.assert_family(make_block(*dims, FlowParams(), shape=mf.family(name), stretch_k=sk), name)
            cube = make_block(*dims, FlowParams(), stretch_k=sk)
            assert not mf.THRESHOLDS[name](mf.recount(cube), cube), (name, dims, "the default map passes this family's recount")
            with pytest.raises(AssertionError):
                mf.assert_family(make_block(*dims, FlowParams(), shape=mf.Cube(), stretch_k=sk), name)
    if name == "pole":
        b = make_block(10, 9, 8, FlowParams(), shape=mf.family(name))
        assert mf.zero_length_normals(b, 3) == 80 and mf.zero_length_normals(b, 4) == 0 and n["zero_faces"][1] == dims[0] * dims[2]


def test_recounted_figures():
    """the figures DESIGN §5 tabulates, at (70, 9, 12) (measured; bounds with slack)"""
    r = {name: mf.recount(make_block(70, 9, 12, FlowParams(), shape=mf.family(name))) for name in mf.FAMILIES}
    assert r["annulus"]["turning"] > 115.0 and r["annulus"]["vol_ratio"] > 1e5 and r["annulus"]["aspect"] > 50.0
    assert r["annulus"]["vol_min"] < 5e-6
    assert r["sheared"]["min_angle"] < 25.0 and r["sheared"]["vol_ratio"] < 1.05
    assert r["clustered"]["vol_ratio"] > 1e5 and r["clustered"]["aspect"] > 500.0 and r["clustered"]["vol_min"] < 2e-8
    assert r["pole"]["zero_faces"] == (0, 70 * 12, 0) and r["pole"]["vol_min"] > 9e-6


def test_one_ulp_move_keeps_a_collapsed_face_collapsed():
    b = make_block(10, 9, 8, FlowParams(), shape=mf.family("pole"))
    m = mf.one_ulp_moved(b)
    assert mf.zero_length_normals(m, 3) == 80
    d = np.abs(m["x"] - b["x"])
    assert d.max() <= np.spacing(np.abs(b["x"]).max()) and (d[b["x"] != 0.0] > 0.0).all()


def test_gate_fails_on_the_default_map_and_on_a_checker_that_drops_the_shape():
    """mesh_checks.on: the recount runs on the keywords the checker gets, and a checker that filters `shape` or `lengths` away before
    make_block is caught by the spy"""
    from adflow_amd import synth
    case, built = mc.CASE["annulus"], []

    def checker(engine, dims, prm, drop=(), **mk):
        built.append(synth.make_block(*dims, prm, **{k: v for k, v in mk.items() if k not in drop}))

    mk = case.mk()
    mc.on(case, checker, None, (12, 8, 6), FlowParams(), **mk)
    assert built and built[0].shape is mk["shape"]
    for drop in (("shape",), ("lengths",)):
        c = mc.CASE["units-annulus-2^-20"]
        with pytest.raises(AssertionError):
            mc.on(c, checker, None, (12, 8, 6), FlowParams(), drop=drop, **c.mk())
    with pytest.raises(AssertionError):              # the case's keywords replaced by the cube's: the recount itself
        mc.on(case, checker, None, (12, 8, 6), FlowParams(), shape=mf.Cube())
    topo = case.brick((6, 8, 6))
    with pytest.raises(AssertionError):              # ... and on a brick through frame
        mc.on(case, lambda e, t, p, **k: None, None, topo, FlowParams(), shape=mf.Cube())
    with pytest.raises(AssertionError):              # a checker that builds no block at all
        mc.on(case, lambda e, t, p, **k: None, None, topo, FlowParams(), **case.brick_mk())


# ---- the random sweep's cases --------------------------------------------------------------------------------------------------
def test_random_parity_sweep_draws_the_recorded_cases():
    """the 300 cases of tests/test_gpu_adversarial.py::test_random_parity_sweep are, draw for draw, the ones recorded before the
    family draw existed (tests/golden/fuzz_sweep_cases.json); with the family drawn, sizes / options / entries stay the same"""
    import fuzz_parity
    gold = json.load(open(os.path.join(GOLDEN, "fuzz_sweep_cases.json")))
    plain = list(fuzz_parity.cases_of(300, 20260926))
    assert [fuzz_parity.describe(*c[1:]) for c in plain] == gold
    fam = list(fuzz_parity.cases_of(150, 20260926, families=True))
    drawn = 0
    for a, b in zip(plain, fam):
        extra = {k: v for k, v in b[3].items() if k not in a[3]}
        same = lambda m: {k: v for k, v in m.items() if k in a[3] and k != "stretch_k"}      # (a family brings its own clustering)
        assert set(extra) <= {"shape", "lengths", "stretch_k"} and same(b[3]) == same(a[3])
        assert "shape" in b[3] or b[3].get("stretch_k") == a[3].get("stretch_k")
        assert a[1:3] == b[1:3] and a[4:] == b[4:]
        drawn += bool(extra)
    assert drawn > 50


# ---- the reference's own conditioning, and the emulator twins --------------------------------------------------------------------
PAIRS = mc.pairs()


@needs_ref
@pytest.mark.parametrize("case,entry", PAIRS)
def test_entry_on_mesh(hostsim_engine, case, entry):
    mc.run(hostsim_engine, case, entry, big=False)


@needs_ref
@pytest.mark.parametrize("case,entry", [p for p in PAIRS if p[1] not in mc.NO_FLOOR])
def test_reference_is_finite_and_its_conditioning_floor_is_a_tenth_of_the_bar(hostsim_engine, case, entry):
    """the reference's outputs are finite, and moving every node by one ulp changes them by less than a tenth of the bars: what a
    GPU comparison at TOL / LOCAL_TOL finds on this pair is the library's.  At the shapes of the GPU tier."""
    g, l = mc.reference_floor(hostsim_engine, case, entry, big=entry.startswith("res-") and entry != "res-bc")
    print(f"conditioning floor {case} {entry}: global {g:.2e}, local {l:.2e}")
    bar, local_bar = mc.BARS.get(entry, (TOL, LOCAL_TOL))
    assert g <= 0.1 * bar and (local_bar is None or l <= 0.1 * local_bar), (case, entry, g, l)
