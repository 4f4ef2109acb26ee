"""GPU parity (real MI355X, through the C-ABI) in the enqueue-only mode, adflow_gpu_set_async(1): the mode bench.py and tools/ time
in and a host with device vectors runs in.  Chains of hot-path calls with ONE synchronise at the end -- residual evaluations (plain,
split around the exchange, through RCCL messages to the own rank), the mixed hot path with its guards, smoothers and multigrid cycles
(direct, captured, replayed), the assembled-matrix entries, the ANK step of both kinds, the mesh warp -- each against the reference
with the yardstick of its synchronous test AND bit for bit against the same chain with a synchronise after every call
(tests/async_checks.py); and the entries that take a caller's host array, which must have consumed it when they return."""
import pytest

import async_checks as ac
import checks
from adflow_amd.params import FlowParams, RANSEquations, DADI, upwind, noResAveraging, alwaysResAveraging
from adflow_amd.topology import BrickTopology, ell_topology
from device_vectors import device_vectors

pytestmark = pytest.mark.gpu

# iteration caps of the ANK solves: scipy's gmres with the numpy ILU(0) as right preconditioner needs at most half of them on these
# inputs (async_checks asserts that as well); the caps of tests/test_gpu_ank.py and tests/test_gpu_ank_turb.py
CAP_FLOW, CAP_TURB = 16, 8
T1 = BrickTopology(1, 1, 1, 70, 9, 11)        # a partial 64-column tile, a partial 4-row tile, several tiles


@pytest.fixture
def dv(request):
    return device_vectors(request.config)


@pytest.mark.parametrize("prm", [ac.RANS, ac.LAMINAR_MATRIX], ids=["rans-roe", "laminar-matrix"])
def test_residual_chain_wall_bounded_block(engine, dv, prm):
    """three nk_residual_dev with three states back to back: the work space of call N + 1 against the reads of call N"""
    ac.check_residual_chain(engine, dv, T1, prm, bc_spec=ac.jm.WALL, stretch_k=2.0)


def test_split_evaluation_chain(engine, dv):
    """split_eval = 2 on a non-periodic 2 x 1 x 1 brick with boundary subfaces: state write, whole blocketteRes, residual copy, three
    times; the interior tiles run on the side queue while the next link's state write waits behind the join"""
    ac.check_split_chain(engine, dv, BrickTopology(2, 1, 1, 70, 9, 11, periodic=(False, False, False)))


def test_residual_chain_rccl_self(engine, dv):
    """every interface of a 2 x 2 x 1 brick an RCCL message to the own rank, overlapped on the exchange queue"""
    ac.check_residual_chain(engine, dv, BrickTopology(2, 2, 1, 9, 7, 5), ac.RANS, stretch_k=2.0, rccl_self=True)


def test_refused_calls_inside_a_chain(engine, dv):
    """wrong n, no factor, no base, a cycle that fails after it forced the mode on: each returns its error, the queue stays usable and
    the results are those of the chain without them.  The mode itself cannot be read back through the ABI: that a refused call and
    every exit of adflow_gpu_mg_cycle leave it as the caller set it rests on reading api.hip (mg_cycle saves g_async in front of
    mg_cycle_enqueue and restores it before it looks at the result, in the direct and in the capture path; no other entry writes it)"""
    ac.check_residual_chain(engine, dv, T1, ac.RANS, bc_spec=ac.jm.WALL, stretch_k=2.0, refusals=True)


def test_hot_path_chain(engine, dv):
    ac.check_hot_path_chain(engine, dv, (70, 9, 11))


def test_rk_sweeps(engine):
    ac.check_sweeps_chain(engine, checks.check_rk_smoother, BrickTopology(2, 2, 2, 7, 5, 4), FlowParams(resAveraging=alwaysResAveraging), nsweeps=2)


def test_dadi_and_sa_sweeps_with_bc(engine):
    rans = FlowParams(equations=RANSEquations, smoother=DADI, resAveraging=noResAveraging, cfl=1.5, nSubiterations=2, nSubIterTurb=2)
    ac.check_sweeps_chain(engine, checks.check_smoother_with_bc, (16, 10, 7), rans, ac.jm.WALL, nsweeps=2, sa_solve=True, stretch_k=2.0)


def test_mg_cycles_direct_captured_replayed(engine):
    """three identical V cycles in a row: the first runs directly, the second is captured into a graph, the third replays it"""
    with ac.tuning(engine, {"mg_graph": (1, 1)}):           # (the default; setting it also clears an earlier failed capture)
        ac.check_sweeps_chain(engine, checks.check_mg_cycle, BrickTopology(1, 1, 1, 8, 8, 4), FlowParams(), [0, 1, 0, -1], ncycles=3,
                              bc_spec={1: -6, 2: -6, 3: -5, 4: -6, 5: -1, 6: -1})


def test_matrix_chain_blocks_of_different_sizes(engine, dv):
    ac.check_matrix_chain(engine, dv, topo=ell_topology(), prm=FlowParams(spaceDiscr=upwind))


def test_matrix_chain_rans_block(engine, dv):
    ac.check_matrix_chain(engine, dv, dims=(7, 6, 5))


def test_ank_flow_chain(engine, dv):
    ac.check_ank_flow_chain(engine, dv, (10, 7, 6), CAP_FLOW)


def test_ank_turbulence_chain(engine, dv):
    ac.check_ank_turb_chain(engine, dv, (10, 7, 6), CAP_TURB)


@pytest.mark.parametrize("dims", [(70, 9, 11), (16, 8, 1)])
def test_mesh_warp_chain(engine, dims):
    ac.check_mesh_warp_chain(engine, dims)


def test_update_wall_distances_consumes_xsurf(engine, dv):
    """xSurf in pinned memory, overwritten with NaN as soon as the call returns, residual evaluations of a 70 x 24 x 40 block in the
    queue in front of the copy: an entry that takes a caller's host array has consumed it when it returns, whatever the mode"""
    ac.check_update_wall_distances_consumes_xsurf(engine, dv, (70, 24, 40))


def test_wall_distance_register_consumes_its_arrays(engine, dv):
    ac.check_wall_distance_register_consumes_its_arrays(engine, dv, (70, 24, 40))
