"""CPU-only twin of tests/test_gpu_async.py: the chains of tests/async_checks.py on the kernel-logic emulator (tests/hostsim).  Its
queues are synchronous, so every chain is trivially ordered here: the twin proves the test logic, the references and the host-side
state handling (guards, slots, refusals) before the run on the device."""
import pytest

import async_checks as ac
import checks
from adflow_amd.params import FlowParams, RANSEquations, DADI, upwind, noResAveraging, alwaysResAveraging
from adflow_amd.topology import BrickTopology, ell_topology
from device_vectors import HostVectors
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")

DV = HostVectors()
# iteration caps of the ANK solves: scipy's gmres with the numpy ILU(0) as right preconditioner needs at most half of them on these
# inputs (async_checks asserts that as well); the caps of tests/test_gpu_ank.py and tests/test_gpu_ank_turb.py
CAP_FLOW, CAP_TURB = 16, 8
T1 = BrickTopology(1, 1, 1, 70, 9, 11)


@pytest.mark.parametrize("prm", [ac.RANS, ac.LAMINAR_MATRIX], ids=["rans-roe", "laminar-matrix"])
def test_residual_chain_wall_bounded_block(hostsim_engine, prm):
    ac.check_residual_chain(hostsim_engine, DV, T1, prm, bc_spec=ac.jm.WALL, stretch_k=2.0)


def test_split_evaluation_chain(hostsim_engine):
    """split_eval = 2 on a non-periodic 2 x 1 x 1 brick with boundary subfaces: state write, whole blocketteRes, residual copy, three
    times; the interior tiles run on the side queue while the next link's state write waits behind the join"""
    ac.check_split_chain(hostsim_engine, DV, BrickTopology(2, 1, 1, 70, 9, 11, periodic=(False, False, False)))


def test_residual_chain_brick(hostsim_engine):
    """(the emulator is built without RCCL: the interfaces are the same-process copies here)"""
    ac.check_residual_chain(hostsim_engine, DV, BrickTopology(2, 2, 1, 9, 7, 5), ac.RANS, stretch_k=2.0)


def test_refused_calls_inside_a_chain(hostsim_engine):
    ac.check_residual_chain(hostsim_engine, DV, T1, ac.RANS, bc_spec=ac.jm.WALL, stretch_k=2.0, refusals=True)


def test_rk_sweeps(hostsim_engine):
    ac.check_sweeps_chain(hostsim_engine, checks.check_rk_smoother, BrickTopology(2, 2, 2, 7, 5, 4), FlowParams(resAveraging=alwaysResAveraging),
                          nsweeps=2)


def test_dadi_and_sa_sweeps_with_bc(hostsim_engine):
    rans = FlowParams(equations=RANSEquations, smoother=DADI, resAveraging=noResAveraging, cfl=1.5, nSubiterations=2, nSubIterTurb=2)
    ac.check_sweeps_chain(hostsim_engine, checks.check_smoother_with_bc, (16, 10, 7), rans, ac.jm.WALL, nsweeps=2, sa_solve=True, stretch_k=2.0)


def test_mg_cycles(hostsim_engine):
    ac.check_sweeps_chain(hostsim_engine, checks.check_mg_cycle, BrickTopology(1, 1, 1, 8, 8, 4), FlowParams(), [0, 1, 0, -1], ncycles=3,
                          bc_spec={1: -6, 2: -6, 3: -5, 4: -6, 5: -1, 6: -1})


def test_matrix_chain_blocks_of_different_sizes(hostsim_engine):
    ac.check_matrix_chain(hostsim_engine, DV, topo=ell_topology(), prm=FlowParams(spaceDiscr=upwind))


def test_matrix_chain_rans_block(hostsim_engine):
    ac.check_matrix_chain(hostsim_engine, DV, dims=(7, 6, 5))


def test_update_wall_distances_consumes_xsurf(hostsim_engine):
    ac.check_update_wall_distances_consumes_xsurf(hostsim_engine, DV, (70, 24, 40))


def test_wall_distance_register_consumes_its_arrays(hostsim_engine):
    ac.check_wall_distance_register_consumes_its_arrays(hostsim_engine, DV, (70, 24, 40))


def test_hot_path_chain(hostsim_engine):
    ac.check_hot_path_chain(hostsim_engine, DV, (70, 9, 11))


@pytest.mark.parametrize("dims", [(70, 9, 11), (16, 8, 1)])
def test_mesh_warp_chain(hostsim_engine, dims):
    ac.check_mesh_warp_chain(hostsim_engine, dims)


def test_ank_flow_chain(hostsim_engine):
    ac.check_ank_flow_chain(hostsim_engine, DV, (10, 7, 6), CAP_FLOW)


def test_ank_turbulence_chain(hostsim_engine):
    ac.check_ank_turb_chain(hostsim_engine, DV, (10, 7, 6), CAP_TURB)
