"""CPU-only twin of tests/test_gpu_pc_mg.py: the kernels of adflow_amd/csrc/kernels_pc_mg.hip compiled with g++ (tests/hostsim) on
the small shapes of the same cases, against the numpy cycle of tests/pc_mg_checks.py."""
import pytest

import ank_checks as ank
import jacmult_checks as jm
import pc_checks as pc
import pc_mg_checks as mg
from adflow_amd.params import FlowParams, dissScalar, upwind
from adflow_amd.topology import BrickTopology, ell_topology
from device_vectors import HostVectors
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")

# iteration cap of the ANK solve: restart = maxIts = cap; scipy's gmres with the numpy cycle must converge inside it as well
CAP_ANK = 32


@pytest.mark.parametrize("levels", [2, 3])
def test_euler_remainder_aggregates(hostsim_engine, levels):
    """Euler, nState 5, 7 x 5 x 4: 7 -> 4 -> 2 and 5 -> 3 -> 2 leave a one-cell remainder aggregate in i and j on both coarsenings,
    4 -> 2 -> 1 reaches a direction of one cell"""
    mg.check_single(hostsim_engine, (7, 5, 4), mg.pcf.EULER_JST, jm.EULER, [(levels, 1, 0, 0)], cells={2: (140, 24), 3: (140, 24, 4)})


@pytest.mark.parametrize("fills", [(2, 1), (1, 2)])
def test_rans_three_levels_two_smoothing_iterations(hostsim_engine, fills):
    """RANS SA, nState 6, 7 x 6 x 5 -> 4 x 3 x 3 -> 2 x 2 x 2, nSmooth 2: the residual kernel of the second Richardson iteration, the
    fill kernels on coarse blocks two cells thick"""
    mg.check_single(hostsim_engine, (7, 6, 5), pc.RANS, jm.WALL, [(3, 2) + fills], cells={3: (210, 36, 8)}, stretch_k=2.0)


@pytest.mark.parametrize("fills", [(2, 1), (1, 2)])
def test_rans_coarse_block_one_cell_thick(hostsim_engine, fills):
    """6 x 5 x 2 -> 3 x 3 x 1 -> 2 x 2 x 1: the fill kernels on a coarse block one cell thick"""
    mg.check_single(hostsim_engine, (6, 5, 2), pc.RANS, jm.WALL, [(3, 2) + fills], cells={3: (60, 9, 4)}, stretch_k=2.0)


def test_turb_only(hostsim_engine):
    mg.check_single(hostsim_engine, (8, 7, 6), pc.RANS, jm.WALL, [(2, 1, 0, 0)], cells={2: (336, 48)}, useTurbOnly=True, stretch_k=2.0)   # nState 1


def test_blocks_of_different_sizes(hostsim_engine):
    mg.check_brick(hostsim_engine, ell_topology(), FlowParams(spaceDiscr=upwind), seed=251)


def test_periodic_brick(hostsim_engine):
    mg.check_brick(hostsim_engine, BrickTopology(2, 2, 1, 6, 5, 4), FlowParams(spaceDiscr=dissScalar))


def test_gmres_count_equals_scipy(hostsim_engine):
    mg.check_gmres(hostsim_engine, (12, 8, 6))


def test_ank_time_step_on_every_level(hostsim_engine):
    mg.check_ank(hostsim_engine, (7, 6, 5))


def test_ank_solve(hostsim_engine):
    mg.check_ank_solve(hostsim_engine, (7, 6, 5), ank.RANS_JST, jm.WALL, CAP_ANK, stretch_k=2.0)


def test_slots_and_bit_identity(hostsim_engine):
    mg.check_slots_and_identity(hostsim_engine)


def test_enqueue_only_chain(hostsim_engine):
    mg.check_enqueue_only(hostsim_engine, HostVectors())


def test_refusals(hostsim_engine):
    mg.check_refusals(hostsim_engine)
