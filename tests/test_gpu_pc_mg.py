"""GPU parity (real MI355X, through the C-ABI): the multigrid preconditioner of amg.F90 on the 7-point preconditioner matrix
(adflow_gpu_pc_set_mg, _pc_mg_info, _pc_mg_download) and everything that takes a factor on top of a hierarchy: pc_apply, gmres_solve,
ank_pc_setup, ank_solve, the two slots, the enqueue-only mode.  Against the numpy cycle of tests/pc_mg_checks.py in float64 and
longdouble: the library may be at most 10 x as far from the longdouble result as the float64 numpy run is."""
import pytest

import ank_checks as ank
import jacmult_checks as jm
import pc_checks as pc
import pc_mg_checks as mg
from adflow_amd.params import FlowParams, dissScalar, upwind
from adflow_amd.topology import BrickTopology, ell_topology

pytestmark = pytest.mark.gpu

# iteration cap of the ANK solve: restart = maxIts = cap; scipy's gmres with the numpy cycle must converge inside it as well
CAP_ANK = 32


@pytest.mark.parametrize("levels", [2, 3])
def test_euler_remainder_aggregates(engine, levels):
    """Euler, nState 5, 7 x 5 x 4: 7 -> 4 -> 2 and 5 -> 3 -> 2 leave a one-cell remainder aggregate in i and j on both coarsenings,
    4 -> 2 -> 1 reaches a direction of one cell"""
    mg.check_single(engine, (7, 5, 4), mg.pcf.EULER_JST, jm.EULER, [(levels, 1, 0, 0)], cells={2: (140, 24), 3: (140, 24, 4)})


@pytest.mark.parametrize("fills", [(2, 1), (1, 2)])
def test_rans_three_levels_two_smoothing_iterations(engine, fills):
    """RANS SA, nState 6, 7 x 6 x 5 -> 4 x 3 x 3 -> 2 x 2 x 2, nSmooth 2: the residual kernel of the second Richardson iteration, the
    fill kernels on coarse blocks two cells thick"""
    mg.check_single(engine, (7, 6, 5), pc.RANS, jm.WALL, [(3, 2) + fills], cells={3: (210, 36, 8)}, stretch_k=2.0)


@pytest.mark.parametrize("fills", [(2, 1), (1, 2)])
def test_rans_coarse_block_one_cell_thick(engine, fills):
    """6 x 5 x 2 -> 3 x 3 x 1 -> 2 x 2 x 1: the fill kernels on a coarse block one cell thick"""
    mg.check_single(engine, (6, 5, 2), pc.RANS, jm.WALL, [(3, 2) + fills], cells={3: (60, 9, 4)}, stretch_k=2.0)


def test_turb_only(engine):
    mg.check_single(engine, (8, 7, 6), pc.RANS, jm.WALL, [(2, 1, 0, 0)], cells={2: (336, 48)}, useTurbOnly=True, stretch_k=2.0)   # nState 1


def test_blocks_of_different_sizes(engine):
    mg.check_brick(engine, ell_topology(), FlowParams(spaceDiscr=upwind), seed=251)


def test_periodic_brick(engine):
    mg.check_brick(engine, BrickTopology(2, 2, 1, 6, 5, 4), FlowParams(spaceDiscr=dissScalar))


def test_coarse_rows_wider_than_a_wave(engine):
    """131 x 6 x 5, nState 5: the coarse i has 66 cells, more than one wave, with an odd remainder at the end"""
    mg.check_single(engine, (131, 6, 5), mg.pcf.EULER_JST, jm.EULER, [(2, 1, 0, 0)], cells={2: (3930, 594)})


def test_gmres_count_equals_scipy(engine):
    mg.check_gmres(engine, (12, 8, 6))


def test_ank_time_step_on_every_level(engine):
    mg.check_ank(engine, (7, 6, 5))


def test_ank_solve(engine):
    mg.check_ank_solve(engine, (7, 6, 5), ank.RANS_JST, jm.WALL, CAP_ANK, stretch_k=2.0)


def test_slots_and_bit_identity(engine):
    mg.check_slots_and_identity(engine)


def test_enqueue_only_chain(engine, request):
    mg.check_enqueue_only(engine, __import__("device_vectors").device_vectors(request.config))


def test_refusals(engine):
    mg.check_refusals(engine)
