"""GPU parity (real MI355X, through the C-ABI): adflow_gpu_pc_set_coupled(1) -- the ILU(0) of the 7-point preconditioner matrix over
the whole level, one subdomain per process as setupStandardKSP (adjointUtils.F90:1374-1562) gives it, the couplings across block
interfaces inside M (csrc/kernels_pc_coupled.hip).  Against pc_checks.NumpyILU0._factor on one row list for the level, in float64
and in longdouble (tests/pc_coupled_checks.py): the library may be at most 10 x as far from the longdouble result as the float64
numpy run is.  Every shape is the smallest at which its mechanism is exercised (at most 1728 cells)."""
import pytest

import pc_coupled_checks as pcc
from adflow_amd.topology import BrickTopology

pytestmark = pytest.mark.gpu


def test_periodic_brick(engine):
    """2 x 2 x 1 periodic blocks of 9 x 8 x 6: 382 cells with more than three lower neighbours, wraps inside the own block along k,
    38 level sets, several longer than one wave"""
    pcc.check_periodic_brick(engine, BrickTopology(2, 2, 1, 9, 8, 6), nsets=38, many_lower=382)


def test_rotated_interfaces(engine):
    """the blocks of ell_topology at half size: the back slot is not the opposite direction, sets of blocks of different sizes"""
    pcc.check_rotated(engine)


def test_wall_brick_apply_and_gmres(engine):
    """the benchmark layout in miniature, RANS Roe by forward mode, nState 6: the apply check and gmresSolve"""
    pcc.check_wall_brick_gmres(engine)


def test_wall_brick_frozen_turb_and_turb_only(engine):
    pcc.check_wall_brick_apply(engine, frozenTurb=True)        # nState = 5
    pcc.check_wall_brick_apply(engine, useTurbOnly=True)       # nState = 1


def test_wall_brick_ank_pc_setup(engine):
    pcc.check_wall_brick_ank(engine)


def test_equivalence_and_isolation(engine):
    pcc.check_equivalence_and_isolation(engine)


def test_refusals(engine):
    pcc.check_refusals(engine)


def test_enqueue_only_chain(engine, request):
    from device_vectors import device_vectors
    pcc.check_enqueue_only_chain(engine, device_vectors(request.config))
