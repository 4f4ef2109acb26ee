"""GPU parity (real MI355X, through the C-ABI): adflow_gpu_pc_setup / _pc_apply -- the block ILU(0) of the 7-point preconditioner
matrix, one subdomain per block, the PCApply of setupStandardKSP (adjointUtils.F90:1374-1562) as PCBJACOBI / ILU(0) / natural
ordering -- and adflow_gpu_gmres_solve.  Against a general pattern-restricted ILU(0) in numpy on the library's downloaded blocks,
run in float64 and in longdouble (tests/pc_checks.py): the library may be at most 10 x as far from the longdouble result as the
float64 numpy run is.  The GMRES solution of the adjoint's order of calls is compared with scipy's spsolve on the reference's
forward-mode blocks (oracle/_ref, ref_ad_jacobian)."""
import numpy as np
import pytest

import jacmult_checks as jm
import pc_checks as pc
from adflow_amd.params import FlowParams, dissScalar, upwind, minmod
from adflow_amd.topology import BrickTopology, ell_topology

pytestmark = pytest.mark.gpu

# iteration caps of the GMRES cases: scipy's gmres with the numpy ILU(0) as right preconditioner needs at most half of them on these
# inputs (pc_checks asserts that as well)
CAP_PC, CAP_ADJOINT = 44, 60


def test_euler_pc_matrix(engine):
    pc.check_single(engine, (12, 9, 7), FlowParams(spaceDiscr=dissScalar), jm.EULER)


def test_rans_pc_matrix_forward_mode(engine):
    pc.check_single(engine, (12, 8, 6), pc.RANS, jm.WALL, stretch_k=2.0)


def test_frozen_turb_and_turb_only(engine):
    rm = pc.RANS.replace(limiter=minmod)
    pc.check_single(engine, (10, 7, 6), rm, jm.WALL, frozenTurb=True, stretch_k=2.0)       # nState = 5
    pc.check_single(engine, (10, 7, 6), rm, jm.WALL, useTurbOnly=True, stretch_k=2.0)      # nState = 1


def test_blocks_are_subdomains_periodic_brick(engine):
    """2 x 2 x 1 blocks of 9 x 8 x 6, periodic: the interfaces carry couplings in the matrix and none in M"""
    pc.check_brick(engine, BrickTopology(2, 2, 1, 9, 8, 6), FlowParams(spaceDiscr=dissScalar))


def test_blocks_are_subdomains_rotated_interfaces(engine):
    """four blocks of different sizes (adflow_amd.topology.ell_topology): hyperplanes of different lengths in one launch"""
    pc.check_brick(engine, ell_topology(), FlowParams(spaceDiscr=upwind), seed=251)


def test_tile_sized_block(engine):
    """RANS upwind preconditioner matrix by forward mode on 70 x 24 x 40: partial waves, 132 hyperplanes"""
    pc.check_single(engine, (70, 24, 40), pc.RANS, jm.WALL, stretch_k=2.0)
    assert engine.pcInfo()[1] == 132
    engine.pcRelease()


def test_factor_persists_and_is_released(engine):
    pc.check_persistence(engine, (12, 8, 6))


def test_refusals_and_no_side_effects(engine):
    pc.check_refusals_and_side_effects(engine)


def test_gmres_on_the_pc_matrix(engine):
    pc.check_gmres_on_pc_matrix(engine, (12, 8, 6), CAP_PC, restart=CAP_PC)


def test_gmres_adjoint_order_against_reference_solve(engine):
    pc.check_gmres_adjoint_order(engine, (8, 7, 6), CAP_ADJOINT)


def test_dev_forms_return_what_the_host_forms_return(engine, request):
    """pc_apply_dev (four blocks of unequal size) and gmres_solve_dev (7 x 5 x 4 with the cap of that shape) on torch tensors against
    their host twins, bit for bit"""
    from device_vectors import device_vectors
    pc.check_dev_twins(engine, device_vectors(request.config), ell_topology(), (7, 5, 4), 32)
