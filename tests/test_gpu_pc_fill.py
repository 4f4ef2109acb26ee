"""GPU parity (real MI355X, through the C-ABI): the block ILU(1) / ILU(2) of the 7-point preconditioner matrix in the natural
ordering (adflow_gpu_pc_set_fill, adflow_gpu_pc_info2; PCFactorSetLevels of setupStandardKSP, adjointUtils.F90:1559), and everything
that takes a factor on top of one: pc_apply, gmres_solve, ank_pc_setup, the two slots.  Against a general symbolic ILU(k) and a
pattern-restricted IKJ factorisation in numpy on the library's downloaded blocks, in float64 and longdouble
(tests/pc_fill_checks.py): the library may be at most 10 x as far from the longdouble result as the float64 numpy run is."""
import pytest

import jacmult_checks as jm
import pc_checks as pc
import pc_fill_checks as pcf
from adflow_amd.params import FlowParams, upwind
from adflow_amd.topology import ell_topology

pytestmark = pytest.mark.gpu

# iteration cap of the GMRES case: scipy's gmres with the numpy ILU(k) as right preconditioner needs at most half of it on this
# input at either fill (pc_fill_checks asserts that as well); the cap of the fill-0 case of tests/test_gpu_pc.py
CAP_PC = 44

def test_euler_pc_matrix_all_offsets(engine):
    """scalar-JST Euler on 7 x 6 x 5, nState 5: every offset of both stencils occurs, present and cut at a face"""
    pcf.check_single(engine, (7, 6, 5), pcf.EULER_JST, jm.EULER, expect={1: (1, 13, 29), 2: (2, 23, 50)}, all_offsets=True)


def test_rans_pc_matrix_forward_mode(engine):
    pcf.check_single(engine, (7, 6, 5), pc.RANS, jm.WALL, stretch_k=2.0)                        # nState = 6


def test_frozen_turb(engine):
    pcf.check_single(engine, (7, 6, 5), pc.RANS, jm.WALL, frozenTurb=True, stretch_k=2.0)       # nState = 5


def test_turb_only(engine):
    pcf.check_single(engine, (7, 6, 5), pc.RANS, jm.WALL, useTurbOnly=True, stretch_k=2.0)      # nState = 1


@pytest.mark.parametrize("dims", [(5, 4, 2), (6, 1, 5)])
def test_thin_blocks(engine, dims):
    """two-step offsets are cut everywhere; level sets of 1 to 5 cells"""
    pcf.check_single(engine, dims, pcf.EULER_JST, jm.EULER)


def test_blocks_of_different_sizes(engine):
    pcf.check_brick(engine, ell_topology(), FlowParams(spaceDiscr=upwind))


def test_level_sets_wider_than_a_workgroup(engine):
    """64 x 12 x 10, nState 1: the largest level set has 120 cells at fill 1 and 99 at fill 2"""
    pcf.check_largest_sets(engine, (64, 12, 10), {1: 120, 2: 99})


def test_ank_factors_both_slots(engine):
    pcf.check_ank(engine)


def test_gmres_on_the_pc_matrix(engine):
    pcf.check_gmres(engine, (12, 8, 6), CAP_PC)


def test_refusals_and_fill0_bit_identity(engine):
    pcf.check_refusals_and_fill0_identity(engine)


def test_dev_form_returns_what_the_host_form_returns(engine, request):
    """pc_apply_dev at fill 2 on four blocks of unequal size, torch tensors, against pc_apply bit for bit"""
    from device_vectors import device_vectors
    pcf.check_dev_twin(engine, device_vectors(request.config), ell_topology())
