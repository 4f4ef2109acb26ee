"""CPU-only twin of tests/test_gpu_pc_fill.py: the kernels of adflow_amd/csrc/kernels_pc_fill.hip compiled with g++ (tests/hostsim)
on the same cases, against the general numpy ILU(k) of tests/pc_fill_checks.py."""
import pytest

import jacmult_checks as jm
import pc_checks as pc
import pc_fill_checks as pcf
from adflow_amd.params import FlowParams, upwind
from adflow_amd.topology import ell_topology
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")

# iteration cap of the GMRES case: scipy's gmres with the numpy ILU(k) as right preconditioner needs at most half of it on this
# input at either fill (pc_fill_checks asserts that as well); the cap of the fill-0 case of tests/test_gpu_pc.py
CAP_PC = 44

def test_euler_pc_matrix_all_offsets(hostsim_engine):
    """scalar-JST Euler on 7 x 6 x 5, nState 5: every offset of both stencils occurs, present and cut at a face"""
    pcf.check_single(hostsim_engine, (7, 6, 5), pcf.EULER_JST, jm.EULER, expect={1: (1, 13, 29), 2: (2, 23, 50)}, all_offsets=True)


def test_rans_pc_matrix_forward_mode(hostsim_engine):
    pcf.check_single(hostsim_engine, (7, 6, 5), pc.RANS, jm.WALL, stretch_k=2.0)                        # nState = 6


def test_frozen_turb(hostsim_engine):
    pcf.check_single(hostsim_engine, (7, 6, 5), pc.RANS, jm.WALL, frozenTurb=True, stretch_k=2.0)       # nState = 5


def test_turb_only(hostsim_engine):
    pcf.check_single(hostsim_engine, (7, 6, 5), pc.RANS, jm.WALL, useTurbOnly=True, stretch_k=2.0)      # nState = 1


@pytest.mark.parametrize("dims", [(5, 4, 2), (6, 1, 5)])
def test_thin_blocks(hostsim_engine, dims):
    """two-step offsets are cut everywhere; level sets of 1 to 5 cells"""
    pcf.check_single(hostsim_engine, dims, pcf.EULER_JST, jm.EULER)


def test_blocks_of_different_sizes(hostsim_engine):
    pcf.check_brick(hostsim_engine, ell_topology(), FlowParams(spaceDiscr=upwind))


def test_level_sets_wider_than_a_workgroup(hostsim_engine):
    """64 x 12 x 10, nState 1: the largest level set has 120 cells at fill 1 and 99 at fill 2"""
    pcf.check_largest_sets(hostsim_engine, (64, 12, 10), {1: 120, 2: 99})


def test_ank_factors_both_slots(hostsim_engine):
    pcf.check_ank(hostsim_engine)


def test_gmres_on_the_pc_matrix(hostsim_engine):
    pcf.check_gmres(hostsim_engine, (12, 8, 6), CAP_PC, scipy_fill_order=True)


def test_refusals_and_fill0_bit_identity(hostsim_engine):
    pcf.check_refusals_and_fill0_identity(hostsim_engine)


def test_dev_form_returns_what_the_host_form_returns(hostsim_engine):
    from device_vectors import HostVectors
    pcf.check_dev_twin(hostsim_engine, HostVectors(), ell_topology())
