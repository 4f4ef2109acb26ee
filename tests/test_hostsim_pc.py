"""CPU-only twin of tests/test_gpu_pc.py: the kernels of adflow_amd/csrc/kernels_pc.hip compiled with g++ (tests/hostsim) on small
cases, against the general numpy ILU(0) of tests/pc_checks.py.  The 70 x 24 x 40 block runs on the GPU only."""
import pytest

import jacmult_checks as jm
import pc_checks as pc
from adflow_amd.params import FlowParams, dissScalar, upwind, minmod
from adflow_amd.topology import BrickTopology, ell_topology
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")

# iteration caps of the GMRES cases: scipy's gmres with the numpy ILU(0) as right preconditioner needs at most half of them on these
# inputs (pc_checks asserts that as well)
CAP_PC, CAP_ADJOINT = 32, 50


def test_euler_pc_matrix(hostsim_engine):
    pc.check_single(hostsim_engine, (7, 6, 5), FlowParams(spaceDiscr=dissScalar), jm.EULER)


def test_rans_pc_matrix_forward_mode(hostsim_engine):
    pc.check_single(hostsim_engine, (7, 5, 4), pc.RANS, jm.WALL, stretch_k=2.0)


def test_frozen_turb_and_turb_only(hostsim_engine):
    rm = pc.RANS.replace(limiter=minmod)
    pc.check_single(hostsim_engine, (7, 5, 4), rm, jm.WALL, frozenTurb=True, stretch_k=2.0)       # nState = 5
    pc.check_single(hostsim_engine, (7, 5, 4), rm, jm.WALL, useTurbOnly=True, stretch_k=2.0)      # nState = 1


def test_blocks_are_subdomains_periodic_brick(hostsim_engine):
    pc.check_brick(hostsim_engine, BrickTopology(2, 2, 1, 6, 5, 4), FlowParams(spaceDiscr=dissScalar))


def test_blocks_are_subdomains_rotated_interfaces(hostsim_engine):
    pc.check_brick(hostsim_engine, ell_topology(), FlowParams(spaceDiscr=upwind), seed=251)


def test_factor_persists_and_is_released(hostsim_engine):
    pc.check_persistence(hostsim_engine)


def test_refusals_and_no_side_effects(hostsim_engine):
    pc.check_refusals_and_side_effects(hostsim_engine)


def test_gmres_on_the_pc_matrix(hostsim_engine):
    pc.check_gmres_on_pc_matrix(hostsim_engine, (7, 5, 4), CAP_PC, restart=CAP_PC)


def test_gmres_adjoint_order_against_reference_solve(hostsim_engine):
    pc.check_gmres_adjoint_order(hostsim_engine, (7, 5, 4), CAP_ADJOINT)


def test_dev_forms_return_what_the_host_forms_return(hostsim_engine):
    from device_vectors import HostVectors
    pc.check_dev_twins(hostsim_engine, HostVectors(), ell_topology(), (7, 5, 4), CAP_PC)
