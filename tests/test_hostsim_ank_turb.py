"""CPU-only twin of tests/test_gpu_ank_turb.py: the turbulence kernels of adflow_amd/csrc/kernels_ank.hip, the approxSA select of the SA
source and the NS = 1 shift of k_pc_factor compiled with g++ (tests/hostsim) at (7, 5, 4), against the yardsticks of
tests/ank_turb_checks.py.  The 70 x 24 x 40 block runs on the GPU only."""
import pytest

import ank_turb_checks as tc
from adflow_amd.topology import ell_topology
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")

DIMS = (7, 5, 4)
# iteration cap of the solve: scipy's gmres with the shifted numpy ILU(0) as right preconditioner needs at most half of it on this
# input (ank_turb_checks.check_solve asserts that as well)
CAP = 8


def test_approx_sa_residual(hostsim_engine):
    tc.check_approx_sa_residual(hostsim_engine, DIMS)


def test_turb_first_order_flag(hostsim_engine):
    tc.check_turb_first_order(hostsim_engine, DIMS)


def test_approx_sa_assembly(hostsim_engine):
    tc.check_approx_sa_assembly(hostsim_engine)


def test_turbulence_T_and_shifted_factor(hostsim_engine):
    tc.check_shifted_factor(hostsim_engine, DIMS)


def test_turbulence_operator(hostsim_engine):
    tc.check_operator(hostsim_engine, DIMS, False, edge_cases=True)


def test_turbulence_operator_approx_sa(hostsim_engine):
    tc.check_operator(hostsim_engine, DIMS, True)


def test_turbulence_solve(hostsim_engine):
    tc.check_solve(hostsim_engine, DIMS, CAP)


def test_physicality_check_turb(hostsim_engine):
    tc.check_physicality(hostsim_engine, ell_topology())


@pytest.mark.parametrize("kind", ["flow", "coupled", "turb"])
def test_unsteady_residual(hostsim_engine, kind):
    tc.check_unsteady(hostsim_engine, DIMS, kind)


def test_factor_slots(hostsim_engine):
    tc.check_slots(hostsim_engine, DIMS)


def test_refusals_and_no_side_effects(hostsim_engine):
    tc.check_refusals_and_side_effects(hostsim_engine)


def test_dev_forms_return_what_the_host_forms_return(hostsim_engine):
    from device_vectors import HostVectors
    tc.check_dev_twins(hostsim_engine, HostVectors(), (7, 6, 5), CAP)
