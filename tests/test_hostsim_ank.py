"""CPU-only twin of tests/test_gpu_ank.py: the kernels of adflow_amd/csrc/kernels_ank.hip (and the shifted k_pc_factor) compiled with
g++ (tests/hostsim) on the small shapes of tests/test_hostsim_pc.py, against the yardsticks of tests/ank_checks.py.  The 70 x 24 x 40
block runs on the GPU only."""
import pytest

import ank_checks as ank
import jacmult_checks as jm
from adflow_amd.topology import ell_topology
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")

# iteration caps of the solves: scipy's gmres with the shifted numpy ILU(0) as right preconditioner needs at most half of them on
# these inputs (ank_checks asserts that as well)
CAP_EULER, CAP_RANS = 12, 16


def test_time_step_blocks_euler(hostsim_engine):
    ank.check_T_single(hostsim_engine, (7, 6, 5), ank.EULER_JST, jm.EULER, False)


def test_time_step_blocks_rans_decoupled(hostsim_engine):
    ank.check_T_single(hostsim_engine, (7, 5, 4), ank.RANS_UPWIND, jm.WALL, False, stretch_k=2.0)


def test_time_step_blocks_rans_coupled(hostsim_engine):
    ank.check_T_single(hostsim_engine, (7, 5, 4), ank.RANS_COUPLED, jm.WALL, True, stretch_k=2.0)


def test_shifted_factor_rans_decoupled(hostsim_engine):
    ank.check_shifted_single(hostsim_engine, (7, 5, 4))


def test_shifted_factor_rotated_interfaces(hostsim_engine):
    ank.check_shifted_ell(hostsim_engine, ell_topology())


def test_operator_exact_euler(hostsim_engine):
    ank.check_operator(hostsim_engine, (7, 6, 5), ank.EULER_JST, jm.EULER, False, False, edge_cases=True)


def test_operator_exact_rans_decoupled(hostsim_engine):
    ank.check_operator(hostsim_engine, (7, 5, 4), ank.RANS_UPWIND, jm.WALL, False, False, stretch_k=2.0)


def test_operator_approximate_euler(hostsim_engine):
    ank.check_operator(hostsim_engine, (7, 6, 5), ank.EULER_JST, ank.EULER_AD, False, True)


def test_operator_exact_euler_differentiated_faces(hostsim_engine):
    """every face of a kind the forward-mode assembly differentiates (ank_checks.EULER_AD): J v + T v is the derivative everywhere"""
    out = ank.check_operator(hostsim_engine, (7, 6, 5), ank.EULER_JST, ank.EULER_AD, False, False)
    assert out[2] <= 1e-5, out[2]


def test_operator_extrapolation_faces_match_the_reference_quotient(hostsim_engine):
    """jm.EULER has an extrapolation and a supersonic-outflow face, which no forward-mode matrix differentiates: the operator is of
    order one away from J v + T v next to them -- exactly as far as the reference's own difference quotient (the MARGIN rule holds)"""
    ank.check_operator(hostsim_engine, (7, 6, 5), ank.EULER_JST, jm.EULER, False, True)


def test_operator_approximate_rans_decoupled(hostsim_engine):
    ank.check_operator(hostsim_engine, (7, 5, 4), ank.RANS_JST, jm.WALL, False, True, stretch_k=2.0)


def test_operator_exact_rans_coupled(hostsim_engine):
    ank.check_operator(hostsim_engine, (7, 5, 4), ank.RANS_COUPLED, jm.WALL, True, False, stretch_k=2.0)


def test_solve_euler(hostsim_engine):
    ank.check_solve(hostsim_engine, (7, 6, 5), ank.EULER_JST, ank.EULER_AD, CAP_EULER)


def test_solve_rans_decoupled(hostsim_engine):
    ank.check_solve(hostsim_engine, (7, 5, 4), ank.RANS_JST, jm.WALL, CAP_RANS, stretch_k=2.0)


def test_physicality_check_decoupled(hostsim_engine):
    ank.check_physicality(hostsim_engine, ell_topology(), False)


def test_physicality_check_coupled(hostsim_engine):
    ank.check_physicality(hostsim_engine, ell_topology(), True)


def test_refusals_and_no_side_effects(hostsim_engine):
    ank.check_refusals_and_side_effects(hostsim_engine)


@pytest.mark.parametrize("kind", ["flow", "coupled"])
def test_dev_forms_return_what_the_host_forms_return(hostsim_engine, kind):
    from device_vectors import HostVectors
    ank.check_dev_twins(hostsim_engine, HostVectors(), (7, 6, 5), kind, CAP_RANS)


def test_nk_residual_dev_returns_what_the_host_form_returns(hostsim_engine):
    from device_vectors import HostVectors
    ank.check_nk_residual_dev_twin(hostsim_engine, HostVectors())
