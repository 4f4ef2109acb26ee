"""GPU parity (real MI355X, through the C-ABI): the flow update of the approximate Newton-Krylov step -- adflow_gpu_ank_time_step,
_ank_pc_setup, _ank_set_base / _ank_mult, _ank_solve, _ank_physicality_check -- against the yardsticks of tests/ank_checks.py: T from
its formulas in numpy, the shifted factor against the numpy ILU(0) of J + T, the operator against J v + T v next to the reference's
own difference quotient (oracle/_ref, blocketteResCore), the step limiter against a numpy restatement.  Shapes: those of
tests/test_gpu_pc.py; cfl = 5."""
import numpy as np
import pytest

import ank_checks as ank
import jacmult_checks as jm
from adflow_amd.topology import ell_topology

pytestmark = pytest.mark.gpu

# iteration caps of the solves: scipy's gmres with the shifted numpy ILU(0) as right preconditioner needs at most half of them on
# these inputs (ank_checks asserts that as well)
CAP_EULER, CAP_RANS = 12, 16


def test_time_step_blocks_euler(engine):
    ank.check_T_single(engine, (12, 9, 7), ank.EULER_JST, jm.EULER, False)


def test_time_step_blocks_rans_decoupled(engine):
    ank.check_T_single(engine, (12, 8, 6), ank.RANS_UPWIND, jm.WALL, False, stretch_k=2.0)


def test_time_step_blocks_rans_coupled(engine):
    ank.check_T_single(engine, (12, 8, 6), ank.RANS_COUPLED, jm.WALL, True, stretch_k=2.0)


def test_shifted_factor_rans_decoupled(engine):
    ank.check_shifted_single(engine, (12, 8, 6))


def test_shifted_factor_rotated_interfaces(engine):
    ank.check_shifted_ell(engine, ell_topology())


def test_operator_exact_euler(engine):
    ank.check_operator(engine, (12, 9, 7), ank.EULER_JST, jm.EULER, False, False, edge_cases=True)


def test_operator_exact_rans_decoupled(engine):
    ank.check_operator(engine, (12, 8, 6), ank.RANS_UPWIND, jm.WALL, False, False, stretch_k=2.0)


def test_operator_approximate_euler(engine):
    ank.check_operator(engine, (12, 9, 7), ank.EULER_JST, ank.EULER_AD, False, True)


def test_operator_exact_euler_differentiated_faces(engine):
    """every face of a kind the forward-mode assembly differentiates (ank_checks.EULER_AD): J v + T v is the derivative everywhere"""
    out = ank.check_operator(engine, (12, 9, 7), ank.EULER_JST, ank.EULER_AD, False, False)
    assert out[2] <= 1e-5, out[2]


def test_operator_extrapolation_faces_match_the_reference_quotient(engine):
    """jm.EULER has an extrapolation and a supersonic-outflow face, which no forward-mode matrix differentiates: the operator is of
    order one away from J v + T v next to them -- exactly as far as the reference's own difference quotient (the MARGIN rule holds)"""
    ank.check_operator(engine, (12, 9, 7), ank.EULER_JST, jm.EULER, False, True)


def test_operator_approximate_rans_decoupled(engine):
    ank.check_operator(engine, (12, 8, 6), ank.RANS_JST, jm.WALL, False, True, stretch_k=2.0)


def test_operator_exact_rans_coupled(engine):
    ank.check_operator(engine, (12, 8, 6), ank.RANS_COUPLED, jm.WALL, True, False, stretch_k=2.0)


def test_solve_euler(engine):
    ank.check_solve(engine, (12, 9, 7), ank.EULER_JST, ank.EULER_AD, CAP_EULER)


def test_solve_rans_decoupled(engine):
    ank.check_solve(engine, (12, 8, 6), ank.RANS_JST, jm.WALL, CAP_RANS, stretch_k=2.0)


def test_physicality_check_decoupled(engine):
    ank.check_physicality(engine, ell_topology(), False)


def test_physicality_check_coupled(engine):
    ank.check_physicality(engine, ell_topology(), True)


def test_refusals_and_no_side_effects(engine):
    ank.check_refusals_and_side_effects(engine)


def test_tile_sized_block(engine):
    """RANS decoupled on 70 x 24 x 40: partial waves at size.  The exact operator against J v + T v (the 33-point forward-mode
    blocks), and a 5-iteration solve on the factor's 132 hyperplanes"""
    ank.check_tile_sized(engine, (70, 24, 40))


@pytest.mark.parametrize("kind", ["flow", "coupled"])
def test_dev_forms_return_what_the_host_forms_return(engine, request, kind):
    """every adflow_gpu_ank_*_dev entry on torch tensors against its host twin, bit for bit: nState 5 and 6"""
    from device_vectors import device_vectors
    ank.check_dev_twins(engine, device_vectors(request.config), (7, 6, 5), kind, CAP_RANS)


def test_nk_residual_dev_returns_what_the_host_form_returns(engine, request):
    from device_vectors import device_vectors
    ank.check_nk_residual_dev_twin(engine, device_vectors(request.config))
