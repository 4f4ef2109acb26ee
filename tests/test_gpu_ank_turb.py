"""The turbulence half of the approximate Newton-Krylov step on a real MI355X: approxSA, the turbulence KSP (ADFLOW_ANK_TURB), the
line-search residual and the two factor slots, against the yardsticks of tests/ank_turb_checks.py."""
import pytest

import ank_turb_checks as tc
from adflow_amd.topology import ell_topology
from oracle import ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")]

DIMS = (12, 8, 6)
BIG = (70, 24, 40)          # partial waves, more than one reduction workgroup
# iteration cap of the solve: scipy's gmres with the shifted numpy ILU(0) as right preconditioner needs at most half of it on this
# input (ank_turb_checks.check_solve asserts that as well)
CAP = 8


def test_approx_sa_residual(engine):
    tc.check_approx_sa_residual(engine, DIMS)


def test_turb_first_order_flag(engine):
    tc.check_turb_first_order(engine, DIMS)


def test_approx_sa_assembly(engine):
    tc.check_approx_sa_assembly(engine)


def test_turbulence_T_and_shifted_factor(engine):
    tc.check_shifted_factor(engine, DIMS)


def test_turbulence_operator(engine):
    tc.check_operator(engine, DIMS, False, edge_cases=True)


def test_turbulence_operator_approx_sa(engine):
    tc.check_operator(engine, DIMS, True)


def test_turbulence_solve(engine):
    tc.check_solve(engine, DIMS, CAP)


def test_physicality_check_turb(engine):
    tc.check_physicality(engine, ell_topology())


@pytest.mark.parametrize("kind", ["flow", "coupled", "turb"])
def test_unsteady_residual(engine, kind):
    tc.check_unsteady(engine, DIMS, kind)


def test_factor_slots(engine):
    tc.check_slots(engine, DIMS)


def test_refusals_and_no_side_effects(engine):
    tc.check_refusals_and_side_effects(engine)


@pytest.mark.parametrize("kind", ["flow", "turb"])
def test_unsteady_residual_several_reduction_workgroups(engine, kind):
    tc.check_unsteady(engine, BIG, kind)
    engine.releaseWorkspace()


def test_dev_forms_return_what_the_host_forms_return(engine, request):
    """the _dev entries of the turbulence kind (nState 1) on torch tensors against their host twins, bit for bit"""
    from device_vectors import device_vectors
    tc.check_dev_twins(engine, device_vectors(request.config), (7, 6, 5), CAP)
