"""Derivatives of the surface integration on the MI355X: adflow_gpu_wall_integrate_fwd and adflow_gpu_wall_integrate_bwd against the
reference chain differentiated numerically (tests/wall_deriv_checks.py).  tests/test_hostsim_wall_deriv.py holds one twin per test."""
import pytest

import wall_deriv_checks as wd
from device_vectors import device_vectors

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", wd.FORWARD)
def test_forward_against_the_reference(engine, name):
    wd.check_forward(engine, name)


@pytest.mark.parametrize("name", wd.TRANSPOSE)
def test_transpose_against_the_reference_and_identity(engine, name):
    wd.check_transpose(engine, name)


@pytest.mark.parametrize("name,flags", wd.FLAGGED, ids=["frozen-turb"])
def test_state_ranges(engine, name, flags):
    wd.check_forward(engine, name, **flags)
    wd.check_transpose(engine, name, **flags)


@pytest.mark.parametrize("name", wd.COLOURING)
def test_colouring_is_valid(engine, name):
    wd.check_colouring(engine, name)


def test_turbulence_alone_has_a_zero_derivative(engine):
    wd.check_turb_only(engine)


def test_several_weight_sets(engine):
    wd.check_multi(engine)


def test_nothing_moves(engine, request):
    wd.check_nothing_moves(engine, device_vectors(request.config))


def test_refusals(engine):
    wd.check_refusals(engine)
