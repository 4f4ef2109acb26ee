"""Flow integration on the MI355X: adflow_gpu_flow_integrate against the numpy yardstick of flowIntegrationFace fed the reference's
fields, and adflow_gpu_flow_integrate_fwd / _bwd against the reference chain differentiated numerically (tests/flow_int_checks.py).
tests/test_hostsim_flow_int.py holds one twin per test."""
import pytest

import flow_int_checks as fc
from device_vectors import device_vectors

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d", [0, 1, 2], ids=["i", "j", "k"])
def test_subsonic_in_and_outflow_in_every_direction(engine, d):
    fc.check_direction(engine, d)


def test_supersonic_in_and_outflow(engine):
    fc.check_supersonic(engine)


def test_rans(engine):
    fc.check_rans(engine)


def test_two_workgroups_per_subface(engine):
    fc.check_sizes(engine)


def test_split_face_and_three_groups(engine):
    fc.check_split_and_groups(engine)


def test_blanking(engine):
    fc.check_blanking(engine)


def test_internal_flow_flag(engine):
    fc.check_internal_flow(engine)


def test_moving_block(engine):
    fc.check_moving(engine)
    fc.check_moving_is_refused_by_the_derivatives(engine)


def test_brick_of_eight_blocks(engine):
    fc.check_brick(engine)


def test_determinism_and_enqueue_only(engine, request):
    fc.check_determinism_and_async(engine, device_vectors(request.config))


def test_wall_plus_flow_is_integrate_surfaces(engine):
    fc.check_wall_plus_flow(engine)


def test_errors(engine):
    fc.check_errors(engine)


@pytest.mark.parametrize("name", fc.FORWARD)
def test_forward_against_the_reference(engine, name):
    fc.check_forward(engine, name)


@pytest.mark.parametrize("name", fc.TRANSPOSE)
def test_transpose_against_the_reference_and_identity(engine, name):
    fc.check_transpose(engine, name)


@pytest.mark.parametrize("name,flags", fc.FLAGGED, ids=["frozen-turb"])
def test_state_ranges(engine, name, flags):
    fc.check_forward(engine, name, **flags)
    fc.check_transpose(engine, name, **flags)


def test_turbulence_alone_has_a_zero_derivative(engine):
    fc.check_turb_only(engine)


@pytest.mark.parametrize("name", fc.COLOURING)
def test_colouring_is_valid(engine, name):
    fc.check_colouring(engine, name)


def test_four_weight_sets(engine):
    fc.check_multi(engine)


def test_chained_and_nothing_moves(engine, request):
    fc.check_chained(engine, device_vectors(request.config))
