"""Surface integration on the MI355X: adflow_gpu_wall_integrate and the per-face arrays against the numpy yardstick of
tests/wall_force_checks.py on the reference's own fields.  tests/test_hostsim_wall_forces.py holds one twin per test."""
import pytest

import wall_force_checks as wf
from device_vectors import device_vectors

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fid", [1, 2, 3, 4, 5, 6])
def test_ns_wall_on_every_face(engine, fid):
    wf.check_ns_face(engine, fid)


def test_rans_adiabatic_and_isothermal_yplus(engine):
    wf.check_rans(engine)


def test_euler_walls_have_no_viscous_part(engine):
    wf.check_euler(engine)


def test_more_than_one_workgroup_and_a_single_face(engine):
    wf.check_sizes(engine)


def test_wall_split_in_two_subfaces(engine):
    wf.check_split(engine)


def test_two_blocks_three_groups(engine):
    wf.check_groups(engine)


def test_blanking(engine):
    wf.check_blanking(engine)


@pytest.mark.parametrize("cavExponent", [0, 2])
def test_cavitation_in_two_calls(engine, cavExponent):
    wf.check_cavitation(engine, cavExponent)


def test_reference_point_axis_lref_direction(engine):
    wf.check_reference_point(engine)


def test_block_far_from_the_origin(engine):
    wf.check_translated(engine)


@pytest.mark.parametrize("name", ["annulus", "sheared", "clustered", "pole"])
def test_mesh_families(engine, name):
    wf.check_family(engine, name)


def test_determinism_and_enqueue_only(engine, request):
    wf.check_determinism_and_async(engine, device_vectors(request.config))


def test_errors(engine):
    wf.check_errors(engine)
