"""CPU-only: the surface integration (csrc/kernels_wallint.hip behind adflow_gpu_wall_integrate) on the kernel-logic emulator, one
twin per test of tests/test_gpu_wall_forces.py under the same bars, and the new entries in the header and the emulator library."""
import os
import re

import pytest

import wall_force_checks as wf
from device_vectors import HostVectors
from oracle import ref

needs_ref = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")
NEW = ["adflow_gpu_bc_set_families", "adflow_gpu_wall_integrate", "adflow_gpu_wall_integrate_dev", "adflow_gpu_download_wall_forces"]


def test_new_entries_are_declared_and_exported(hostsim_engine):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "adflow_gpu.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(hostsim_engine.lib, name), name
    for name, value in (("ADFLOW_WALLINT_NPAR", wf.capi.WALLINT_NPAR), ("ADFLOW_WALLINT_CPMIN_FAMILY", wf.capi.WALLINT_CPMIN_FAMILY)):
        assert re.search(r"\b%s = %d\b" % (name, value), txt), name
    assert re.search(r"#define ADFLOW_WALLINT_STRIDE %d\b" % wf.capi.WALLINT_STRIDE, txt)


@needs_ref
@pytest.mark.parametrize("fid", [1, 2, 3, 4, 5, 6])
def test_ns_wall_on_every_face(hostsim_engine, fid):
    wf.check_ns_face(hostsim_engine, fid)


@needs_ref
def test_rans_adiabatic_and_isothermal_yplus(hostsim_engine):
    wf.check_rans(hostsim_engine)


@needs_ref
def test_euler_walls_have_no_viscous_part(hostsim_engine):
    wf.check_euler(hostsim_engine)


@needs_ref
def test_more_than_one_workgroup_and_a_single_face(hostsim_engine):
    wf.check_sizes(hostsim_engine)


@needs_ref
def test_wall_split_in_two_subfaces(hostsim_engine):
    wf.check_split(hostsim_engine)


@needs_ref
def test_two_blocks_three_groups(hostsim_engine):
    wf.check_groups(hostsim_engine)


@needs_ref
def test_blanking(hostsim_engine):
    wf.check_blanking(hostsim_engine)


@needs_ref
@pytest.mark.parametrize("cavExponent", [0, 2])
def test_cavitation_in_two_calls(hostsim_engine, cavExponent):
    wf.check_cavitation(hostsim_engine, cavExponent)


@needs_ref
def test_reference_point_axis_lref_direction(hostsim_engine):
    wf.check_reference_point(hostsim_engine)


@needs_ref
def test_block_far_from_the_origin(hostsim_engine):
    wf.check_translated(hostsim_engine)


@needs_ref
@pytest.mark.parametrize("name", ["annulus", "sheared", "clustered", "pole"])
def test_mesh_families(hostsim_engine, name):
    wf.check_family(hostsim_engine, name)


@needs_ref
def test_determinism_and_enqueue_only(hostsim_engine):
    wf.check_determinism_and_async(hostsim_engine, HostVectors())


@needs_ref
def test_errors(hostsim_engine):
    wf.check_errors(hostsim_engine)
