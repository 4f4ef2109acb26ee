"""CPU-only: the derivatives of the surface integration (csrc/kernels_wallint.hip compiled for dual numbers behind
adflow_gpu_wall_integrate_fwd / _bwd) on the kernel-logic emulator, one twin per test of tests/test_gpu_wall_deriv.py under the same
bars, the new entries in the header and the emulator library, and the noise floor of the yardstick that the bar was taken from.  The
twins of the colouring test take every column (no cell is left out: share 0)."""
import os
import re

import pytest

import wall_deriv_checks as wd
from device_vectors import HostVectors
from oracle import ref

needs_ref = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")
NEW = ["adflow_gpu_wall_integrate_fwd", "adflow_gpu_wall_integrate_fwd_dev", "adflow_gpu_wall_integrate_bwd", "adflow_gpu_wall_integrate_bwd_dev"]


def test_new_entries_are_declared_and_exported(hostsim_engine):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "adflow_gpu.h")).read(), flags=re.S)
    shim = open(os.path.join(root, "adflow_amd", "fortran", "adflow_gpu_shim.F90")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(hostsim_engine.lib, name), name
    for name in ("gpuWallIntegrateFwd", "gpuWallIntegrateBwd", "adflow_gpu_wall_integrate_fwd_dev", "adflow_gpu_wall_integrate_bwd_dev"):
        assert name in shim, name


@needs_ref
def test_the_bar_is_ten_times_the_measured_floor(hostsim_engine):
    """FLOOR is the yardstick's noise as measured here, BAR ten times it, and the forward product holds the bar on the case whose
    yardstick is the noisiest"""
    worst, where = wd.measure_floor()
    assert wd.BAR == 10.0 * wd.FLOOR
    assert abs(worst - wd.FLOOR) <= 1e-3 * wd.FLOOR, ("FLOOR is not the measured floor", worst, wd.FLOOR)
    wd.check_forward(hostsim_engine, where)


@needs_ref
@pytest.mark.parametrize("name", wd.FORWARD)
def test_forward_against_the_reference(hostsim_engine, name):
    wd.check_forward(hostsim_engine, name)


@needs_ref
@pytest.mark.parametrize("name", wd.TRANSPOSE)
def test_transpose_against_the_reference_and_identity(hostsim_engine, name):
    wd.check_transpose(hostsim_engine, name)


@needs_ref
@pytest.mark.parametrize("name,flags", wd.FLAGGED, ids=["frozen-turb"])
def test_state_ranges(hostsim_engine, name, flags):
    wd.check_forward(hostsim_engine, name, **flags)
    wd.check_transpose(hostsim_engine, name, **flags)


@needs_ref
@pytest.mark.parametrize("name", wd.COLOURING)
def test_colouring_is_valid(hostsim_engine, name):
    wd.check_colouring(hostsim_engine, name)


@needs_ref
def test_turbulence_alone_has_a_zero_derivative(hostsim_engine):
    wd.check_turb_only(hostsim_engine)


@needs_ref
def test_several_weight_sets(hostsim_engine):
    wd.check_multi(hostsim_engine)


@needs_ref
def test_nothing_moves(hostsim_engine):
    wd.check_nothing_moves(hostsim_engine, HostVectors())


@needs_ref
def test_refusals(hostsim_engine):
    wd.check_refusals(hostsim_engine)
