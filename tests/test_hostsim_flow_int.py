"""CPU-only: the flow integration and its derivatives (the flow kernels of csrc/kernels_wallint.hip behind adflow_gpu_flow_integrate,
_fwd and _bwd) on the kernel-logic emulator, one twin per test of tests/test_gpu_flow_int.py under the same bars, the new entries in
the header, the bindings and the shim, and the noise floor of the yardstick that the bar of the derivatives was taken from."""
import os
import re

import pytest

import flow_int_checks as fc
from device_vectors import HostVectors
from oracle import ref

needs_ref = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")
NEW = ["adflow_gpu_flow_integrate", "adflow_gpu_flow_integrate_dev", "adflow_gpu_flow_integrate_fwd", "adflow_gpu_flow_integrate_fwd_dev",
       "adflow_gpu_flow_integrate_bwd", "adflow_gpu_flow_integrate_bwd_dev"]


def test_new_entries_are_declared_and_exported(hostsim_engine):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    full = open(os.path.join(root, "include", "adflow_gpu.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    shim = open(os.path.join(root, "adflow_amd", "fortran", "adflow_gpu_shim.F90")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(hostsim_engine.lib, name) and name in fc.capi.EXPORTS, name
    for name in ("gpuFlowIntegrate", "gpuFlowIntegrateFwd", "gpuFlowIntegrateBwd", "adflow_gpu_flow_integrate_dev",
                 "adflow_gpu_flow_integrate_fwd_dev", "adflow_gpu_flow_integrate_bwd_dev"):
        assert name in shim, name
    for name in ("POINTREF", "INTERNALFLOW", "RHOREF", "RGASDIM", "NPAR"):
        assert re.search(r"\bADFLOW_FLOWINT_%s = %d\b" % (name, getattr(fc.capi, "FLOWINT_" + name)), txt), name
    for lst in re.findall(r"Not here[^:]*:(.*?)(?:\*/|\n \*\n)", full, flags=re.S):
        assert "flowIntegrationFace" not in lst


@needs_ref
def test_the_bar_is_ten_times_the_measured_floor(hostsim_engine):
    """FLOOR is the yardstick's noise as measured here, BAR ten times it, and the forward product holds the bar on the case whose
    yardstick is the noisiest"""
    worst, where = fc.measure_floor()
    assert fc.BAR == 10.0 * fc.FLOOR
    assert abs(worst - fc.FLOOR) <= 1e-3 * fc.FLOOR, ("FLOOR is not the measured floor", worst, fc.FLOOR)
    fc.check_forward(hostsim_engine, where)


@needs_ref
@pytest.mark.parametrize("d", [0, 1, 2], ids=["i", "j", "k"])
def test_subsonic_in_and_outflow_in_every_direction(hostsim_engine, d):
    fc.check_direction(hostsim_engine, d)


@needs_ref
def test_supersonic_in_and_outflow(hostsim_engine):
    fc.check_supersonic(hostsim_engine)


@needs_ref
def test_rans(hostsim_engine):
    fc.check_rans(hostsim_engine)


@needs_ref
def test_two_workgroups_per_subface(hostsim_engine):
    fc.check_sizes(hostsim_engine)


@needs_ref
def test_split_face_and_three_groups(hostsim_engine):
    fc.check_split_and_groups(hostsim_engine)


@needs_ref
def test_blanking(hostsim_engine):
    fc.check_blanking(hostsim_engine)


@needs_ref
def test_internal_flow_flag(hostsim_engine):
    fc.check_internal_flow(hostsim_engine)


@needs_ref
def test_moving_block(hostsim_engine):
    fc.check_moving(hostsim_engine)
    fc.check_moving_is_refused_by_the_derivatives(hostsim_engine)


@needs_ref
def test_brick_of_eight_blocks(hostsim_engine):
    fc.check_brick(hostsim_engine)


@needs_ref
def test_determinism_and_enqueue_only(hostsim_engine):
    fc.check_determinism_and_async(hostsim_engine, HostVectors())


@needs_ref
def test_wall_plus_flow_is_integrate_surfaces(hostsim_engine):
    fc.check_wall_plus_flow(hostsim_engine)


@needs_ref
def test_errors(hostsim_engine):
    fc.check_errors(hostsim_engine)


@needs_ref
@pytest.mark.parametrize("name", fc.FORWARD)
def test_forward_against_the_reference(hostsim_engine, name):
    fc.check_forward(hostsim_engine, name)


@needs_ref
@pytest.mark.parametrize("name", fc.TRANSPOSE)
def test_transpose_against_the_reference_and_identity(hostsim_engine, name):
    fc.check_transpose(hostsim_engine, name)


@needs_ref
@pytest.mark.parametrize("name,flags", fc.FLAGGED, ids=["frozen-turb"])
def test_state_ranges(hostsim_engine, name, flags):
    fc.check_forward(hostsim_engine, name, **flags)
    fc.check_transpose(hostsim_engine, name, **flags)


@needs_ref
def test_turbulence_alone_has_a_zero_derivative(hostsim_engine):
    fc.check_turb_only(hostsim_engine)


@needs_ref
@pytest.mark.parametrize("name", fc.COLOURING)
def test_colouring_is_valid(hostsim_engine, name):
    fc.check_colouring(hostsim_engine, name)


@needs_ref
def test_four_weight_sets(hostsim_engine):
    fc.check_multi(hostsim_engine)


@needs_ref
def test_chained_and_nothing_moves(hostsim_engine):
    fc.check_chained(hostsim_engine, HostVectors())
