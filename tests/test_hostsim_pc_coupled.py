"""CPU-only twin of tests/test_gpu_pc_coupled.py: the kernels of adflow_amd/csrc/kernels_pc_coupled.hip compiled with g++
(tests/hostsim) on the same cases, the periodic brick at 6 x 5 x 4, against the numpy ILU(0) over the level of
tests/pc_coupled_checks.py."""
import pytest

import pc_coupled_checks as pcc
from adflow_amd.topology import BrickTopology
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")


def test_periodic_brick(hostsim_engine):
    pcc.check_periodic_brick(hostsim_engine, BrickTopology(2, 2, 1, 6, 5, 4))


def test_rotated_interfaces(hostsim_engine):
    pcc.check_rotated(hostsim_engine)


def test_wall_brick_apply_and_gmres(hostsim_engine):
    pcc.check_wall_brick_gmres(hostsim_engine)


def test_wall_brick_frozen_turb_and_turb_only(hostsim_engine):
    pcc.check_wall_brick_apply(hostsim_engine, frozenTurb=True)        # nState = 5
    pcc.check_wall_brick_apply(hostsim_engine, useTurbOnly=True)       # nState = 1


def test_wall_brick_ank_pc_setup(hostsim_engine):
    pcc.check_wall_brick_ank(hostsim_engine)


def test_equivalence_and_isolation(hostsim_engine):
    pcc.check_equivalence_and_isolation(hostsim_engine)


def test_refusals(hostsim_engine):
    pcc.check_refusals(hostsim_engine)


def test_enqueue_only_chain(hostsim_engine):
    from device_vectors import HostVectors
    pcc.check_enqueue_only_chain(hostsim_engine, HostVectors())
