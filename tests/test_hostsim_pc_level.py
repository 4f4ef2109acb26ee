"""CPU-only twin of tests/test_gpu_pc_level.py: the kernels of adflow_amd/csrc/kernels_pc_level.hip compiled with g++ (tests/hostsim)
on the same cases, the periodic brick at 6 x 5 x 4 throughout, against the numpy ILU(k) over the level of tests/pc_level_checks.py."""
import pytest

import pc_level_checks as pl
from adflow_amd.topology import BrickTopology
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")


def test_periodic_brick_fill_0_1(hostsim_engine):
    pl.check_periodic_brick(hostsim_engine, BrickTopology(2, 2, 1, 6, 5, 4), (0, 1))


def test_periodic_brick_fill_2_3(hostsim_engine):
    pl.check_periodic_brick(hostsim_engine, BrickTopology(2, 2, 1, 6, 5, 4), (2, 3))


def test_rotated_interfaces(hostsim_engine):
    pl.check_rotated(hostsim_engine)


def test_wall_brick_apply_and_gmres(hostsim_engine):
    pl.check_wall_brick_gmres(hostsim_engine)


def test_wall_brick_frozen_turb_and_turb_only(hostsim_engine):
    pl.check_wall_brick_apply(hostsim_engine, 1, frozenTurb=True)        # nState = 5
    pl.check_wall_brick_apply(hostsim_engine, 1, useTurbOnly=True)       # nState = 1


def test_wall_brick_ank_pc_setup(hostsim_engine):
    pl.check_wall_brick_ank(hostsim_engine)


def test_single_block(hostsim_engine):
    pl.check_single_block(hostsim_engine)


def test_single_block_fill_3(hostsim_engine):
    pl.check_single_block_fill3(hostsim_engine)


def test_period_of_three_cells(hostsim_engine):
    pl.check_period_of_three(hostsim_engine)


def test_refusals(hostsim_engine):
    pl.check_refusals(hostsim_engine)


def test_isolation(hostsim_engine):
    pl.check_isolation(hostsim_engine)


def test_several_columns_and_bytes(hostsim_engine):
    pl.check_multi_and_bytes(hostsim_engine)


def test_table_reuse(hostsim_engine):
    pl.check_table_reuse(hostsim_engine)


def test_enqueue_only_chain(hostsim_engine):
    from device_vectors import HostVectors
    pl.check_enqueue_only_chain(hostsim_engine, HostVectors())
