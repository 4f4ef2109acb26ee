"""CPU-only twin of tests/test_gpu_pc_its.py: the kernels of adflow_amd/csrc/kernels_pc_rich.hip and the nesting of pc_apply_enqueue
compiled with g++ (tests/hostsim) on the same cases at the same sizes, against the yardsticks of tests/pc_its_checks.py."""
import pytest

import pc_its_checks as pi
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")


def test_single_block(hostsim_engine):
    pi.check_single(hostsim_engine)


@pytest.mark.parametrize("fill", (0, 1))
def test_periodic_brick_block_local(hostsim_engine, fill):
    pi.check_brick(hostsim_engine, fill)


def test_rotated_interfaces(hostsim_engine):
    pi.check_rotated(hostsim_engine)


def test_period_of_three_cells(hostsim_engine):
    pi.check_period_of_three(hostsim_engine)


def test_level_fill_table_reuse_redoes_the_copy(hostsim_engine):
    pi.check_level_table_reuse(hostsim_engine)


def test_wall_brick_level_fill_2_outer_3_and_gmres(hostsim_engine):
    pi.check_wall_brick(hostsim_engine)


def test_wall_brick_ank_pc_setup(hostsim_engine):
    pi.check_wall_brick_ank(hostsim_engine)


@pytest.mark.parametrize("brick", (False, True))
def test_hierarchy(hostsim_engine, brick):
    pi.check_hierarchy(hostsim_engine, brick)


def test_several_columns(hostsim_engine):
    pi.check_multi(hostsim_engine)


def test_defaults_are_bit_identical(hostsim_engine):
    pi.check_defaults(hostsim_engine)


def test_slots_and_persistence(hostsim_engine):
    pi.check_slots_and_persistence(hostsim_engine)


def test_enqueue_only_chain(hostsim_engine):
    from device_vectors import HostVectors
    pi.check_enqueue_only_chain(hostsim_engine, HostVectors())


def test_refusals(hostsim_engine):
    pi.check_refusals(hostsim_engine)
