"""CPU-only twin of tests/test_gpu_pc_order.py: the kernels of adflow_amd/csrc/kernels_pc_level.hip and the host tables of api.hip
compiled with g++ (tests/hostsim) on the same cases, against the relabelled numpy ILU(k) of tests/pc_order_checks.py."""
import pytest

import pc_order_checks as po
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")


def test_rcm_periodic_brick(hostsim_engine):
    po.check_rcm_periodic_brick(hostsim_engine)


def test_random_permutation(hostsim_engine):
    po.check_random_permutation(hostsim_engine)


def test_red_black(hostsim_engine):
    po.check_red_black(hostsim_engine)


def test_rcm_rotated_interfaces(hostsim_engine):
    po.check_rcm_rotated(hostsim_engine)


def test_rcm_period_of_three_cells(hostsim_engine):
    po.check_rcm_period_of_three(hostsim_engine)


def test_rcm_wall_brick_gmres(hostsim_engine):
    po.check_wall_brick_gmres(hostsim_engine)


def test_rcm_ank_pc_setup(hostsim_engine):
    po.check_wall_brick_ank(hostsim_engine)


def test_bit_identity(hostsim_engine):
    po.check_bit_identity(hostsim_engine)


def test_refusals(hostsim_engine):
    po.check_refusals(hostsim_engine)


def test_isolation(hostsim_engine):
    po.check_isolation(hostsim_engine)


def test_table_reuse(hostsim_engine):
    po.check_table_reuse(hostsim_engine)


def test_several_columns_iterations_and_bytes(hostsim_engine):
    po.check_multi_its_and_bytes(hostsim_engine)


def test_enqueue_only_chain(hostsim_engine):
    from device_vectors import HostVectors
    po.check_enqueue_only_chain(hostsim_engine, HostVectors())
