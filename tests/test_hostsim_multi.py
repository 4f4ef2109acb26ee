"""CPU-only twin of tests/test_gpu_multi.py: the multi-vector kernels of adflow_amd/csrc compiled with g++ (tests/hostsim) on small
cases, against the numpy yardsticks of tests/multi_checks.py.  The 70 x 24 x 40 block runs on the GPU only.

The cases are those of tests/test_gpu_multi.py -- the same matrices, stencils, nState, fills, widths, topologies and checks -- on the
SMALLER shapes tests/test_hostsim_pc.py and test_hostsim_pc_fill.py use for the same matrices (7 x 5 x 4 / 7 x 6 x 5 blocks, a brick
of 6 x 5 x 4), not on the shapes of the GPU file: the emulator spends its time in the forward-mode assembly, which every case
starts with (about 2.4 s for one 12 x 8 x 6 RANS block, and the three longest tests here already take 40 to 60 s each on 8 cores
with these shapes).  ell_topology() is the same on both sides."""
import pytest

import multi_checks as mc
from adflow_amd.topology import BrickTopology, ell_topology
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")

# iteration caps: those of tests/test_hostsim_pc.py for the same shapes
CAP_PC, CAP_ADJOINT = 32, 50


def test_products(hostsim_engine):
    mc.check_product_cases(hostsim_engine, (7, 6, 5), (7, 6, 5), (7, 5, 4), BrickTopology(2, 2, 1, 6, 5, 4), ell_topology())


def test_sweeps_every_fill_and_nstate(hostsim_engine):
    mc.check_sweep_cases(hostsim_engine, (7, 5, 4), (7, 5, 4))


def test_sweeps_blocks_of_unequal_size_stay_subdomains(hostsim_engine):
    mc.check_sweeps_rotated_interfaces(hostsim_engine, ell_topology())


def test_factor_slots(hostsim_engine):
    mc.check_factor_slots(hostsim_engine, (7, 5, 4))


def test_ank_factor(hostsim_engine):
    mc.check_ank_factor(hostsim_engine)


def test_one_column_is_the_single_entry_and_columns_are_independent(hostsim_engine):
    mc.check_one_column_and_independence(hostsim_engine, (7, 5, 4), CAP_PC)


def test_gmres_columns_on_the_pc_matrix(hostsim_engine):
    mc.check_gmres_on_pc_matrix(hostsim_engine, (7, 5, 4), CAP_PC)


def test_gmres_columns_in_the_adjoint_order(hostsim_engine):
    mc.check_gmres_adjoint_order(hostsim_engine, (7, 5, 4), CAP_ADJOINT)


def test_refusals_and_no_side_effects(hostsim_engine):
    mc.check_refusals_and_side_effects(hostsim_engine)


def test_dev_forms_and_enqueue_only_mode(hostsim_engine):
    from device_vectors import HostVectors
    mc.check_dev_twins_and_async(hostsim_engine, HostVectors(), ell_topology(), (7, 5, 4), CAP_PC)
