"""GPU parity (real MI355X, through the C-ABI) of the multi-vector entries adflow_gpu_jacobian_mult_multi, _pc_apply_multi and
_gmres_solve_multi: several right-hand sides through one pass over the matrix, one walk through the level sets of the factor and
one lock-step GMRES.  Every column is held to the yardstick of its single entry (tests/multi_checks.py)."""
import pytest

import multi_checks as mc
import jacmult_checks as jm
import pc_checks as pc
from adflow_amd.topology import BrickTopology, ell_topology

pytestmark = pytest.mark.gpu

# iteration caps: those of tests/test_gpu_pc.py for the same shapes
CAP_PC, CAP_ADJOINT = 44, 60


def test_products(engine):
    mc.check_product_cases(engine, (7, 6, 5), (12, 9, 7), (10, 7, 6), BrickTopology(2, 2, 1, 9, 8, 6), ell_topology())


def test_sweeps_every_fill_and_nstate(engine):
    mc.check_sweep_cases(engine, (12, 8, 6), (10, 7, 6))


def test_sweeps_blocks_of_unequal_size_stay_subdomains(engine):
    mc.check_sweeps_rotated_interfaces(engine, ell_topology())


def test_sweeps_tile_sized_block(engine):
    """70 x 24 x 40 at fill 0 with 3 columns: partial waves, 132 hyperplanes.  The numpy factorisation of 67200 cells in two
    precisions is most of this test's time (as in test_gpu_pc.test_tile_sized_block); it is applied to one column, which is checked
    in each of the three positions of the call"""
    _, op = pc.single_block(engine, (70, 24, 40), pc.RANS, jm.WALL, stretch_k=2.0)
    engine.pcSetup(1)
    assert engine.pcInfo()[1] == 132
    mc.check_sweeps_every_lane(engine, op, 0, 491, "70 x 24 x 40")
    engine.pcRelease()
    engine.releaseWorkspace()


def test_factor_slots(engine):
    mc.check_factor_slots(engine, (7, 6, 5))


def test_ank_factor(engine):
    mc.check_ank_factor(engine)


def test_one_column_is_the_single_entry_and_columns_are_independent(engine):
    mc.check_one_column_and_independence(engine, (7, 6, 5), CAP_PC)


def test_gmres_columns_on_the_pc_matrix(engine):
    mc.check_gmres_on_pc_matrix(engine, (12, 8, 6), CAP_PC)


def test_gmres_columns_in_the_adjoint_order(engine):
    mc.check_gmres_adjoint_order(engine, (8, 7, 6), CAP_ADJOINT)


def test_refusals_and_no_side_effects(engine):
    mc.check_refusals_and_side_effects(engine)


def test_dev_forms_and_enqueue_only_mode(engine, request):
    from device_vectors import device_vectors
    mc.check_dev_twins_and_async(engine, device_vectors(request.config), ell_topology(), (7, 5, 4), 32)
