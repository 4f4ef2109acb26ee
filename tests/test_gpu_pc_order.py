"""GPU parity (real MI355X, through the C-ABI): adflow_gpu_pc_set_ordering -- the ILU(k) over the whole level in the RCM ordering
(PCFactorSetMatOrderingType of setupStandardKSP, adjointUtils.F90:1555) or in a caller's permutation.  Against the rows of the level
relabelled by the permutation, completed and factored in numpy in float64 and in longdouble (tests/pc_order_checks.py): the library
may be at most 10 x as far from the longdouble result as the float64 numpy run is, adflow_gpu_pc_ordering_info and _level_info give
the numpy counts, and the RCM permutation is the one of a Python GENRCM.  Every shape is the smallest that carries its mechanism (at
most 1008 cells)."""
import pytest

import pc_order_checks as po

pytestmark = pytest.mark.gpu


def test_rcm_periodic_brick(engine):
    """2 x 2 x 1 periodic blocks of 6 x 5 x 4, fill 0, 1, 2"""
    po.check_rcm_periodic_brick(engine)


def test_random_permutation(engine):
    """2 x 1 x 1 of 3 x 4 x 4, fill 1 and 2: lower entries at any distance, rows of very different lengths in one slice, merge keys in
    no geometric order"""
    po.check_random_permutation(engine)


def test_red_black(engine):
    """one (12, 8, 6) RANS wall block, nState 6, fill 0: exactly two level sets of 288 rows"""
    po.check_red_black(engine)


def test_rcm_rotated_interfaces(engine):
    """the mirror entries of the transpose under a permutation, fill 1 and 2"""
    po.check_rcm_rotated(engine)


def test_rcm_period_of_three_cells(engine):
    po.check_rcm_period_of_three(engine)


def test_rcm_wall_brick_gmres(engine):
    po.check_wall_brick_gmres(engine)


def test_rcm_ank_pc_setup(engine):
    po.check_wall_brick_ank(engine)


def test_bit_identity(engine):
    po.check_bit_identity(engine)


def test_refusals(engine):
    po.check_refusals(engine)


def test_isolation(engine):
    po.check_isolation(engine)


def test_table_reuse(engine):
    po.check_table_reuse(engine)


def test_several_columns_iterations_and_bytes(engine):
    po.check_multi_its_and_bytes(engine)


def test_enqueue_only_chain(engine, request):
    from device_vectors import device_vectors
    po.check_enqueue_only_chain(engine, device_vectors(request.config))
