"""GPU parity (real MI355X, through the C-ABI): adflow_gpu_pc_set_its -- the Richardson iterations setupStandardKSP
(adjointUtils.F90:1374-1562) and the mg shell (amg.F90:487-615) wrap around the ILU: outerPreconIts on the 7-point matrix of the whole
level, innerPreconIts[Coarse] on the matrix the factor was built from (csrc/kernels_pc_rich.hip, pc_apply_enqueue of csrc/api.hip).
Against the numpy factors of the sibling files wrapped in the recurrences of the header, in float64 and in longdouble
(tests/pc_its_checks.py): the library may be at most 10 x as far from the longdouble result as the float64 numpy run is.  Every shape is
the smallest at which its mechanism is exercised (at most 1008 cells)."""
import pytest

import pc_its_checks as pi

pytestmark = pytest.mark.gpu


def test_single_block(engine):
    """7 x 6 x 5, Euler JST, fill 0: (outer, inner) = (2,1), (3,1), (1,2), (2,2), pcItsInfo and the bytes"""
    pi.check_single(engine)


@pytest.mark.parametrize("fill", (0, 1))
def test_periodic_brick_block_local(engine, fill):
    """2 x 1 x 1 periodic blocks of 4 x 4 x 4: A_sub is not A_full, and outer = 2 couples the blocks"""
    pi.check_brick(engine, fill)


def test_rotated_interfaces(engine):
    """coupled = 1 at (3,1) and level fill 1 at (2,2): the mirror entries across rotated interfaces"""
    pi.check_rotated(engine)


def test_period_of_three_cells(engine):
    pi.check_period_of_three(engine)


def test_level_fill_table_reuse_redoes_the_copy(engine):
    pi.check_level_table_reuse(engine)


def test_wall_brick_level_fill_2_outer_3_and_gmres(engine):
    """the reference's default adjoint preconditioner on one process, apart from the ordering"""
    pi.check_wall_brick(engine)


def test_wall_brick_ank_pc_setup(engine):
    pi.check_wall_brick_ank(engine)


@pytest.mark.parametrize("brick", (False, True))
def test_hierarchy(engine, brick):
    """pcSetMg(2, nSmooth = 2) with pcSetIts(2, 2, 2), then (1, 1, 2): only the coarse level iterates"""
    pi.check_hierarchy(engine, brick)


def test_several_columns(engine):
    pi.check_multi(engine)


def test_defaults_are_bit_identical(engine):
    pi.check_defaults(engine)


def test_slots_and_persistence(engine):
    pi.check_slots_and_persistence(engine)


def test_enqueue_only_chain(engine, request):
    from device_vectors import device_vectors
    pi.check_enqueue_only_chain(engine, device_vectors(request.config))


def test_refusals(engine):
    pi.check_refusals(engine)
