"""GPU parity (real MI355X, through the C-ABI): adflow_gpu_pc_set_level_fill -- the ILU(k), k = 0 .. 3, of the 7-point preconditioner
matrix over the whole level on a general block pattern, what setupStandardKSP (adjointUtils.F90:1374-1562) gives one process with
PCFactorSetLevels(fill) (csrc/kernels_pc_level.hip).  Against pc_checks.NumpyILU0._factor on the rows of the level completed by
pc_fill_checks.NumpyILUk._symbolic, in float64 and in longdouble (tests/pc_level_checks.py): the library may be at most 10 x as far
from the longdouble result as the float64 numpy run is, and adflow_gpu_pc_level_info gives the numpy counts.  Every shape is the
smallest at which its mechanism is exercised (at most 1728 cells)."""
import pytest

import pc_level_checks as pl
from adflow_amd.topology import BrickTopology

pytestmark = pytest.mark.gpu


def test_periodic_brick_fill_0_1(engine):
    """2 x 2 x 1 periodic blocks of 9 x 8 x 6: at fill 0 a level set is longer than one wave (two workgroups in a launch); wraps inside
    the own block along k make lower entries with larger offsets; rows of up to 17 entries at fill 1"""
    pl.check_periodic_brick(engine, BrickTopology(2, 2, 1, 9, 8, 6), (0, 1), two_workgroups=0)


def test_periodic_brick_fill_2_3(engine):
    """2 x 2 x 1 of 6 x 5 x 4: rows of up to 37 / 74 entries"""
    pl.check_periodic_brick(engine, BrickTopology(2, 2, 1, 6, 5, 4), (2, 3))


def test_rotated_interfaces(engine):
    """the blocks of ell_topology at half size, fill 1 and 2: the mirror entry is not at the opposite offset, blocks of different sizes"""
    pl.check_rotated(engine)


def test_wall_brick_apply_and_gmres(engine):
    """the benchmark layout in miniature, RANS Roe by forward mode, nState 6, fill 2: the applications and gmresSolve, then the
    coupled fill-0 and the block-local fill-2 factor of the same matrix"""
    pl.check_wall_brick_gmres(engine)


def test_wall_brick_frozen_turb_and_turb_only(engine):
    pl.check_wall_brick_apply(engine, 1, frozenTurb=True)        # nState = 5
    pl.check_wall_brick_apply(engine, 1, useTurbOnly=True)       # nState = 1


def test_wall_brick_ank_pc_setup(engine):
    pl.check_wall_brick_ank(engine)


def test_single_block(engine):
    """(12, 8, 6) without self-interfaces: the counts of the block-local factors at fill 0, 1, 2"""
    pl.check_single_block(engine)


def test_single_block_fill_3(engine):
    pl.check_single_block_fill3(engine)


def test_period_of_three_cells(engine):
    pl.check_period_of_three(engine)


def test_refusals(engine):
    pl.check_refusals(engine)


def test_isolation(engine):
    pl.check_isolation(engine)


def test_several_columns_and_bytes(engine):
    pl.check_multi_and_bytes(engine)


def test_table_reuse(engine):
    pl.check_table_reuse(engine)


def test_enqueue_only_chain(engine, request):
    from device_vectors import device_vectors
    pl.check_enqueue_only_chain(engine, device_vectors(request.config))
