"""GPU parity (real MI355X, through the C-ABI): adflow_gpu_jacobian_mult -- y = J x and y = J^T x with the matrix
adflow_gpu_fd_jacobian left on the device, the MatMult of solveAdjoint's GMRES on dRdwT (adjointAPI.F90:661-863, :741, :806).
Against numpy applying the reference's own forward-mode blocks (oracle/_ref, ref_ad_jacobian) and, to rounding, the library's
downloaded blocks through the donor map of the 2-layer pattern (tests/jacmult_checks.py)."""
import numpy as np
import pytest

import checks
import jacmult_checks as jm
from adflow_amd.params import FlowParams, RANSEquations, dissScalar, upwind, vanAlbeda, minmod
from adflow_amd.topology import BrickTopology, ell_topology

pytestmark = pytest.mark.gpu

RANS = FlowParams(equations=RANSEquations, spaceDiscr=upwind, limiter=vanAlbeda)


def test_euler_pc_against_reference_blocks(engine):
    jm.check_against_reference(engine, (12, 9, 7), FlowParams(spaceDiscr=dissScalar), jm.EULER)


def test_rans_pc_against_reference_blocks(engine):
    jm.check_against_reference(engine, (12, 8, 6), RANS, jm.WALL, stretch_k=2.0)


def test_rans_exact_drdw_against_reference_blocks(engine):
    """the 33-point matrix of the adjoint; OPEN: non-zero blocks on halo columns without a donor, which are dropped"""
    jm.check_against_reference(engine, (8, 7, 6), RANS, jm.WALL, usePC=False, stretch_k=2.0)
    op = jm.check_against_reference(engine, (9, 8, 6), RANS, jm.OPEN, usePC=False, stretch_k=2.0)
    nx, ny, nz = op.dims[1]
    s_open = [s for s in range(op.st.shape[0]) if tuple(op.st[s]) == (-1, 0, 0)][0]      # column i + 1: a halo at the open face 2
    assert np.abs(op.J[1][nx - 1, :, :, :, :, s_open]).max() > 0.0


def test_frozen_turb_and_turb_only(engine):
    rm = RANS.replace(limiter=minmod)
    jm.check_against_reference(engine, (10, 7, 6), rm, jm.WALL, frozenTurb=True, stretch_k=2.0)       # nState = 5
    jm.check_against_reference(engine, (10, 7, 6), rm, jm.WALL, useTurbOnly=True, stretch_k=2.0)      # nState = 1


def test_across_blocks_periodic_brick(engine):
    """2 x 2 x 1 blocks of 9 x 8 x 6, periodic: a block is its own neighbour in k, halos share donors, corner halos have donors;
    then every interface as a message to the own rank (pack, ncclSend / ncclRecv, unpack forward; the same messages the other way
    with the accumulating unpack for the transposed product); the adjoint identity"""
    jm.check_brick(engine, BrickTopology(2, 2, 1, 9, 8, 6), FlowParams(spaceDiscr=dissScalar), rccl_self=True)
    jm.check_brick(engine, BrickTopology(2, 2, 1, 9, 8, 6), FlowParams(equations=RANSEquations, spaceDiscr=upwind), seed=241)


def test_across_rotated_interfaces(engine):
    """four blocks of different sizes joined with orientation changes (adflow_amd.topology.ell_topology)"""
    jm.check_brick(engine, ell_topology(), FlowParams(spaceDiscr=upwind), seed=251, rccl_self=True)


def test_tile_sized_block_and_workspace(engine):
    """RANS upwind preconditioner matrix by forward mode on 70 x 24 x 40: several waves per row, partial waves, several k chunks;
    the work space is handed back and laid out again"""
    dims = (70, 24, 40)
    blk, _, _ = checks.setup_block_with_bc(engine, dims, RANS, jm.WALL, 107, stretch_k=2.0)
    engine.setupStateResidualMatrix(1, True, useAD=True)
    op = jm.operator_of(engine, {1: blk})
    first = jm.assert_products_to_rounding(engine, op, 261, "70 x 24 x 40")
    nbytes = engine.releaseWorkspace()
    assert nbytes >= 2 * 6 * 8 * (dims[0] + 4) * (dims[1] + 4) * (dims[2] + 4), nbytes
    assert engine.releaseWorkspace() == 0
    for tr in (False, True):
        x, y = first[tr]
        assert np.array_equal(engine.jacobianMult(x, 1, transpose=tr), y)
    engine.releaseWorkspace()


def test_refusals_and_no_side_effects(engine):
    jm.check_refusals_and_side_effects(engine)


def test_dev_form_returns_what_the_host_form_returns(engine, request):
    """adflow_gpu_jacobian_mult_dev on torch tensors against adflow_gpu_jacobian_mult, bit for bit"""
    from device_vectors import device_vectors
    jm.check_dev_twin(engine, device_vectors(request.config), ell_topology())
