"""GPU parity (real MI355X, through the C-ABI): adflow_gpu_jacfree_mult[_dev] -- y = dR/dw x by one forward-mode evaluation seeded with x,
the shell product dRdwMatMult (adjointAPI.F90:1050-1128) -- and adflow_gpu_jacfree_solve[_dev], the GMRES of solveDirectForRHS on it.
Against numpy applying the reference's own forward-mode blocks (oracle/_ref, ref_ad_jacobian) and the library's own assembled blocks
through the donor map of the 2-layer pattern (tests/jacfree_checks.py)."""
import numpy as np
import pytest

import jacfree_checks as jf
import jacmult_checks as jm
from adflow_amd.params import FlowParams, RANSEquations, dissScalar, dissMatrix, upwind, vanAlbeda, minmod
from adflow_amd.topology import BrickTopology, ell_topology

pytestmark = pytest.mark.gpu

RANS = jf.RANS
# restart = maxIts of the solves: the assembled solve on the 2 x 2 x 2 wall-bounded brick converges inside it in the emulator tier
CAP = 120


def test_euler_pc_against_reference_blocks(engine):
    jf.check_against_reference(engine, (12, 9, 7), FlowParams(spaceDiscr=dissScalar), jm.EULER)


def test_rans_pc_against_reference_blocks(engine):
    jf.check_against_reference(engine, (12, 8, 6), RANS, jm.WALL, stretch_k=2.0)


def test_rans_exact_against_reference_blocks(engine):
    """the 33-point operator; OPEN: non-zero blocks on halo columns without a donor, which must contribute nothing"""
    jf.check_against_reference(engine, (8, 7, 6), RANS, jm.WALL, usePC=False, stretch_k=2.0)
    op, _ = jf.check_against_reference(engine, (9, 8, 6), RANS, jm.OPEN, usePC=False, stretch_k=2.0)
    nx = op.dims[1][0]
    s_open = [s for s in range(op.st.shape[0]) if tuple(op.st[s]) == (-1, 0, 0)][0]      # column i + 1: a halo at the open face 2
    assert np.abs(op.J[1][nx - 1, :, :, :, :, s_open]).max() > 0.0


def test_frozen_turb_and_turb_only(engine):
    rm = RANS.replace(limiter=minmod)
    jf.check_against_reference(engine, (10, 7, 6), rm, jm.WALL, frozenTurb=True, stretch_k=2.0)       # nState = 5
    jf.check_against_reference(engine, (10, 7, 6), rm, jm.WALL, useTurbOnly=True, stretch_k=2.0)      # nState = 1


def test_approx_sa(engine):
    jf.check_against_reference(engine, (10, 7, 6), RANS, jm.WALL, approxSA=True, stretch_k=2.0)


def test_exact_with_matrix_dissipation(engine):
    jf.check_against_reference(engine, (8, 7, 6), FlowParams(equations=RANSEquations, spaceDiscr=dissMatrix), jm.WALL, usePC=False,
                               stretch_k=2.0)


def test_across_blocks_periodic_brick(engine):
    """2 x 2 x 1 blocks of 9 x 8 x 6, periodic: a block is its own neighbour in k, halos share donors, corner halos have donors; once
    more with every interface as a message to the own rank (pack, ncclSend / ncclRecv, unpack)"""
    jf.check_brick(engine, BrickTopology(2, 2, 1, 9, 8, 6), FlowParams(spaceDiscr=dissScalar), rccl_self=True)
    jf.check_brick(engine, BrickTopology(2, 2, 1, 9, 8, 6), FlowParams(equations=RANSEquations, spaceDiscr=upwind), seed=241)


def test_across_rotated_interfaces(engine):
    jf.check_brick(engine, ell_topology(), FlowParams(spaceDiscr=upwind), seed=251)


def test_tile_sized_block_and_workspace(engine):
    jf.check_tile_sized_block(engine)


def test_determinism_and_side_effects(engine):
    jf.check_determinism_and_side_effects(engine)


def test_dev_form_returns_what_the_host_form_returns(engine, request):
    from device_vectors import device_vectors
    jf.check_dev_twin(engine, device_vectors(request.config))


def test_enqueue_only_chain(engine, request):
    from device_vectors import device_vectors
    jf.check_enqueue_only_chain(engine, device_vectors(request.config))


def test_solve_agrees_with_the_assembled_solve(engine):
    jf.check_solve(engine, CAP, CAP)


def test_solve_frozen_turbulence(engine):
    jf.check_solve(engine, CAP, CAP, frozenTurb=True)


def test_refusals(engine):
    jf.check_refusals(engine)
