"""CPU-only twin of tests/test_gpu_jacfree.py: the seed and read-out kernels of the matrix-free product (adflow_amd/csrc/kernels_ad.hip)
and its host path compiled with g++ (tests/hostsim) on small cases.  The RCCL leg and the tile-sized block run on the GPU only."""
import numpy as np
import pytest

import jacfree_checks as jf
import jacmult_checks as jm
from adflow_amd.params import FlowParams, RANSEquations, dissScalar, dissMatrix, upwind, vanAlbeda, minmod
from adflow_amd.topology import BrickTopology, ell_topology
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")

RANS = jf.RANS
# restart = maxIts of the solves: the assembled solve on the 2 x 2 x 2 wall-bounded brick converges inside it in this tier
CAP = 120


def test_euler_pc_against_reference_blocks(hostsim_engine):
    jf.check_against_reference(hostsim_engine, (7, 6, 5), FlowParams(spaceDiscr=dissScalar), jm.EULER)


def test_rans_pc_against_reference_blocks(hostsim_engine):
    jf.check_against_reference(hostsim_engine, (7, 5, 4), RANS, jm.WALL, stretch_k=2.0)


def test_rans_exact_against_reference_blocks(hostsim_engine):
    """the 33-point operator; OPEN: non-zero blocks on halo columns without a donor, which must contribute nothing"""
    jf.check_against_reference(hostsim_engine, (5, 4, 3), RANS, jm.WALL, usePC=False, stretch_k=2.0)
    op, _ = jf.check_against_reference(hostsim_engine, (6, 5, 4), RANS, jm.OPEN, usePC=False, stretch_k=2.0)
    nx = op.dims[1][0]
    s_open = [s for s in range(op.st.shape[0]) if tuple(op.st[s]) == (-1, 0, 0)][0]      # column i + 1: a halo at the open face 2
    assert np.abs(op.J[1][nx - 1, :, :, :, :, s_open]).max() > 0.0


def test_frozen_turb_and_turb_only(hostsim_engine):
    rm = RANS.replace(limiter=minmod)
    jf.check_against_reference(hostsim_engine, (7, 5, 4), rm, jm.WALL, frozenTurb=True, stretch_k=2.0)       # nState = 5
    jf.check_against_reference(hostsim_engine, (7, 5, 4), rm, jm.WALL, useTurbOnly=True, stretch_k=2.0)      # nState = 1


def test_approx_sa(hostsim_engine):
    jf.check_against_reference(hostsim_engine, (7, 5, 4), RANS, jm.WALL, approxSA=True, stretch_k=2.0)


def test_exact_with_matrix_dissipation(hostsim_engine):
    jf.check_against_reference(hostsim_engine, (5, 4, 3), FlowParams(equations=RANSEquations, spaceDiscr=dissMatrix), jm.WALL, usePC=False,
                               stretch_k=2.0)


def test_across_blocks_periodic_brick(hostsim_engine):
    jf.check_brick(hostsim_engine, BrickTopology(2, 2, 1, 6, 5, 4), FlowParams(spaceDiscr=dissScalar))
    jf.check_brick(hostsim_engine, BrickTopology(2, 2, 1, 6, 5, 4), FlowParams(equations=RANSEquations, spaceDiscr=upwind), seed=241)


def test_across_rotated_interfaces(hostsim_engine):
    jf.check_brick(hostsim_engine, ell_topology(), FlowParams(spaceDiscr=upwind), seed=251)


def test_determinism_and_side_effects(hostsim_engine):
    jf.check_determinism_and_side_effects(hostsim_engine)


def test_dev_form_returns_what_the_host_form_returns(hostsim_engine):
    from device_vectors import HostVectors
    jf.check_dev_twin(hostsim_engine, HostVectors())


def test_enqueue_only_chain(hostsim_engine):
    from device_vectors import HostVectors
    jf.check_enqueue_only_chain(hostsim_engine, HostVectors())


def test_solve_agrees_with_the_assembled_solve(hostsim_engine):
    jf.check_solve(hostsim_engine, CAP, CAP)


def test_solve_frozen_turbulence(hostsim_engine):
    jf.check_solve(hostsim_engine, CAP, CAP, frozenTurb=True)


def test_refusals(hostsim_engine):
    jf.check_refusals(hostsim_engine)
