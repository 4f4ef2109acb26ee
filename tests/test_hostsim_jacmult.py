"""CPU-only twin of tests/test_gpu_jacmult.py: the kernels of adflow_amd/csrc/kernels_jacmult.hip compiled with g++ (tests/hostsim)
on small cases.  The RCCL leg and the tile-sized block run on the GPU only."""
import numpy as np
import pytest

import checks
import jacmult_checks as jm
from adflow_amd.params import FlowParams, RANSEquations, dissScalar, upwind, vanAlbeda, minmod
from adflow_amd.topology import BrickTopology, ell_topology
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")

RANS = FlowParams(equations=RANSEquations, spaceDiscr=upwind, limiter=vanAlbeda)


def test_euler_pc_against_reference_blocks(hostsim_engine):
    jm.check_against_reference(hostsim_engine, (7, 6, 5), FlowParams(spaceDiscr=dissScalar), jm.EULER)


def test_rans_against_reference_blocks(hostsim_engine):
    jm.check_against_reference(hostsim_engine, (7, 5, 4), RANS, jm.WALL, stretch_k=2.0)
    jm.check_against_reference(hostsim_engine, (6, 5, 4), RANS, jm.OPEN, usePC=False, stretch_k=2.0)


def test_frozen_turb_and_turb_only(hostsim_engine):
    rm = RANS.replace(limiter=minmod)
    jm.check_against_reference(hostsim_engine, (7, 5, 4), rm, jm.WALL, frozenTurb=True, stretch_k=2.0)
    jm.check_against_reference(hostsim_engine, (7, 5, 4), rm, jm.WALL, useTurbOnly=True, stretch_k=2.0)


def test_across_blocks_periodic_brick(hostsim_engine):
    jm.check_brick(hostsim_engine, BrickTopology(2, 2, 1, 6, 5, 4), FlowParams(spaceDiscr=dissScalar))


def test_across_rotated_interfaces(hostsim_engine):
    jm.check_brick(hostsim_engine, ell_topology(), FlowParams(spaceDiscr=upwind), seed=251)


def test_workspace_released_and_laid_out_again(hostsim_engine):
    e = hostsim_engine
    dims = (9, 6, 5)
    blk, _, _ = checks.setup_block_with_bc(e, dims, RANS, jm.WALL, 107, stretch_k=2.0)
    e.setupStateResidualMatrix(1, True, useAD=True)
    first = jm.assert_products_to_rounding(e, jm.operator_of(e, {1: blk}), 261, "9 x 6 x 5")
    assert e.releaseWorkspace() >= 2 * 6 * 8 * (dims[0] + 4) * (dims[1] + 4) * (dims[2] + 4)
    for tr in (False, True):
        x, y = first[tr]
        assert np.array_equal(e.jacobianMult(x, 1, transpose=tr), y)
    e.releaseWorkspace()


def test_refusals_and_no_side_effects(hostsim_engine):
    jm.check_refusals_and_side_effects(hostsim_engine)


def test_dev_form_returns_what_the_host_form_returns(hostsim_engine):
    from device_vectors import HostVectors
    jm.check_dev_twin(hostsim_engine, HostVectors(), ell_topology())
