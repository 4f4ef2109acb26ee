"""GPU parity on curved, skewed, clustered and collapsed meshes and on meshes in other units of length (tests/mesh_families.py):
every entry of the library through the checkers that exist (tests/mesh_checks.py), at the project's bars.  Each case asserts its
family's recount first; that the reference is finite and well conditioned on every pair is asserted by the CPU tier
(tests/test_hostsim_meshes.py), and a non-finite reference fails every comparison here (NaN <= tol is false)."""
import pytest

import mesh_checks as mc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,entry", mc.pairs())
def test_entry_on_mesh(engine, case, entry):
    mc.run(engine, case, entry, big=True)


def test_random_parity_sweep_mesh_families(engine):
    """tests/fuzz_parity.py with the mesh family and the unit of length drawn per case: 150 cases"""
    import fuzz_parity
    n, failure = fuzz_parity.sweep(engine, 150, seed=20260926, quiet=True, families=True)
    assert failure is None, failure
