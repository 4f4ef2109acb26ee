"""The cases of tests/test_gpu_options.py on the kernel-logic emulator (the same kernel sources compiled for the host), and the
guards of tests/option_checks.py, which need the reference only: every (group, entry) pair moves the reference's own output of the
entry's checker by 1e4 TOL on the same input, every single option does so on at least one entry unless NO_EFFECT names the line of
the reference that shows why not, and no row of NO_EFFECT moves anything after all.  (The emulator never captures a multigrid cycle:
the change of flight condition runs on the direct path here.)"""
import dataclasses

import pytest

import option_checks as oc
import test_gpu_options as tg
from adflow_amd.params import FlowParams


@pytest.mark.parametrize("group,entry", oc.CASES, ids=[f"{g}:{e}" for g, e in oc.CASES])
def test_option_group(hostsim_engine, group, entry):
    """under the default dispatch; with the marches off the same case runs inside the guard below"""
    oc.run_case(hostsim_engine, group, entry, dispatches=(True,))


@pytest.mark.parametrize("group,entry", oc.GUARDED, ids=[f"{g}:{e}" for g, e in oc.GUARDED])
def test_reference_reads_the_group_on_this_entry(hostsim_engine, group, entry):
    """(the guard's first run IS the parity of the case with the marches switched off)"""
    moved = oc.sensitivity(hostsim_engine, entry, oc.GROUPS[group])
    assert moved >= oc.MOVED, (group, entry, moved)


@pytest.mark.parametrize("option", sorted(oc.SINGLE_OPTIONS))
def test_reference_reads_every_single_option(hostsim_engine, option):
    value, entries = oc.SINGLE_OPTIONS[option]
    moved = {e: oc.sensitivity(hostsim_engine, e, {option: value}) for e in entries}
    assert max(moved.values()) >= oc.MOVED, (option, moved)


def test_every_option_is_varied_or_named():
    """every field of FlowParams is in a group, in NO_EFFECT or in the list of those that are no option of the path"""
    varied = set(oc.SINGLE_OPTIONS) | {k for g in oc.GROUPS.values() for k in g} | {o for o, _ in oc.NO_EFFECT if o not in oc.GROUPS}
    missing = {f.name for f in dataclasses.fields(FlowParams)} - varied - set(oc.VARIED_ELSEWHERE) - set(oc.NOT_AN_OPTION)
    assert not missing, missing


@pytest.mark.parametrize("option,entry", sorted(oc.NO_EFFECT), ids=[f"{o}:{e}" for o, e in sorted(oc.NO_EFFECT)])
def test_no_effect_rows_have_no_effect(hostsim_engine, option, entry):
    assert oc.sensitivity(hostsim_engine, entry, oc.no_effect_options(option)) == 0.0


@pytest.mark.parametrize("group", ["mach2", "alpha-7", "sideslip"])
def test_farfield_all_four_characteristic_classes(hostsim_engine, group):
    tg.test_farfield_all_four_characteristic_classes(hostsim_engine, group)


@pytest.mark.parametrize("group", ["mach1.3", "alpha35"])
def test_farfield_mach_1_3(hostsim_engine, group):
    tg.test_farfield_mach_1_3(hostsim_engine, group)


@pytest.mark.parametrize("marches", [True, False])
def test_farfield_supersonic_whole_residual(hostsim_engine, marches):
    tg.test_farfield_supersonic_whole_residual(hostsim_engine, marches)


@pytest.mark.parametrize("ad", [False, True])
@pytest.mark.parametrize("usePC", [True, False])
def test_farfield_supersonic_linearised(hostsim_engine, ad, usePC):
    tg.test_farfield_supersonic_linearised(hostsim_engine, ad, usePC)


def test_flight_condition_changes_on_registered_blocks(hostsim_engine):
    tg.test_flight_condition_changes_on_registered_blocks(hostsim_engine)


def test_kato_launder_production_is_refused(hostsim_engine):
    tg.test_kato_launder_production_is_refused(hostsim_engine)
