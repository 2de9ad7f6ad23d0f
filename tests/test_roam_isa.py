"""The layout of k_step_roam's trip loop in the built library (tools/roam_isa.py): no scratch, the stop flag's load a
whole shadow away from the next vmcnt wait, and the pair across the trip boundary no longer than the ones inside it.

The tool walks the shortest cycle of the kernel's control flow through the flag load and looks at nothing but
`s_waitcnt`, `global_load_*`, `ds_*` and branch mnemonics.  Skipped where the ROCm LLVM tools are missing."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_step_roam<true, 256, false>', 'k_step_roam<true, 256, true>', 'k_step_roam<true, 512, false>']


def _tool():
    spec = importlib.util.spec_from_file_location('roam_isa', os.path.join(ROOT, 'tools', 'roam_isa.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def layout():
    tool = _tool()
    if tool.find_objdump() is None:
        pytest.skip('llvm-objdump of the ROCm LLVM not found')
    from ssrs_amd import _native
    rep = tool.report(_native.LIB_PATH)
    for k, r in rep.items():
        print(k, r)
    return rep


@pytest.mark.parametrize('kernel', KERNELS)
def test_no_scratch_and_the_lds_budget(layout, kernel):
    r = layout[kernel]
    assert r['scratch'] == 0, r
    # (the feeder kernel's 159 872 bytes are the budget: window, ring, tags and the small arrays)
    assert r['lds'] <= 159872, r


@pytest.mark.parametrize('kernel', KERNELS)
def test_trip_has_four_gathers_and_their_waits(layout, kernel):
    r = layout[kernel]
    assert len(r['pairs']) == 4, r
    assert sum(p['boundary'] for p in r['pairs']) == 1 and r['pairs'][3]['boundary'], r
    assert all(p['wait_vmcnt'] in (0, 1) for p in r['pairs']), r


@pytest.mark.parametrize('kernel', KERNELS)
def test_flag_load_is_a_shadow_away_from_the_next_wait(layout, kernel):
    # (an ordinary shadow is 58 instructions)
    r = layout[kernel]
    assert r['flag_to_wait'] >= 50, r


@pytest.mark.parametrize('kernel', KERNELS)
def test_boundary_pair_is_no_longer_than_the_others(layout, kernel):
    r = layout[kernel]
    inside = [p['gather_to_wait'] for p in r['pairs'] if not p['boundary']]
    across = [p['gather_to_wait'] for p in r['pairs'] if p['boundary']]
    assert len(inside) == 3 and len(across) == 1, r
    assert across[0] <= max(inside) + 16, r
