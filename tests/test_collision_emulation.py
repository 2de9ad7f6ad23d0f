"""K19 without a GPU: ssrs_amd/csrc/rotor_transits.hip -- the one file both ssrs_rotor_transits and
ssrs_rotor_collision_risk are made of -- compiled with g++ against tests/hip_host_stub and run on the CPU, with the stubs
and the stand-in for dynamic LDS of tests/test_transit_emulation.py.  The kernel's own code runs here as it stands: the ring
from the test's two numbers, the table lookup, the pending (key, count, sum) and its hand-overs to the uint32 counters and
the uint64 sums in LDS and, past the LDS rule's limit, to global memory, the pending per-track sum across lane, span and
track changes -- on the cases of tests/collision_ref.py, which tests/test_gpu_collision_risk.py runs on the device.  What it
does not cover: the device's own arithmetic (the f64 operations and the division are the host's here, under
-ffp-contract=off), blocks that run at the same time, and speed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import collision_ref as ref
import test_transit_emulation as tte
import transit_ref as tref

ROOT = tte.ROOT
LDS_WORDS = 15 * 1024


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    from ssrs_amd import _native
    work = tmp_path_factory.mktemp('collision_emu')
    # (the uint64 sums live in the stand-in for LDS: the array is aligned as the device's LDS is)
    assert tte.ERR_CPP.count('uint32_t s_trn_lds[16384];') == 1
    (work / 'err.cpp').write_text(tte.ERR_CPP.replace('uint32_t s_trn_lds[16384];', 'alignas(16) uint32_t s_trn_lds[16384];'))
    (work / 'collision_emu_extra.h').write_text(tte.EXTRA_H)
    lib = work / 'libcollision_emu.so'
    csrc = os.path.join(ROOT, 'ssrs_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-fPIC', '-shared', '-pthread', '-ffp-contract=off',
                    '-I', os.path.join(ROOT, 'tests', 'hip_host_stub'), '-I', csrc, '-include',
                    str(work / 'collision_emu_extra.h'), '-x', 'c++', os.path.join(csrc, 'rotor_transits.hip'),
                    str(work / 'err.cpp'), '-o', str(lib)], check=True)
    L = C.CDLL(str(lib))
    L.ssrs_last_error.restype = C.c_char_p
    L.emu_launches.restype = L.emu_blocks.restype = L.emu_lds_bytes.restype = C.c_longlong
    L.emu_lds.restype = C.POINTER(C.c_uint32)
    L.ssrs_rotor_transits.argtypes = _native.ROTOR_TRANSITS_ARGTYPES
    L.ssrs_rotor_collision_risk.argtypes = _native.ROTOR_COLLISION_RISK_ARGTYPES
    return L


def lds_words(shape, nturb):
    """(mask words or 0, turbines with counters in LDS, words asked for) by the header's rule: the mask padded to an even
    number of words, then two uint32 and two uint64 a turbine."""
    nbins = -(-shape[0] // 32) * -(-shape[1] // 32)
    mask_words = (nbins + 31) // 32
    room = (mask_words + 1) & ~1
    mask = mask_words <= 8192 and room + 6 * nturb <= LDS_WORDS
    cnt = nturb if mask else min(nturb, 2560)
    return (mask_words if mask else 0), cnt, (room if mask else 0) + 6 * cnt


def call(L, c, off=None, hits=None, transits=None, risk=None, track_risk=None, shift=None, alt_shift=None, want_tracks=True,
         plain=False):
    """One call on a case over the tracks of `off` (default: all).  Returns (hits uint32, transits, risk, track_risk int64);
    plain: ssrs_rotor_transits of the same build instead (risk and track_risk come back None)."""
    ptr = tte.ptr
    traj, alt, offsets = tref.flat(c)
    off = np.ascontiguousarray(offsets[1:] if off is None else off)
    ntracks = off.size - 1
    nturb = len(c['reach'])
    shift = c['shift'] if shift is None else shift
    o1, traj_v = tte.place(traj, shift)
    o2, alt_v = tte.place(alt, shift if alt_shift is None else alt_shift)
    info = tref.packed(c['elev'])
    bin_start, bin_items = tref.bins(c)
    xy = np.ascontiguousarray(c['xy'], dtype=np.float64)
    reach = np.ascontiguousarray(c['reach'], dtype=np.float64)
    hub = np.ascontiguousarray(c['hub'], dtype=np.int32)
    axis = np.ascontiguousarray(c['axis'], dtype=np.float64)
    cls = np.ascontiguousarray(c['cls'], dtype=np.int32)
    table = np.ascontiguousarray(c['table'], dtype=np.uint32)
    hits = np.zeros((ntracks, (nturb + 31) // 32), dtype=np.uint32) if hits is None else hits
    transits = np.zeros((nturb, 2), dtype=np.uint64) if transits is None else transits
    args = (ptr(traj_v), ptr(off), ntracks, ptr(alt_v), ptr(info), c['shape'][0], c['shape'][1], ptr(xy), ptr(reach), ptr(hub),
            ptr(axis), tref.MM, nturb, ptr(bin_start), ptr(bin_items), ptr(hits), ptr(transits))
    before = L.emu_launches()
    if plain:
        assert L.ssrs_rotor_transits(*args, None) == 0, L.ssrs_last_error()
        return hits, transits.astype(np.int64), None, None
    risk = np.zeros((nturb, 2), dtype=np.uint64) if risk is None else risk
    if want_tracks:
        track_risk = np.zeros(ntracks, dtype=np.uint64) if track_risk is None else track_risk
    rc = L.ssrs_rotor_collision_risk(*args, ptr(cls), ptr(table), table.shape[0], ptr(risk),
                                     ptr(track_risk) if want_tracks else None, None)
    assert rc == 0, L.ssrs_last_error()
    if L.emu_launches() > before:
        _, _, words = lds_words(c['shape'], nturb)
        asked = L.emu_lds_bytes()
        assert asked == 4 * words <= 4 * LDS_WORDS
        behind = np.ctypeslib.as_array(L.emu_lds(), shape=(16384,))[asked // 4:]
        assert (behind == 0xA5A5A5A5).all(), 'the kernel wrote past the dynamic LDS it asked for'
    return hits, transits.astype(np.int64), risk.astype(np.int64), track_risk.astype(np.int64) if want_tracks else None


def check(res, out):
    hits, transits, risk, track_risk = out
    assert np.array_equal(hits, res['bitmap']) and np.array_equal(transits, res['transits'])
    assert np.array_equal(risk, res['risk'])
    assert track_risk is None or np.array_equal(track_risk, res['track_risk'])


@pytest.mark.parametrize('c', ref.CASES, ids=ref.CASE_IDS)
def test_emulated_case(emu, c):
    res = ref.expected(c['name'])
    out = call(emu, c)
    check(res, out)
    # hits and transits are ssrs_rotor_transits' of the same build
    plain = call(emu, c, plain=True)
    assert np.array_equal(plain[0], out[0]) and np.array_equal(plain[1], out[1])
    assert res['risk'].sum() > 0


@pytest.mark.parametrize('name', ['planted', 'pingpong', 'cuts', 'rings'])
def test_emulated_every_placement(emu, name):
    """Both buffers at the three misaligned placements, the point-by-point path with `alt` alone off the boundary, and the
    same without per-track sums (track_risk NULL)."""
    c = ref.case(name)
    for shift, alt_shift in ((1, 1), (2, 2), (3, 3), (0, 1), (0, 0)):
        check(ref.expected(name), call(emu, c, shift=shift, alt_shift=alt_shift))
    for shift in (0, 1):
        check(ref.expected(name), call(emu, c, shift=shift, want_tracks=False))


def test_emulated_accumulation(emu):
    """Calls over disjoint track ranges into one `risk` and the rows of one `track_risk` equal one call, and what all four
    outputs held before is kept."""
    c = ref.case('rings')
    res = ref.expected('rings')
    _, _, offsets = tref.flat(c)
    off = offsets[1:]
    ntracks, nturb = off.size - 1, len(c['reach'])
    hits = np.full((ntracks, 1), 1 << 30, dtype=np.uint32)
    transits = np.full((nturb, 2), 7, dtype=np.uint64)
    risk = np.full((nturb, 2), 2 ** 40 + 5, dtype=np.uint64)
    track_risk = np.full(ntracks, 11, dtype=np.uint64)
    for lo, hi in ((0, 3), (3, 4), (4, ntracks - 2), (ntracks - 2, ntracks - 1), (ntracks - 1, ntracks)):
        call(emu, c, off=off[lo:hi + 1], hits=hits[lo:hi], transits=transits, risk=risk, track_risk=track_risk[lo:hi])
    assert np.array_equal(hits, res['bitmap'] | np.uint32(1 << 30))
    assert np.array_equal(transits.astype(np.int64) - 7, res['transits'])
    assert np.array_equal(risk.astype(np.int64) - (2 ** 40 + 5), res['risk'])
    assert np.array_equal(track_risk.astype(np.int64) - 11, res['track_risk'])


@pytest.mark.parametrize('nturb', [2559, 2560, 2561, 7681])
def test_emulated_lds_boundary(emu, nturb):
    """Either side of K19's LDS rule: on this raster 2559 turbines keep the mask, 2560 fill the 60 KB with counters and
    sums, from 2561 on the hand-overs of the last ones go to global memory; 7681 is past K18's limit too."""
    c = ref.many_turbines(nturb)
    mask_words, cnt, words = lds_words(c['shape'], nturb)
    assert (mask_words, cnt, words) == ((1, nturb, 2 + 6 * nturb) if nturb < 2560 else (0, 2560, LDS_WORDS))
    res = ref.compute(c)
    assert all(res['risk'][t].sum() > 0 for t in (2559, 2560, nturb - 1) if t < nturb)
    out = call(emu, c)
    check(res, out)
    plain = call(emu, c, plain=True)
    assert np.array_equal(plain[0], out[0]) and np.array_equal(plain[1], out[1])


def test_emulated_nothing_to_do_touches_nothing(emu):
    c = ref.case('rings')
    hits = np.full((3, 1), 9, dtype=np.uint32)
    transits = np.full((len(c['reach']), 2), 9, dtype=np.uint64)
    risk, track_risk = transits.copy(), np.full(3, 9, dtype=np.uint64)
    before = emu.emu_launches()
    call(emu, c, off=np.array([5], dtype=np.int64), hits=hits[:0], transits=transits, risk=risk, track_risk=track_risk[:0])
    call(emu, c, off=np.array([5, 5, 5, 5], dtype=np.int64), hits=hits, transits=transits, risk=risk, track_risk=track_risk)
    assert emu.emu_launches() == before
    assert (hits == 9).all() and (transits == 9).all() and (risk == 9).all() and (track_risk == 9).all()
