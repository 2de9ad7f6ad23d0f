"""K23 without a GPU: ssrs_amd/csrc/bridge.hip compiled with g++ against tests/hip_host_stub under -ffp-contract=off and run
on the CPU, as test_score_emulation.py does for K21.  The kernel cooperates through dynamic LDS and __syncthreads() only, so
its own code runs here as it stands: the scan for the longest job, the statuses in their order, the window and its clipping,
the rectangles of every step, the source-indexed planes, lane 0's read of B -- on the cases of tests/bridge_ref.py, which
tests/test_gpu_bridge.py runs on the device.  The dynamic LDS is handed over full of NaN with a guard behind it.  What it
does not cover: the device's own arithmetic (the f64 operations, log2 and pow are the host's here), workgroups that run at
the same time, whether the runtime grants the LDS, and speed."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bridge_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
ERR_CPP = '''#include "common.h"
namespace ssrs {
char *error_buffer() { static thread_local char buf[512] = ""; return buf; }
int set_error(int code, const char *fmt, ...)
{ va_list ap; va_start(ap, fmt); vsnprintf(error_buffer(), 512, fmt, ap); va_end(ap); return code; }
}
extern "C" const char *ssrs_last_error(void) { return ssrs::error_buffer(); }
extern "C" long long emu_launches(void) { return emu_launch_count; }
extern "C" long long emu_lds_bytes(void) { return emu_lds_last; }
extern "C" long long emu_lds_overruns(void) { return emu_lds_overrun_count; }
extern "C" long long emu_threads(void) { return emu_threads_last; }
extern "C" void emu_offer_lds(int bytes) { emu_lds_offered = bytes; }
'''
# what the kernel uses beyond the stub: dynamic LDS (a buffer of the launch's size, filled with NaN, with a guard behind it
# that is checked after the launch), the 64-bit atomic maximum, the copies, the memset, the device attribute and the
# function attribute; launches are counted
EXTRA_H = '''#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
inline unsigned long long atomicMax(unsigned long long *p, unsigned long long v)
{
    unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
constexpr int hipMemcpyDeviceToHost = 2;
constexpr int hipDeviceAttributeMaxSharedMemoryPerBlock = 1, hipFuncAttributeMaxDynamicSharedMemorySize = 8;
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline int emu_lds_offered = 163840;
inline hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
inline hipError_t hipDeviceGetAttribute(int *v, int, int) { *v = emu_lds_offered; return hipSuccess; }
inline hipError_t hipFuncSetAttribute(const void *, int, int) { return hipSuccess; }
constexpr size_t kEmuGuard = 4096;
inline std::vector<unsigned char> emu_lds;
inline long long emu_launch_count = 0, emu_lds_last = 0, emu_lds_overrun_count = 0, emu_threads_last = 0;
inline void emu_lds_begin(size_t bytes)
{
    emu_lds.assign(bytes + kEmuGuard, 0xFF);
    memset(emu_lds.data() + bytes, 0xA5, kEmuGuard);
    emu_lds_last = static_cast<long long>(bytes);
}
inline void emu_lds_end()
{
    for (size_t i = 0; i < kEmuGuard; ++i)
        if (emu_lds[static_cast<size_t>(emu_lds_last) + i] != 0xA5) { ++emu_lds_overrun_count; break; }
}
#define HIP_DYNAMIC_SHARED(type, var) type *var = reinterpret_cast<type *>(emu_lds.data());
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \\
    (++emu_launch_count, emu_threads_last = dim3(block).x, emu_lds_begin(lds), \\
     emu_launch(grid, block, [&] { kernel(__VA_ARGS__); }), emu_lds_end())
'''


def build(work, name='libbridge_emu.so'):
    """The CPU build of bridge.hip in `work`, bound by the library's own prototype."""
    (work / 'err.cpp').write_text(ERR_CPP)
    (work / 'bridge_emu_extra.h').write_text(EXTRA_H)
    lib = work / name
    csrc = os.path.join(ROOT, 'ssrs_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-fPIC', '-shared', '-pthread', '-ffp-contract=off',
                    '-I', os.path.join(ROOT, 'tests', 'hip_host_stub'), '-I', csrc, '-include',
                    str(work / 'bridge_emu_extra.h'), '-x', 'c++', os.path.join(csrc, 'bridge.hip'),
                    str(work / 'err.cpp'), '-o', str(lib)], check=True)
    return bind(lib)


def bind(lib):
    from ssrs_amd import _native
    L = C.CDLL(str(lib))
    L.ssrs_last_error.restype = C.c_char_p
    L.emu_launches.restype = L.emu_lds_bytes.restype = L.emu_lds_overruns.restype = L.emu_threads.restype = C.c_longlong
    L.emu_offer_lds.argtypes = [C.c_int]
    L.ssrs_tracks_bridge.argtypes = _native.BRIDGE_ARGTYPES
    return L


@pytest.fixture(scope='module')
def work(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    return tmp_path_factory.mktemp('bridge_emu')


@pytest.fixture(scope='module')
def emu(work):
    return build(work)


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def params_of(c):
    from ssrs_amd import movmodel
    p = movmodel.make_track_params(c['shape'], c['move_dirn'], 1, c['nu'])
    assert [p.prior[k] for k in range(9)] == ref.sref.prior_of(c['move_dirn'])
    return p


def call(L, c, jobs=None, want_arrivals=True, rc=0):
    """One call on case c (its own jobs, or `jobs`), the outputs pre-filled with junk and guarded.  Returns a dict like
    bridge_ref.score's."""
    jobs = np.ascontiguousarray(c['jobs'] if jobs is None else jobs, dtype=np.int32).reshape(-1, 6)
    m = len(jobs)
    pad = 3
    g = np.full((m + 2 * pad, 9), -7.)
    status = np.full(m + 2 * pad, 99, dtype=np.uint8)
    surprisal = np.full(m + 2 * pad, 0xDEAD, dtype=np.uint64)
    arrivals = np.full((m + 2 * pad, ref.MAX_MOVES), -7.)
    upd = None if c['updraft'] is None else np.ascontiguousarray(c['updraft'], dtype=np.float64)
    pot = None if c['potential'] is None else np.ascontiguousarray(c['potential'], dtype=np.float32)
    prm = params_of(c)
    got = L.ssrs_tracks_bridge(C.cast(C.byref(prm), C.c_void_p), ptr(upd), ptr(pot), ptr(jobs), m, ptr(g[pad:]),
                               ptr(status[pad:]), ptr(surprisal[pad:]), ptr(arrivals[pad:]) if want_arrivals else None, None)
    assert got == rc, L.ssrs_last_error()
    inner = slice(pad, pad + m)
    outer = np.r_[0:pad, pad + m:m + 2 * pad]
    assert (g[outer] == -7.).all() and (status[outer] == 99).all() and (surprisal[outer] == 0xDEAD).all()
    assert (arrivals[outer] == -7.).all() and (want_arrivals or (arrivals == -7.).all())
    assert L.emu_lds_overruns() == 0
    if rc == 0 and m:
        assert (status[inner] != 99).all(), 'a status is written for every job'
    return dict(g=g[inner], status=status[inner], surprisal=surprisal[inner].view(np.int64),
                arrivals=arrivals[inner] if want_arrivals else None)


@pytest.mark.parametrize('name', ref.case_names())
def test_emulated_case(emu, name):
    c = ref.case(name)
    ref.check(c, call(emu, c), ref.expected(c))


def test_cases_cover_what_they_are_for():
    """Every status occurs; the windows are clipped on every side and unclipped at 33 x 33; every incoming state occurs; the
    thinned tracks are reachable; the properties the definition promises hold on the reference itself."""
    seen = np.zeros(5, dtype=np.int64)
    for c in ref.cases():
        seen += np.bincount(ref.expected(c)['status'], minlength=5)
    assert (seen > 0).all()
    assert (ref.expected(ref.case('huge_potential'))['status'] == ref.UNDEFINED).sum() > 3
    for c in ref.cases():
        e = ref.expected(c)
        ok = np.isin(e['status'], (ref.SCORED, ref.ZERO, ref.UNDEFINED))
        n = c['jobs'][:, 5]
        # arrivals[n - 1] is P; nothing past n
        assert ref.same_bits(e['arrivals'][ok, n[ok] - 1], e['p'][ok])
        assert all(not e['arrivals'][i, (n[i] if ok[i] else 0):].any() for i in range(len(n)))
        far = ok & (np.maximum(np.abs(c['jobs'][:, 0] - c['jobs'][:, 3]), np.abs(c['jobs'][:, 1] - c['jobs'][:, 4])) > n)
        assert (e['status'][far] == ref.ZERO).all()
    small = ref.case('7x9_nu1')
    assert set(small['jobs'][:, 2].tolist()) >= set(range(9))
    e = ref.expected(small)
    rim = (small['jobs'][:, 3] == 0) | (small['jobs'][:, 4] == 0) | (small['jobs'][:, 3] == 6) | (small['jobs'][:, 4] == 8)
    assert (e['status'][rim] == ref.SCORED).sum() >= 3, 'B on the rim is reached'
    # the gaps thinned from oracle tracks are reachable by construction (all of a case's jobs behind the planted ones)
    for name, planted in (('7x9_nu1', len(ref.planted((7, 9)))), ('12x40_upd', 40), ('12x40_drw_d250_nu0.5', 40), ('g7_nu1', 25)):
        e = ref.expected(ref.case(name))
        assert len(e['status']) > planted + 10 and (e['status'][planted:] == ref.SCORED).all(), name
    g7 = ref.case('g7_nu1')
    assert (g7['jobs'][:, 5] == 32).sum() >= 6 and (ref.expected(g7)['status'][:2] == ref.SCORED).all()
    # n = 1 is the model's probability of the move (K21's p): a gap of one move is a move
    c = ref.case('7x9_nu2')
    model = ref.Model(c)
    ones = [job for job, st in zip(c['jobs'], ref.expected(c)['status']) if job[5] == 1 and st in (ref.SCORED, ref.ZERO)]
    assert len(ones) >= 12
    for job in ones:
        d = (job[3] - job[0], job[4] - job[1])
        want = model.p(int(job[0]), int(job[1]), int(job[2]))[ref.state_of(d)] if max(abs(d[0]), abs(d[1])) <= 1 else 0.
        assert model.job(job)[2] == want


def test_reference_conserves_mass_and_composes():
    """On the reference itself, away from the rim: the states after 5 steps sum to 1, and Chapman-Kolmogorov holds --
    P_n(A -> B) is the sum over the states (x, d) after k steps of their mass times P_{n-k}((x, d) -> B)."""
    for name in ('12x40_ff_nu2', '12x40_drw_d250_nu0.5', 'g7_nu1'):
        c = ref.case(name)
        model = ref.Model(c)
        a = (c['shape'][0] // 2, c['shape'][1] // 2)
        passes = model.forward(a, 4, 5)
        assert abs(sum(sum(v) for v in passes[5].values()) - 1.) < 1e-14      # (the rim is five rows away: nothing is lost yet)
        n, k = 5, 2
        for b, total in ((x, sum(v)) for x, v in list(passes[n].items())[:6]):
            parts = 0.
            for x, states in passes[k].items():
                for d in range(9):
                    if states[d] != 0.:
                        parts += states[d] * model.job(x + (d,) + b + (n - k,))[2]
            assert abs(parts - total) <= 1e-14 * total


def test_emulated_order_chunks_and_outputs(emu):
    """Permuted jobs give permuted outputs bit for bit; three calls equal one; arrivals may be left out; one job; none."""
    c = ref.case('12x40_ff_nu2')
    whole = call(emu, c)
    m = len(c['jobs'])
    order = np.random.default_rng(5).permutation(m)
    mixed = call(emu, c, jobs=c['jobs'][order])
    for key in ('g', 'status', 'surprisal', 'arrivals'):
        assert ref.same_bits(mixed[key].astype(np.float64), whole[key][order].astype(np.float64)) if key in ('g', 'arrivals') \
            else np.array_equal(mixed[key], whole[key][order]), key
    parts = [call(emu, c, jobs=c['jobs'][lo:hi]) for lo, hi in ((0, 7), (7, 8), (8, m))]
    for key in ('g', 'arrivals'):
        assert ref.same_bits(np.concatenate([p[key] for p in parts]), whole[key])
    assert np.array_equal(np.concatenate([p['surprisal'] for p in parts]), whole['surprisal'])
    bare = call(emu, c, want_arrivals=False)
    assert ref.same_bits(bare['g'], whole['g']) and np.array_equal(bare['status'], whole['status'])
    before = emu.emu_launches()
    assert len(call(emu, c, jobs=c['jobs'][:0])['status']) == 0 and emu.emu_launches() == before


def test_emulated_lds_follows_the_longest_valid_job(emu):
    """144 (N + 1)^2 bytes for the largest N in [1, 32] of the call; 512 lanes past 512 cells; jobs that are all refused still
    get their statuses."""
    c = ref.case('g7_nu1')
    for jobs, n_max, threads in (([(48, 64, 4, 49, 64, 3), (48, 64, 4, 48, 64, 40)], 3, 256),
                                 ([(48, 64, 4, 49, 64, 21)], 21, 256), ([(48, 64, 4, 49, 64, 22), (0, 0, 0, 0, 0, 0)], 22, 512),
                                 ([(48, 64, 4, 50, 64, 32)], 32, 512), ([(48, 64, 4, 48, 64, 33), (1, 1, 1, 1, 1, -1)], 0, 256)):
        jobs = np.array(jobs, dtype=np.int32)
        got = call(emu, c, jobs=jobs)
        assert emu.emu_lds_bytes() == 144 * (n_max + 1) ** 2 and emu.emu_threads() == threads
        want = ref.score(c, jobs)
        ref.check(c, got, want, jobs=jobs)
    assert 144 * 33 ** 2 == 156816


def test_emulated_refusal_when_the_device_offers_less(work):
    """A device whose hipDeviceAttributeMaxSharedMemoryPerBlock is less than the call needs is refused by name before the
    gaps are launched (the attribute is read once, so this runs in a library of its own)."""
    from ssrs_amd import _native
    copy = work / 'libbridge_emu_small.so'
    if not (work / 'libbridge_emu.so').exists():
        build(work)
    shutil.copy(work / 'libbridge_emu.so', copy)
    L = bind(copy)
    L.emu_offer_lds(65536)
    c = ref.case('g7_nu1')
    before = L.emu_launches()
    got = call(L, c, jobs=np.array([(48, 64, 4, 50, 64, 32)], dtype=np.int32), rc=_native.SSRS_ERR_INVALID)
    assert b'ssrs_tracks_bridge' in L.ssrs_last_error() and b'156816 bytes of LDS' in L.ssrs_last_error() and \
        b'offers 65536' in L.ssrs_last_error()
    assert L.emu_launches() == before + 1, 'the scan ran, the gaps did not'
    assert (got['status'] == 99).all() and (got['g'] == -7.).all()
    # what fits is served
    short = np.array([(48, 64, 4, 50, 64, 20)], dtype=np.int32)
    ref.check(c, call(L, c, jobs=short), ref.score(c, short), jobs=short)
