"""K11 without a GPU: ssrs_amd/csrc/smooth.hip compiled with g++ against tests/hip_host_stub and run on the CPU, as
test_shelter_sector_emulation.py does for K9.  This exercises the kernels' own logic -- the reflected staging of the halo,
the transposed tile of the second pass, the register windows and their rotation, the two LDS capacities, the global path,
the weights' way into the workspace, the shared plane of a batch -- on the cases of tests/test_gpu_smooth.py.  On the CPU
every operation is IEEE f64 in the stated order, so `smooth` must also be tests/smooth_ref.py's statement of that order
bit for bit."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import smooth_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = {'auto': 0, 'lds': 1, 'global': 2}
SSRS_ERR_INVALID = -1
ERR_CPP = '''#include "common.h"
namespace ssrs {
char *error_buffer() { static thread_local char buf[512] = ""; return buf; }
int set_error(int code, const char *fmt, ...)
{ va_list ap; va_start(ap, fmt); vsnprintf(error_buffer(), 512, fmt, ap); va_end(ap); return code; }
}
extern "C" const char *ssrs_last_error(void) { return ssrs::error_buffer(); }
'''


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    work = tmp_path_factory.mktemp('smooth_emu')
    (work / 'err.cpp').write_text(ERR_CPP)
    lib = work / 'libsmooth_emu.so'
    csrc = os.path.join(ROOT, 'ssrs_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-ffp-contract=off', '-fPIC', '-shared', '-pthread',
                    '-I', os.path.join(ROOT, 'tests', 'hip_host_stub'), '-I', csrc, '-x', 'c++',
                    os.path.join(csrc, 'smooth.hip'), str(work / 'err.cpp'), '-o', str(lib)], check=True)
    L = C.CDLL(str(lib))
    L.ssrs_last_error.restype = C.c_char_p
    L.ssrs_smooth_workspace_bytes.restype = C.c_size_t
    L.ssrs_smooth_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double]
    L.ssrs_smooth_reflect.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def emu_smooth(L, x, sigma, path='auto', want=(True, True, True), min_val=ref.MIN_VAL, threshold=ref.THRESHOLD):
    """(smooth, orograph, usable) of a raster (rows, cols) or (B, rows, cols); None where not asked for."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    x3 = x if x.ndim == 3 else x[None]
    batch, rows, cols = x3.shape
    nbytes = L.ssrs_smooth_workspace_bytes(rows, cols, batch, sigma)
    assert nbytes == (8 * (ref.radius(sigma) + 1) + 255) // 256 * 256 + 8 * rows * cols       # does not grow with batch
    ws = np.full(nbytes // 8, np.nan)
    outs = [np.full(x3.shape, np.nan, dt) if w else None for w, dt in zip(want, (np.float64, np.float32, np.float64))]
    rc = L.ssrs_smooth_reflect(ptr(x3), sigma, PATHS[path], min_val, threshold, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                               rows, cols, batch, ptr(ws), nbytes, None)
    assert rc == 0, L.ssrs_last_error()
    return tuple(None if o is None else o.reshape(x.shape) for o in outs)


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize('name, shape, sigma, holes', ref.CASES, ids=ref.CASE_IDS)
def test_emulated_smoothing(emu, name, shape, sigma, holes):
    """Every case: within the bound of scipy, the clamp and the threshold function of the kernel's own sum, the bits of
    the stated order, and the same bits on every path that serves the radius."""
    x = ref.case_input(shape, holes)
    smooth, oro, use = emu_smooth(emu, x, sigma)
    ref.check_outputs(x, sigma, smooth, oro, use, name)
    assert same_bits(smooth, ref.kernel_order_smooth(x, sigma)), name
    for path in ('global',) + (('lds',) if ref.radius(sigma) <= ref.LDS_MAX_RADIUS else ()):
        other = emu_smooth(emu, x, sigma, path)
        assert all(same_bits(a, b) for a, b in zip((smooth, oro, use), other)), (name, path)
    if ref.radius(sigma) == 0:
        assert same_bits(smooth, ref.sanitised(x))                       # the identity, then the clamp
        assert (oro >= 0.).all() and (oro == 0.).any()


def test_emulated_clamp_lifted_and_raised(emu):
    x = ref.holed(ref.field((33, 65)))
    for min_val in (-np.inf, -0.25, 1.5):
        smooth, oro, use = emu_smooth(emu, x, 1.3, min_val=min_val)
        ref.check_outputs(x, 1.3, smooth, oro, use, f'min {min_val:g}', min_val=min_val)
    assert (emu_smooth(emu, x, 1.3, min_val=-np.inf)[1] < 0.).any()


def test_emulated_batch_of_3_equals_single_calls(emu):
    """The cases share the one f64 plane of the workspace, case after case."""
    for shape, sigma in (((70, 45), 8.), ((33, 65), 1.3), ((40, 50), 40.)):
        x = np.stack([ref.holed(ref.field(shape, seed)) for seed in range(3)])
        batch = emu_smooth(emu, x, sigma)
        for b in range(3):
            single = emu_smooth(emu, x[b], sigma)
            assert all(same_bits(g[b], s) for g, s in zip(batch, single)), (shape, b)


def test_emulated_null_outputs(emu):
    """Any of the three outputs may be NULL: the others keep their bits.  All NULL is refused."""
    x = ref.holed(ref.field((33, 65)))
    for sigma, path in ((8., 'lds'), (8., 'global')):
        full = emu_smooth(emu, x, sigma, path)
        for want in itertools.product((False, True), repeat=3):
            if not any(want):
                continue
            got = emu_smooth(emu, x, sigma, path, want=want)
            for w, g, f in zip(want, got, full):
                assert (g is None) if not w else same_bits(g, f), (path, want)
    ws = np.zeros(1 << 12)
    rc = emu.ssrs_smooth_reflect(ptr(x), 8., 0, 0., 0.75, None, None, None, 33, 65, 1, ptr(ws), ws.nbytes, None)
    assert rc == SSRS_ERR_INVALID and b'all NULL' in emu.ssrs_last_error()


def test_emulated_forced_lds_that_does_not_fit_is_refused(emu):
    x = ref.field((40, 50))
    ws, out = np.zeros(1 << 12), np.zeros((40, 50))
    rc = emu.ssrs_smooth_reflect(ptr(x), 40., PATHS['lds'], 0., 0.75, ptr(out), None, None, 40, 50, 1, ptr(ws), ws.nbytes, None)
    assert rc == SSRS_ERR_INVALID and b'does not fit' in emu.ssrs_last_error()
