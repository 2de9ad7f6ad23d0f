"""The C-ABI library loads on a CPU-only box and exports every symbol that
include/ssrs_hip.h declares; argument validation runs before any GPU work."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    text = open(os.path.join(ROOT, 'include', 'ssrs_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(ssrs_[a-z0-9_]+)\s*\(', text)))


def header_code(name='ssrs_hip.h'):
    """include/ssrs_hip.h (or another header of include/) without comments and preprocessor lines."""
    text = open(os.path.join(ROOT, 'include', name)).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'//[^\n]*', '', text)
    return '\n'.join(line for line in text.splitlines() if not line.lstrip().startswith('#'))


def header_defines():
    """{name: value} of the header's integer `#define SSRS_...` lines."""
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ssrs_hip.h')).read(), flags=re.S)
    found = re.findall(r'^[ \t]*#[ \t]*define[ \t]+(SSRS_[A-Z0-9_]+)[ \t]+(\(?-?[0-9][0-9 <]*\)?)[ \t]*$', text, flags=re.M)
    return {name: eval(value, {'__builtins__': {}}) for name, value in found}


SCALARS = {'int': C.c_int, 'double': C.c_double, 'size_t': C.c_size_t, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64}
RETURNS = {'int': C.c_int, 'size_t': C.c_size_t, 'int64_t': C.c_int64, 'const char *': C.c_char_p,
           'SsrsTrajRecorder *': C.c_void_p, 'void': None}


# `ret ssrs_name(params);` -> (ret, name, params); tests/stream_order.py reads the parameter names with it
PROTOTYPE = r'([A-Za-z_][\w\s\*]*?)\b(ssrs_[a-z0-9_]+)\s*\(([^()]*)\)\s*;'


def declared_prototypes():
    """{name: (restype, [argtypes])} of every `ret ssrs_name(params);` of the header, by the rules of the binding: the five
    scalar kinds by value, every pointer parameter a void pointer.  A type outside that vocabulary is an error."""
    protos = {}
    for ret, name, params in re.findall(PROTOTYPE, header_code()):
        ret = ' '.join(ret.replace('*', ' * ').split())
        assert ret in RETURNS, f'{name}: return type {ret!r} is not in the binding\'s vocabulary'
        argtypes = []
        for param in [' '.join(p.split()) for p in params.split(',')]:
            if param == 'void' and ',' not in params:
                break
            if '*' in param:
                argtypes.append(C.c_void_p)
                continue
            ctype, _, pname = param.rpartition(' ')
            assert ctype in SCALARS and re.fullmatch(r'[A-Za-z_]\w*', pname), \
                f'{name}: parameter {param!r} is not in the binding\'s vocabulary'
            argtypes.append(SCALARS[ctype])
        assert name not in protos, f'{name} declared twice'
        protos[name] = (RETURNS[ret], argtypes)
    return protos


def test_prototypes_match_the_header():
    """Every export carries the restype and argtypes that include/ssrs_hip.h declares for it."""
    from ssrs_amd import _native
    lib = _native.lib()
    protos = declared_prototypes()
    assert len(protos) == 79
    assert sorted(protos) == declared_functions() == sorted(_native.EXPORTS)
    assert len(set(_native.EXPORTS)) == len(_native.EXPORTS)
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(argtypes), name
        assert list(fn.argtypes) == argtypes, name
        assert fn.restype is restype, name


def test_typed_calls_convert_and_refuse():
    """A bare Python float is converted where the header has a double, refused where it has an int, and an argument count
    that differs from the header's is refused; all on paths that return before any GPU work."""
    from ssrs_amd import _native
    lib = _native.lib()
    rc = lib.ssrs_slope_aspect(None, 1, 10., None, None, 1, 10, 10, None)
    assert rc == _native.SSRS_ERR_INVALID and b'dem is NULL' in lib.ssrs_last_error()
    with pytest.raises(C.ArgumentError):
        lib.ssrs_slope_aspect(None, 1, 10., None, None, 1, 10.5, 10, None)
    with pytest.raises(TypeError):
        lib.ssrs_slope_aspect(None, 1, 10., None, None, 1, 10, 10)
    p = _native.SsrsTrackParams()
    assert lib.ssrs_track_params_init(C.byref(p), 500, 600, 1, 1.0) == 0
    assert (p.rows, p.cols, p.burnin, p.max_moves) == (500, 600, 50, 75000)
    assert (p.memory_parameter, p.scaling_parameter) == (1, 1.0)
    assert lib.ssrs_track_params_init(C.byref(p), 31, 33, 3, 1.0) == 0
    assert (p.burnin, p.max_moves, p.memory_parameter) == (3, 256, 3)
    assert lib.ssrs_track_params_init(C.byref(p), 3, 600, 1, 1.0) == _native.SSRS_ERR_INVALID


def test_constants_match_the_header():
    """Every SSRS_* integer of ssrs_amd/_native.py, and every value of its SSRS_* dicts, is the header's #define."""
    from ssrs_amd import _native
    defines = header_defines()
    assert defines['SSRS_ERR_START'] == -3 and defines['SSRS_ALLEN_MAX_UPDRAFTS'] == 1 << 22      # the parser's own check
    prefixes = {'SSRS_RAY_AXES': 'SSRS_RAY_', 'SSRS_SHELTER_PATH': 'SSRS_SHELTER_', 'SSRS_SMOOTH_PATH': 'SSRS_SMOOTH_',
                'SSRS_ALLEN_PATH': 'SSRS_ALLEN_', 'SSRS_INTERP': 'SSRS_INTERP_'}
    mirrored = {}
    for name, value in vars(_native).items():
        if not name.startswith('SSRS_'):
            continue
        if isinstance(value, dict):
            assert name in prefixes, f'{name}: a dict of constants this test does not know'
            mirrored.update({prefixes[name] + key.upper(): v for key, v in value.items()})
        else:
            assert isinstance(value, int), name
            mirrored[name] = value
    for name in ('SSRS_TRACKS_THR_TABLE', 'SSRS_TURBINE_BIN', 'SSRS_TURBINE_MAX', 'SSRS_ROTOR_TIMED_LDS_TURBINES',
                 'SSRS_OCCUPANCY_MAX_PLANES', 'SSRS_ALTITUDE_TILE', 'SSRS_ALLEN_MAX_UPDRAFTS', 'SSRS_ALLEN_TABLE_COLS',
                 'SSRS_ALLEN_GLOBAL', 'SSRS_SHELTER_LDS', 'SSRS_SMOOTH_AUTO', 'SSRS_RAY_ROW_EAST', 'SSRS_INTERP_CUBIC'):
        assert name in mirrored, name
    for name, value in mirrored.items():
        assert name in defines, f'{name} of _native.py is no #define of the header'
        assert value == defines[name], (name, value, defines[name])


def test_header_symbols_are_exported():
    from ssrs_amd import _native
    lib = _native.lib()
    names = declared_functions()
    assert len(names) >= 18
    for name in names:
        assert hasattr(lib, name), f'{name} declared in ssrs_hip.h but not exported'
    assert sorted(_native.EXPORTS) == names, 'ssrs_amd._native.EXPORTS out of sync with the header'


def test_version_and_error_text():
    from ssrs_amd import _native
    lib = _native.lib()
    assert lib.ssrs_version() == 109
    assert isinstance(lib.ssrs_last_error(), bytes)


def test_threshold_table_size_includes_its_guard_bands():
    """Eight planes at a power-of-two stride between two guard bands of (cols + 2) entries, rounded up to
    256 bytes (the stepper's speculative gathers of boundary cells land there); a table too large for
    32-bit offsets is refused by the builder."""
    from ssrs_amd import _native
    lib = _native.lib()
    lib.ssrs_transition_thr_bytes.restype = C.c_size_t
    for rows, cols in ((5000, 6000), (96, 128), (5, 5)):
        stride = 256
        while stride < rows * cols * 4:
            stride *= 2
        guard = -(-(cols + 2) * 4 // 256) * 256
        assert lib.ssrs_transition_thr_bytes(rows, cols) == 8 * stride + 2 * guard
    assert lib.ssrs_transition_thr_bytes(0, 10) == 0
    dummy = (C.c_double * 9)()
    buf = (C.c_char * 64)()
    rc = lib.ssrs_transition_thr_build(buf, None, dummy, buf, 9000, 9000, None)      # 8.1e7 cells > 2^26
    assert rc == _native.SSRS_ERR_INVALID and b'2^26' in lib.ssrs_last_error()


def test_argument_validation_needs_no_gpu():
    from ssrs_amd import _native
    lib = _native.lib()
    rc = lib.ssrs_slope_aspect(None, 1, C.c_double(10.), None, None, 1, 10, 10, None)
    assert rc == _native.SSRS_ERR_INVALID and b'dem is NULL' in lib.ssrs_last_error()
    rc = lib.ssrs_threshold_updraft(None, C.c_double(0.75), None, C.c_size_t(4), None)
    assert rc == _native.SSRS_ERR_INVALID
    p = _native.SsrsTrackParams()
    assert lib.ssrs_track_params_init(C.byref(p), 500, 600, 1, C.c_double(1.0)) == 0
    assert (p.rows, p.cols, p.burnin, p.max_moves) == (500, 600, 50, 75000)
    assert lib.ssrs_track_params_init(C.byref(p), 5000, 6000, 1, C.c_double(1.0)) == 0
    assert (p.burnin, p.max_moves) == (500, 7500000)
    assert lib.ssrs_track_params_init(C.byref(p), 31, 33, 3, C.c_double(1.0)) == 0
    assert (p.burnin, p.max_moves, p.memory_parameter) == (3, 256, 3)    # ceil(255.75)
    assert lib.ssrs_track_params_init(C.byref(p), 3, 600, 1, C.c_double(1.0)) == _native.SSRS_ERR_INVALID
    p.memory_parameter = 9
    rc = lib.ssrs_tracks_simulate(C.byref(p), None, None, None, None, C.c_int64(1), C.c_uint64(0),
                                  C.c_uint64(0), None, None, None, None, None, None,
                                  C.c_size_t(0), None, None)
    assert rc == _native.SSRS_ERR_INVALID
    with pytest.raises(ValueError):
        _native.check(rc)


def test_roam_tables_selftest_refuses_before_any_gpu_work():
    from ssrs_amd import _native
    lib = _native.lib()
    prior = (C.c_double * 9)()
    words = (C.c_uint32 * 38)()
    raw = (C.c_char * 256)()
    base = C.addressof(raw)
    a64 = (base + 63) // 64 * 64                       # a 64-byte aligned address inside `raw` (never dereferenced)

    def call(updraft=a64, potential=None, prior=C.addressof(prior), thr=a64, rows=8, cols=8, pair=a64, fine=a64):
        return lib.ssrs_roam_tables_selftest(updraft, potential, prior, thr, rows, cols, pair, fine, C.addressof(words), None)

    for kw in ({'updraft': None}, {'prior': None}, {'thr': None}, {'pair': None}, {'fine': None}):
        assert call(**kw) == _native.SSRS_ERR_INVALID and b'is NULL' in lib.ssrs_last_error(), kw
    for kw in ({'rows': 2}, {'cols': 2}):
        assert call(**kw) == _native.SSRS_ERR_INVALID and b'rows, cols >= 3' in lib.ssrs_last_error(), kw
    assert call(rows=8192, cols=4097) == _native.SSRS_ERR_INVALID and b'2^25' in lib.ssrs_last_error()
    assert call(thr=a64 + 32) == _native.SSRS_ERR_INVALID and b'64-byte aligned' in lib.ssrs_last_error()
    assert call(pair=a64 + 8) == _native.SSRS_ERR_INVALID and b'16-byte aligned' in lib.ssrs_last_error()
    assert call(fine=a64 + 8) == _native.SSRS_ERR_INVALID and b'16-byte aligned' in lib.ssrs_last_error()
    assert list(words) == [0] * 38                     # nothing was written either


def test_product_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    import numpy as np
    from ssrs_amd import layers
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        layers.compute_slope_degrees(np.zeros((8, 8)), 10.)


def test_ctypes_structs_match_the_header(tmp_path):
    """The header's structs, compiled as plain C (gcc), have the size and field offsets of
    their ctypes mirrors in ssrs_amd/_native.py."""
    import ctypes, shutil, subprocess
    from ssrs_amd import _native as nat
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    bodies = dict(re.findall(r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}', header_code(), flags=re.S))
    assert {'SsrsTrackParams', 'SsrsTrackStats', 'SsrsSolveStats', 'SsrsShelterParams', 'SsrsProjection',
            'SsrsAltitudeParams', 'SsrsFlightTimeParams'} <= set(bodies)
    structs = {}
    for name, body in bodies.items():
        assert hasattr(nat, name), f'struct {name} of ssrs_hip.h has no ctypes mirror in ssrs_amd/_native.py'
        structs[name] = getattr(nat, name)
        declared = [re.sub(r'\[.*', '', f.split()[-1]) for decl in body.split(';') if decl.strip() for f in decl.split(',')]
        assert [f for f, _ in structs[name]._fields_] == declared, name
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssrs_hip.h"', 'int main(void) {']
    for name, cls in structs.items():
        lines.append(f'  printf("{name} %zu", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf(" %zu", offsetof({name}, {field}));')
        lines.append('  printf("\\n");')
    lines += ['  return 0;', '}']
    src = tmp_path / 'abi.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'abi'
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', inc, str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for line in out:
        name, size, *offsets = line.split()
        cls = structs[name]
        assert int(size) == ctypes.sizeof(cls), name
        assert [int(o) for o in offsets] == [getattr(cls, f).offset for f, _ in cls._fields_], name


def test_graft_entry_build_checks_the_headers_version():
    """__graft_entry__.build() compares the library with the version include/ssrs_hip.h declares (it used to carry a literal
    that two ABI bumps of round 4 left behind: the driver's build check would have failed)."""
    import os, re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, '__graft_entry__.py')).read()
    assert 'SSRS_VERSION' in src and not re.search(r'ssrs_version\(\)\s*==\s*\d', src)
    from ssrs_amd import _native
    declared = int(re.search(r'#define\s+SSRS_VERSION\s+(\d+)', open(os.path.join(root, 'include', 'ssrs_hip.h')).read()).group(1))
    assert _native.lib().ssrs_version() == declared
