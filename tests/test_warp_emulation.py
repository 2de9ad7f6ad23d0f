"""K10 without a GPU: ssrs_amd/csrc/georef.hip compiled as plain C++ against tests/hip_host_stub (tests/
georef_emulation.cpp) and its kernel run on the CPU, one OS thread per GPU thread.  It checks the kernel's logic -- which
lane owns which cells, the scalar tail and the packed stores, the indices of the gather, missing pixels -- against the
NumPy restatement bit for bit (the same IEEE operations in the same order, x86 without contraction), and the inverse
projection within 1e-11 degrees.  It says nothing about the device's arithmetic or speed, and the uncovered count is
not checked here (a ballot of the emulation sees one lane): the gpu-marked tests cover those."""
import os
import subprocess

import numpy as np
import pytest

from ssrs_amd.csrc import build
from ssrs_amd.georef import Projection
from warp_ref import bilinear_ref, geometries, pixel_coordinates

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def emulation(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('warp_emu') / 'georef_emulation')
    subprocess.run([build.hipcc(), '-std=c++17', '-O1', '-ffp-contract=off', '-pthread', '-I', os.path.join(HERE, 'hip_host_stub'),
                    '-I', os.path.join(os.path.dirname(HERE), 'ssrs_amd', 'csrc'), '-x', 'c++',
                    os.path.join(HERE, 'georef_emulation.cpp'), '-o', exe], check=True)
    return exe


def test_kernel_logic_on_the_cpu(emulation, tmp_path):
    rng = np.random.default_rng(3)
    src_file, prefix = str(tmp_path / 'src.bin'), str(tmp_path / 'out')
    case = 0
    for overhang in (False, True):
        for geo in geometries(overhang):
            values = geo.values.copy()
            values[rng.random(values.shape) < 0.03] = -9999.
            # every destination over every source, twice; types, row order and alignment take turns
            for src_dtype, dst_dtype in ((np.float32, np.float64), (np.float64, np.float32)):
                north_up, offset = bool(case & 1), (case >> 1) & 1
                case += 1
                raster = geo.raster(src_dtype, north_up, values=values, nodata=-9999.)
                raster.data.tofile(src_file)
                args = [src_file, int(src_dtype == np.float64), *raster.shape, raster.lon0, raster.lat0, raster.dlon,
                        raster.dlat, -9999., geo.west, geo.south, geo.res, int(dst_dtype == np.float64), *geo.shape, prefix,
                        offset, *(getattr(geo.proj, f) for f in Projection.FIELDS[:8])]
                out = subprocess.run([emulation] + [repr(a) if isinstance(a, float) else str(a) for a in args],
                                     capture_output=True, text=True, timeout=120)
                assert out.returncode == 0, (out.returncode, out.stderr)
                dst = np.fromfile(prefix + '_dst.bin', dst_dtype).reshape(geo.shape)
                lon = np.fromfile(prefix + '_lon.bin').reshape(geo.shape)
                lat = np.fromfile(prefix + '_lat.bin').reshape(geo.shape)
                assert max(np.abs(lon - geo.lon).max(), np.abs(lat - geo.lat).max()) <= 1e-11
                want, _ = bilinear_ref(raster.data, *pixel_coordinates(raster, lon, lat), nodata=-9999.)
                assert np.array_equal(np.isnan(dst), np.isnan(want))
                assert bool(np.isnan(want).any()) and not bool(np.isnan(want).all())
                ok = ~np.isnan(want)
                assert np.array_equal(dst[ok], want.astype(dst_dtype)[ok])
    assert case == 16
