"""The injected wind entries of `Simulator`, resolved on the host: every entry is checked and classified here, once,
before any device work (numpy only; nothing in this module touches the GPU or the native library)."""
from dataclasses import dataclass
from datetime import datetime as _datetime

import numpy as np
import torch

METHODS = ('nearest', 'linear', 'cubic')                       # scipy griddata's (reference: ssrs/config.py:44)
WIND_PAIR = ('wspeed', 'wdirn')                                # keys of Simulator.wtk_layers
THERMAL_LAYERS = ('pressure', 'temperature', 'blheight', 'surfheatflux')


def host_f64(a):
    """numpy / tensor / sequence -> numpy f64 on the host."""
    return np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


@dataclass
class Samples:
    """Fields of one wind case that share a form.
    'raster': x_km = y_km = None, values = the caller's own (rows, cols) objects (numpy or tensor, left where they are);
    'lattice': the axes x_km (nx,), y_km (ny,), values f64 (F, ny, nx);
    'scattered': the points x_km, y_km (npts,), values f64 (F, npts)."""
    form: str
    x_km: np.ndarray
    y_km: np.ndarray
    values: object

    def as_points(self):
        """A lattice as its meshgrid points (the reference triangulates whatever points it gets); others unchanged."""
        if self.form != 'lattice':
            return self
        x, y = (a.ravel() for a in np.meshgrid(self.x_km, self.y_km))
        return Samples('scattered', x, y, self.values.reshape(len(self.values), -1))

    def same_points(self, other):
        return np.array_equal(self.x_km, other.x_km) and np.array_equal(self.y_km, other.y_km)


@dataclass
class WindCase:
    case_id: str
    datetime: object
    wind: Samples
    thermal: Samples = None


def classify(fields, x_km, y_km, gridsize, case, group='the four thermal layers'):
    """`fields` = [(name, array), ...] of one case as `Samples`: with coordinates, (npts,) arrays are scattered samples and
    (ny, nx) arrays a lattice; arrays of shape `gridsize` are rasters.  ValueError names the case and the field that fits
    none of these, or that comes in another form than the first."""
    has_xy = x_km is not None and y_km is not None
    x = host_f64(x_km).ravel() if has_xy else None
    y = host_f64(y_km).ravel() if has_xy else None
    arrays, form0 = [], None
    for name, val in fields:
        shape = tuple(np.shape(val))
        if has_xy and shape == (x.size,) and x.size == y.size:
            form = 'scattered'
        elif has_xy and shape == (y.size, x.size):
            form = 'lattice'
        elif shape == tuple(gridsize):
            form = 'raster'
        else:
            raise ValueError(
                f'{case}: layer {name!r} has shape {shape}: expected a raster {tuple(gridsize)}' +
                (f', samples ({x.size},) at x_km / y_km or a lattice {(y.size, x.size)}' if has_xy else
                 ' (samples need x_km and y_km)'))
        if form != (form0 or form):
            raise ValueError(f'{case}: layer {name!r} is given as {form} but {fields[0][0]!r} as {form0}: {group} must '
                             'come in one form')
        form0 = form
        arrays.append(val if form == 'raster' else host_f64(val))
    if form0 == 'raster':
        return Samples('raster', None, None, arrays)
    return Samples(form0, x, y, np.stack(arrays))


def resolve_wind(wind, sim_mode, time_format, gridsize, wtk_interp_type, want_thermal, wtk_layers, project=None,
                 thermal_model='wtk'):
    """The `wind=` argument of Simulator as one `WindCase` per entry.  project(lon, lat) -> x_km, y_km serves entries
    whose samples sit at 'lon', 'lat' (degrees)."""
    if isinstance(wind, dict):
        wind = [dict(case_id=k, wspeed=v[0], wdirn=v[1]) for k, v in wind.items()]
    method = str(wtk_interp_type).lower()
    out = []
    for item in wind:
        dt = item.get('datetime')
        if dt is not None and not isinstance(dt, _datetime):
            dt = _datetime(*dt)
        case = item.get('case_id')
        if case is None:
            if dt is None:
                raise ValueError("each wind entry needs 'datetime' or 'case_id'")
            case = dt.strftime(time_format)                            # simulator.py:126
        x, y, to_km = item.get('x_km'), item.get('y_km'), None
        if 'lon' in item or 'lat' in item:
            x, y, to_km = _degrees(item, case, project)
        elif (x is None) != (y is None):
            raise ValueError(f"{case}: wind samples need both 'x_km' and 'y_km'")
        for name in WIND_PAIR:
            if item.get(name) is None:
                raise ValueError(f'{case}: the wind entry needs the layer {name!r} ({wtk_layers[name]})')
        group = classify([(name, item[name]) for name in WIND_PAIR], x, y, gridsize, case, "'wspeed' and 'wdirn'")
        if x is not None:
            # the reference hands wtk_interp_type to scipy's griddata ('nearest' | 'linear' | 'cubic',
            # simulator.py:774-775), which raises ValueError for anything else
            if method not in METHODS:
                raise ValueError(f'wtk_interp_type = {wtk_interp_type!r}: expected one of {METHODS}')
            if group.form == 'raster':
                raise ValueError(f"{case}: layers 'wspeed' / 'wdirn' are rasters {tuple(gridsize)} beside sample "
                                 'coordinates: with x_km / y_km (or lon / lat) the wind pair must be samples '
                                 f'({np.size(x)},) or a lattice {(np.size(y), np.size(x))}')
        entry = WindCase(case, dt, to_km(group) if to_km else group)
        if not (entry.wind.form == 'lattice' and method == 'linear'):      # (a lattice is not triangulated for 'linear')
            _need_three(case, 'wspeed', entry.wind, method)
        if want_thermal:
            for name in THERMAL_LAYERS:
                if item.get(name) is None:
                    raise ValueError(f"{case}: thermal_model = {thermal_model!r} needs the layer {name!r} "
                                     f'({wtk_layers[name]}) in every wind entry')
            group = classify([(name, item[name]) for name in THERMAL_LAYERS], x, y, gridsize, case)
            entry.thermal = to_km(group) if to_km else group
            _need_three(case, 'pressure', entry.thermal, method)
        out.append(entry)
    if sim_mode.lower() == 'snapshot' and len(out) != 1:
        raise ValueError('snapshot mode takes exactly one wind entry')
    return out


def _need_three(case, name, samples, method):
    npts = 3 if samples.form == 'raster' else samples.as_points().x_km.size
    if npts < 3 and method != 'nearest':
        raise ValueError(f"{case}: layer {name!r} has {npts} samples: 'linear' and 'cubic' need at least 3")


def _degrees(item, case, project):
    """A wind entry whose samples sit at 'lon', 'lat' (degrees) instead of 'x_km', 'y_km': the WTK points as they are
    delivered.  Scattered points (npts,) or the axes (nx,), (ny,) of a lattice whose arrays are (ny, nx).  Returns the
    coordinates to classify against and the function that turns the classified samples into scattered samples in
    kilometres from the centre of cell (0, 0) -- a lattice in degrees is no lattice on the projected grid."""
    if 'x_km' in item or 'y_km' in item:
        raise ValueError(f"{case}: the wind samples have both 'lon' / 'lat' and 'x_km' / 'y_km': give one pair")
    if 'lon' not in item or 'lat' not in item:
        raise ValueError(f"{case}: wind samples in degrees need both 'lon' and 'lat'")
    if project is None:
        raise ValueError(f"{case}: wind samples at 'lon', 'lat' need a projection")
    lon, lat = host_f64(item['lon']).ravel(), host_f64(item['lat']).ravel()
    if lon.size != lat.size and all(np.ndim(item.get(name)) != 2 for name in WIND_PAIR + THERMAL_LAYERS):
        raise ValueError(f"{case}: 'lon' has {lon.size} values and 'lat' {lat.size}: scattered samples need as many "
                         'of each, a lattice arrays of shape (lat, lon)')

    def to_km(samples):
        if samples.form == 'raster':
            return samples
        points = samples.as_points()
        x_km, y_km = project(points.x_km, points.y_km)
        return Samples('scattered', np.asarray(x_km), np.asarray(y_km), points.values)
    return lon, lat, to_km
