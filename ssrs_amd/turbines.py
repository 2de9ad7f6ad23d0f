"""Wind turbines (K8 host side): `Turbines`, the injected stand-in for the reference's TurbinesUSWTB
(ssrs/turbines.py there; the USWTDB download stays out of scope, its `xlong` / `ylat` columns are projected by
`with_projected_columns` in a georeferenced run), and the
encounter pass of the trajectories against them -- which simulated tracks came within R of which turbine, and
after how many moves (include/ssrs_hip.h "turbines").
"""

import numpy as np
import torch

from . import _native as nat
from ._device import device, stream_ptr, to_dev, is_tensor

BIN = nat.SSRS_TURBINE_BIN
MAX_TURBINES = nat.SSRS_TURBINE_MAX


class Turbines:
    """Turbine table with the query methods of TurbinesUSWTB.

    data: dict of equally long columns, a pandas DataFrame or another `Turbines`.  Columns `x`, `y` are projected
    metres in the frame of `Simulator(origin=...)`; `p_name` (project), `t_hh` (hub height, m) and `t_rd` (rotor
    diameter, m) are optional, anything else is carried along.  The constructor filters like turbines.py:68-71:
    x within [bounds[0], bounds[2]] and y within [bounds[1], bounds[3]], both ends included, and -- when `t_hh` is
    given -- min_hubheight <= t_hh < 10000.  bounds=None keeps every position.  pandas is never imported
    unless `dframe` is asked for."""

    def __init__(self, data, bounds=None, min_hubheight: float = 50., print_verbose: bool = False):
        if isinstance(data, Turbines):
            cols = dict(data.columns)
        elif hasattr(data, 'columns') and hasattr(data, 'to_numpy'):            # a DataFrame, without importing pandas
            cols = {str(name): data[name].to_numpy() for name in data.columns}
        elif isinstance(data, dict):
            cols = {str(name): np.asarray(val) for name, val in data.items()}
        else:
            raise TypeError(f'turbines: expected a dict of columns, a DataFrame or a Turbines, not {type(data).__name__}')
        for name in ('x', 'y'):
            if name not in cols:
                raise ValueError(f"turbines: column {name!r} is missing (projected metres, the frame of origin=)")
            cols[name] = np.asarray(cols[name], dtype=np.float64).reshape(-1)
        n = cols['x'].size
        for name, val in cols.items():
            if np.ndim(val) != 1 or np.shape(val)[0] != n:
                raise ValueError(f'turbines: column {name!r} has shape {np.shape(val)}, expected ({n},)')
        keep = np.ones(n, dtype=bool)
        if bounds is not None:
            keep &= (cols['x'] >= bounds[0]) & (cols['x'] <= bounds[2])         # between(..., 'both')
            keep &= (cols['y'] >= bounds[1]) & (cols['y'] <= bounds[3])
        if 't_hh' in cols:
            hh = np.asarray(cols['t_hh'], dtype=np.float64)
            keep &= (hh >= float(min_hubheight)) & (hh < 10000.)                # between(min, 10000., 'left')
        self.columns = {name: val[keep] for name, val in cols.items()}
        if print_verbose:
            self.print_details()

    def __len__(self):
        return int(self.columns['x'].size)

    @property
    def dframe(self):
        """The table as a pandas DataFrame (the reference's attribute)."""
        import pandas as pd
        return pd.DataFrame(self.columns)

    def get_locations(self):
        """(x, y) of every turbine (turbines.py:80-83)."""
        return self.columns['x'], self.columns['y']

    def _project(self, pname):
        if 'p_name' not in self.columns:
            raise KeyError('p_name')
        return self.columns['p_name'] == pname

    def get_locations_for_this_project(self, pname: str):
        """(x, y) of the turbines of one project (turbines.py:85-91); empty arrays for an unknown name."""
        sel = self._project(pname)
        return self.columns['x'][sel], self.columns['y'][sel]

    def get_project_names(self):
        """Project names in order of first appearance (pandas' unique(), turbines.py:93-95)."""
        if 'p_name' not in self.columns:
            raise KeyError('p_name')
        names = self.columns['p_name']
        _, first = np.unique(names, return_index=True)
        return names[np.sort(first)]

    def cell_coordinates(self, bounds, resolution):
        """(n, 2) f64 [x, y] in cell units relative to the centre of cell (0, 0): x along columns, y along rows."""
        x, y = self.get_locations()
        return np.stack([(x - float(bounds[0])) / float(resolution), (y - float(bounds[1])) / float(resolution)], 1)

    def print_details(self):
        if len(self) == 0:
            print('Turbines: No wind turbines found within the bounds!')
            return
        if 'p_name' in self.columns:
            print(f'Number of projects: {self.get_project_names().size}')
        print(f'Number of turbines: {len(self)}')
        for name, label in (('t_hh', 'Hub height'), ('t_rd', 'Rotor Dia')):
            if name in self.columns:
                v = np.asarray(self.columns[name], dtype=np.float64)
                print(f'{label} (min,median,max): {v.min()}, {np.median(v)}, {v.max()}')


def _column_names(data):
    if isinstance(data, Turbines):
        return list(data.columns)
    if isinstance(data, dict) or (hasattr(data, 'columns') and hasattr(data, 'to_numpy')):
        return [str(name) for name in (data if isinstance(data, dict) else data.columns)]
    return []


def has_lonlat_only(data):
    """A table with the USWTDB position columns `xlong`, `ylat` (degrees) and neither `x` nor `y`."""
    names = _column_names(data)
    return 'xlong' in names and 'ylat' in names and 'x' not in names and 'y' not in names


def with_projected_columns(data, projection):
    """The columns of such a table plus `x`, `y` = projection.forward(xlong, ylat), as a dict (turbines.py:52-62 of
    the reference); the degrees are carried along."""
    if isinstance(data, Turbines):
        data = data.columns
    cols = {name: np.asarray(data[name].to_numpy() if hasattr(data[name], 'to_numpy') else data[name])
            for name in _column_names(data)}
    lon, lat = (np.asarray(cols[name], dtype=np.float64).reshape(-1) for name in ('xlong', 'ylat'))
    if lon.shape != lat.shape:
        raise ValueError(f'turbines: xlong has {lon.size} values, ylat {lat.size}')
    cols['x'], cols['y'] = projection.forward(lon, lat)
    return cols


def windplant_window(xloc, yloc, pad, bounds, resolution, gridsize):
    """(r0, r1, c0, c1), ends exclusive: the cells whose centres (bounds[0] + c * res, bounds[1] + r * res) lie in
    [min(x) - pad, max(x) + pad] x [min(y) - pad, max(y) + pad] (the axis limits of simulator.py:589-590), clipped
    to the raster by construction.  ValueError when there is no such cell."""
    xloc, yloc = np.asarray(xloc, dtype=np.float64), np.asarray(yloc, dtype=np.float64)
    if xloc.size == 0:
        raise ValueError('windplant window: no turbine locations')
    out = []
    for origin, n, loc in ((bounds[1], gridsize[0], yloc), (bounds[0], gridsize[1], xloc)):
        centres = float(origin) + np.arange(int(n)) * float(resolution)
        inside = np.nonzero((centres >= loc.min() - pad) & (centres <= loc.max() + pad))[0]
        if inside.size == 0:
            raise ValueError('windplant window: it holds no cell of the raster')
        out += [int(inside[0]), int(inside[-1]) + 1]
    return tuple(out)


def build_bins(xy_cells, radius_cells, gridshape):
    """The cull lists of ssrs_turbine_encounters / ssrs_rotor_encounters: (bin_start int32 (nbr * nbc + 1), bin_items
    int32), a CSR over bins of 32 x 32 cells listing, in ascending order, the turbines whose disk can reach a cell of the
    bin.  radius_cells: one radius for all (a negative or NaN one raises), or one per turbine (nturb,) -- there a NaN or
    negative entry puts its turbine in no list.
    Conservative: the disk's bounding box, one cell wider on every side than the real numbers ask for (the exact
    test rounds c - xt before it squares), against the bin's cells.  A turbine with a NaN coordinate is in no list."""
    rows, cols = int(gridshape[0]), int(gridshape[1])
    xy = np.asarray(xy_cells, dtype=np.float64).reshape(-1, 2)
    if np.ndim(radius_cells) == 0:
        if not float(radius_cells) >= 0.:
            raise ValueError(f'radius_cells = {radius_cells!r}: expected a number >= 0')
        radius = np.full(xy.shape[0], float(radius_cells))
    else:
        radius = np.asarray(radius_cells, dtype=np.float64).reshape(-1)
        if radius.shape != (xy.shape[0],):
            raise ValueError(f'radius_cells has {radius.size} entries for {xy.shape[0]} turbines')
        radius = np.where(radius >= 0., radius, np.nan)          # (NaN travels through the box below into `ok`)
    nbr, nbc = -(-rows // BIN), -(-cols // BIN)
    bins, items = [], []
    # first / last cell of the widened box, clipped to the raster (in floats first: coordinates may be huge)
    c_lo = np.clip(np.floor(xy[:, 0] - radius) - 1, 0, cols)
    c_hi = np.clip(np.ceil(xy[:, 0] + radius) + 1, -1, cols - 1)
    r_lo = np.clip(np.floor(xy[:, 1] - radius) - 1, 0, rows)
    r_hi = np.clip(np.ceil(xy[:, 1] + radius) + 1, -1, rows - 1)
    ok = ~(np.isnan(c_lo) | np.isnan(c_hi) | np.isnan(r_lo) | np.isnan(r_hi))
    for t in np.nonzero(ok)[0]:
        c0, c1, r0, r1 = int(c_lo[t]), int(c_hi[t]), int(r_lo[t]), int(r_hi[t])
        if c0 > c1 or r0 > r1:
            continue
        br = np.arange(r0 // BIN, r1 // BIN + 1, dtype=np.int64)
        bc = np.arange(c0 // BIN, c1 // BIN + 1, dtype=np.int64)
        b = (br[:, None] * nbc + bc[None, :]).ravel()
        bins.append(b)
        items.append(np.full(b.size, t, dtype=np.int32))
    bins = np.concatenate(bins) if bins else np.zeros(0, dtype=np.int64)
    items = np.concatenate(items) if items else np.zeros(0, dtype=np.int32)
    if bins.size >= 2 ** 31:
        raise ValueError(f'build_bins: {bins.size} list entries do not fit int32 (radius_cells up to {np.nanmax(radius)})')
    order = np.argsort(bins, kind='stable')                # turbines were appended in ascending order
    bin_start = np.zeros(nbr * nbc + 1, dtype=np.int64)
    np.cumsum(np.bincount(bins, minlength=nbr * nbc), out=bin_start[1:])
    return bin_start.astype(np.int32), np.ascontiguousarray(items[order], dtype=np.int32)


def _check_bins(bin_start, bin_items, nbins, nturb):
    bs, bi = np.asarray(bin_start), np.asarray(bin_items)
    if bs.shape != (nbins + 1,) or bi.ndim != 1:
        raise ValueError(f'bins: bin_start has shape {bs.shape}, expected ({nbins + 1},) for this raster')
    if bs[0] != 0 or bs[-1] != bi.size or (np.diff(bs) < 0).any():
        raise ValueError('bins: bin_start must ascend from 0 to len(bin_items)')
    if bi.size and (bi.min() < 0 or bi.max() >= nturb):
        raise ValueError(f'bins: bin_items outside [0, {nturb})')


def turbine_encounters(traj, offsets, xy_cells, radius_cells, gridshape, bins=None, hits=None, first_step=None):
    """ssrs_turbine_encounters on device tensors.  traj int16 (points, 2) and offsets int64 (ntracks + 1) as
    movmodel.simulate_tracks / TrackBatch.iter_device_chunks() give them (`offsets` may be a slice of a longer
    vector: its first entry need not be 0); xy_cells (nturb, 2) f64 in cell units (Turbines.cell_coordinates).
    bins: (bin_start, bin_items) of build_bins, numpy (checked) or int32 device tensors (trusted); built here when
    None.  hits: int32 tensor (ntracks, ceil(nturb / 32)) holding the uint32 bitmap, ORed into when given;
    first_step: int32 (ntracks), min-ed into when given (-1 = none).  Returns (hits, first_step)."""
    rows, cols = int(gridshape[0]), int(gridshape[1])
    xy = xy_cells if is_tensor(xy_cells) else np.asarray(xy_cells, dtype=np.float64).reshape(-1, 2)
    xy = to_dev(xy, torch.float64).reshape(-1, 2)
    nturb = int(xy.shape[0])
    if not 1 <= nturb <= MAX_TURBINES:
        raise ValueError(f'turbine_encounters: {nturb} turbines, expected 1 to {MAX_TURBINES}')
    off = to_dev(offsets, torch.int64).reshape(-1)
    ntracks = int(off.numel()) - 1
    if ntracks < 0:
        raise ValueError('turbine_encounters: offsets needs at least one entry')
    pts = to_dev(traj, torch.int16).reshape(-1, 2)
    words = (nturb + 31) // 32
    dev = device()
    if hits is None:
        hits = torch.zeros((ntracks, words), dtype=torch.int32, device=dev)
    if first_step is None:
        first_step = torch.full((ntracks,), -1, dtype=torch.int32, device=dev)
    if hits.dtype != torch.int32 or tuple(hits.shape) != (ntracks, words) or not hits.is_contiguous() or not hits.is_cuda:
        raise ValueError(f'turbine_encounters: hits must be a contiguous int32 device tensor ({ntracks}, {words})')
    if first_step.dtype != torch.int32 or tuple(first_step.shape) != (ntracks,) or not first_step.is_contiguous() \
            or not first_step.is_cuda:
        raise ValueError(f'turbine_encounters: first_step must be a contiguous int32 device tensor ({ntracks},)')
    nbins = -(-rows // BIN) * -(-cols // BIN)
    if bins is None:
        bins = build_bins(xy.cpu().numpy(), radius_cells, gridshape)
    if not is_tensor(bins[0]):
        _check_bins(bins[0], bins[1], nbins, nturb)
    bin_start, bin_items = to_dev(bins[0], torch.int32), to_dev(bins[1], torch.int32)
    if int(bin_start.numel()) != nbins + 1:
        raise ValueError(f'bins: bin_start has {bin_start.numel()} entries, expected {nbins + 1} for this raster')
    if ntracks == 0 or pts.numel() == 0 or bin_items.numel() == 0:
        # nothing to read, or no disk reaches the raster (empty tensors have no address to hand over); the radius
        # is still the library's to judge
        if not float(radius_cells) >= 0.:
            raise ValueError(f'radius_cells = {radius_cells!r}: expected a number >= 0')
        return hits, first_step
    nat.check(nat.lib().ssrs_turbine_encounters(
        nat.ptr(pts), nat.ptr(off), ntracks, nat.ptr(xy), nturb, float(radius_cells),
        nat.ptr(bin_start), nat.ptr(bin_items), rows, cols, nat.ptr(hits), nat.ptr(first_step), stream_ptr()))
    return hits, first_step


def encounter_counts(hits, nturb):
    """ssrs_turbine_encounter_counts: (tracks_per_turbine int64 (nturb), turbines_per_track int32 (ntracks)),
    device tensors, from the bitmap of turbine_encounters."""
    h = to_dev(hits, torch.int32)
    nturb = int(nturb)
    ntracks = int(h.shape[0])
    if h.dim() != 2 or int(h.shape[1]) != (nturb + 31) // 32:
        raise ValueError(f'encounter_counts: hits has shape {tuple(h.shape)}, expected (ntracks, {(nturb + 31) // 32})')
    per_turbine = torch.zeros(nturb, dtype=torch.int64, device=h.device)
    per_track = torch.zeros(ntracks, dtype=torch.int32, device=h.device)
    if ntracks:
        nat.check(nat.lib().ssrs_turbine_encounter_counts(
            nat.ptr(h), ntracks, nturb, nat.ptr(per_turbine), nat.ptr(per_track), stream_ptr()))
    return per_turbine, per_track


def base_cells(xy_cells, gridshape):
    """(rb, cb, known): the cell a turbine stands on -- the nearest one, clamped into the raster -- and whether both of its
    coordinates are numbers (rb = cb = 0 where not)."""
    rows, cols = int(gridshape[0]), int(gridshape[1])
    xy = np.asarray(xy_cells, dtype=np.float64).reshape(-1, 2)
    known = ~np.isnan(xy).any(1)
    rb = np.clip(np.rint(np.where(known, xy[:, 1], 0.)), 0, rows - 1).astype(np.int64)
    cb = np.clip(np.rint(np.where(known, xy[:, 0], 0.)), 0, cols - 1).astype(np.int64)
    return rb, cb, known


def _mm(metres):
    """rint(1000 x) as int64, NaN -> 0 (the caller masks it), clipped far inside int64."""
    with np.errstate(invalid='ignore'):
        v = np.clip(np.rint(1000. * np.asarray(metres, dtype=np.float64)), -2. ** 62, 2. ** 62)
    return np.where(np.isnan(v), 0., v).astype(np.int64)


def rotor_geometry(turbines, dem, bounds, resolution, clearance=0.):
    """The cylinders of ssrs_rotor_encounters from a `Turbines` with `t_hh` and `t_rd`: (reach f64 (nturb,) in cells, zband
    int32 (nturb, 2) in mm above the DEM's datum).  rad = t_rd / 2 + clearance metres; reach = rad / resolution; the band
    is [base + mm(t_hh - rad), base + mm(t_hh + rad)] with mm(x) = rint(1000 x), summed in int64 and clipped to int32,
    where base is the elevation of the cell the turbine stands on (base_cells) by cellinfo's own formula,
    clip(rint(1000 z), +-2^30).  A NaN base (nodata), t_hh or t_rd gives the empty band (1, 0) and reach = NaN: such a
    turbine is hit by nothing.  dem: numpy or a device tensor (rows, cols); only nturb of its values are gathered."""
    missing = [name for name in ('t_hh', 't_rd') if name not in turbines.columns]
    if missing:
        raise ValueError(f'rotor_geometry: the turbines have no column {" / ".join(missing)} '
                         '(t_hh = hub height, t_rd = rotor diameter, metres)')
    resolution, clearance = float(resolution), float(clearance)
    if not resolution > 0. or clearance != clearance:
        raise ValueError(f'rotor_geometry: resolution = {resolution!r}, clearance = {clearance!r} (resolution > 0)')
    if len(np.shape(dem)) != 2:
        raise ValueError(f'rotor_geometry: dem has shape {tuple(np.shape(dem))}, expected (rows, cols)')
    rb, cb, known = base_cells(turbines.cell_coordinates(bounds, resolution), np.shape(dem))
    if is_tensor(dem):
        z = dem[torch.from_numpy(rb).to(dem.device), torch.from_numpy(cb).to(dem.device)].cpu().numpy()
    else:
        z = np.asarray(dem)[rb, cb]
    z = np.where(known, z.astype(np.float64), np.nan)
    hh = np.asarray(turbines.columns['t_hh'], dtype=np.float64)
    rad = np.asarray(turbines.columns['t_rd'], dtype=np.float64) / 2. + clearance
    empty = np.isnan(z) | np.isnan(hh) | np.isnan(rad)
    base = np.clip(_mm(z), -2 ** 30, 2 ** 30)
    i32 = np.iinfo(np.int32)
    z_lo = np.clip(base + _mm(hh - rad), i32.min, i32.max)
    z_hi = np.clip(base + _mm(hh + rad), i32.min, i32.max)
    zband = np.stack([np.where(empty, 1, z_lo), np.where(empty, 0, z_hi)], 1).astype(np.int32)
    return np.where(empty, np.nan, rad / resolution), zband


def rotor_encounters(traj, alt, offsets, cellinfo, xy_cells, reach, zband, gridshape, bins=None, hits=None, first_step=None,
                     points=None, dt=None, time=None):
    """ssrs_rotor_encounters on device tensors (K15): the tracks through every turbine's own cylinder, and the points inside
    it.  traj, offsets, xy_cells, bins, hits and first_step as turbine_encounters takes them; alt int32 (points) as
    flight.compute_track_altitudes(want_alt=True) gives it, indexed like traj; cellinfo of flight.altitude_cellinfo; reach
    (nturb,) f64 and zband (nturb, 2) int32 of rotor_geometry.  bins are built here from `reach` when None.  points: int64
    device tensor (nturb,), ADDED to when given (the exposure).  first_step=False / points=False leave that output out
    (None is returned in its place).  Returns (hits, first_step, points).
    dt: int32 (points) as flight.compute_track_times(want_dt=True) gives it, indexed like traj: the call is then
    ssrs_rotor_encounters_timed and returns (hits, first_step, points, time); time: int64 device tensor (nturb,) holding
    uint64 microseconds, ADDED to when given and created zero otherwise -- the dt of the points inside each cylinder."""
    who = 'rotor_encounters'
    rows, cols = int(gridshape[0]), int(gridshape[1])
    xy = xy_cells if is_tensor(xy_cells) else np.asarray(xy_cells, dtype=np.float64).reshape(-1, 2)
    xy = to_dev(xy, torch.float64).reshape(-1, 2)
    nturb = int(xy.shape[0])
    if not 1 <= nturb <= MAX_TURBINES:
        raise ValueError(f'{who}: {nturb} turbines, expected 1 to {MAX_TURBINES}')
    reach_dev = to_dev(reach if is_tensor(reach) else np.asarray(reach, dtype=np.float64), torch.float64).reshape(-1)
    zband_dev = to_dev(zband if is_tensor(zband) else np.asarray(zband, dtype=np.int32), torch.int32)
    if int(reach_dev.numel()) != nturb or tuple(zband_dev.shape) != (nturb, 2):
        raise ValueError(f'{who}: reach has {reach_dev.numel()} entries and zband shape {tuple(zband_dev.shape)} for '
                         f'{nturb} turbines, expected ({nturb},) and ({nturb}, 2)')
    off = to_dev(offsets, torch.int64).reshape(-1)
    ntracks = int(off.numel()) - 1
    if ntracks < 0:
        raise ValueError(f'{who}: offsets needs at least one entry')
    pts = to_dev(traj, torch.int16).reshape(-1, 2)
    heights = to_dev(alt, torch.int32).reshape(-1)
    if int(heights.numel()) != int(pts.shape[0]):
        raise ValueError(f'{who}: alt has {heights.numel()} entries for {pts.shape[0]} points (it is indexed like traj)')
    if dt is None and time is not None:
        raise ValueError(f'{who}: time is given without dt (the exposure time is summed from dt)')
    if dt is not None:
        if (dt.dtype != torch.int32) if is_tensor(dt) else (np.asarray(dt).dtype != np.int32):
            raise ValueError(f'{who}: dt must be int32 microseconds indexed like traj (compute_track_times(want_dt=True))')
        moves = to_dev(dt, torch.int32).reshape(-1)
        if int(moves.numel()) != int(pts.shape[0]):
            raise ValueError(f'{who}: dt has {moves.numel()} entries for {pts.shape[0]} points (it is indexed like traj)')
    if not is_tensor(cellinfo) or cellinfo.dtype != torch.int32 or tuple(cellinfo.shape) != (rows, cols, 2) or \
            not cellinfo.is_contiguous() or not cellinfo.is_cuda:
        raise ValueError(f'{who}: cellinfo must be a contiguous int32 device tensor ({rows}, {cols}, 2) (altitude_cellinfo)')
    words = (nturb + 31) // 32
    dev = device()
    if dt is not None and time is None:
        time = torch.zeros(nturb, dtype=torch.int64, device=dev)
    if dt is not None and (not is_tensor(time) or time.dtype != torch.int64 or tuple(time.shape) != (nturb,) or
                           not time.is_contiguous() or not time.is_cuda):
        raise ValueError(f'{who}: time must be a contiguous int64 device tensor ({nturb},)')
    if hits is None:
        hits = torch.zeros((ntracks, words), dtype=torch.int32, device=dev)
    if first_step is None:
        first_step = torch.full((ntracks,), -1, dtype=torch.int32, device=dev)
    if points is None:
        points = torch.zeros(nturb, dtype=torch.int64, device=dev)
    first_step = None if first_step is False else first_step
    points = None if points is False else points
    if hits.dtype != torch.int32 or tuple(hits.shape) != (ntracks, words) or not hits.is_contiguous() or not hits.is_cuda:
        raise ValueError(f'{who}: hits must be a contiguous int32 device tensor ({ntracks}, {words})')
    if first_step is not None and (first_step.dtype != torch.int32 or tuple(first_step.shape) != (ntracks,) or
                                   not first_step.is_contiguous() or not first_step.is_cuda):
        raise ValueError(f'{who}: first_step must be a contiguous int32 device tensor ({ntracks},)')
    if points is not None and (points.dtype != torch.int64 or tuple(points.shape) != (nturb,) or
                               not points.is_contiguous() or not points.is_cuda):
        raise ValueError(f'{who}: points must be a contiguous int64 device tensor ({nturb},)')
    nbins = -(-rows // BIN) * -(-cols // BIN)
    if bins is None:
        bins = build_bins(xy.cpu().numpy(), reach_dev.cpu().numpy(), gridshape)
    if not is_tensor(bins[0]):
        _check_bins(bins[0], bins[1], nbins, nturb)
    bin_start, bin_items = to_dev(bins[0], torch.int32), to_dev(bins[1], torch.int32)
    if int(bin_start.numel()) != nbins + 1:
        raise ValueError(f'bins: bin_start has {bin_start.numel()} entries, expected {nbins + 1} for this raster')
    if ntracks == 0 or pts.numel() == 0 or bin_items.numel() == 0:
        # nothing to read, or no cylinder reaches the raster (empty tensors have no address to hand over)
        return (hits, first_step, points) if dt is None else (hits, first_step, points, time)
    if dt is not None:
        nat.check(nat.lib().ssrs_rotor_encounters_timed(
            nat.ptr(pts), nat.ptr(off), ntracks, nat.ptr(heights), nat.ptr(moves), nat.ptr(cellinfo), rows, cols,
            nat.ptr(xy), nat.ptr(reach_dev), nat.ptr(zband_dev), nturb, nat.ptr(bin_start), nat.ptr(bin_items),
            nat.ptr(hits), nat.ptr(first_step), nat.ptr(points), nat.ptr(time), stream_ptr()))
        return hits, first_step, points, time
    nat.check(nat.lib().ssrs_rotor_encounters(
        nat.ptr(pts), nat.ptr(off), ntracks, nat.ptr(heights), nat.ptr(cellinfo), rows, cols, nat.ptr(xy),
        nat.ptr(reach_dev), nat.ptr(zband_dev), nturb, nat.ptr(bin_start), nat.ptr(bin_items), nat.ptr(hits),
        nat.ptr(first_step), nat.ptr(points), stream_ptr()))
    return hits, first_step, points


def rotor_disks(turbines, dem, bounds, resolution, clearance=0.):
    """The disks of ssrs_rotor_transits (K18) from a `Turbines` with `t_hh` and `t_rd`: (xy_cells f64 (nturb, 2), reach f64
    (nturb,) in cells, hub int32 (nturb,) in mm above the DEM's datum, n_empty).  reach = (t_rd / 2 + clearance) / resolution;
    hub = base + rint(1000 t_hh), summed in int64 and clipped to int32, with rotor_geometry's base: the elevation of the cell
    the turbine stands on (base_cells), clip(rint(1000 z), +-2^30).  A NaN base (nodata), t_hh or t_rd gives reach = NaN
    (and hub = 0): nothing transits such a turbine; n_empty counts them.  dem: numpy or a device tensor (rows, cols)."""
    missing = [name for name in ('t_hh', 't_rd') if name not in turbines.columns]
    if missing:
        raise ValueError(f'rotor_disks: the turbines have no column {" / ".join(missing)} '
                         '(t_hh = hub height, t_rd = rotor diameter, metres)')
    resolution, clearance = float(resolution), float(clearance)
    if not resolution > 0. or clearance != clearance:
        raise ValueError(f'rotor_disks: resolution = {resolution!r}, clearance = {clearance!r} (resolution > 0)')
    if len(np.shape(dem)) != 2:
        raise ValueError(f'rotor_disks: dem has shape {tuple(np.shape(dem))}, expected (rows, cols)')
    xy = turbines.cell_coordinates(bounds, resolution)
    rb, cb, known = base_cells(xy, np.shape(dem))
    if is_tensor(dem):
        z = dem[torch.from_numpy(rb).to(dem.device), torch.from_numpy(cb).to(dem.device)].cpu().numpy()
    else:
        z = np.asarray(dem)[rb, cb]
    z = np.where(known, z.astype(np.float64), np.nan)
    hh = np.asarray(turbines.columns['t_hh'], dtype=np.float64)
    rad = np.asarray(turbines.columns['t_rd'], dtype=np.float64) / 2. + clearance
    empty = np.isnan(z) | np.isnan(hh) | np.isnan(rad)
    base = np.clip(_mm(z), -2 ** 30, 2 ** 30)
    i32 = np.iinfo(np.int32)
    hub = np.where(empty, 0, np.clip(base + _mm(hh), i32.min, i32.max)).astype(np.int32)
    return xy, np.where(empty, np.nan, rad / resolution), hub, int(empty.sum())


def rotor_axes(wdirn, ray_axes, nturb=None):
    """The axes of ssrs_rotor_transits: (n, 2) f64 [ax, ay], the upwind unit step along +col and +row of a wind from `wdirn`
    degrees (clockwise from north), from layers.ray_step as (uc, ur).  wdirn: one direction per turbine, or a scalar, which
    serves all turbines: one row, or `nturb` equal rows when that is given.  A NaN direction gives a NaN axis: nothing
    transits such a turbine."""
    from . import layers
    ur, uc = layers.ray_step(wdirn, ray_axes)
    axis = np.ascontiguousarray(np.stack([uc, ur], 1), dtype=np.float64)
    if nturb is not None and axis.shape[0] != int(nturb):
        if axis.shape[0] != 1:
            raise ValueError(f'rotor_axes: {axis.shape[0]} directions for {int(nturb)} turbines')
        axis = np.ascontiguousarray(np.repeat(axis, int(nturb), 0))
    return axis


TRANSIT_CULL_MARGIN = 1.5     # cells added to the reach for the cull lists of rotor_transits (include/ssrs_hip_transits.h)


def rotor_transits(traj, alt, offsets, cellinfo, xy_cells, reach, hub, axis, gridshape, resolution, bins=None, hits=None,
                   transits=None):
    """ssrs_rotor_transits on device tensors (K18): the moves through every turbine's rotor disk, per direction.  traj, alt,
    offsets, cellinfo, xy_cells and hits as rotor_encounters takes them (host or device); reach (nturb,) f64, hub (nturb,)
    int32 of rotor_disks; axis (nturb, 2) f64 of rotor_axes (one row serves all turbines); resolution in metres
    (mm_per_cell = 1000 * resolution).  bins: the cull lists, built here from reach + 1.5 when None -- the bin of a move's
    FIRST point decides which turbines are tested.  transits: int64 device tensor (nturb, 2), ADDED to when given.
    Returns dict(hits, tracks_per_turbine int64 (nturb), turbines_per_track int32 (ntracks), transits int64 (nturb, 2):
    [with the wind, against the wind]), device tensors."""
    return _transit_pass('rotor_transits', traj, alt, offsets, cellinfo, xy_cells, reach, hub, axis, gridshape, resolution, bins,
                         hits, transits)


def _transit_pass(who, traj, alt, offsets, cellinfo, xy_cells, reach, hub, axis, gridshape, resolution, bins, hits, transits,
                  collision=None):
    """rotor_transits' checks and call; with collision = (cls, table, risk, track_risk) rotor_collision_risk's, whose one
    pass gives the transits too."""
    rows, cols = int(gridshape[0]), int(gridshape[1])
    xy = xy_cells if is_tensor(xy_cells) else np.asarray(xy_cells, dtype=np.float64).reshape(-1, 2)
    xy = to_dev(xy, torch.float64).reshape(-1, 2)
    nturb = int(xy.shape[0])
    if not 1 <= nturb <= MAX_TURBINES:
        raise ValueError(f'{who}: {nturb} turbines, expected 1 to {MAX_TURBINES}')
    mm_per_cell = 1000. * float(resolution)
    if not (mm_per_cell > 0. and np.isfinite(mm_per_cell)):
        raise ValueError(f'{who}: resolution = {resolution!r}, expected metres > 0')
    reach_dev = to_dev(reach if is_tensor(reach) else np.asarray(reach, dtype=np.float64), torch.float64).reshape(-1)
    hub_dev = to_dev(hub if is_tensor(hub) else np.asarray(hub, dtype=np.int32), torch.int32).reshape(-1)
    axis_dev = to_dev(axis if is_tensor(axis) else np.asarray(axis, dtype=np.float64), torch.float64).reshape(-1, 2)
    if int(axis_dev.shape[0]) == 1 and nturb > 1:
        axis_dev = axis_dev.expand(nturb, 2)
    axis_dev = axis_dev.contiguous()
    if int(reach_dev.numel()) != nturb or int(hub_dev.numel()) != nturb or tuple(axis_dev.shape) != (nturb, 2):
        raise ValueError(f'{who}: reach has {reach_dev.numel()} entries, hub {hub_dev.numel()} and axis shape '
                         f'{tuple(axis_dev.shape)} for {nturb} turbines, expected ({nturb},), ({nturb},) and ({nturb}, 2)')
    off = to_dev(offsets, torch.int64).reshape(-1)
    ntracks = int(off.numel()) - 1
    if ntracks < 0:
        raise ValueError(f'{who}: offsets needs at least one entry')
    pts = to_dev(traj, torch.int16).reshape(-1, 2)
    heights = to_dev(alt, torch.int32).reshape(-1)
    if int(heights.numel()) != int(pts.shape[0]):
        raise ValueError(f'{who}: alt has {heights.numel()} entries for {pts.shape[0]} points (it is indexed like traj)')
    if not is_tensor(cellinfo) or cellinfo.dtype != torch.int32 or tuple(cellinfo.shape) != (rows, cols, 2) or \
            not cellinfo.is_contiguous() or not cellinfo.is_cuda:
        raise ValueError(f'{who}: cellinfo must be a contiguous int32 device tensor ({rows}, {cols}, 2) (altitude_cellinfo)')
    words = (nturb + 31) // 32
    dev = device()
    if hits is None:
        hits = torch.zeros((ntracks, words), dtype=torch.int32, device=dev)
    if transits is None:
        transits = torch.zeros((nturb, 2), dtype=torch.int64, device=dev)
    if hits.dtype != torch.int32 or tuple(hits.shape) != (ntracks, words) or not hits.is_contiguous() or not hits.is_cuda:
        raise ValueError(f'{who}: hits must be a contiguous int32 device tensor ({ntracks}, {words})')
    if not is_tensor(transits) or transits.dtype != torch.int64 or tuple(transits.shape) != (nturb, 2) or \
            not transits.is_contiguous() or not transits.is_cuda:
        raise ValueError(f'{who}: transits must be a contiguous int64 device tensor ({nturb}, 2)')
    if collision is not None:
        cls, table, risk, track_risk = collision
        cls_dev = to_dev(cls if is_tensor(cls) else np.asarray(cls, dtype=np.int32), torch.int32).reshape(-1)
        if not is_tensor(table):
            table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint32).view(np.int32))
        table_dev = to_dev(table, torch.int32)                 # (uint32 bit patterns in int32, as hits)
        nclass = int(table_dev.shape[0]) if table_dev.dim() == 3 else 0
        if int(cls_dev.numel()) != nturb or nclass < 1 or tuple(table_dev.shape) != (nclass, 2, COLLISION_RINGS):
            raise ValueError(f'{who}: cls has {cls_dev.numel()} entries and table shape {tuple(table_dev.shape)} for {nturb} '
                             f'turbines, expected ({nturb},) and (nclass >= 1, 2, {COLLISION_RINGS})')
        table_dev = table_dev.contiguous()
        if risk is None:
            risk = torch.zeros((nturb, 2), dtype=torch.int64, device=dev)
        if track_risk is None:
            track_risk = torch.zeros((ntracks,), dtype=torch.int64, device=dev)
        if not is_tensor(risk) or risk.dtype != torch.int64 or tuple(risk.shape) != (nturb, 2) or \
                not risk.is_contiguous() or not risk.is_cuda:
            raise ValueError(f'{who}: risk must be a contiguous int64 device tensor ({nturb}, 2)')
        if not is_tensor(track_risk) or track_risk.dtype != torch.int64 or tuple(track_risk.shape) != (ntracks,) or \
                not track_risk.is_contiguous() or not track_risk.is_cuda:
            raise ValueError(f'{who}: track_risk must be a contiguous int64 device tensor ({ntracks},)')
    nbins = -(-rows // BIN) * -(-cols // BIN)
    if bins is None:
        bins = build_bins(xy.cpu().numpy(), reach_dev.cpu().numpy() + TRANSIT_CULL_MARGIN, gridshape)
    if not is_tensor(bins[0]):
        _check_bins(bins[0], bins[1], nbins, nturb)
    bin_start, bin_items = to_dev(bins[0], torch.int32), to_dev(bins[1], torch.int32)
    if int(bin_start.numel()) != nbins + 1:
        raise ValueError(f'bins: bin_start has {bin_start.numel()} entries, expected {nbins + 1} for this raster')
    if ntracks and pts.numel() and bin_items.numel():
        # (otherwise nothing to read, or no disk reaches the raster: empty tensors have no address to hand over)
        args = (nat.ptr(pts), nat.ptr(off), ntracks, nat.ptr(heights), nat.ptr(cellinfo), rows, cols, nat.ptr(xy),
                nat.ptr(reach_dev), nat.ptr(hub_dev), nat.ptr(axis_dev), mm_per_cell, nturb, nat.ptr(bin_start),
                nat.ptr(bin_items), nat.ptr(hits), nat.ptr(transits))
        if collision is None:
            nat.check(nat.lib().ssrs_rotor_transits(*args, stream_ptr()))
        else:
            nat.check(nat.lib().ssrs_rotor_collision_risk(*args, nat.ptr(cls_dev), nat.ptr(table_dev), nclass, nat.ptr(risk),
                                                          nat.ptr(track_risk), stream_ptr()))
    per_turbine, per_track = encounter_counts(hits, nturb)
    out = dict(hits=hits, tracks_per_turbine=per_turbine, turbines_per_track=per_track, transits=transits)
    if collision is not None:
        out.update(risk=risk, track_risk=track_risk)
    return out


COLLISION_RINGS = nat.COLLISION_RINGS     # equal-area rings of the disk (include/ssrs_hip_collision.h)
BAND_CHORD_NODES = np.arange(1, 21) * 0.05     # r / R of the chord profile's 20 values


def band_probability(r, rotor_radius, rpm, max_chord, pitch, blades, speed, bird_length, bird_wingspan, flapping=False,
                     model_3d=True, chord_profile=None, upwind=True):
    """Band's (2012) probability that ONE transit of the rotor at radius r (metres, array) collides, for one rotor (scalars:
    radius R in metres, rpm, max chord in metres, pitch in degrees, blades) and one bird (speed v through the disk in m/s,
    length L and wingspan W in metres):
        Omega = 2 pi rpm / 60     alpha = v / (r Omega)     beta = L / W
        p = (b Omega / 2 pi v) (K |+- c sin(pitch) + alpha c cos(pitch)| + (L if alpha < beta else W alpha F))
    with + for a bird flying upwind, - downwind, F = 1 flapping and 2 / pi gliding, K = 1 for the 3-D model and 0 for the 1-D
    one, c = max_chord * the chord profile at r / R (20 values at 0.05, 0.10, ..., 1.00, linear between them, constant below
    0.05); clipped to [0, 1]; 0 for r > R and where r, b, Omega or v is not positive.  The formula and the default profile
    are recalled from the published model and NOT verified (DESIGN.md limit 18)."""
    r = np.asarray(r, dtype=np.float64)
    R, v, L, W = float(rotor_radius), float(speed), float(bird_length), float(bird_wingspan)
    omega = 2. * np.pi * float(rpm) / 60.
    b = float(blades)
    if not (b > 0. and omega > 0. and v > 0. and R > 0.):
        return np.zeros(r.shape)
    if not (L > 0. and W > 0.):
        raise ValueError(f'band_probability: bird_length = {bird_length!r}, bird_wingspan = {bird_wingspan!r} (metres > 0)')
    profile = np.asarray(chord_profile, dtype=np.float64).reshape(-1)
    if profile.shape != BAND_CHORD_NODES.shape or not (profile >= 0.).all():
        raise ValueError(f'band_probability: the chord profile needs {BAND_CHORD_NODES.size} values >= 0 '
                         '(r / R = 0.05, 0.10, ..., 1.00)')
    inside = (r > 0.) & (r <= R)
    rr = np.where(inside, r, R)                                             # (no division by zero; masked below)
    chord = float(max_chord) * np.interp(rr / R, BAND_CHORD_NODES, profile)
    gamma = np.deg2rad(float(pitch))
    alpha = v / (rr * omega)
    sign = 1. if upwind else -1.
    swept = np.abs(sign * chord * np.sin(gamma) + alpha * chord * np.cos(gamma)) if model_3d else 0.
    body = np.where(alpha < L / W, L, W * alpha * (1. if flapping else 2. / np.pi))
    p = b * omega / (2. * np.pi * v) * (swept + body)
    return np.where(inside, np.clip(p, 0., 1.), 0.)


def band_parameters(turbines, blades, rpm, max_chord, pitch):
    """f64 (nturb, 4) [rpm, max chord, pitch, blades]: the turbine columns `t_rpm`, `t_chord`, `t_pitch`, `t_blades` where
    the `Turbines` carry them, the given scalars otherwise."""
    n = len(turbines)
    cols = [np.asarray(turbines.columns[name], dtype=np.float64) if name in turbines.columns else np.full(n, float(default))
            for name, default in (('t_rpm', rpm), ('t_chord', max_chord), ('t_pitch', pitch), ('t_blades', blades))]
    return np.stack(cols, 1).reshape(n, 4)


def band_collision_table(rotor_radius, clearance, params, speed, bird_length, bird_wingspan, flapping=False, model_3d=True,
                         chord_profile=None):
    """The classes and the table of ssrs_rotor_collision_risk (K19): (cls int32 (nturb,), table uint32 (nclass, 2, 256),
    classes f64 (nclass, 6)).  rotor_radius (nturb,) = t_rd / 2 in metres; clearance metres (reach = R + clearance, the disk
    K18 tests); params (nturb, 4) of band_parameters.  A class is a distinct row [R, reach, rpm, max chord, pitch, blades],
    numbered in order of first appearance; a turbine with a NaN in its row gets class -1 and contributes nothing.  Ring k
    is the equal-area annulus k / 256 <= rho^2 / reach^2 < (k + 1) / 256; its entry is band_probability at the area midpoint
    r = reach sqrt((k + 0.5) / 256), min(2^32 - 1, rint(p 2^32)); [c, 0] is with the wind (the bird flies downwind, the
    formula's -), [c, 1] against it (+).  Without a valid turbine the table is one row of zeros."""
    R = np.asarray(rotor_radius, dtype=np.float64).reshape(-1)
    params = np.asarray(params, dtype=np.float64).reshape(-1, 4)
    if params.shape[0] != R.size:
        raise ValueError(f'band_collision_table: params has {params.shape[0]} rows for {R.size} turbines')
    rows = np.concatenate([R[:, None], R[:, None] + float(clearance), params], 1)
    cls = np.full(R.size, -1, dtype=np.int32)
    classes = []
    for t, row in enumerate(rows):
        if np.isnan(row).any():
            continue
        key = tuple(row.tolist())
        if key not in classes:
            classes.append(key)
        cls[t] = classes.index(key)
    table = np.zeros((max(1, len(classes)), 2, COLLISION_RINGS), dtype=np.uint32)
    mid = np.sqrt((np.arange(COLLISION_RINGS) + 0.5) / COLLISION_RINGS)
    for c, (radius, reach, rpm, chord, pitch, blades) in enumerate(classes):
        for dirn in (0, 1):
            p = band_probability(reach * mid, radius, rpm, chord, pitch, blades, speed, bird_length, bird_wingspan, flapping,
                                 model_3d, chord_profile, upwind=dirn == 1)
            table[c, dirn] = np.minimum(2. ** 32 - 1., np.rint(p * 2. ** 32)).astype(np.uint32)
    return cls, table, np.array(classes, dtype=np.float64).reshape(-1, 6)


def rotor_collision_risk(traj, alt, offsets, cellinfo, xy_cells, reach, hub, axis, cls, table, gridshape, resolution, bins=None,
                         hits=None, transits=None, risk=None, track_risk=None):
    """ssrs_rotor_collision_risk on device tensors (K19): rotor_transits' pass, every transit also weighted with its class's
    collision probability at the ring of the disk it goes through.  Every argument of rotor_transits as there (the cull
    lists are built from reach + 1.5 when None); cls (nturb,) int32 and table uint32 (nclass, 2, 256) of
    band_collision_table (host or device; a device table is int32 holding the uint32 bit patterns).  risk: int64 device
    tensor (nturb, 2), track_risk: int64 (ntracks,), both ADDED to when given.  Returns rotor_transits' dict plus risk and
    track_risk: the raw uint64 sums in units of 2^-32, [with the wind, against the wind] per turbine."""
    return _transit_pass('rotor_collision_risk', traj, alt, offsets, cellinfo, xy_cells, reach, hub, axis, gridshape, resolution,
                         bins, hits, transits, collision=(cls, table, risk, track_risk))


SITE_MAX_REACH = nat.SITE_MAX_REACH     # cells: the largest reach of a candidate class (include/ssrs_hip_sites.h)


def site_collision_risk(traj, alt, offsets, cellinfo, reach, hub_mm, axis, table, gridshape, resolution, transits=None, risk=None,
                        want_transits=True):
    """ssrs_site_collision_risk on device tensors (K20): rotor_collision_risk turned inside out -- for every cell of the
    raster the transits through the disk of ONE candidate turbine class standing on that cell, and their summed collision
    probabilities.  traj, alt, offsets and cellinfo as rotor_transits takes them (host or device; cellinfo a device tensor);
    reach in cells (0 .. SITE_MAX_REACH; NaN or negative: nothing is transited), hub_mm the hub's height above the ground of
    its cell in mm; axis f64 (2,) -- one upwind step [ax, ay] for all sites, rotor_axes' row -- or (rows, cols, 2), one per
    cell (16 bytes a cell on the device); table uint32 (2, 256), one class's rows of band_collision_table (host or device; a
    device table is int32 holding the uint32 bit patterns); resolution in metres.  transits, risk: int64 device tensors
    (rows, cols, 2), ADDED to when given; want_transits=False leaves the counts out (transits comes back None).
    Returns dict(transits, risk): [with the wind, against the wind] per cell, risk the raw uint64 sums in units of 2^-32."""
    who = 'site_collision_risk'
    rows, cols = int(gridshape[0]), int(gridshape[1])
    mm_per_cell = 1000. * float(resolution)
    if not (mm_per_cell > 0. and np.isfinite(mm_per_cell)):
        raise ValueError(f'{who}: resolution = {resolution!r}, expected metres > 0')
    reach = float(reach)
    if reach > SITE_MAX_REACH:
        raise ValueError(f'{who}: reach = {reach!r} cells, expected at most {SITE_MAX_REACH}')
    hub_mm = int(hub_mm)
    if not -2 ** 31 <= hub_mm < 2 ** 31:
        raise ValueError(f'{who}: hub_mm = {hub_mm} does not fit int32')
    axis_dev = to_dev(axis if is_tensor(axis) else np.asarray(axis, dtype=np.float64), torch.float64).contiguous()
    if tuple(axis_dev.shape) not in ((2,), (rows, cols, 2)):
        raise ValueError(f'{who}: axis has shape {tuple(axis_dev.shape)}, expected (2,) or ({rows}, {cols}, 2)')
    per_cell = axis_dev.dim() == 3
    off = to_dev(offsets, torch.int64).reshape(-1)
    ntracks = int(off.numel()) - 1
    if ntracks < 0:
        raise ValueError(f'{who}: offsets needs at least one entry')
    pts = to_dev(traj, torch.int16).reshape(-1, 2)
    heights = to_dev(alt, torch.int32).reshape(-1)
    if int(heights.numel()) != int(pts.shape[0]):
        raise ValueError(f'{who}: alt has {heights.numel()} entries for {pts.shape[0]} points (it is indexed like traj)')
    if not is_tensor(cellinfo) or cellinfo.dtype != torch.int32 or tuple(cellinfo.shape) != (rows, cols, 2) or \
            not cellinfo.is_contiguous() or not cellinfo.is_cuda:
        raise ValueError(f'{who}: cellinfo must be a contiguous int32 device tensor ({rows}, {cols}, 2) (altitude_cellinfo)')
    if not is_tensor(table):
        table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint32).view(np.int32))
    table_dev = to_dev(table, torch.int32).contiguous()            # (uint32 bit patterns in int32)
    if tuple(table_dev.shape) != (2, COLLISION_RINGS):
        raise ValueError(f'{who}: table has shape {tuple(table_dev.shape)}, expected (2, {COLLISION_RINGS}): one class')
    dev = device()
    if risk is None:
        risk = torch.zeros((rows, cols, 2), dtype=torch.int64, device=dev)
    if transits is None and want_transits:
        transits = torch.zeros((rows, cols, 2), dtype=torch.int64, device=dev)
    for name, out in (('risk', risk), ('transits', transits)):
        if out is None:
            continue
        if not is_tensor(out) or out.dtype != torch.int64 or tuple(out.shape) != (rows, cols, 2) or \
                not out.is_contiguous() or not out.is_cuda:
            raise ValueError(f'{who}: {name} must be a contiguous int64 device tensor ({rows}, {cols}, 2)')
    if ntracks and pts.numel():
        nat.check(nat.lib().ssrs_site_collision_risk(
            nat.ptr(pts), nat.ptr(off), ntracks, nat.ptr(heights), nat.ptr(cellinfo), rows, cols, reach, hub_mm,
            nat.ptr(axis_dev), int(per_cell), mm_per_cell, nat.ptr(table_dev), nat.ptr(transits), nat.ptr(risk), stream_ptr()))
    return dict(transits=transits, risk=risk)
