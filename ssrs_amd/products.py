"""Track products: everything `Simulator.simulate_tracks` accumulates from the trajectory chunks of one (case, realisation)
item.  A product is four short methods:

  __init__(sim)                  the constants and device uploads of one simulate_tracks call, made once
  prepare(case_id, inputs)       what it reads per wind case, left in inputs[product] (on the preparing thread)
  begin(item, ntracks, device)   the item's zeroed accumulators: its state
  consume(state, chunk)          the device calls for one `Chunk`
  store(state, key, sharded)     invariant check, sum over the ranks, keep in the Simulator's dict, rank 0 saves

`enabled(sim)` lists the products of a call.  Everything below is in the order of that list, and this is the one place that
states it; tests/test_gpu_track_products.py pins both sequences.

Per chunk:
   1. encounters (K: turbine_encounters on the chunk)
   2. occupancy (K13)
   3. passage (K17)
   4. heights (K14), which leaves chunk.masked / chunk.alt, then its sub-products:
   5.   cylinders (K15), unless rotor_exposure_time defers them to 10
   6.   disks: K18 (rotor_transits), or K19 in its place with collision_risk
   7.   sites (K20)
   8.   encounters on chunk.masked (the points in the rotor zone)
   9. time (K16), which reads chunk.masked and leaves chunk.dt
  10. cylinders in their timed form (K15 with dt= and time=), when deferred

Per item, `store` and with it the collectives of a track-sharded run, which every rank must issue in this order:
   1. encounters: _allreduce_sum (nturb)
   2. occupancy: reduce_histogram
   3. passage: reduce_histogram
   4. heights: reduce_histogram of band_hist, then
        rotor-zone encounters: _allreduce_sum (nturb)
        cylinders: _allreduce_sum (2 nturb), then the exposure time: _allreduce_sum (nturb)
        collision risk: _allreduce_sum (2 nturb)
        site risk: reduce_histogram, then site transits: reduce_histogram
        transits: _allreduce_sum (3 nturb), only with rotor_transits
   5. time: reduce_histogram of time_hist, then of band_time_hist
   6. (last, in simulate_tracks itself: reduce_histogram of the presence histogram)
"""
import os
import warnings
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch

from . import distributed, flight, presence
from . import turbines as turbines_mod
from ._device import to_dev


@dataclass
class Chunk:
    """One device chunk of trajectories: the tracks [t0, t1) of the item on this rank, and what the products leave for
    those behind them in the list (None until the one that makes it has run)."""
    t0: int
    t1: int
    traj: torch.Tensor
    off: torch.Tensor
    masked: torch.Tensor = None     # K14's traj_band: the points, (-1, -1) where not in the rotor zone
    alt: torch.Tensor = None        # K14's height at every point, mm
    dt: torch.Tensor = None         # K16's duration of the move that leaves every point, microseconds


def _upload_turbines(cells, reach, third, bins):
    return (to_dev(cells, torch.float64), to_dev(reach, torch.float64), to_dev(third, torch.int32),
            tuple(to_dev(a, torch.int32) for a in bins))


def _bitmap(ntracks, nturb, device):
    """(hits, first_step) of the encounter kernels: one bit per track and turbine, and every track's first step."""
    return (torch.zeros((ntracks, (nturb + 31) // 32), dtype=torch.int32, device=device),
            torch.full((ntracks,), -1, dtype=torch.int32, device=device))


class Product:
    def __init__(self, sim):
        self.sim = sim

    def prepare(self, case_id, inputs):
        pass

    def begin(self, item, ntracks, device):
        return None

    def consume(self, state, chunk):
        pass

    def store(self, state, key, sharded):
        pass

    # the tail every store shares: sum over the ranks of a track-sharded run -> keep -> rank 0 saves <id>_<stem>.npy
    def _summed(self, counts, sharded):
        """int64 counts of any shape, summed over the ranks (a collective: every rank, in the same item order)."""
        if sharded:
            counts = np.asarray(self.sim._allreduce_sum(counts.reshape(-1)), dtype=np.int64).reshape(counts.shape)
        return counts

    def _keep(self, name, key, value, sharded, stem=None):
        """value into the Simulator's dict `name`; the rank that owns the item (rank 0 when track-sharded) saves it."""
        getattr(self.sim, name)[key] = value
        self._save(stem or name, key, value, sharded)

    def _save(self, stem, key, value, sharded):
        if not sharded or self.sim._rank() == 0:
            np.save(os.path.join(self.sim.mode_data_dir, f'{self.sim._get_id_string(*key)}_{stem}.npy'), value)

    def _keep_raster(self, name, stem, key, counts, expected, sharded, what, of_what):
        """A uint32 raster checked by its checksum -- this rank's counts must add up to `expected` -- then summed over the
        ranks the way the histogram is (shards hold disjoint tracks, so the sum is exact) and kept as numpy int32."""
        counted = int((counts.to(torch.int64) & 0xFFFFFFFF).sum().item())
        if counted != expected:
            raise RuntimeError(f'{self.sim._get_id_string(*key)}: {what}: the raster adds up to {counted}, the {of_what} to '
                               f'{expected}')
        if sharded:
            counts = distributed.reduce_histogram(counts, all_ranks=True)
        self._keep(name, key, counts.to(torch.int32).cpu().numpy(), sharded, stem)


class Encounters(Product):
    """The tracks that came within turbine_encounter_radius of each turbine: <id>_turbine_encounters.npy (int64 (nturb,)) and
    turbine_encounters[key]; with zone=True, as a sub-product of the heights, the same of the points in the rotor zone
    (chunk.masked): rotor_turbine_encounters.  turbines_per_track / first_step stay this rank's tracks."""
    name, source = 'turbine_encounters', 'traj'

    def __init__(self, sim, geometry=None, zone=False):
        super().__init__(sim)
        # (one upload for all cases and both forms: the kernel reads the turbines and their cull lists from the device)
        self.geometry = geometry or (to_dev(sim._turbine_cells, torch.float64),
                                     tuple(to_dev(a, torch.int32) for a in sim._turbine_bins))
        self.nturb = int(self.geometry[0].shape[0])
        self.radius_cells = float(sim.turbine_encounter_radius) / float(sim.resolution)
        if zone:
            self.name, self.source = 'rotor_turbine_encounters', 'masked'

    def begin(self, item, ntracks, device):
        hits, first_step = _bitmap(ntracks, self.nturb, device)
        return SimpleNamespace(hits=hits, first_step=first_step)

    def consume(self, state, chunk):
        xy, bins = self.geometry
        turbines_mod.turbine_encounters(getattr(chunk, self.source), chunk.off, xy, self.radius_cells, self.sim.gridsize,
                                        bins=bins, hits=state.hits[chunk.t0:chunk.t1],
                                        first_step=state.first_step[chunk.t0:chunk.t1])

    def store(self, state, key, sharded):
        per_turbine, per_track = turbines_mod.encounter_counts(state.hits, self.nturb)
        self.store_counts(key, per_turbine.cpu().numpy(), per_track.cpu().numpy(), state.first_step.cpu().numpy(), sharded)

    def store_counts(self, key, tracks_per_turbine, turbines_per_track, first_step, sharded):
        """The host half of store, on numpy arrays: the one place that issues the encounters' collective."""
        per_turbine = self._summed(np.asarray(tracks_per_turbine, dtype=np.int64), sharded)
        getattr(self.sim, self.name)[key] = dict(
            tracks_per_turbine=per_turbine, turbines_per_track=np.asarray(turbines_per_track, dtype=np.int32),
            first_step=np.asarray(first_step, dtype=np.int32))
        self._save(self.name, key, per_turbine, sharded)


class DistinctTracks(Product):
    """Per cell, the distinct tracks of the item: through the cell (K13, `occupancy`) or within track_passage_radius of it
    (K17, `passage`).  One raster per item, added to over chunks and parts, one workspace for all chunks (a call leaves it
    clean), and `cells`, the sum of the chunks' cells_per_track: the checksum.  <id>_<stem>.npy, int32 holding uint32."""

    def __init__(self, sim, name, stem, what, of_what, workspace, kernel):
        super().__init__(sim)
        self.name, self.stem, self.what, self.of_what, self.workspace, self.kernel = name, stem, what, of_what, workspace, kernel

    def begin(self, item, ntracks, device):
        planes = presence.occupancy_planes(ntracks, self.sim.gridsize)
        return SimpleNamespace(counts=torch.zeros(self.sim.gridsize, dtype=torch.int32, device=device),
                               cells=torch.zeros((), dtype=torch.int64, device=device), planes=planes,
                               workspace=self.workspace(self.sim.gridsize, planes))

    def consume(self, state, chunk):
        _, per_track = self.kernel(chunk.traj, offsets=chunk.off, counts=state.counts, cells_per_track=True,
                                   planes=state.planes, workspace=state.workspace)
        state.cells.add_(per_track.sum(dtype=torch.int64))

    def store(self, state, key, sharded):
        self._keep_raster(self.name, self.stem, key, state.counts, int(state.cells.item()), sharded, self.what, self.of_what)


def occupancy(sim):
    return DistinctTracks(sim, 'track_occupancy_counts', 'occupancy', 'track occupancy', 'distinct cells of the tracks',
                          presence.occupancy_workspace,
                          lambda traj, **kw: presence.compute_track_occupancy(traj, sim.gridsize, **kw))


def passage(sim):
    r2 = presence.passage_r2(sim.track_passage_radius, sim.resolution)
    return DistinctTracks(sim, 'track_passage_counts', 'passage', 'track passage', 'cells within the radius of the tracks',
                          presence.passage_workspace,
                          lambda traj, **kw: presence.compute_track_passage(traj, sim.gridsize, r2, **kw))


class Heights(Product):
    """The flight-height scan (K14): the rotor-zone raster <id>_rotor_presence.npy (int32 holding uint32, checked against the
    in-zone points of this rank's tracks) and <id>_flight_heights.npy (int32 (tracks, 3): [points in the zone, least, greatest
    height in mm], this rank's tracks).  It owns the item's cellinfo -- from the item's UN-thresholded updraft and the DEM --
    and the sub-products that read it with chunk.alt / chunk.masked: `subs` in the order of their calls per chunk, `stores` in
    the order of their collectives per item (the module docstring's)."""

    def __init__(self, sim, encounters=None):
        super().__init__(sim)
        self.dem = to_dev(sim._terrain['Elevation'], torch.float64)
        self.kw, self.airspeed, self.sink = sim._flight_params()
        cylinders = Cylinders(sim) if sim._rotor_per_turbine() else None
        disks = Disks(sim) if sim.rotor_transits or sim.collision_risk else None
        sites = Sites(sim) if sim.site_collision_risk else None
        zone = Encounters(sim, encounters.geometry, zone=True) if encounters is not None else None
        # (rotor_exposure_time: the cylinders' call waits for K16's dt -- `Deferred`, behind the time in the list)
        self.deferred = cylinders if sim.rotor_exposure_time else None
        self.subs = [p for p in (cylinders, disks, sites, zone) if p is not None and p is not self.deferred]
        self.stores = [p for p in (zone and zone.store, cylinders and cylinders.store, disks and disks.store_risk,
                                   sites and sites.store, disks and disks.store_transits) if p is not None]
        self.want_masked = bool(sim.flight_time) or zone is not None
        self.want_alt = cylinders is not None or sites is not None

    def prepare(self, case_id, inputs):
        # (the un-thresholded field of every realisation, whatever the movement model)
        inputs[self] = list(self.sim._updraft_fields(case_id, lambda fname: to_dev(np.load(fname), torch.float32)))
        for sub in self.subs:
            sub.prepare(case_id, inputs)

    def begin(self, item, ntracks, device):
        sim = self.sim
        state = SimpleNamespace(
            band_hist=torch.zeros(sim.gridsize, dtype=torch.int32, device=device),
            rows=torch.zeros((ntracks, 3), dtype=torch.int32, device=device),
            cellinfo=flight.altitude_cellinfo(item.inputs[self][item.real_id], self.dem, sim.resolution, self.airspeed, self.sink))
        state.subs = {sub: sub.begin(item, ntracks, device) for sub in self.subs + [self.deferred] if sub is not None}
        for sub_state in state.subs.values():
            sub_state.cellinfo = state.cellinfo
        return state

    def consume(self, state, chunk):
        out = flight.compute_track_altitudes(chunk.traj, state.cellinfo, self.sim.gridsize, offsets=chunk.off,
                                             band_hist=state.band_hist, want_masked=self.want_masked, want_alt=self.want_alt,
                                             **self.kw)
        state.rows[chunk.t0:chunk.t1] = out['heights']
        chunk.masked, chunk.alt = out.get('masked'), out.get('alt')
        for sub in self.subs:
            sub.consume(state.subs[sub], chunk)

    def store(self, state, key, sharded):
        self._keep_raster('rotor_presence_counts', 'rotor_presence', key, state.band_hist,
                          int(state.rows[:, 0].sum(dtype=torch.int64).item()), sharded, 'rotor presence',
                          'in-zone points of the tracks')
        self._keep('flight_heights', key, state.rows.cpu().numpy(), sharded)
        for store in self.stores:
            store(state.subs[store.__self__], key, sharded)


class Deferred(Product):
    """A sub-product of the heights whose call per chunk waits for a later product's chunk.dt: the heights begin and store
    it, this position in the list calls it."""

    def __init__(self, heights):
        self.heights, self.sub = heights, heights.deferred

    def begin(self, item, ntracks, device):
        return item.state[self.heights].subs[self.sub]

    def consume(self, state, chunk):
        self.sub.consume(state, chunk)


class Cylinders(Product):
    """rotor_geometry = 'turbine' (K15): the tracks through every turbine's own cylinder and the points inside it,
    <id>_turbine_rotor_encounters.npy, int64 (nturb, 2) [tracks, points]; with rotor_exposure_time the call takes chunk.dt and
    also sums the time inside, <id>_turbine_rotor_time.npy, int64 (nturb,) microseconds.  Track-sharded runs sum the columns
    over the ranks; the per-track rows stay this rank's."""

    def __init__(self, sim):
        super().__init__(sim)
        self.cells, self.reach, self.zband, self.bins = _upload_turbines(*sim._rotor_cylinders)
        self.nturb, self.timed = int(self.cells.shape[0]), bool(sim.rotor_exposure_time)

    def begin(self, item, ntracks, device):
        hits, first_step = _bitmap(ntracks, self.nturb, device)
        return SimpleNamespace(hits=hits, first_step=first_step,
                               points=torch.zeros(self.nturb, dtype=torch.int64, device=device),
                               time=torch.zeros(self.nturb, dtype=torch.int64, device=device) if self.timed else None)

    def consume(self, state, chunk):
        # (dt is None, and the call the untimed one, unless K16 ran before: the position in the list decides)
        turbines_mod.rotor_encounters(chunk.traj, chunk.alt, chunk.off, state.cellinfo, self.cells, self.reach, self.zband,
                                      self.sim.gridsize, bins=self.bins, hits=state.hits[chunk.t0:chunk.t1],
                                      first_step=state.first_step[chunk.t0:chunk.t1], points=state.points,
                                      dt=chunk.dt, time=state.time)

    def store(self, state, key, sharded):
        per_turbine, per_track = turbines_mod.encounter_counts(state.hits, int(state.points.numel()))
        both = torch.stack([per_turbine, state.points], 1).cpu().numpy().astype(np.int64)
        spent = state.time.cpu().numpy().astype(np.int64) if state.time is not None else None
        if spent is not None:
            # the cheap invariant that stands in for a checksum -- K16 writes 0 <= dt <= 2^31 - 1, so a turbine's time is at
            # most that much per point inside it, and none without a point
            # (Python integers: points x (2^31 - 1) passes int64 from 2^32 points on)
            most = both[:, 1].astype(object) * (2 ** 31 - 1)
            wrong = np.nonzero((spent < 0) | (spent.astype(object) > most).astype(bool))[0]
            if wrong.size:
                t = int(wrong[0])
                raise RuntimeError(f'{self.sim._get_id_string(*key)}: rotor exposure time: turbine {t} has '
                                   f'{int(spent[t]) % 2 ** 64} us for {int(both[t, 1])} points inside its cylinder '
                                   f'({wrong.size} turbines like it)')
        both = self._summed(both, sharded)
        kept = dict(tracks_per_turbine=both[:, 0].copy(), points_per_turbine=both[:, 1].copy(),
                    turbines_per_track=per_track.cpu().numpy().astype(np.int32),
                    first_step=state.first_step.cpu().numpy().astype(np.int32))
        if spent is not None:
            kept['time_per_turbine'] = spent = self._summed(spent, sharded)
        self.sim.turbine_rotor_encounters[key] = kept
        self._save('turbine_rotor_encounters', key, both, sharded)
        if spent is not None:
            self._save('turbine_rotor_time', key, spent, sharded)


class Disks(Product):
    """rotor_transits / collision_risk: the moves through every turbine's disk, yawed into the case's axes, by direction --
    K18, or with collision_risk K19, whose one pass gives the same transits and their summed collision probabilities by
    turbine and by track.  Two stores, on either side of the sites' in the order of the collectives."""

    def __init__(self, sim):
        super().__init__(sim)
        self.cells, self.reach, self.hub, self.bins = _upload_turbines(*sim._rotor_disks)
        self.nturb = int(self.cells.shape[0])
        self.classes = None
        if sim.collision_risk:
            # (the uint32 table travels as int32 bit patterns, like the bitmaps)
            cls, table = sim._collision_table
            self.classes = (to_dev(cls, torch.int32), to_dev(np.ascontiguousarray(table).view(np.int32), torch.int32))

    def prepare(self, case_id, inputs):
        """The rotors' axes of one case (turbines.rotor_axes, on the device): rotor_yaw >= 0 is that compass direction for
        every turbine; otherwise every rotor faces the wind K16 reads -- uniform_winddirn in uniform mode, else the case's
        wdirn raster (_wind_rasters, at wtk_orographic_height) at the cell the turbine stands on -- in the frame of
        _time_ray_axes().  A NaN direction gives a turbine nothing can transit; one warning says how many."""
        sim = self.sim
        cells = sim._rotor_disks[0]
        if float(sim.rotor_yaw) >= 0.:
            wdirn = float(sim.rotor_yaw)
        elif sim.sim_mode.lower() == 'uniform':
            wdirn = float(sim.uniform_winddirn)
        else:
            entry = next(w for w in sim._wind if w.case_id == case_id)
            rb, cb, known = turbines_mod.base_cells(cells, sim.gridsize)
            raster = sim._wind_rasters(entry)[1]
            wdirn = raster[torch.from_numpy(rb).to(raster.device), torch.from_numpy(cb).to(raster.device)].cpu().numpy()
            wdirn = np.where(known, wdirn.astype(np.float64), np.nan)
        axes = turbines_mod.rotor_axes(wdirn, sim._time_ray_axes(), self.nturb)
        lost = int(np.isnan(axes).any(1).sum())
        if lost:
            warnings.warn(f'rotor_transits: {case_id}: {lost} of the {self.nturb} turbines have no wind direction (NaN) at the '
                          'cell they stand on; nothing transits them')
        inputs[self] = to_dev(axes, torch.float64)
        torch.cuda.current_stream().synchronize()       # (finished before a worker's stream reads it)

    def begin(self, item, ntracks, device):
        state = SimpleNamespace(axes=item.inputs[self], hits=_bitmap(ntracks, self.nturb, device)[0],
                                transits=torch.zeros((self.nturb, 2), dtype=torch.int64, device=device))
        if self.classes is not None:
            state.risk = torch.zeros((self.nturb, 2), dtype=torch.int64, device=device)
            state.track_risk = torch.zeros((ntracks,), dtype=torch.int64, device=device)
        return state

    def consume(self, state, chunk):
        sim, hits = self.sim, state.hits[chunk.t0:chunk.t1]
        args = (chunk.traj, chunk.alt, chunk.off, state.cellinfo, self.cells, self.reach, self.hub, state.axes)
        if self.classes is None:
            turbines_mod.rotor_transits(*args, sim.gridsize, sim.resolution, bins=self.bins, hits=hits, transits=state.transits)
        else:
            turbines_mod.rotor_collision_risk(*args, *self.classes, sim.gridsize, sim.resolution, bins=self.bins, hits=hits,
                                              transits=state.transits, risk=state.risk,
                                              track_risk=state.track_risk[chunk.t0:chunk.t1])

    def store_risk(self, state, key, sharded):
        """collision_risk: <id>_turbine_collision_risk.npy, int64 (nturb, 2) raw sums in units of 2^-32 [with the wind, against
        the wind], and <id>_track_collision_risk.npy, int64 (tracks,), this rank's tracks.  The invariants that stand in for a
        checksum: a transit adds less than 2^32, and the tracks' sums add up to the turbines'."""
        if self.classes is None:
            return
        id_str = self.sim._get_id_string(*key)
        risk = state.risk.cpu().numpy().astype(np.int64)
        per_track = state.track_risk.cpu().numpy().astype(np.int64)
        passes = state.transits.cpu().numpy().astype(np.int64)
        wrong = np.nonzero(((risk < 0) | (risk.astype(object) > passes.astype(object) * (2 ** 32 - 1)).astype(bool)).any(1))[0]
        if wrong.size:
            t = int(wrong[0])
            raise RuntimeError(f'{id_str}: collision risk: turbine {t} has the sums {risk[t].tolist()} (2^-32) for '
                               f'{passes[t].tolist()} transits ({wrong.size} turbines like it)')
        if int(per_track.astype(object).sum()) != int(risk.astype(object).sum()):
            raise RuntimeError(f'{id_str}: collision risk: the tracks add up to {int(per_track.astype(object).sum())}, '
                               f'the turbines to {int(risk.astype(object).sum())} (2^-32)')
        self._keep('turbine_collision_risk', key, self._summed(risk, sharded), sharded)
        self._keep('track_collision_risk', key, per_track, sharded)

    def store_transits(self, state, key, sharded):
        """rotor_transits: <id>_turbine_rotor_transits.npy, int64 (nturb, 3) [tracks, with the wind, against the wind].  The
        cheap invariant that stands in for a checksum: a turbine has tracks iff it has transits."""
        if not self.sim.rotor_transits:
            return
        per_turbine, _ = turbines_mod.encounter_counts(state.hits, int(state.transits.shape[0]))
        three = torch.cat([per_turbine[:, None], state.transits], 1).cpu().numpy().astype(np.int64)
        wrong = np.nonzero((three[:, 0] > 0) != (three[:, 1:].sum(1) > 0))[0]
        if wrong.size:
            t = int(wrong[0])
            raise RuntimeError(f'{self.sim._get_id_string(*key)}: rotor transits: turbine {t} has {int(three[t, 0])} tracks for '
                               f'{int(three[t, 1])} + {int(three[t, 2])} transits ({wrong.size} turbines like it)')
        self._keep('turbine_rotor_transits', key, self._summed(three, sharded), sharded)


class Sites(Product):
    """site_collision_risk (K20): a candidate turbine on every cell, its summed collision probabilities and its transits by
    direction: <id>_site_collision_risk.npy, int64 (rows, cols, 2) raw sums in units of 2^-32 [with the wind, against the
    wind], and <id>_site_transits.npy, int64 (rows, cols, 2)."""

    def __init__(self, sim):
        super().__init__(sim)
        self.reach, self.hub_mm, table = sim._site_class
        self.table = to_dev(table.view(np.int32), torch.int32)

    def prepare(self, case_id, inputs):
        """The axis of the candidate turbines of one case, on the device: rotor_yaw >= 0 is that compass direction, and in
        uniform mode the rotors face uniform_winddirn -- one pair [ax, ay] for all sites; otherwise every site faces the wind
        of its own cell, the case's wdirn raster (_wind_rasters, at wtk_orographic_height) through layers.ray_step in the
        frame of _time_ray_axes(): f64 (rows, cols, 2), 16 B a cell on the device.  A NaN direction gives a site nothing can
        transit."""
        sim = self.sim
        if float(sim.rotor_yaw) >= 0. or sim.sim_mode.lower() == 'uniform':
            wdirn = float(sim.rotor_yaw) if float(sim.rotor_yaw) >= 0. else float(sim.uniform_winddirn)
            axes = turbines_mod.rotor_axes(wdirn, sim._time_ray_axes())[0]
        else:
            entry = next(w for w in sim._wind if w.case_id == case_id)
            wdirn = sim._wind_rasters(entry)[1].cpu().numpy().astype(np.float64).reshape(-1)
            axes = turbines_mod.rotor_axes(wdirn, sim._time_ray_axes()).reshape(tuple(sim.gridsize) + (2,))
        inputs[self] = to_dev(axes, torch.float64)
        torch.cuda.current_stream().synchronize()       # (finished before a worker's stream reads it)

    def begin(self, item, ntracks, device):
        risk = torch.zeros(tuple(self.sim.gridsize) + (2,), dtype=torch.int64, device=device)
        return SimpleNamespace(axes=item.inputs[self], risk=risk, transits=torch.zeros_like(risk))

    def consume(self, state, chunk):
        turbines_mod.site_collision_risk(chunk.traj, chunk.alt, chunk.off, state.cellinfo, self.reach, self.hub_mm, state.axes,
                                         self.table, self.sim.gridsize, self.sim.resolution, transits=state.transits,
                                         risk=state.risk)

    def store(self, state, key, sharded):
        risk, passes = state.risk, state.transits
        if sharded:
            risk = distributed.reduce_histogram(risk, all_ranks=True)
            passes = distributed.reduce_histogram(passes, all_ranks=True)
        risk, passes = risk.cpu().numpy().astype(np.int64), passes.cpu().numpy().astype(np.int64)
        # the invariant that stands in for a checksum: a transit adds less than 2^32
        # (sum <= transits x (2^32 - 1) as ceil(sum / (2^32 - 1)) <= transits: the product passes int64 from 2^31 transits
        # on; a negative sum is a wrapped one)
        wrong = np.argwhere((risk < 0) | (passes < 0) | ((risk + (2 ** 32 - 2)) // (2 ** 32 - 1) > passes))
        if wrong.size:
            r, c, d = (int(v) for v in wrong[0])
            raise RuntimeError(f'{self.sim._get_id_string(*key)}: site collision risk: cell ({r}, {c}) has the sum '
                               f'{int(risk[r, c, d])} (2^-32) for {int(passes[r, c, d])} transits in direction {d} '
                               f'({wrong.shape[0]} entries like it)')
        self._keep('site_collision_risk_sums', key, risk, sharded, 'site_collision_risk')
        self._keep('site_transit_counts', key, passes, sharded, 'site_transits')


class Time(Product):
    """The flight-time kernel (K16): one raster of microseconds per item, <id>_residence_time.npy (int64 holding uint64), with
    flight_height (chunk.masked) a second of the moves that leave a point in the rotor zone, <id>_rotor_residence_time.npy,
    and <id>_flight_times.npy (int64 (tracks, 2): [total, in the rotor zone], this rank's tracks).  Checked by its checksums:
    each raster of this rank must add up, modulo 2^64, to its column of the rows.  With rotor_exposure_time it leaves
    chunk.dt."""

    def __init__(self, sim):
        super().__init__(sim)
        self.kw, self.ray_axes = sim._time_params(), sim._time_ray_axes()
        self.banded, self.want_dt = bool(sim.flight_height), bool(sim.rotor_exposure_time)

    def prepare(self, case_id, inputs):
        """The wind of one case: the scalar pair in uniform mode, otherwise the windinfo raster of the case's per-cell wind
        (_wind_rasters, at wtk_orographic_height)."""
        sim = self.sim
        if sim.sim_mode.lower() == 'uniform':
            inputs[self] = float(sim.uniform_windspeed), float(sim.uniform_winddirn)
            return
        entry = next(w for w in sim._wind if w.case_id == case_id)
        inputs[self] = flight.wind_cellinfo(*sim._wind_rasters(entry), self.ray_axes)
        torch.cuda.current_stream().synchronize()       # (finished before a worker's stream reads it)

    def begin(self, item, ntracks, device):
        time_hist = torch.zeros(self.sim.gridsize, dtype=torch.int64, device=device)
        return SimpleNamespace(wind=item.inputs[self], time_hist=time_hist,
                               band_time_hist=torch.zeros_like(time_hist) if self.banded else None,
                               rows=torch.zeros((ntracks, 2), dtype=torch.int64, device=device))

    def consume(self, state, chunk):
        out = flight.compute_track_times(chunk.traj, self.sim.gridsize, offsets=chunk.off, wind=state.wind,
                                         ray_axes=self.ray_axes, masked=chunk.masked, time_hist=state.time_hist,
                                         band_time_hist=state.band_time_hist, want_dt=self.want_dt, **self.kw)
        state.rows[chunk.t0:chunk.t1] = out['times']
        chunk.dt = out.get('dt')

    def store(self, state, key, sharded):
        for raster, column, name, stem in ((state.time_hist, 0, 'residence_time_counts', 'residence_time'),
                                           (state.band_time_hist, 1, 'rotor_residence_time_counts', 'rotor_residence_time')):
            if raster is None:
                continue
            # (int64 sums wrap like the uint64 ones they hold: equal modulo 2^64 is equal here)
            counted, summed = int(raster.sum().item()), int(state.rows[:, column].sum().item())
            if counted != summed:
                raise RuntimeError(f'{self.sim._get_id_string(*key)}: flight time: the {stem} raster adds up to '
                                   f'{counted % 2 ** 64} us, the tracks to {summed % 2 ** 64} us')
            if sharded:
                raster = distributed.reduce_histogram(raster, all_ranks=True)
            self._keep(name, key, raster.cpu().numpy(), sharded, stem)
        self._keep('flight_times', key, state.rows.cpu().numpy(), sharded)


def enabled(sim):
    """The products of one simulate_tracks call, in the order of the module docstring (the constructor saw to what each
    needs of the others)."""
    encounters = Encounters(sim) if float(sim.turbine_encounter_radius) > 0. else None
    heights = Heights(sim, encounters) if sim.flight_height else None
    return [p for p in (encounters,
                        occupancy(sim) if sim.track_occupancy else None,
                        passage(sim) if float(sim.track_passage_radius) > 0. else None,
                        heights,
                        Time(sim) if sim.flight_time else None,
                        Deferred(heights) if heights is not None and heights.deferred is not None else None)
            if p is not None]
