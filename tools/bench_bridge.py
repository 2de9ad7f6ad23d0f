"""K23's speed: movmodel.score_gaps on G7's raster (96 x 128) with the reference's own updraft and potential
(tests/golden/g7_tracks.npz), on gaps thinned from the stepper's own tracks on those fields.

The stepper runs --tracks tracks (memory 1, nu 1) from starts spread over the raster's southern rows; their points past the
burn-in are thinned by n = 4, 16 and 32 (movmodel.thin_track, movmodel.fix_gaps: the true number of moves, incoming 4 except
after a unit pair), the whole pairs of n moves are kept and tiled up to the number of gaps of a timed call.  Every n is
scored at nu = 1 (directed: a few dozen occupied states) and at nu = 0 (dense: every state of the window).  HIP events
around the whole Python call (the allocation of the outputs from torch's cache, the scan for the longest job and its
read-back, one launch); the number of gaps of a call is chosen from a first short call so that a call takes about --ms
milliseconds; after a warm-up --runs calls (default 7), the median.  One reference point: movmodel.score_tracks on the
unthinned tracks, the same points walked move by move.

The LDS of a workgroup is 144 (n + 1)^2 bytes; the resident workgroups per CU are computed here, not measured: the least of
163 840 / LDS and 12 waves (3 a SIMD at 142 VGPRs) over the workgroup's waves.

--only n,nu scores one combination and nothing else (for a counter run of its own)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--tracks', type=int, default=2048)
ap.add_argument('--runs', type=int, default=7)
ap.add_argument('--ms', type=float, default=200.)
ap.add_argument('--only', default=None, help='n,nu: one combination, one warm-up and one call of --gaps gaps')
ap.add_argument('--gaps', type=int, default=20000)
ap.add_argument('--out', default=None, help='write the markdown table here as well')
args = ap.parse_args()


def residency(n):
    side = n + 1
    lds = 144 * side * side
    threads = 512 if side * side > 512 else 256
    return lds, threads, min(163840 // lds, 12 // (threads // 64))


def main():
    import torch
    from ssrs_amd import movmodel
    g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'g7_tracks.npz'), allow_pickle=False))
    shape = tuple(g['updraft'].shape)
    upd, pot = torch.from_numpy(g['updraft']).cuda(), torch.from_numpy(g['potential']).cuda()
    rng = np.random.default_rng(23)
    starts = np.stack([rng.integers(2, 12, args.tracks), rng.integers(8, shape[1] - 8, args.tracks)], 1)
    batch = movmodel.simulate_tracks(0., starts, shape, 1, 1., upd, pot, seed=23, want_tracks=True)
    skip = int(min(shape) / 10) + 1
    tracks = [t[skip:] for t in batch.tracks() if len(t) > skip + 33]
    points = sum(len(t) for t in tracks)

    def timed(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), res

    def jobs_of(n):
        jobs = np.concatenate([movmodel.fix_gaps(*movmodel.thin_track(t, n))[0] for t in tracks])
        return jobs[jobs[:, 5] == n]

    def tiled(jobs, count):
        return torch.from_numpy(np.ascontiguousarray(np.tile(jobs, (-(-count // len(jobs)), 1))[:count])).cuda()

    def call(dev_jobs, nu):
        return lambda: movmodel.score_gaps(dev_jobs, shape, 0., nu, upd, pot)

    if args.only:
        n, nu = args.only.split(',')
        dev_jobs = tiled(jobs_of(int(n)), args.gaps)
        timed(call(dev_jobs, float(nu)))
        ms, res = timed(call(dev_jobs, float(nu)))
        print(json.dumps(dict(n=int(n), nu=float(nu), gaps=args.gaps, ms=ms, counts=res.counts())))
        return

    rows = []
    for n in (4, 16, 32):
        jobs = jobs_of(n)
        for nu in (1., 0.):
            probe = tiled(jobs, 2048)
            timed(call(probe, nu))
            ms, _ = timed(call(probe, nu))
            count = int(min(max(2048 * args.ms / max(ms, 1e-3), 2048), 4e6))
            dev_jobs = tiled(jobs, count)
            _, res = timed(call(dev_jobs, nu))
            counts = res.counts()
            runs = [timed(call(dev_jobs, nu))[0] for _ in range(args.runs)]
            lds, threads, resident = residency(n)
            rows.append(dict(n=n, nu=nu, distinct=len(jobs), gaps=count, median_ms=float(np.median(runs)), min_ms=min(runs),
                             max_ms=max(runs), gaps_per_s=count / np.median(runs) * 1e3, scored=counts['scored'], lds=lds,
                             threads=threads, resident=resident))
    # the reference point: the same points walked move by move under K21
    traj = torch.from_numpy(np.concatenate(tracks)).cuda()
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)).cuda()
    k21 = lambda: movmodel.score_tracks(traj, shape, 0., 1, 1., upd, pot, offsets=off)
    timed(k21)
    k21_runs = [timed(k21)[0] for _ in range(args.runs)]
    lines = [f'{shape[0]} x {shape[1]}, {torch.cuda.get_device_name(0)}, {len(tracks)} tracks, {points} points past the burn-in, '
             f'{args.runs} runs a call', '',
             '| n | nu | distinct gaps | gaps a call | median ms | min .. max ms | gaps/s | SCORED | LDS B / workgroup | lanes | workgroups / CU |',
             '|---|---|---|---|---|---|---|---|---|---|---|']
    for r in rows:
        lines.append(f"| {r['n']} | {r['nu']:g} | {r['distinct']} | {r['gaps']} | {r['median_ms']:.3f} | {r['min_ms']:.3f} .. "
                     f"{r['max_ms']:.3f} | {r['gaps_per_s']:.3e} | {r['scored']} | {r['lds']} | {r['threads']} | {r['resident']} |")
    lines += ['', f'score_tracks (K21) on the {points} unthinned points, one call: median {np.median(k21_runs):.3f} ms '
              f'({min(k21_runs):.3f} .. {max(k21_runs):.3f}), {points / np.median(k21_runs) * 1e3:.3e} points/s']
    text = '\n'.join(lines)
    print(text)
    print(json.dumps(dict(rows=rows, k21_ms=float(np.median(k21_runs)), points=points)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


main()
