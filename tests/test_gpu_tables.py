"""The stepper's five decision tables against tests/table_ref.py, state by state, on small nasty rasters.

k_step_thr / k_step_roam take the reference's decision iff every non-flag entry T of a table satisfies
T - 1 <= 2^N B <= T + 1 for the reference's own f64 boundary B (N = 16: threshold table, the priors' zero_e / rev_e / thr9;
N = 32: fine table); the bound is that derivation, not a measurement.  Flags must sit exactly where the classes of
table_ref put them, and poison -- always safe -- must not spread beyond what the f32 builder documents: an updraft above
1e19 in the window, a weight that is not finite, a row total outside [1e-29, 1e29] / 2^23; a zero row is never poison and
a reversal is always its flag, whatever the sizes of the updrafts around them.
The pair table is checked against its successor rule on the threshold table read back in the same test (integers only);
the f64 and ring tables bit for bit against the oracle's weights.

Each test prints the largest |T - 2^N B| it saw (entries below the clamp); profiles/table_margins.md keeps them."""
import numpy as np
import pytest
import torch

import table_ref as tr

pytestmark = pytest.mark.gpu

CASES = [(recipe, shape, True) for recipe in tr.RECIPES for shape in tr.SHAPES] + \
        [(recipe, shape, False) for recipe in ('benign', 'magnitudes', 'poison') for shape in ((5, 5), (17, 65), (48, 129))]
IDS = [f'{recipe}-{shape[0]}x{shape[1]}-{"pot" if pot else "nopot"}' for recipe, shape, pot in CASES]
MARGINS = {}                 # (table, case id) -> (largest |T - 2^N B|, heading)


def _note(table, case, heading, value):
    key = (table, f'{case[0]}-{case[1][0]}x{case[1][1]}-{"pot" if case[2] else "nopot"}')
    if value >= MARGINS.get(key, (-1., None))[0]:
        MARGINS[key] = (value, heading)


def _where(mask, limit=6):
    idx = np.argwhere(mask)
    return f'{len(idx)} states, first {idx[:limit].tolist()}'


def _fields(gpu, case):
    from ssrs_amd._device import to_dev
    f = tr.field_ref(*case)
    upd = to_dev(f.updraft, torch.float64)
    pot = None if f.potential is None else to_dev(f.potential, torch.float32)
    return f, upd, pot


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_f64_table_is_the_oracles_weights(gpu, case):
    from ssrs_amd import movmodel
    f, upd, pot = _fields(gpu, case)
    got = movmodel.build_transition_table(upd, pot).cpu().numpy()
    assert got.shape == (f.rows, f.cols, 8)
    eight = [k for k in range(9) if k != 4]
    has_nan = np.isnan(f.w).any(axis=2) & f.interior
    assert np.isnan(got[has_nan]).all(), _where(has_nan & ~np.isnan(got).all(axis=2))
    ok = f.interior & ~has_nan
    want = f.clipped()[:, :, eight]
    differ = (got.view(np.uint64) != np.ascontiguousarray(want).view(np.uint64)).any(axis=2) & ok
    assert not differ.any(), _where(differ)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_ring_table_records_and_zero_mask(gpu, case):
    from ssrs_amd import movmodel
    f, upd, pot = _fields(gpu, case)
    records, mask = tr.ring_decode(movmodel.build_transition_table(upd, pot, ring=True).cpu().numpy(), f.rows, f.cols)
    bits = records.view(np.uint32)
    bad_cell = f.nonfinite
    assert np.isnan(records[bad_cell]).all() and (mask[bad_cell] == 0).all()
    ok = f.interior & ~bad_cell
    want_mask = np.zeros((f.rows, f.cols), dtype=np.uint8)
    for j in range(10):
        c = (j + 7) % 8
        w = f.w[:, :, tr.RING_K[c]]
        positive = w > 0.
        with np.errstate(over='ignore', under='ignore'):
            want = np.where(positive, w.astype(np.float32).view(np.uint32), np.uint32(0x80000000))
        differ = (bits[:, :, j] != want) & ok
        assert not differ.any(), (j, _where(differ))
        if j < 8:
            want_mask |= np.where(~positive, np.uint8(1 << c), np.uint8(0))
    differ = (mask != want_mask) & ok
    assert not differ.any(), _where(differ)


def _check_threshold_planes(f, h, planes, case):
    cls = np.moveaxis(h.cls, 2, 0)                       # (8, rows, cols) like the planes
    b1, b2 = np.moveaxis(h.b12[..., 0], 2, 0), np.moveaxis(h.b12[..., 1], 2, 0)
    t1, t2 = planes & 0xFFFF, planes >> 16
    for c, flag in ((tr.EDGE, tr.THR_BOUNDARY), (tr.NONFINITE, tr.THR_POISON), (tr.REVERSAL, tr.THR_REVERSAL)):
        wrong = (cls == c) & (planes != flag)
        assert not wrong.any(), (c, _where(wrong))
    rest = (cls == tr.ORDINARY) | (cls == tr.ZERO_ROW)
    poison = rest & (planes == tr.THR_POISON)
    live = rest & ~poison
    wrong = live & (t1 > t2)
    assert not wrong.any(), _where(wrong)
    with np.errstate(invalid='ignore'):
        wrong = live & ~(tr.within_one(t1, b1, 16) & tr.within_one(t2, b2, 16))
    assert not wrong.any(), (_where(wrong), planes[wrong][:6], b1[wrong][:6] * 65536., b2[wrong][:6] * 65536.)
    # where poison is not allowed
    in_range = (f.window_updraft_max <= 1e19)[None]
    tot = np.moveaxis(f.admissible_sum(), 2, 0) * 8388608.
    must = (cls == tr.ORDINARY) & in_range & (tot >= 1e-29) & (tot <= 1e29)
    wrong = must & poison
    assert not wrong.any(), (_where(wrong), tot[wrong][:6])
    wrong = (cls == tr.ZERO_ROW) & poison
    assert not wrong.any(), _where(wrong)
    n_far = int((rest & ~in_range).sum())
    worst = max(tr.margin(t1[live], b1[live], 16), tr.margin(t2[live], b2[live], 16)) if live.any() else 0.
    _note('thr', case, h.heading, worst)
    return worst, int(poison.sum()), int(rest.sum()), n_far


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_threshold_table_every_state(gpu, case):
    from ssrs_amd import movmodel
    f, upd, pot = _fields(gpu, case)
    for heading in tr.HEADINGS:
        h = tr.heading_ref(case[0], case[1], heading, case[2])
        table = movmodel.build_transition_table(upd, pot, thr=True, move_dirn=float(heading))
        header, planes = tr.thr_decode(table.cpu().numpy(), f.rows, f.cols)
        assert header['magic'] == b'SSRSTHR1' and (header['rows'], header['cols']) == (f.rows, f.cols)
        assert header['prior'].tobytes() == np.array(h.prior, dtype=np.float64).tobytes()
        worst, npoison, nrest, n_far = _check_threshold_planes(f, h, planes, case)
        print(f'thr {case} heading {heading}: max |T - 2^16 B| = {worst:.4f}; poison {npoison} of {nrest} rows with '
              f'finite weights ({n_far} of those have an updraft above 1e19 in their window)')


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_roam_tables_every_state(gpu, case):
    from ssrs_amd import movmodel
    f, upd, pot = _fields(gpu, case)
    for heading in tr.HEADINGS:
        h = tr.heading_ref(case[0], case[1], heading, case[2])
        table = movmodel.build_transition_table(upd, pot, thr=True, move_dirn=float(heading))
        pair, fine, words = movmodel.roam_tables_selftest(upd, pot, float(heading), thr=table)
        assert pair.shape == (f.rows, f.cols, 8, 4) and fine.shape == (f.rows, f.cols, 8, 2) and words.shape == (38,)
        _, planes = tr.thr_decode(table.cpu().numpy(), f.rows, f.cols)
        pw = tr.prior_words_decode(words)

        # ---- the priors' own words
        assert pw['reversal'] == h.reversal_mask and pw['fine_reversal'] == h.reversal_mask
        assert (pw['rev_ok'], pw['rev_rc'] if h.rev_ok else 0) == (h.rev_ok, h.rev_rc)
        worst16 = worst32 = 0.
        for rc in range(8):
            if (h.reversal_mask >> rc) & 1:
                continue
            e, b = pw['zero_e'][rc], h.zero_b12[rc]
            ts = (e & 0xFFFF, e >> 16)
            assert ts[0] <= ts[1] and tr.within_one(ts, b, 16).all(), (rc, hex(e), b * 65536.)
            worst16 = max(worst16, tr.margin(ts, b, 16))
            ts = (pw['zero_t1'][rc], pw['zero_t2'][rc])
            assert ts[0] <= ts[1] and tr.within_one(ts, b, 32).all(), (rc, ts, b * 2. ** 32)
            worst32 = max(worst32, tr.margin(ts, b, 32))
        assert tr.within_one(pw['thr9'], h.rev9, 16).all(), (pw['thr9'], h.rev9 * 65536.)
        worst16 = max(worst16, tr.margin(pw['thr9'], h.rev9, 16))
        if h.rev_ok:
            ts = (pw['rev_e'] & 0xFFFF, pw['rev_e'] >> 16)
            assert ts[0] <= ts[1] and tr.within_one(ts, h.rev_b12, 16).all(), (hex(pw['rev_e']), h.rev_b12)
            worst16 = max(worst16, tr.margin(ts, h.rev_b12, 16))
        _note('prior16', case, heading, worst16)
        _note('prior32', case, heading, worst32)

        # ---- pair table: the successor rule on the threshold table, integers only
        want = tr.pair_expected(planes, h.rev_ok, h.rev_rc, pw['rev_e'])
        differ = (pair != want).any(axis=3)
        assert not differ.any(), (_where(differ), pair[differ][:4], want[differ][:4])

        # ---- fine table
        t1, t2 = fine[..., 0], fine[..., 1]
        flag = t1 > t2
        must_flag = (h.cls == tr.EDGE) | (h.cls == tr.NONFINITE) | (h.cls == tr.REVERSAL)
        assert not (must_flag & ~flag).any(), _where(must_flag & ~flag)
        assert not (~must_flag & flag).any(), _where(~must_flag & flag)
        live = ~must_flag
        with np.errstate(invalid='ignore'):
            wrong = live & ~(tr.within_one(t1, h.b12[..., 0], 32) & tr.within_one(t2, h.b12[..., 1], 32))
        assert not wrong.any(), (_where(wrong), fine[wrong][:6], h.b12[wrong][:6] * 2. ** 32)
        worst = max(tr.margin(t1[live], h.b12[..., 0][live], 32), tr.margin(t2[live], h.b12[..., 1][live], 32)) if live.any() else 0.
        _note('fine', case, heading, worst)
        print(f'roam {case} heading {heading}: max |T - 2^32 B| = {worst:.6f} (fine), priors {worst16:.4f} at 16 bits, '
              f'{worst32:.6f} at 32 bits')


def test_zz_margins_summary(gpu):
    """The largest margins of this session per table (printed: run with -s)."""
    for table in ('thr', 'fine', 'prior16', 'prior32'):
        rows = [(v[0], k[1], v[1]) for k, v in MARGINS.items() if k[0] == table]
        if rows:
            worst = max(rows)
            print(f'MARGIN {table}: {worst[0]:.6f} on {worst[1]} heading {worst[2]}')
            assert worst[0] <= 1.0
