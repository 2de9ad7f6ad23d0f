"""K15's timed form as its definition (include/ssrs_hip.h, ssrs_rotor_encounters_timed) in plain numpy: for every case of
tests/rotor_ref.py a dt per point and time_per_turbine[t] = the sum of dt over the points inside turbine t, by
rotor_ref.inside_matrix -- the brute force over ALL (point, turbine) pairs.  tests/test_rotor_time_host.py (this restatement
against a second form) and tests/test_gpu_rotor_time.py (the device) share it.  Every comparison is integer equality."""
import numpy as np

import rotor_ref

CAP = 2 ** 31 - 1               # the largest dt, microseconds
LEAD_DT = 1_999_999_999         # on the points in front of the first track: a kernel that read them would show
PATTERNS = ('random', 'zeros', 'negative')


def time_per_turbine(inside, dt):
    """int64 (nturb,) holding the sum modulo 2^64 of the sign-extended dt over the True rows of `inside` (points, nturb)."""
    dt = np.asarray(dt).astype(np.int64)
    with np.errstate(over='ignore'):
        return np.where(inside, dt[:, None], np.int64(0)).sum(0, dtype=np.int64)


def time_per_turbine_python(inside, dt):
    """The same in Python integers: a list of nturb exact sums (not reduced modulo 2^64)."""
    dt = [int(v) for v in np.asarray(dt)]
    return [sum(dt[k] for k in np.nonzero(inside[:, t])[0]) for t in range(inside.shape[1])]


def inside_of(c):
    """rotor_ref.inside_matrix of a case over its flat points (the lead points included), computed once per call."""
    traj, alt, _ = rotor_ref.flat(c)
    return rotor_ref.inside_matrix(traj, alt, c['elev'], c['xy'], c['reach'], c['zband'], c['shape'])


def dt_of(c, pattern='random'):
    """int32 (lead + points): the dt of a case, indexed like rotor_ref.flat(c)'s traj.  'random': values in [0, 2^31 - 1],
    with 2^31 - 1 throughout the 4097-point track of the loiter cases (a lane's pending sum and a block's sum both pass
    2^32); 'zeros': that, with 0 on every other point inside a cylinder (points counted, no time); 'negative': 'random' with
    one negative value planted on a point inside turbine 0 (the sign extension).  The lead points get LEAD_DT."""
    rng = np.random.default_rng(16)
    lengths = [len(t) for t in c['tracks']]
    dt = rng.integers(0, CAP + 1, c['lead'] + sum(lengths)).astype(np.int32)
    dt[:c['lead']] = LEAD_DT
    if 'loiter' in c['name']:
        at = c['lead'] + sum(lengths[:11])
        dt[at:at + lengths[11]] = CAP
    if pattern == 'random':
        return dt
    hit = np.nonzero(inside_of(c)[c['lead']:].any(1))[0] + c['lead']
    assert hit.size > 20
    if pattern == 'zeros':
        dt[hit[::2]] = 0
    elif pattern == 'negative':
        planted = c['lead'] + sum(lengths[:10]) + 100           # (20, 31) of rotor_ref._base: inside turbines 0 and 1
        assert planted in hit
        dt[planted] = -123_456_789
    else:
        raise ValueError(pattern)
    return dt


_expected = {}


def expected(name, pattern='random'):
    """(dt int32 (lead + points), time int64 (nturb,)) of a case: the restatement over the points [lead, end), computed once
    and shared (read-only)."""
    if (name, pattern) not in _expected:
        c = rotor_ref.case(name)
        dt = dt_of(c, pattern)
        time = time_per_turbine(inside_of(c)[c['lead']:], dt[c['lead']:])
        dt.setflags(write=False)
        time.setflags(write=False)
        _expected[(name, pattern)] = (dt, time)
    return _expected[(name, pattern)]
