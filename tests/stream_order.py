"""The stream contract of include/ssrs_hip*.h under a hostile execution condition (tests/test_gpu_stream_order.py).

A plain helper module: a proxy that stands in for ssrs_amd._native._lib while watching() is active, so that every
`nat.lib().ssrs_*` call of the package and of the tests' own C-ABI drivers goes through it.  For every export whose last
parameter in the headers is a pointer named `stream` (streamed_exports(): parsed, not listed) the proxy, before it forwards
the call unchanged,

  * checks the handle: non-NULL and the calling thread's torch.cuda.current_stream().cuda_stream.  A wrapper or a driver
    that passes None as the stream fails here, by name;
  * enqueues a device-side delay, by mode:
      'late_stream'  a first-touch copy of every device tensor that was handed to _native.ptr() for this call, the delay,
                     and the copies written back, all on the current side stream S.  Whatever the export enqueues on S
                     runs late.  What it puts elsewhere (the null stream, a stream of its own without an event wait on S)
                     runs early: before the launches on S that it depends on, and before the write-back, which then puts
                     the tensors' earlier contents over what the early launch wrote.  (The write-back stores the values
                     the inputs already hold: an early launch never reads garbage, so a mis-streamed kernel gives wrong
                     values, not a fault.)
      'late_null'    the delay goes on the null stream.  What the export wrongly puts there finishes late; the checker,
                     which consumes the results on S and synchronises S only, reads what was there before.
      'check'        the handle check alone (host threads).

The delay is torch.cuda._sleep, its cycles per millisecond measured once per process with events; DELAY_MS is the chosen
length (profiles/stream_contract.md: how it was measured and chosen), and the proxy times its first delay with events so
that the test can assert the length was reached.  Torch's pool streams share a few hardware queues with the null stream,
and on a shared queue mis-streamed work is ordered by accident: side_stream() tries up to 8 fresh torch.cuda.Stream()
objects and returns the first on which both positive controls fire.

Importing this module needs no GPU."""
import contextlib
import ctypes as C
import glob
import os
import re
import threading
import time

import test_native_abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ('late_stream', 'late_null')
# The chosen length (profiles/stream_contract.md).  Both controls fired from 0.02 ms on, and both mutations of that note were
# caught from 0.04 ms, twice that, on.  The controls are three torch calls, though; in 'late_stream' the delay must also
# outlast what the host puts between it and the export's launches: a write-back per tensor (collision risk hands over 18)
# and the export's own host time (median 0.15 ms on the recorded stepper's calls).  1 ms covers that with room to spare
# and costs 1.25 ms a call; a longer delay is the more hostile condition, never the weaker one.
DELAY_MS = 1.0
CANDIDATES = 8
# streamed exports the families do not run, each with its reason
EXCLUSIONS = {'ssrs_hist_reduce': 'needs a communicator; test_gpu_integration_stub.py and test_gpu_multirank.py run it'}


# ------------------------------------------------------------------------------------------------ the headers
def header_parameters():
    """{export: [(type, name) of each parameter]} of every prototype of include/ssrs_hip*.h, by the parse of
    tests/test_native_abi.py (its PROTOTYPE pattern on its header_code())."""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, 'include', 'ssrs_hip*.h'))):
        for _, name, params in re.findall(abi.PROTOTYPE, abi.header_code(os.path.basename(path))):
            assert name not in out, f'{name} declared twice'
            out[name] = []
            for param in [' '.join(p.split()) for p in params.split(',')]:
                if param == 'void':
                    continue
                m = re.fullmatch(r'(.*?)([A-Za-z_]\w*)', param)
                assert m, f'{name}: parameter {param!r}'
                out[name].append((m.group(1).strip(), m.group(2)))
    return out


def streamed_exports():
    """The exports whose last parameter is a pointer named `stream`, sorted."""
    return sorted(name for name, params in header_parameters().items()
                  if params and params[-1][1] == 'stream' and params[-1][0].endswith('*'))


# ------------------------------------------------------------------------------------------------ the delay
_cycles_per_ms = None


def cycles_per_ms():
    """torch.cuda._sleep's cycles in a millisecond, from three timed sleeps (the fastest clock of the three, so that a
    delay sized by it is not short); once per process."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        import torch
        torch.cuda._sleep(1_000_000)                                  # (the first launch loads the kernel)
        torch.cuda.synchronize()
        rates = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(5_000_000)
            b.record()
            b.synchronize()
            rates.append(5_000_000 / a.elapsed_time(b))
        _cycles_per_ms = max(rates)
    return _cycles_per_ms


def delay(stream, ms=None, timed=False):
    """A device-side wait of at least `ms` (default DELAY_MS) enqueued on `stream`; timed: -> the two events around it."""
    import torch
    cycles = int(1.25 * (DELAY_MS if ms is None else ms) * cycles_per_ms())
    with torch.cuda.stream(stream):
        if not timed:
            torch.cuda._sleep(cycles)
            return None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        return a, b


# ------------------------------------------------------------------------------------------------ the positive controls
def control_copy_off_the_stream(side, ms=None):
    """(a) a delay on `side`, a producer on `side`, a copy of the producer's output enqueued on the null stream
    -> what the copy holds: 0. the stale values, 1. the producer's."""
    import torch
    null = torch.cuda.default_stream()
    x = torch.zeros(1 << 16, dtype=torch.float32, device='cuda')
    y = torch.full((1 << 16,), -1., dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    delay(side, ms)
    with torch.cuda.stream(side):
        x.fill_(1.)
    with torch.cuda.stream(null):
        y.copy_(x)
    torch.cuda.synchronize()
    lo, hi = float(y.min()), float(y.max())
    return lo if lo == hi else -1.                                    # (-1.: the copy ran while the producer wrote)


def control_consumer_on_the_stream(side, ms=None):
    """(b) a delay on the null stream, a producer on the null stream, a consumer on `side` with `side` alone synchronised
    -> what the consumer saw: 0. the stale values, 1. the producer's."""
    import torch
    null = torch.cuda.default_stream()
    x = torch.zeros(1 << 16, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    delay(null, ms)
    with torch.cuda.stream(null):
        x.fill_(1.)
    with torch.cuda.stream(side):
        seen = x.cpu()                                                # (a blocking copy: it synchronises `side` alone)
        side.synchronize()
    torch.cuda.synchronize()
    lo, hi = float(seen.min()), float(seen.max())
    return lo if lo == hi else -1.


def separates(side, ms=None):
    """Both controls fire on `side`: work put on the null stream is not ordered with it by accident."""
    return control_copy_off_the_stream(side, ms) == 0. and control_consumer_on_the_stream(side, ms) == 0.


_side = None


def side_stream():
    """(stream, index): the first of up to CANDIDATES fresh torch.cuda.Stream() objects on which both controls fire, chosen
    once per process; (None, None) where none separates from the null stream."""
    global _side
    if _side is None:
        import torch
        _side = (None, None)
        kept = []                                                     # (a dropped Stream object changes nothing in the pool)
        for k in range(CANDIDATES):
            kept.append(torch.cuda.Stream())
            if separates(kept[-1]):
                _side = (kept[-1], k)
                break
    return _side


# ------------------------------------------------------------------------------------------------ the proxy
class _Export:
    """One streamed export behind the proxy: the checks, then the library's own function with the same arguments."""

    def __init__(self, proxy, name, fn):
        self._proxy, self._name, self._fn = proxy, name, fn

    def __getattr__(self, attr):                                      # argtypes, restype, ...
        return getattr(self._fn, attr)

    def __call__(self, *args):
        import torch
        proxy, name = self._proxy, self._name
        tensors = proxy.take_pointers()
        current = torch.cuda.current_stream()
        handle = args[-1].value if isinstance(args[-1], C.c_void_p) else args[-1]
        problem = None
        if not handle:
            problem = f'{name}: called with a NULL stream'
        elif handle != current.cuda_stream:
            problem = f'{name}: called with stream {handle:#x}, the thread\'s current stream is {current.cuda_stream:#x}'
        if problem is None and proxy.mode == 'late_stream':
            seen, copies = set(), []
            for t in tensors:
                key = (t.data_ptr(), t.numel() * t.element_size())
                if t.is_cuda and t.numel() and key not in seen:
                    seen.add(key)
                    copies.append((t, t.clone()))                     # the first touch of the inputs on S
            proxy.timed_delay(current)
            for t, copy in copies:
                t.copy_(copy)
            del copies
        elif problem is None and proxy.mode == 'late_null':
            proxy.timed_delay(torch.cuda.default_stream())
        t0 = time.perf_counter()
        rc = None if problem else self._fn(*args)
        with proxy.lock:
            proxy.calls.append((name, handle or 0, time.perf_counter() - t0))
            if problem:
                proxy.problems.append(problem)
        assert problem is None, problem
        return rc


class Proxy:
    """Stands in for the ctypes library object.  calls: (export, stream handle, host seconds) of every streamed call;
    problems: the handle check's findings (kept here as well as raised, should a caller swallow the exception)."""

    def __init__(self, real, mode):
        assert mode in MODES + ('check',), mode
        self._real, self.mode = real, mode
        self._streamed = set(streamed_exports())
        self._local = threading.local()
        self.lock = threading.Lock()
        self.calls, self.problems, self.events, self._timed = [], [], None, False

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self._streamed:
            if name.startswith('ssrs_'):
                self.take_pointers()
            return fn
        return _Export(self, name, fn)

    def note_pointer(self, t):
        if t is not None:
            if getattr(self._local, 'tensors', None) is None:
                self._local.tensors = []
            self._local.tensors.append(t)

    def take_pointers(self):
        """The tensors handed to _native.ptr() in this thread since the last library call."""
        out = getattr(self._local, 'tensors', None) or []
        self._local.tensors = []
        return out

    def timed_delay(self, stream):
        """The delay on `stream`; the first one of this proxy between two events."""
        with self.lock:
            first, self._timed = not self._timed, True
        if first:
            self.events = delay(stream, timed=True)
        else:
            delay(stream)

    def seen(self):
        return sorted({name for name, _, _ in self.calls})

    def achieved_ms(self):
        """The length of the first delay, by its events (after the streams were synchronised)."""
        a, b = self.events
        return a.elapsed_time(b)


@contextlib.contextmanager
def watching(mode):
    """The proxy in place of ssrs_amd._native._lib, and _native.ptr noting the tensors it is given; both put back."""
    from ssrs_amd import _native as nat
    real, real_ptr = nat.lib(), nat.ptr
    proxy = Proxy(real, mode)

    def ptr(t):
        proxy.note_pointer(t)
        return real_ptr(t)

    nat._lib, nat.ptr = proxy, ptr
    try:
        yield proxy
    finally:
        nat._lib, nat.ptr = real, real_ptr
