"""An arena that stands in for torch's tensor factories, so that a kernel runs on dirty, guarded memory.

    with dirty(0xFF) as arena:
        out = layers.something(...)          # every torch.empty / zeros / full / *_like of the wrapper lands in the arena
        arena.assert_clean()

Inside the block each factory call for a tensor of the target device type gets ONE flat uint8 buffer

    [ guard | payload (n bytes) | pad to 256 | guard ]

whose guards and pad hold CANARY and whose payload is returned as a contiguous view of the requested dtype and shape, at
a 256-byte aligned address like torch.empty's own.  `empty` payloads hold the fill:

    0x00         what a fresh process usually sees, and what most of the suite therefore tests;
    0xFF         NaN in f32 / f64, -1 in every integer width, all bits set in masks;
    'leavings'   the payload is not touched: a buffer that an earlier tensor of the arena used and dropped is handed out
                 again first (smallest one that fits), with whatever that tensor left in it.  A buffer counts as dropped
                 when nothing but the arena refers to its storage, so a live tensor is never aliased.  A request that no
                 dropped buffer fits gets a fresh zero payload, as the first call of a process does.

`zeros` and `full` keep their values and get the guards.  CPU tensors (for a 'cuda' arena), out=, pin_memory= and
non-strided layouts pass through to torch untouched.

arena.violations() synchronises once and returns, for every buffer whose canaries changed, its shape, dtype and the byte
offset of the first changed byte relative to the payload's first byte (negative: before the payload; >= nbytes: after).
arena.assert_clean() raises AssertionError with that list.

Limits: the arena sees a stray WRITE only within a guard's width (GUARD bytes) of a buffer it handed out, and it sees no
stray READ at all; a write that lands inside another tensor's payload shows, if at all, in that tensor's values."""
import contextlib
import operator

import torch

GUARD = 64 * 1024            # bytes on each side: a multiple of 256, at least 64 KiB
ALIGN = 256
CANARY = 0xA5                # neither fill, not a plausible f32 / index pattern

# the factories ssrs_amd/*.py allocate device tensors with; test_dirty_memory_host.py checks the package against this set
COVERED = ('empty', 'zeros', 'full', 'empty_like', 'zeros_like', 'full_like')
FILLS = (0x00, 'leavings', 0xFF)

_active = None


def _use_count(raw):
    """Holders of raw's storage (this probe's own temporary included)."""
    return torch._C._storage_Use_Count(raw.untyped_storage()._cdata)


class _Buffer:
    __slots__ = ('raw', 'lead', 'cap', 'nbytes', 'shape', 'dtype', 'factory', 'idle_count')

    def payload(self):
        return self.raw[self.lead:self.lead + self.nbytes]


class Arena:
    def __init__(self, fill, device_type='cuda'):
        if fill not in FILLS:
            raise ValueError(f'fill is one of {FILLS}, not {fill!r}')
        self.fill = fill
        self.device_type = device_type
        self.buffers = []            # every buffer handed out, in order (a reused one appears once, with its last tenant)
        self.reused = 0              # 'leavings': requests served from a dropped buffer
        self.passed = []             # (factory, reason) of target-device requests that were NOT placed in the arena
        self._orig = {}
        self._stashed = []           # violations of buffers that were handed out again since

    # ---- allocation -------------------------------------------------------------------------------------------------
    def _fresh(self, npad, device):
        raw = self._orig['empty'](GUARD + npad + GUARD + ALIGN, dtype=torch.uint8, device=device)
        b = _Buffer()
        b.raw = raw
        b.lead = GUARD + (-(raw.data_ptr() + GUARD)) % ALIGN
        b.cap = npad
        b.idle_count = _use_count(raw)
        raw.fill_(CANARY)
        return b

    def _dropped(self, npad, device):
        best = None
        for b in self.buffers:
            if b.cap >= npad and b.raw.device == device and _use_count(b.raw) == b.idle_count:
                if best is None or b.cap <= best.cap:      # of equals, the one used last
                    best = b
        return best

    def _place(self, factory, shape, dtype, device, value):
        """value: None for `empty` (the arena's fill), else the number zeros / full ask for."""
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        itemsize = self._orig['empty']((), dtype=dtype).element_size()
        n = numel * itemsize
        npad = -(-n // ALIGN) * ALIGN
        b = self._dropped(npad, device) if (self.fill == 'leavings' and value is None) else None
        if b is not None:
            self.reused += 1
            self.buffers.remove(b)
            seen = self._check(b)                    # the previous tenant's guards, before they are rewritten
            if seen:
                self._stashed.append(seen)
            b.raw[b.lead + n:].fill_(CANARY)         # the previous tenant's tail becomes pad and guard; the payload stays
        else:
            b = self._fresh(npad, device)
            if value is None:
                b.raw[b.lead:b.lead + n].fill_(0xFF if self.fill == 0xFF else 0x00)
        b.nbytes, b.shape, b.dtype, b.factory = n, shape, dtype, factory
        self.buffers.append(b)
        out = b.payload().view(dtype).view(shape)
        if value is not None:
            out.fill_(value)
        return out

    # ---- the patched factories -------------------------------------------------------------------------------------
    def _wants(self, device, kw):
        dev = torch.device(device) if device is not None else _default_device()
        if dev.type != self.device_type:
            return None
        if kw.get('out') is not None or kw.get('pin_memory'):
            return None
        if kw.get('layout', torch.strided) is not torch.strided:
            self.passed.append(('layout', str(kw['layout'])))
            return None
        if dev.type == 'cuda' and dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        return dev

    @staticmethod
    def _finish(t, kw):
        return t.requires_grad_() if kw.get('requires_grad') else t

    def _sized(self, name, value_of):
        orig = self._orig[name]

        def factory(*args, **kw):
            rest = list(args)
            if 'size' in kw:
                size = kw['size']
            elif name == 'full' or (len(rest) == 1 and isinstance(rest[0], (tuple, list, torch.Size))):
                size = rest.pop(0)
            else:
                size, rest = rest, []
            dev = self._wants(kw.get('device'), kw)
            try:
                size = [operator.index(s) for s in size]           # numpy integers too
            except TypeError:
                dev = None
            if dev is None:
                return orig(*args, **kw)
            value = value_of(rest, kw)
            dtype = kw.get('dtype')
            if dtype is None:
                dtype = self._orig['full']((), value).dtype if name == 'full' else torch.get_default_dtype()
            return self._finish(self._place(name, size, dtype, dev, value), kw)
        factory.__name__ = name
        return factory

    def _like(self, name, value_of):
        orig = self._orig[name]

        def factory(other, *args, **kw):
            dev = self._wants(kw.get('device', other.device), kw)
            if dev is not None and kw.get('memory_format') in (None, torch.preserve_format) and not other.is_contiguous():
                self.passed.append((name, 'like a non-contiguous tensor'))
                dev = None
            if dev is None:
                return orig(other, *args, **kw)
            value = value_of(list(args), kw)
            return self._finish(self._place(name, other.shape, kw.get('dtype') or other.dtype, dev, value), kw)
        factory.__name__ = name
        return factory

    def _enter(self):
        fill_value = lambda args, kw: kw['fill_value'] if 'fill_value' in kw else args[0]
        for name in COVERED:
            self._orig[name] = getattr(torch, name)
        made = {
            'empty': self._sized('empty', lambda a, k: None),
            'zeros': self._sized('zeros', lambda a, k: 0),
            'full': self._sized('full', fill_value),
            'empty_like': self._like('empty_like', lambda a, k: None),
            'zeros_like': self._like('zeros_like', lambda a, k: 0),
            'full_like': self._like('full_like', fill_value),
        }
        for name in COVERED:
            setattr(torch, name, made[name])

    def _exit(self):
        for name, f in self._orig.items():
            setattr(torch, name, f)

    # ---- the guards ------------------------------------------------------------------------------------------------
    @staticmethod
    def _check(b):
        before = (b.raw[:b.lead] != CANARY).nonzero()
        after = (b.raw[b.lead + b.nbytes:] != CANARY).nonzero()
        if not before.numel() and not after.numel():
            return None
        if before.numel():
            side, offset = 'before', int(before[0]) - b.lead
        else:
            side, offset = 'after', b.nbytes + int(after[0])
        return {'factory': b.factory, 'shape': b.shape, 'dtype': b.dtype, 'nbytes': b.nbytes, 'side': side,
                'offset': offset, 'changed_bytes': int(before.numel() + after.numel())}

    def violations(self):
        if self.device_type == 'cuda' and torch.cuda.is_available():
            torch.cuda.synchronize()
        found = list(self._stashed)
        if self.buffers:
            flags = torch.stack([(b.raw[:b.lead] != CANARY).any() | (b.raw[b.lead + b.nbytes:] != CANARY).any()
                                 for b in self.buffers]).tolist()
            found += [self._check(b) for b, bad in zip(self.buffers, flags) if bad]
        return found

    def assert_clean(self):
        found = self.violations()
        if found:
            raise AssertionError('writes outside a buffer:\n' + '\n'.join(
                f"  {v['factory']} {v['shape']} {v['dtype']}: first changed byte at offset {v['offset']} "
                f"({v['side']} the {v['nbytes']}-byte payload), {v['changed_bytes']} changed" for v in found))


def _default_device():
    get = getattr(torch, 'get_default_device', None)
    return get() if get is not None else torch.device('cpu')


@contextlib.contextmanager
def dirty(fill, device_type='cuda'):
    """Patch torch's factories for the block; see the module's docstring.  Not re-entrant: the factories are global."""
    global _active
    if _active is not None:
        raise RuntimeError('dirty() is already active: one arena at a time (the patched factories are global)')
    arena = Arena(fill, device_type)
    _active = arena
    try:
        arena._enter()
        yield arena
    finally:
        arena._exit()
        _active = None
