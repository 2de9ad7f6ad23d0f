"""tests/dirty_memory.py on CPU tensors: what the arena hands out, what it leaves alone, what its guards report, and
that every factory ssrs_amd/*.py allocates with is one it covers."""
import ast
import glob
import os

import numpy as np
import pytest
import torch

from dirty_memory import ALIGN, CANARY, COVERED, GUARD, dirty

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _buffer_of(arena, t):
    (b,) = [b for b in arena.buffers if b.raw.data_ptr() + b.lead == t.data_ptr()]
    return b


def test_guard_geometry():
    assert GUARD % 256 == 0 and GUARD >= 64 * 1024 and ALIGN == 256 and CANARY not in (0x00, 0xFF)


@pytest.mark.parametrize('fill, f64, i32', [(0x00, 0., 0), (0xFF, np.nan, -1)])
def test_empty_in_every_calling_convention(fill, f64, i32):
    with dirty(fill, 'cpu') as arena:
        made = [
            torch.empty(3, 5),                                               # varargs, default dtype and device
            torch.empty((3, 5)),                                             # a tuple
            torch.empty([3, 5], dtype=torch.float64),                        # a list, dtype=
            torch.empty(torch.Size((3, 5)), dtype=torch.float64, device='cpu'),
            torch.empty(3, 5, dtype=torch.float64, device=torch.device('cpu')),
            torch.empty(size=(3, 5), dtype=torch.float64),
            torch.empty((np.int64(3), np.int32(5)), dtype=torch.float64),    # numpy integers, as shapes often are
        ]
        ints = [torch.empty(7, dtype=dt) for dt in (torch.int8, torch.int16, torch.int32, torch.int64)]
        mask = torch.empty(9, dtype=torch.uint8)
        none = torch.empty(0, dtype=torch.float32)
        scalar = torch.empty((), dtype=torch.float64)
        assert len(arena.buffers) == len(made) + len(ints) + 3 and not arena.passed
        for t in made:
            assert tuple(t.shape) == (3, 5) and t.is_contiguous() and t.data_ptr() % 256 == 0
            assert np.array_equal(t.numpy(), np.full((3, 5), f64, t.numpy().dtype), equal_nan=True)
        assert made[0].dtype == torch.get_default_dtype() and made[2].dtype == torch.float64
        for t in ints:
            assert t.data_ptr() % 256 == 0 and (t == i32).all()
        assert (mask == (fill & 0xFF)).all() and none.numel() == 0 and scalar.dim() == 0
        arena.assert_clean()
        # the payload is followed by canaries up to the next multiple of 256 and a whole guard on either side
        b = _buffer_of(arena, mask)
        assert b.nbytes == 9 and b.lead >= GUARD and b.raw.numel() - b.lead - 256 >= GUARD
        assert (b.raw[:b.lead] == CANARY).all() and (b.raw[b.lead + 9:] == CANARY).all()


def test_zeros_full_and_like_keep_their_values_and_get_guards():
    with dirty(0xFF, 'cpu') as arena:
        src = torch.arange(12, dtype=torch.int16).reshape(3, 4)
        assert not arena.buffers                                             # arange is no covered factory
        z = [torch.zeros(2, 3), torch.zeros((2, 3), dtype=torch.int64), torch.zeros(size=(2, 3), device='cpu')]
        f = [torch.full((2, 3), 7), torch.full((2, 3), 1.5), torch.full((2, 3), -2, dtype=torch.int16),
             torch.full(size=(2, 3), fill_value=True), torch.full((2, 3), fill_value=np.nan, dtype=torch.float64)]
        like = [torch.empty_like(src), torch.zeros_like(src), torch.full_like(src, 9),
                torch.empty_like(src, dtype=torch.float32), torch.zeros_like(src, dtype=torch.float64, device='cpu'),
                torch.full_like(src, fill_value=2.5, dtype=torch.float64)]
        assert len(arena.buffers) == len(z) + len(f) + len(like)
        assert all((t == 0).all() and t.data_ptr() % 256 == 0 for t in z) and z[1].dtype == torch.int64
        assert [t.dtype for t in f] == [torch.int64, torch.get_default_dtype(), torch.int16, torch.bool, torch.float64]
        assert (f[0] == 7).all() and (f[1] == 1.5).all() and (f[2] == -2).all() and f[3].all() and f[4].isnan().all()
        assert all(tuple(t.shape) == (3, 4) and t.data_ptr() % 256 == 0 for t in like)
        assert like[0].dtype == torch.int16 and (like[0] == -1).all()       # empty_like: the fill
        assert (like[1] == 0).all() and (like[2] == 9).all() and like[3].isnan().all()
        assert like[4].dtype == torch.float64 and (like[4] == 0).all() and (like[5] == 2.5).all()
        assert torch.zeros(2, requires_grad=True).requires_grad
        arena.assert_clean()


def test_leavings_hand_a_dropped_buffer_out_again_untouched():
    with dirty('leavings', 'cpu') as arena:
        a = torch.empty(100, dtype=torch.int32)
        assert (a == 0).all()                                                # a fresh block
        a.copy_(torch.arange(100, dtype=torch.int32))
        keep = torch.empty(100, dtype=torch.int32)                           # `a` is alive: not aliased
        assert keep.data_ptr() != a.data_ptr() and arena.reused == 0
        keep.fill_(5)
        where = a.data_ptr()
        view = a[10:20]
        del a
        other = torch.empty(100, dtype=torch.int32)
        assert other.data_ptr() != where and arena.reused == 0               # a view still holds it
        del view
        b = torch.empty(50, dtype=torch.int64)                               # same bytes, another dtype: what a left
        assert b.data_ptr() == where and arena.reused == 1
        assert np.array_equal(b.numpy().view(np.int32), np.arange(100, dtype=np.int32))
        del b
        c = torch.empty(30, dtype=torch.int32)                               # smaller: the head of it, canaries behind
        assert c.data_ptr() == where and np.array_equal(c.numpy(), np.arange(30, dtype=np.int32))
        assert (_buffer_of(arena, c).raw[_buffer_of(arena, c).lead + 120:] == CANARY).all()
        z = torch.zeros(100, dtype=torch.int32)                              # zeros never inherit
        assert (z == 0).all() and (keep == 5).all()
        arena.assert_clean()


def test_leavings_keep_the_violation_of_a_buffer_that_is_handed_out_again():
    with dirty('leavings', 'cpu') as arena:
        a = torch.empty(64, dtype=torch.float32)
        b = _buffer_of(arena, a)
        b.raw[b.lead + 256] = 0
        del a, b
        again = torch.empty(64, dtype=torch.float32)
        assert arena.reused == 1
        (v,) = arena.violations()
        assert v['offset'] == 256 and v['side'] == 'after'


def test_the_other_device_type_out_and_pin_memory_pass_through():
    with dirty(0xFF, 'cuda') as arena:                                       # a 'cuda' arena leaves CPU tensors alone
        t = torch.empty(4, 4)
        z = torch.zeros(4, device='cpu')
        e = torch.empty_like(z)
        assert not arena.buffers and (z == 0).all() and e.shape == z.shape and t.shape == (4, 4)
    with dirty(0xFF, 'cpu') as arena:
        out = torch.ones(6)
        got = torch.zeros(6, out=out)
        assert got is out and (out == 0).all()
        # (pinning needs a GPU runtime: the decision is asked for, not the allocation)
        assert arena._wants('cpu', {'pin_memory': True}) is None and arena._wants('cpu', {'pin_memory': False}) is not None
        meta = torch.empty(3, device='meta')
        assert meta.device.type == 'meta' and not arena.buffers
        sparse = torch.zeros(3, 3, layout=torch.sparse_coo)
        assert sparse.layout is torch.sparse_coo and arena.passed == [('layout', 'torch.sparse_coo')]
        nc = torch.arange(12.).reshape(3, 4).t()
        assert torch.empty_like(nc).stride() == nc.stride() and len(arena.passed) == 2   # strides kept: torch's own
        assert len(arena.buffers) == 0


def test_factories_come_back_after_an_exception_and_nesting_is_refused():
    before = {name: getattr(torch, name) for name in COVERED}
    with pytest.raises(ZeroDivisionError):
        with dirty(0x00, 'cpu'):
            assert torch.empty is not before['empty']
            1 / 0
    assert {name: getattr(torch, name) for name in COVERED} == before
    with dirty(0x00, 'cpu'):
        with pytest.raises(RuntimeError, match='one arena at a time'):
            with dirty(0xFF, 'cpu'):
                pass
        assert torch.empty is not before['empty']                            # the outer arena is still in place
    assert {name: getattr(torch, name) for name in COVERED} == before
    with pytest.raises(ValueError):
        with dirty(0x7F, 'cpu'):
            pass
    assert torch.empty is before['empty']


def test_planted_overrun_and_underrun_are_reported_with_buffer_and_offset():
    with dirty(0xFF, 'cpu') as arena:
        fine = torch.empty(11, dtype=torch.float64)
        over = torch.empty((3, 7), dtype=torch.float32)                      # 84 bytes: the pad begins at byte 84
        under = torch.zeros(40, dtype=torch.int16)
        far = torch.empty(256, dtype=torch.uint8)                            # no pad: the guard begins at byte 256
        arena.assert_clean()
        b = _buffer_of(arena, over)
        b.raw[b.lead + 84] = 0                                               # one byte after the payload
        b = _buffer_of(arena, under)
        b.raw[b.lead - 1] = 0                                                # one byte before it
        b = _buffer_of(arena, far)
        b.raw[b.lead + 256 + GUARD - 1] = 1                                  # the guard's last byte
        b.raw[b.lead + 256 + 5] = 1
        found = {v['shape']: v for v in arena.violations()}
        assert set(found) == {(3, 7), (40,), (256,)}
        assert found[(3, 7)]['dtype'] == torch.float32 and found[(3, 7)]['offset'] == 84
        assert found[(3, 7)]['side'] == 'after' and found[(3, 7)]['factory'] == 'empty'
        assert found[(40,)]['dtype'] == torch.int16 and found[(40,)]['offset'] == -1
        assert found[(40,)]['side'] == 'before' and found[(40,)]['factory'] == 'zeros'
        assert found[(256,)]['offset'] == 261 and found[(256,)]['changed_bytes'] == 2
        with pytest.raises(AssertionError, match=r'offset 84 \(after the 84-byte payload\)'):
            arena.assert_clean()
        assert (fine.isnan()).all()


# Factories of ssrs_amd/*.py that the arena does not replace, each because its tensor has no uninitialised payload and is no
# kernel's workspace or output:
HOST_ONLY = {
    'from_numpy',        # wraps a host array (always a CPU tensor); _device.to_dev copies it to the device with .to()
    'tensor',            # distributed.gather_lengths: one element count from a host int, for all_gather
}
# every callable of torch that makes a new tensor from a shape or a pattern tensor; anything of this list that the package
# starts to use must be covered by the arena or argued into HOST_ONLY
FACTORIES = {'empty', 'zeros', 'ones', 'full', 'empty_like', 'zeros_like', 'ones_like', 'full_like', 'empty_strided',
             'rand', 'randn', 'randint', 'rand_like', 'randn_like', 'randint_like', 'arange', 'linspace', 'logspace', 'eye',
             'tensor', 'as_tensor', 'from_numpy', 'frombuffer', 'asarray', 'scalar_tensor', 'tril_indices', 'triu_indices'}


def test_every_factory_of_the_package_is_covered_by_the_arena():
    used = {}
    files = sorted(glob.glob(os.path.join(ROOT, 'ssrs_amd', '*.py')))
    assert len(files) > 10
    for path in files:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
                continue
            name, base = node.func.attr, node.func.value
            if isinstance(base, ast.Name) and base.id == 'torch' and name in FACTORIES:
                used.setdefault(name, []).append(f'{os.path.basename(path)}:{node.lineno}')
            elif name.startswith('new_'):                                    # tensor.new_empty / new_zeros / new_full ...
                used.setdefault('.' + name, []).append(f'{os.path.basename(path)}:{node.lineno}')
    assert 'empty' in used and 'zeros' in used                               # the walk finds what is there
    uncovered = {name: where for name, where in used.items() if name not in COVERED and name not in HOST_ONLY}
    assert not uncovered, f'allocated outside the arena: {uncovered}'
    assert not HOST_ONLY - set(used), 'HOST_ONLY lists a factory the package no longer uses'
