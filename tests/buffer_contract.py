"""Poisoned, guard-banded device memory for the buffer contract of the C ABI (include/deeprob_hip.h, Conventions).

``with contract(pattern) as c:`` replaces, until it exits, the Python-level allocators the operators use --
``torch.empty``, ``torch.empty_like``, ``torch.Tensor.new_empty`` and ``deeprob.hip.Workspace.get`` -- for tensors on a
HIP device (``device_filter`` chooses otherwise: the host tests guard CPU tensors).  Every allocation becomes the interior
of a larger uint8 buffer: GUARD bytes of a fixed pattern on each side, the interior filled ONCE with ``pattern`` (a byte),
the returned tensor a view of exactly the requested bytes with the strides the real allocator would have given.  A reused
``Workspace`` buffer is not poisoned again (its cached tables are legitimate state), and in this mode ``Workspace.get``
hands out exactly ``n_bytes``, so the guard begins where the ``*_workspace_bytes`` answer ends.

It also puts a recording proxy at ``deeprob.hip._lib`` (what every ``load_library()`` returns): ``c.called`` is the set of
``dpk_*`` entry points called inside the context.

``c.check()`` -- run on exit as well -- raises ContractViolation when
  * a guard band of any allocation made inside the context differs from its pattern (a write outside the buffer),
  * a tensor handed to ``c.expect_written(t, ...)`` still holds an element whose bytes are all ``pattern``,
  * a tensor registered with ``c.frozen(*tensors)`` is not bitwise what it was when registered,
and names the allocation: shape, dtype and the Python call site captured when it was made.

Two patterns are in use.  0xFF: an all-ones NaN for f32 / f64 / f16 and -1 for the integers.  0x7F: 3.39e38 for f32,
large positive integers.  Neither is zero, so scratch that is silently taken to be zeroed fails under both, and a kernel
that masks NaN fails under the second.

The context must not be active while a HIP graph is captured (the fills would be captured): allocating then raises.
This is a helper module, not a conftest and not a plugin.
"""
import os
import re
import traceback
from contextlib import contextmanager

import torch

GUARD = 4096            # bytes on each side: keeps the alignment torch's allocators give
GUARD_BYTE = 0xC3
PATTERNS = (0xFF, 0x7F)

_HERE = os.path.abspath(__file__)
_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__))
_active = None


class ContractViolation(AssertionError):
    pass


def hip_devices_only(device: torch.device) -> bool:
    return device.type == 'cuda'


def writer_entry_points(header_text: str):
    """The entry points of a header text that write device memory, in header order: prototypes that return ``int`` and
    have at least one pointer parameter that is neither ``const`` nor the ``stream``."""
    text = re.sub(r'/\*.*?\*/', ' ', header_text, flags=re.S)
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    text = re.sub(r'typedef\s+struct\s*\w*\s*\{.*?\}\s*\w+\s*;', '', text, flags=re.S)
    text = re.sub(r'extern\s+"C"\s*\{', '', text)
    writers = []
    for stmt in filter(None, (s.strip() for s in text.split(';'))):
        m = re.fullmatch(r'(.+?)\b(dpk_\w+)\s*\((.*)\)', stmt, re.S)
        if m is None or m.group(1).split() != ['int']:
            continue
        params = [p.strip() for p in m.group(3).split(',')]
        if any('*' in p and not re.search(r'\bconst\b', p) and not re.search(r'\bstream$', p) for p in params):
            writers.append(m.group(2))
    return writers


def _call_site():
    """'file:line in function' of the innermost frames outside this module and torch, innermost first."""
    frames = [f for f in traceback.extract_stack(limit=14)
              if os.path.abspath(f.filename) != _HERE and not os.path.abspath(f.filename).startswith(_TORCH_DIR)
              and 'contextlib' not in f.filename]
    return ' <- '.join('{}:{} in {}'.format(os.path.relpath(f.filename), f.lineno, f.name) for f in reversed(frames[-3:]))


def _bytes_of(t: torch.Tensor) -> torch.Tensor:
    """The elements of ``t`` as a [numel, itemsize] uint8 tensor (a copy where ``t`` is not contiguous)."""
    t = t.detach()
    if not t.is_contiguous():
        t = t.contiguous()
    return t.reshape(-1).view(torch.uint8).reshape(-1, t.element_size())


class _Allocation:
    __slots__ = ('raw', 'nbytes', 'shape', 'dtype', 'site', 'what')

    def __init__(self, raw, nbytes, shape, dtype, site, what):
        self.raw, self.nbytes, self.shape, self.dtype, self.site, self.what = raw, nbytes, shape, dtype, site, what

    def describe(self):
        return '{} of shape {} {} ({} bytes) allocated at {}'.format(self.what, tuple(self.shape), self.dtype, self.nbytes,
                                                                     self.site)

    def contains(self, t: torch.Tensor) -> bool:
        lo = self.raw.data_ptr() + GUARD
        return t.device == self.raw.device and lo <= t.data_ptr() < lo + max(self.nbytes, 1)


class _Entry:
    """A bound entry point of the library that notes its name when it is CALLED (not when it is looked up)."""

    def __init__(self, fn, name, called):
        self._fn, self.__name__, self._called = fn, name, called

    def __call__(self, *args):
        self._called.add(self.__name__)
        return self._fn(*args)

    def __getattr__(self, name):
        return getattr(self._fn, name)


class _Recorder:
    def __init__(self, lib, called):
        self._lib, self._called, self._entries = lib, called, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('dpk_'):
            return fn
        if name not in self._entries:
            self._entries[name] = _Entry(fn, name, self._called)
        return self._entries[name]


class Contract:
    def __init__(self, pattern: int, device_filter=None):
        assert 0 < int(pattern) <= 0xFF, 'the poison is one non-zero byte'
        self.pattern = int(pattern)
        self.device_filter = device_filter or hip_devices_only
        self.called = set()
        self.allocations = []
        self._expect = []
        self._frozen = []

    # ---- allocation --------------------------------------------------------------------------------------------------
    def _guarded(self, shape, stride, dtype, device, what, requires_grad=False):
        if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('buffer_contract: the contract context must not be active while a HIP graph is captured')
        numel = 1
        for s in shape:
            numel *= int(s)
        itemsize = _orig['empty']((), dtype=dtype, device='meta').element_size()
        nbytes = numel * itemsize
        raw = _orig['empty'](nbytes + 2 * GUARD, dtype=torch.uint8, device=device)
        raw[:GUARD] = GUARD_BYTE
        raw[GUARD + nbytes:] = GUARD_BYTE
        raw[GUARD:GUARD + nbytes] = self.pattern
        self.allocations.append(_Allocation(raw, nbytes, tuple(shape), dtype, _call_site(), what))
        # (a tensor of its own over the interior of raw's storage, not a view of `raw`: autograd then treats an operator's
        # output as it treats one that torch.empty made)
        out = _orig['empty'](0, dtype=dtype, device=device).set_(raw.untyped_storage(), GUARD // itemsize, tuple(shape),
                                                                 tuple(stride))
        if requires_grad:
            out.requires_grad_(True)
        return out

    def _from_meta(self, meta, device, what, requires_grad):
        # (a permuted / channels-last layout is kept, as the real allocator keeps it; anything else comes out contiguous)
        stride = meta.stride() if _dense(meta.shape, meta.stride()) else _orig['empty'](meta.shape, device='meta').stride()
        return self._guarded(meta.shape, stride, meta.dtype, device, what, requires_grad)

    def _wants(self, device, kwargs):
        if kwargs.get('out') is not None or kwargs.get('pin_memory') or kwargs.get('layout', torch.strided) != torch.strided:
            return False
        return self.device_filter(device)

    def _empty(self, *args, **kwargs):
        device = kwargs.get('device')
        device = torch.device(device) if device is not None else _default_device()
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if not self._wants(device, kwargs):
            return _orig['empty'](*args, **kwargs)
        kw = dict(kwargs, device='meta')
        requires_grad = kw.pop('requires_grad', False)
        return self._from_meta(_orig['empty'](*args, **kw), device, 'torch.empty', requires_grad)

    def _empty_like(self, src, **kwargs):
        device = torch.device(kwargs['device']) if kwargs.get('device') is not None else src.device
        if not self._wants(device, kwargs):
            return _orig['empty_like'](src, **kwargs)
        kw = dict(kwargs, device='meta')
        requires_grad = kw.pop('requires_grad', False)
        return self._from_meta(_orig['empty_like'](src, **kw), device, 'torch.empty_like', requires_grad)

    def _new_empty(self, src, *args, **kwargs):
        device = torch.device(kwargs['device']) if kwargs.get('device') is not None else src.device
        if not self._wants(device, kwargs):
            return _orig['new_empty'](src, *args, **kwargs)
        kw = dict(kwargs, device='meta')
        requires_grad = kw.pop('requires_grad', False)
        return self._from_meta(_orig['new_empty'](src, *args, **kw), device, 'Tensor.new_empty', requires_grad)

    def _workspace_get(self, ws, n_bytes, device):
        device = torch.device(device)
        if not self.device_filter(device):
            return _orig['workspace_get'](ws, n_bytes, device)
        if ws.buf is None or ws.buf.numel() < n_bytes or ws.buf.device != device:
            if ws.buf is not None:
                ws._retired.append(ws.buf)
            # exactly n_bytes (not max(n_bytes, 256)): the guard begins where the reported size ends
            ws.buf = self._guarded((int(n_bytes),), (1,), torch.uint8, device, 'Workspace.get')
            ws.struct_key = None
            ws.params_key = None
        return ws.buf

    # ---- what the caller states ----------------------------------------------------------------------------------------
    def expect_written(self, *tensors):
        """These tensors are outputs: at the next check none of their elements may still be the poison."""
        for t in tensors:
            if t is not None:
                self._expect.append((t, _call_site()))
        return tensors[0] if len(tensors) == 1 else tensors

    def frozen(self, *tensors):
        """These tensors are inputs / parameters / buffers of an evaluation: they stay bitwise what they are now."""
        for t in tensors:
            if t is not None:
                self._frozen.append((t, _bytes_of(t).clone(), _call_site()))

    # ---- the checks ----------------------------------------------------------------------------------------------------
    def _describe_tensor(self, t):
        for a in self.allocations:
            if a.contains(t):
                return a.describe()
        return 'tensor of shape {} {} (not allocated inside the context)'.format(tuple(t.shape), t.dtype)

    def violations(self):
        found = []
        by_device = {}
        for a in self.allocations:
            by_device.setdefault(a.raw.device, []).append(a)
        for device, allocs in by_device.items():
            if device.type == 'cuda':
                torch.cuda.synchronize(device)
            bad = torch.stack([(a.raw[:GUARD] != GUARD_BYTE).any() | (a.raw[GUARD + a.nbytes:] != GUARD_BYTE).any()
                               for a in allocs]).cpu()
            for i in bad.nonzero().flatten().tolist():
                a = allocs[i]
                front = (a.raw[:GUARD] != GUARD_BYTE).nonzero().flatten().cpu()
                back = (a.raw[GUARD + a.nbytes:] != GUARD_BYTE).nonzero().flatten().cpu()
                if len(front):
                    found.append('underrun: {} bytes written in front of it, the farthest {} bytes before its start: {}'.format(
                        len(front), GUARD - int(front[0]), a.describe()))
                if len(back):
                    found.append('overrun: {} bytes written behind it, up to {} bytes past its end: {}'.format(
                        len(back), int(back[-1]) + 1, a.describe()))
        for t, site in self._expect:
            if t.numel() == 0:
                continue
            left = (_bytes_of(t) == self.pattern).all(dim=1)
            n = int(left.sum())
            if n:
                first = int(left.nonzero()[0])
                found.append('unwritten: {} of {} elements still hold the poison 0x{:02X} (the first at flat index {}), expected '
                             'written at {}: {}'.format(n, t.numel(), self.pattern, first, site, self._describe_tensor(t)))
        for t, was, site in self._frozen:
            now = _bytes_of(t)
            if now.shape != was.shape or not torch.equal(now, was):
                n = int((now != was).any(dim=1).sum()) if now.shape == was.shape else -1
                found.append('mutated: {} elements of a frozen tensor changed (registered at {}): {}'.format(
                    n, site, self._describe_tensor(t)))
        return found

    def check(self):
        found = self.violations()
        if found:
            raise ContractViolation('buffer contract violated ({}):\n  '.format(len(found)) + '\n  '.join(found))


def _dense(shape, stride) -> bool:
    """Whether these strides address ``prod(shape)`` distinct, gap-free elements (some permutation of contiguous)."""
    expect = 1
    for st, s in sorted((st, s) for s, st in zip(shape, stride) if s != 1):
        if s == 0:
            return True
        if st != expect:
            return False
        expect *= s
    return True


def _default_device():
    get = getattr(torch, 'get_default_device', None)
    return get() if get is not None else torch.device('cpu')


_orig = {}


@contextmanager
def contract(pattern: int, device_filter=None, record: bool = True):
    """See the module docstring.  ``record=False`` leaves the library alone (the host tests have none to load)."""
    global _active
    if _active is not None:
        raise RuntimeError('buffer_contract: contexts do not nest')
    from deeprob import hip
    c = Contract(pattern, device_filter)
    had_new_empty = 'new_empty' in torch.Tensor.__dict__
    _orig.update(empty=torch.empty, empty_like=torch.empty_like, new_empty=torch.Tensor.new_empty,
                 workspace_get=hip.Workspace.get)
    real_lib = None
    if record:
        real_lib = hip.load_library()
    _active = c
    try:
        torch.empty = c._empty
        torch.empty_like = c._empty_like
        torch.Tensor.new_empty = lambda self, *a, **k: c._new_empty(self, *a, **k)
        hip.Workspace.get = lambda self, n_bytes, device: c._workspace_get(self, n_bytes, device)
        if record:
            hip._lib = _Recorder(real_lib, c.called)
        yield c
        c.check()
    finally:
        torch.empty = _orig['empty']
        torch.empty_like = _orig['empty_like']
        if had_new_empty:
            torch.Tensor.new_empty = _orig['new_empty']
        else:
            del torch.Tensor.new_empty
        hip.Workspace.get = _orig['workspace_get']
        if record:
            hip._lib = real_lib
        _active = None
