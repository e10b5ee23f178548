"""ctypes binding of ``libdeeprob_hip.so`` (the C ABI declared in ``include/deeprob_hip.h``).

This module is the ONLY place the Python mirror of the DeeProb-kit interface touches native
code.  There is no CPU / PyTorch fallback: if the shared library is missing, or a tensor is not
a contiguous fp32 tensor on a HIP device, the call raises.  PyTorch is used for device memory,
streams and ``torch.distributed`` only.
"""
import ctypes
import os
import re
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get(  # DEEPROB_HIP_LIB: measurement builds of the same ABI (profiles/README)
    'DEEPROB_HIP_LIB', os.path.normpath(os.path.join(_HERE, '..', '..', 'lib', 'libdeeprob_hip.so')))


class HipError(RuntimeError):
    """Raised when the native library or its header is missing, or a C-ABI call reports a failure."""


# ---- the C ABI: include/deeprob_hip.h is its only declaration -------------------------------------------------------
# The prototypes, the DPK_* constants and the argument structs below are read from the header when this module is
# imported; nothing of them is written down a second time.  The header is regular C: comments, `#define NAME value`,
# `typedef struct { ... } name;` and one prototype per `;`.
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', '..', 'include', 'deeprob_hip.h'))

_SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint32_t': ctypes.c_uint32,
            'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float, 'double': ctypes.c_double}


def _ctype(decl: str, named: bool, where: str, header: str = 'deeprob_hip.h'):
    """ctypes type of ``[const] type [*...] [name]``: every pointer is a ``c_void_p``, a scalar must be a known word."""
    if '*' in decl:
        return ctypes.c_void_p
    words = re.sub(r'\bconst\b', ' ', decl).split()
    if named and len(words) > 1:
        words = words[:-1]
    if len(words) != 1 or words[0] not in _SCALARS:
        raise HipError("{}: cannot read the type of '{}' in {}".format(header, decl.strip(), where))
    return _SCALARS[words[0]]


def parse_header(text: str, prefix: str = 'dpk', header: str = 'deeprob_hip.h'):
    """``(signatures, constants, structs)`` of a header text: ``{name: (restype, argtypes)}``, ``{DPK_NAME: int}`` and
    ``{struct name: [(field, ctype)]}``.  Raises HipError on anything it does not understand -- it never guesses.
    ``prefix``: what the entry points (lower case) and constants (upper case) of this header begin with; ``header``: its
    name in error messages."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    constants = {}
    for m in re.finditer(r'^#define\s+(' + prefix.upper() + r'_\w+)[ \t]+(.*)$', text, re.M):
        value = re.fullmatch(r'\(?(-?\d+)u?\)?', m.group(2).strip())
        if value is None:
            raise HipError("{}: cannot read the value '{}' of {}".format(header, m.group(2).strip(), m.group(1)))
        constants[m.group(1)] = int(value.group(1))
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    structs = {}
    for m in re.finditer(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', text, re.S):
        fields = []
        for line in filter(None, (l.strip() for l in m.group(1).split(';'))):
            first, *more = line.split(',')
            base = re.sub(r'[\s\*]*\w+\s*$', '', first)          # the type words in front of the first declarator
            for d in [first[len(base):]] + more:
                fields.append((d.replace('*', '').strip(), _ctype(base + ' ' + d, True, 'struct ' + m.group(2), header)))
        structs[m.group(2)] = fields
    text = re.sub(r'typedef\s+struct\s*\w*\s*\{.*?\}\s*\w+\s*;', '', text, flags=re.S)
    text = re.sub(r'extern\s+"C"\s*\{', '', text)
    signatures = {}
    for stmt in filter(None, (s.strip() for s in text.split(';'))):
        if stmt == '}':            # (closes extern "C")
            continue
        m = re.fullmatch(r'(.+?)\b(' + prefix + r'_\w+)\s*\((.*)\)', stmt, re.S)
        if m is None:
            raise HipError("{}: not a prototype: '{}'".format(header, stmt))
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        if '*' in ret:
            if re.sub(r'\s+', ' ', ret).strip() != 'const char *':
                raise HipError("{}: cannot read the return type '{}' of {}".format(header, ret.strip(), name))
            restype = ctypes.c_char_p
        else:
            restype = _ctype(ret, False, name, header)
        argtypes = [] if params == 'void' else [_ctype(p, True, name, header) for p in params.split(',')]
        signatures[name] = (restype, argtypes)
    return signatures, constants, structs


def _read_header():
    if not os.path.isfile(HEADER_PATH):
        raise HipError("deeprob_hip.h not found at {} -- it is the declaration of the C ABI this binding is built "
                       "from".format(HEADER_PATH))
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


# name -> (restype, argtypes) of every entry point; DPK_OK, DPK_E*, DPK_FLAG_*, DPK_KERNEL_* as module-level names
SIGNATURES, CONSTANTS, _STRUCT_FIELDS = _read_header()
globals().update(CONSTANTS)
LL_SPREAD = 16            # partial sums in front of the count of a spread {sum LL, count} slot (17 doubles)


def _struct(c_name: str, doc: str):
    return type(c_name, (ctypes.Structure,), {'_fields_': _STRUCT_FIELDS[c_name], '__doc__': doc})


FlatSpnCircuit = _struct('dpk_flat_spn_circuit', "sizes and device addresses of a flattened node-graph SPN")
PairsTablesArgs = _struct('dpk_pairs_tables_args', "one layer of dpk_coupling1d_pairs_tables")
BnFoldArgs = _struct('dpk_bn1d_fold_args', "one layer of dpk_bn1d_fold_many")
SpatialTablesArgs = _struct('dpk_spatial_tables_args', "one level of dpk_spatial_tables")
AdamTensor = _struct('dpk_adam_tensor', "one parameter tensor of dpk_adam_step")

# What the operators pass when a module's cached tables were built from parameters whose addresses, shapes and version
# counters are unchanged.  A write through ``param.data`` (hand-written optimisers, clipping, ``.data.copy_`` loaders)
# moves none of those, so by default the belief is CHECKED ON THE DEVICE (DPK_FLAG_PARAMS_VERIFY: one small fingerprint
# launch per table set and call; tables are rebuilt when the bytes differ).  ``trust_version_counters(True)`` restores
# the unchecked fast path (DPK_FLAG_PARAMS_CACHED) for callers that never write through ``.data``.
_trust_versions = False


def trust_version_counters(flag: bool = True) -> bool:
    """Skip the device-side check of cached parameter tables (see above); returns the previous setting."""
    global _trust_versions
    prev, _trust_versions = _trust_versions, bool(flag)
    return prev


def trust_versions() -> bool:
    return _trust_versions


def cached_tables_flag() -> int:
    return DPK_FLAG_PARAMS_CACHED if _trust_versions else DPK_FLAG_PARAMS_VERIFY


_lib = None


def load_library() -> ctypes.CDLL:
    """Load ``libdeeprob_hip.so`` (built in-tree by ``__graft_entry__.build()``) and bind every symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise HipError(
            "libdeeprob_hip.so not found at {} -- build it with `make -C deeprob-kit_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback".format(LIB_PATH)
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)  # AttributeError if the .so and the header disagree
        except AttributeError:
            if 'DEEPROB_HIP_LIB' in os.environ:   # measurement builds of an older ABI (A/B runs): what exists is bound
                continue
            raise
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(rc: int, fn):
    """Raise ``HipError("<name> failed (<rc>): <last error>")`` for the negative result ``rc`` of entry point ``fn``."""
    if rc < 0:
        msg = load_library().dpk_last_error()
        raise HipError("{} failed ({}): {}".format(fn.__name__, rc, msg.decode() if msg else ''))


def call(fn, *args) -> int:
    """``fn(*args)`` for an entry point that returns a status or a ``*_workspace_bytes`` size: the (non-negative) result,
    HipError on a negative one.  The routing calls that read DPK_EUNSUPPORTED as "take the other route", and the knobs
    whose negative results are values, call ``fn`` itself and get the raw code."""
    rc = fn(*args)
    if rc < 0:
        check(rc, fn)
    return rc


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_device_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    """The kernels take contiguous fp32 HIP tensors.  Anything that is not on a HIP device is an error
    (no CPU path); other floating dtypes / layouts are converted on the device."""
    if not t.is_cuda:
        raise HipError(
            "{} lives on '{}': the deeprob HIP path only evaluates tensors on a HIP device "
            "(there is no CPU fallback)".format(name, t.device)
        )
    if t.dtype != torch.float32:
        if not t.is_floating_point():
            raise HipError("{} must be a floating point tensor, got {}".format(name, t.dtype))
        t = t.float()
    return t.contiguous()


def tensors_key(*tensors) -> tuple:
    """These tensors as they are now -- address, version counter, shape (None stays None): what cached tables are keyed
    on.  A write through ``.data`` moves none of the three: see ``cached_tables_flag``."""
    return tuple(None if t is None else (t.data_ptr(), t._version, tuple(t.shape)) for t in tensors)


# ---- one batched table pass per model forward --------------------------------------------------------------------
# DgcSpn.forward (ops_spatial.tables_prepare) and NormalizingFlow's fused forward (ops_flows.flow1d_prepare) rebuild or
# verify the tables of all their layers in one or two launches and mark what they covered with the forward's token; the
# per-layer operators recognise the token while it is in force and pass DPK_FLAG_PARAMS_CACHED.  Forwards do not nest,
# so one token is in force at a time.
_prepare_token = None


def prepare_begin() -> object:
    """Ends the previous pass; the token of a new one, in force from ``prepare_commit`` (after its launches succeeded)."""
    global _prepare_token
    _prepare_token = None
    return object()


def prepare_commit(token):
    global _prepare_token
    _prepare_token = token


def prepare_release():
    global _prepare_token
    _prepare_token = None


def prepared(token) -> bool:
    """Whether ``token`` (what a batched pass marked an object with) is the pass in force."""
    return token is not None and token is _prepare_token


class Workspace:
    """A growable device scratch buffer owned by a module (never shared between streams), and the module's belief about
    the tables the kernels keep in it -- the cached-table protocol of every fused entry point:

    1. the caller forms a key for "the tables built from these tensors" (``tensors_key`` plus route / mode words);
    2. ``tables_flag(key)`` gives the flag to pass (0: build them) and records the key;
    3. ``outcome(rc, fn, out)`` maps the call's result to *out / None / raise* and forgets the tables after a failure;
    4. an operator that lays other tables over the buffer calls ``forget_tables()`` first; a replaced buffer forgets
       everything."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None
        self.struct_key = None  # what the cached structure tables were built from
        self.params_key = None  # what the cached parameter tables were built from
        self._prep_token = None  # the batched pass (see prepare_begin) that last rebuilt / verified the parameter tables ...
        self._prep_key = None    # ... and the key it did so for
        self._retired = []      # outgrown buffers: a captured HIP graph may still address them

    def __del__(self):
        # the library keeps a few words per workspace ADDRESS (fingerprint slots, the marginalised-evidence hint): hand
        # them back before the allocator reuses the memory
        try:
            if _lib is not None:
                for t in [self.buf] + list(self._retired):
                    if t is not None and t.is_cuda:
                        _lib.dpk_workspace_forget(t.data_ptr(), t.numel())
        except Exception:   # (interpreter shutdown: modules may be gone)
            pass

    def get(self, n_bytes: int, device: torch.device) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < n_bytes or self.buf.device != device:
            if self.buf is not None:
                self._retired.append(self.buf)
            self.buf = torch.empty(max(int(n_bytes), 256), dtype=torch.uint8, device=device)
            self.struct_key = None
            self.params_key = None
        return self.buf

    def sized(self, size_fn, *args, device, or_none: bool = False) -> Optional[torch.Tensor]:
        """The buffer, at least ``size_fn(*args)`` bytes (a ``*_workspace_bytes`` entry point).  A negative size raises;
        with ``or_none`` it means "outside this kernel's envelope" and gives None (the caller takes another route)."""
        n = size_fn(*args)
        if n < 0:
            if or_none:
                return None
            check(n, size_fn)
        return self.get(n, device)

    def structure_flag(self, key) -> int:
        """DPK_FLAG_STRUCT_CACHED when the structure tables were built from ``key``; records it."""
        flag = DPK_FLAG_STRUCT_CACHED if self.struct_key == key else 0
        self.struct_key = key
        return flag

    def holds_tables(self, key) -> bool:
        return self.params_key == key

    def tables_flag(self, key, rebuilt: bool = False) -> int:
        """The flag for a call whose parameter tables are keyed by ``key``: DPK_FLAG_PARAMS_CACHED when this forward's
        batched pass covered them, ``cached_tables_flag()`` when an earlier call built them from the same key, else 0 and
        the key is recorded.  ``rebuilt``: the call rebuilds them whatever is there (its structure tables changed)."""
        if self._prep_token is not None and self._prep_token is _prepare_token and self._prep_key == key:
            return DPK_FLAG_PARAMS_CACHED
        if self.params_key == key and not rebuilt:
            return cached_tables_flag()
        self.params_key = key
        return 0

    def tables_built(self, key, token=None):
        """A launch that SUCCEEDED built the tables for ``key`` (record it only then); ``token``: as part of that batched pass."""
        self.params_key = key
        if token is not None:
            self._prep_token, self._prep_key = token, key

    def forget_tables(self):
        self.params_key = None

    def forget_prepared(self):
        self.params_key = None
        self._prep_token = None

    def forget_structure(self):
        """The structure tables and, built on them, the parameter tables."""
        self.struct_key = None
        self.params_key = None

    def outcome(self, rc: int, fn, out, forget_structure: bool = False):
        """Result of a fused call ``rc = fn(...)`` on this workspace: ``out`` when it ran; None for DPK_EUNSUPPORTED (the
        caller takes the per-layer route); HipError otherwise.  Any failure forgets the parameter tables (a failed call
        built nothing), DPK_EUNSUPPORTED on request the structure tables too."""
        if rc == 0:
            return out
        self.params_key = None
        if rc == DPK_EUNSUPPORTED:
            if forget_structure:
                self.struct_key = None
            return None
        check(rc, fn)
