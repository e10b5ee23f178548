"""ctypes binding of ``libdeeprob_hip.so`` (the C ABI declared in ``include/deeprob_hip.h``).

This module is the ONLY place the Python mirror of the DeeProb-kit interface touches native
code.  There is no CPU / PyTorch fallback: if the shared library is missing, or a tensor is not
a contiguous fp32 tensor on a HIP device, the call raises.  PyTorch is used for device memory,
streams and ``torch.distributed`` only.
"""
from typing import Optional

import torch

from deeprob.hip._binding import Binding, HipError, bound_module, parse_header  # noqa: F401  (re-exported)

# ---- the native libraries: one Binding per header, one shared object per exported prefix ----------------------------
# Each module of this package (learn, clt, dgc, dgcm, spnq, rat, slice) takes its binding from here and adds its operators;
# ALL_BINDINGS is what __graft_entry__.build() checks, BINDINGS what the export test runs over.  A new library is one line here.
MAIN = Binding('hip', 'dpk', env='DEEPROB_HIP_LIB')      # DEEPROB_HIP_LIB: measurement builds (profiles/README)
SLICE = Binding('slice', 'dps', onto=MAIN)               # host-side knobs of a kernel that lives in libdeeprob_hip.so
LEARN = Binding('learn', 'dpl')
# 2 added the ``dpc_cnq_*`` queries of cutset networks (3 added the ``dpc_mar_*`` posterior marginals, 4 the ``dpc_xpc_*`` split of
# the XPC learners: a library without them fails when its symbols are bound)
CLT = Binding('clt', 'dpc', min_abi=2)
DGC = Binding('dgc', 'dpg')
SPNQ = Binding('spnq', 'dpq')
RAT = Binding('rat', 'dpr', not_implemented='DPR_EUNSUPPORTED')
BINDINGS = (MAIN, SLICE, LEARN, CLT, DGC, SPNQ, RAT)
# further headers bound onto a library above: entry points added beside a header whose list is pinned
DGCM = Binding('dgcm', 'dpm', onto=DGC)                  # DgcSpn.posterior_moments, in libdeeprob_dgc.so
EXTENSIONS = (DGCM,)
ALL_BINDINGS = BINDINGS + EXTENSIONS

# name -> (restype, argtypes) of every dpk_ entry point; DPK_OK, DPK_E*, DPK_FLAG_*, DPK_KERNEL_* as module-level names
SIGNATURES, CONSTANTS = MAIN.signatures, MAIN.constants
globals().update(CONSTANTS)
BINDING = MAIN
load_library, check, call, _read_header = MAIN.load, MAIN.check, MAIN.call, MAIN.read_header
bound_module(__name__)        # LIB_PATH, HEADER_PATH and _lib are views of MAIN (tests/buffer_contract.py puts its proxy at _lib)
LL_SPREAD = 16            # partial sums in front of the count of a spread {sum LL, count} slot (17 doubles)

_struct = MAIN.struct
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


# ``call(fn, *args)``: the (non-negative) result of a dpk_ entry point that returns a status or a ``*_workspace_bytes``
# size, HipError("<fn> failed (<rc>): <last error>") on a negative one (``check(rc, fn)`` raises it for a result already in
# hand).  The routing calls that read DPK_EUNSUPPORTED as "take the other route", and the knobs whose negative results are
# values, call ``fn`` itself and get the raw code.


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


def require_model_f32(who: str, t: torch.Tensor, name: str, shape, device: torch.device, keep: list) -> torch.Tensor:
    """``require_device_f32`` of an argument of operator ``who`` that must have ``shape`` (ValueError) and live on the
    model's ``device`` (HipError).  ``keep`` holds what was converted until the launch is queued."""
    if tuple(t.shape) != tuple(shape):
        raise ValueError("{}: expected {} of shape {}, got {}".format(who, name, tuple(shape), tuple(t.shape)))
    t = require_device_f32(t.detach(), name)
    if t.device != device:
        raise HipError("{} lives on '{}', the model on '{}'".format(name, t.device, device))
    keep.append(t)
    return t


def require_labels(who: str, y: torch.Tensor, B: int, classes: int, device: torch.device, trusted: bool = False):
    """``y`` as the contiguous int64 ``[B]`` labels on ``device`` that operator ``who`` passes down.  The kernels clamp a
    label so as not to read past the root's table; a wrong label is the caller's error and is reported here (ValueError),
    at the cost of one read-back of two numbers (``trusted``: the caller drew them itself, no check and no read-back)."""
    yd = y.to(device=device, dtype=torch.int64).contiguous()
    if tuple(yd.shape) != (B,):
        raise ValueError("{}: expected y of shape ({},), got {}".format(who, B, tuple(yd.shape)))
    if B > 0 and not trusted:
        lo, hi = (int(v) for v in torch.stack([yd.min(), yd.max()]).tolist())
        if lo < 0 or hi >= classes:
            raise ValueError("{}: labels must lie in [0, {}), got {} .. {}".format(who, classes, lo, hi))
    return yd


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
            if MAIN.lib is not None:
                for t in [self.buf] + list(self._retired):
                    if t is not None and t.is_cuda:
                        MAIN.lib.dpk_workspace_forget(t.data_ptr(), t.numel())
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
