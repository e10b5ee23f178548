"""CPU tests of the ctypes binding (deeprob/hip/__init__.py): the ABI generated from include/deeprob_hip.h against
prototypes and struct layouts written out by hand here, and the cached-table protocol of ``Workspace`` with no device."""
import ctypes
import os
import struct

import pytest
import torch

from tests.conftest import ROOT, PKG

V, I, I32, I64, U32, U64, F, D = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32,
                                  ctypes.c_uint64, ctypes.c_float, ctypes.c_double)

# written from the header by hand, one entry per parameter: the independent anchor of the generated table
BY_HAND = {
    'dpk_last_error': (ctypes.c_char_p, []),
    'dpk_abi_version': (I, []),
    'dpk_ratspn_workspace_bytes': (I64, [I32, I32, I32, I32, I32, I32, I32, I32]),
    'dpk_ratspn_slice_batch_min': (I64, [I64]),
    'dpk_ratspn_forward': (I, [V, I64, I32, V, V, V, V, V, V, V, I32, I32, I32, I32, I32, V, V, V, V, I64, U32, V]),
    'dpk_coupling1d_pairs_logprob': (I, [V, I64, I32, I32, V, V, V, V, I32, V, V, V, I32, V, V, V, V, V, V, V, V, I64, U32,
                                         V]),
    'dpk_flat_spn_em_step': (I, [V, I64, I32, V, I64, V, D, V, V, I64, V]),
    'dpk_adam_step': (I, [I32, V, F, F, F, F, F, I32, V, V, V]),
    'dpk_leaf_forward_dropout': (I, [I32, V, I64, I32, V, V, V, V, I32, I32, I32, F, U64, V, V]),
    'dpk_spatial_sumprodroot_workspace_bytes_batch': (I64, [I64, I32, I32, I32, V, I32, V, I32]),
}

STRUCTS_BY_HAND = {       # fields in order; the size follows from 64-bit pointers and natural alignment
    'FlatSpnCircuit': ([(n, I32) for n in ('n_nodes', 'root', 'n_sum', 'n_vars', 'n_child', 'n_cat', 'n_slots', 'max_children')] +
                       [(n, V) for n in ('order', 'kind', 'arg0', 'arg1', 'arg2', 'sum_index', 'child_index', 'child_slot',
                                         'node_slot', 'cat_value', 'child_weight', 'child_logw', 'cat_logp', 'par0', 'par1',
                                         'raw0', 'raw1', 'cat_prob')], 8 * 4 + 18 * 8),
    'PairsTablesArgs': ([(n, V) for n in ('W1', 'b1', 'W2', 'b2', 'in_scale', 'in_shift', 'ws')] +
                        [('ws_bytes', I64), ('D', I32), ('units', I32), ('masked_parity', I32), ('affine', I32), ('flags', U32)],
                        7 * 8 + 8 + 5 * 4 + 4),          # (4 bytes of tail padding: the struct is 8-byte aligned)
    'BnFoldArgs': ([(n, V) for n in ('weight', 'bias', 'running_var', 'running_mean', 'scale_in', 'shift_in', 'scale_out',
                                     'shift_out', 'ldj_const')] +
                   [('eps', F), ('D', I32), ('inverse', I32), ('accumulate', I32)], 9 * 8 + 4 * 4),
    'SpatialTablesArgs': ([('sum_weight', V), ('ws', V), ('ws_bytes', I64), ('root_weight', V), ('C', I32), ('Cout', I32),
                           ('OHW', I32), ('K', I32), ('M', I32)], 4 * 8 + 5 * 4 + 4),
    'AdamTensor': ([('param', V), ('grad', V), ('exp_avg', V), ('exp_avg_sq', V), ('numel', I64)], 5 * 8),
}


def _exported_functions(path):
    """Names of the functions an ELF64 shared object defines and exports (its .dynsym), read without binutils."""
    data = open(path, 'rb').read()
    assert data[:5] == b'\x7fELF\x02'
    shoff, = struct.unpack_from('<Q', data, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', data, 0x3A)
    sections = [struct.unpack_from('<IIQQQQIIQQ', data, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, sh_type, _, _, offset, size, link, _, _, entsize in sections:
        if sh_type != 11:       # SHT_DYNSYM
            continue
        str_off = sections[link][4]
        for k in range(size // entsize):
            st_name, st_info, _, st_shndx = struct.unpack_from('<IBBH', data, offset + k * entsize)
            if st_shndx != 0 and (st_info & 0xF) == 2 and (st_info >> 4) in (1, 2):     # defined FUNC, global / weak
                end = data.index(b'\0', str_off + st_name)
                names.add(data[str_off + st_name:end].decode())
    return names


def test_generated_signatures_match_prototypes_written_by_hand():
    from deeprob import hip
    for name, (restype, argtypes) in BY_HAND.items():
        got_res, got_args = hip.SIGNATURES[name]
        assert got_res is restype, name
        assert len(got_args) == len(argtypes), name
        for k, (g, w) in enumerate(zip(got_args, argtypes)):
            assert g is w, (name, k)
    # the bound functions carry exactly the table's types
    lib = hip.load_library()
    for name, (restype, argtypes) in hip.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_every_exported_entry_point_is_declared_once():
    from deeprob import hip
    exported = {n for n in _exported_functions(os.path.join(PKG, 'lib', 'libdeeprob_hip.so')) if n.startswith('dpk_')}
    assert exported == set(hip.SIGNATURES), exported ^ set(hip.SIGNATURES)
    assert len(hip.SIGNATURES) == 118


def test_constants_come_from_the_header():
    from deeprob import hip
    assert (hip.DPK_OK, hip.DPK_EINVAL, hip.DPK_EWORKSPACE, hip.DPK_ELAUNCH, hip.DPK_EUNSUPPORTED) == (0, -1, -2, -3, -4)
    assert (hip.DPK_FLAG_STRUCT_CACHED, hip.DPK_FLAG_UNIT_SCALE, hip.DPK_FLAG_PARAMS_CACHED, hip.DPK_FLAG_PARAMS_VERIFY,
            hip.DPK_FLAG_IN_PIXEL_MAJOR, hip.DPK_FLAG_OUT_PIXEL_MAJOR, hip.DPK_FLAG_LL_SUM_SPREAD) == (1, 2, 4, 8, 16, 32, 64)
    from deeprob.hip.ops import DPK_FLAG_PARAMS_CACHED      # (the operator modules import them by name)
    assert DPK_FLAG_PARAMS_CACHED == 4


@pytest.mark.parametrize('bad', [
    'int dpk_new_entry(const float *x, long n, void *stream);',            # a scalar type the binding does not know
    'int dpk_new_entry(const float *x, unsigned int n);',
    'size_t dpk_new_workspace_bytes(int32_t n);',
    'float *dpk_new_entry(int32_t n);',                                    # only `const char *` is a known pointer return
    'typedef struct { size_t n; } dpk_new_args;',
    'int dpk_new_entry(int32_t n) { return 0; }',                          # not a prototype
    '#define DPK_FLAG_NEW (1u << 7)',                                      # a value that is not a plain integer
])
def test_parser_raises_on_what_it_does_not_know(bad):
    from deeprob import hip
    good = 'const char *dpk_last_error(void);\nint dpk_ok(const float *x, int64_t n /* rows */, uint64_t seed);\n'
    sigs, consts, structs = hip.parse_header(good + '#define DPK_SOME_FLAG 8u\n#define DPK_EBAD (-7)\n')
    assert sigs == {'dpk_last_error': (ctypes.c_char_p, []), 'dpk_ok': (I, [V, I64, U64])}
    assert consts == {'DPK_SOME_FLAG': 8, 'DPK_EBAD': -7} and structs == {}
    with pytest.raises(hip.HipError):
        hip.parse_header(good + bad)


def test_struct_mirrors_match_layouts_written_by_hand():
    from deeprob import hip
    assert {'dpk_flat_spn_circuit', 'dpk_pairs_tables_args', 'dpk_bn1d_fold_args', 'dpk_spatial_tables_args',
            'dpk_adam_tensor'} == set(hip.parse_header(open(os.path.join(ROOT, 'include', 'deeprob_hip.h')).read())[2])
    for name, (fields, size) in STRUCTS_BY_HAND.items():
        cls = getattr(hip, name)
        assert [f[0] for f in cls._fields_] == [f[0] for f in fields], name
        for (fname, got), (_, want) in zip(cls._fields_, fields):
            assert got is want, (name, fname)
        assert ctypes.sizeof(cls) == size, name
    # a multi-declarator line and a field whose name contains a qualifier as a substring
    _, _, structs = hip.parse_header('typedef struct dpk_t { const float *a, *b; float *ldj_const; int32_t n, m; } dpk_t;')
    assert structs == {'dpk_t': [('a', V), ('b', V), ('ldj_const', V), ('n', I32), ('m', I32)]}


def test_missing_header_is_a_hip_error(monkeypatch):
    from deeprob import hip
    monkeypatch.setattr(hip, 'HEADER_PATH', os.path.join(ROOT, 'include', 'no_such_header.h'))
    with pytest.raises(hip.HipError, match='deeprob_hip.h not found'):
        hip._read_header()


def test_checked_call_names_the_entry_point():
    from deeprob import hip
    lib = hip.load_library()
    assert hip.call(lib.dpk_ratspn_workspace_bytes, 784, 32, 196, 2, 2, 8, 2, 1) > 0
    with pytest.raises(hip.HipError, match=r'dpk_ratspn_workspace_bytes failed \(-1\)'):
        hip.call(lib.dpk_ratspn_workspace_bytes, 0, 32, 196, 2, 2, 8, 2, 1)
    with pytest.raises(hip.HipError, match=r'dpk_product_forward failed \(-1\): .*null'):
        hip.call(lib.dpk_product_forward, None, 4, 8, 3, None, None)
    assert lib.dpk_product_forward(None, 4, 8, 3, None, None) == hip.DPK_EINVAL      # the plain handle returns raw codes
    ws, cpu = hip.Workspace(), torch.device('cpu')
    assert ws.sized(lib.dpk_ratspn_workspace_bytes, 784, 32, 196, 2, 2, 8, 2, 1, device=cpu) is ws.buf
    assert ws.sized(lib.dpk_ratspn_workspace_bytes, 0, 32, 196, 2, 2, 8, 2, 1, device=cpu, or_none=True) is None
    with pytest.raises(hip.HipError, match='dpk_ratspn_workspace_bytes'):
        ws.sized(lib.dpk_ratspn_workspace_bytes, 0, 32, 196, 2, 2, 8, 2, 1, device=cpu)


def test_table_cache_protocol_without_a_device():
    from deeprob import hip
    cpu = torch.device('cpu')
    w, v = torch.zeros(4, 3), torch.zeros(4, 3)
    ws = hip.Workspace()
    ws.get(1024, cpu)
    key = ('route', hip.tensors_key(w, None, v))
    assert hip.tensors_key(w, None) == ((w.data_ptr(), w._version, (4, 3)), None)
    try:
        prev = hip.trust_version_counters(False)
        assert ws.tables_flag(key) == 0                                   # first call: build, key recorded
        assert ws.tables_flag(key) == hip.DPK_FLAG_PARAMS_VERIFY          # same tensors: believed current, device checks
        assert hip.trust_version_counters(True) is False and hip.trust_versions()
        assert ws.tables_flag(key) == hip.DPK_FLAG_PARAMS_CACHED          # the caller vouches for the bytes
        hip.trust_version_counters(False)
        assert ws.tables_flag(('other route', key[1])) == 0               # another entry point's tables over them
        assert ws.tables_flag(key) == 0
        w.add_(1.0)                                                       # an in-place update moves the version counter
        assert ws.tables_flag(('route', hip.tensors_key(w, None, v))) == 0
        key = ('route', hip.tensors_key(w, None, v))
        assert ws.tables_flag(key) == hip.DPK_FLAG_PARAMS_VERIFY
        assert ws.tables_flag(key, rebuilt=True) == 0 and ws.holds_tables(key)
        ws.forget_tables()
        assert not ws.holds_tables(key) and ws.tables_flag(key) == 0
        # structure tables, and a replaced buffer
        skey = hip.tensors_key(v)
        assert ws.structure_flag(skey) == 0 and ws.structure_flag(skey) == hip.DPK_FLAG_STRUCT_CACHED
        assert ws.tables_flag(key) == hip.DPK_FLAG_PARAMS_VERIFY
        old = ws.buf
        assert ws.get(512, cpu) is old and ws.structure_flag(skey) == hip.DPK_FLAG_STRUCT_CACHED      # (no growth)
        assert ws.get(4096, cpu) is not old
        assert ws.struct_key is None and ws.params_key is None
        assert ws.structure_flag(skey) == 0 and ws.tables_flag(key) == 0
        ws.forget_structure()
        assert ws.structure_flag(skey) == 0 and ws.tables_flag(key) == 0
        # outcome of a fused call
        fn = hip.load_library().dpk_product_forward
        out = object()
        ws.structure_flag(skey)
        assert ws.outcome(0, fn, out) is out and ws.holds_tables(key)
        assert ws.outcome(hip.DPK_EUNSUPPORTED, fn, out) is None and not ws.holds_tables(key) and ws.struct_key == skey
        ws.tables_flag(key)
        assert ws.outcome(hip.DPK_EUNSUPPORTED, fn, out, forget_structure=True) is None
        assert ws.struct_key is None and ws.params_key is None
        ws.tables_flag(key)
        with pytest.raises(hip.HipError, match=r'dpk_product_forward failed \(-3\)'):
            ws.outcome(hip.DPK_ELAUNCH, fn, out)
        assert not ws.holds_tables(key)
        # one batched pass per forward: its tables are taken as they are while its token is in force
        token = hip.prepare_begin()
        ws.tables_built(key, token)
        assert ws.tables_flag(key) == hip.DPK_FLAG_PARAMS_VERIFY          # (not committed yet: the launch may still fail)
        hip.prepare_commit(token)
        assert hip.prepared(token) and not hip.prepared(None) and not hip.prepared(object())
        assert ws.tables_flag(key) == hip.DPK_FLAG_PARAMS_CACHED
        assert ws.tables_flag(('other route', key[1])) == 0               # a key the pass did not cover
        hip.prepare_release()
        assert not hip.prepared(token) and ws.tables_flag(key) == 0       # (the other route's key was recorded in between)
        token = hip.prepare_begin()
        ws.tables_built(key, token)
        hip.prepare_commit(token)
        ws.forget_prepared()                                              # the pass's launch failed after all
        assert ws.tables_flag(key) == 0
        hip.prepare_begin()                                               # the next forward ends the previous pass
        assert not hip.prepared(token)
    finally:
        hip.prepare_release()
        hip.trust_version_counters(prev)


@pytest.mark.skipif(torch.cuda.is_available(), reason='with a device the launches succeed')
def test_failed_launch_names_the_first_kernel_without_a_device():
    """With no device every launch fails cleanly, so an entry point that launches several kernels must stop at the first
    and name it: a later launch must not erase (or take the blame for) the failure of an earlier one."""
    import numpy as np
    from deeprob import hip
    lib = hip.load_library()
    ptr = lambda a: a.ctypes.data
    # depthwise 2 x 2 product + root layer: the rows' log-softmax runs before the fused kernel
    C, H, W, OH, OW, K, B = 2, 2, 2, 1, 1, 3, 4
    ws_bytes = lib.dpk_spatial_prodroot_workspace_bytes(C, OH, OW, K)
    assert ws_bytes == 512
    x, weight = np.zeros((B, C, H, W), np.float32), np.zeros((K, C * OH * OW), np.float32)
    out, ws = np.zeros((B, K), np.float32), np.zeros(ws_bytes, np.uint8)
    rc = lib.dpk_spatial_prodroot_forward(ptr(x), B, C, H, W, OH, OW, 2, 2, 1, 1, 1, 1, 0, 0, ptr(weight), K, ptr(out),
                                          ptr(ws), ws_bytes, None)
    assert rc == hip.DPK_ELAUNCH
    assert lib.dpk_last_error().decode().startswith('rowwise_logsoftmax_kernel:'), lib.dpk_last_error()
    # masked linear layer: the masked weights are formed before the product
    n_in, n_out = 3, 2
    ws_bytes = lib.dpk_masked_linear_workspace_bytes(n_in, n_out)
    x, Wt, M = np.zeros((B, n_in), np.float32), np.zeros((n_out, n_in), np.float32), np.ones((n_out, n_in), np.float32)
    b, y, ws = np.zeros(n_out, np.float32), np.zeros((B, n_out), np.float32), np.zeros(ws_bytes, np.uint8)
    rc = lib.dpk_masked_linear_forward(ptr(x), B, n_in, n_out, ptr(Wt), ptr(M), ptr(b), ptr(y), ptr(ws), ws_bytes, None)
    assert rc == hip.DPK_ELAUNCH
    assert lib.dpk_last_error().decode().startswith('maf_mul_kernel:'), lib.dpk_last_error()
