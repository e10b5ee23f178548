"""The grid choice of the RAT-SPN slice mapping without a device (csrc/ratspn_gemm_slice.hip: slice_grid through
dps_slice_grid, include/deeprob_slice.h): a launch that shares the compute units with others takes the fewest work-groups
that finish in the same number of block rounds as its share would, and the lane count a caller states round-trips through
the flags of dpk_ratspn_forward."""
import os
import re
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cdiv(a, b):
    return -(-a // b)


def test_slice_header_parses_and_the_library_exports_it():
    from deeprob import hip
    from deeprob.hip import slice as sl
    text = open(os.path.join(ROOT, 'include', 'deeprob_slice.h')).read()
    sigs, consts, structs = hip.parse_header(text, prefix='dps', header='deeprob_slice.h')
    assert sigs == sl.SIGNATURES and not structs
    assert sorted(sigs) == ['dps_slice_grid', 'dps_slice_lanes', 'dps_slice_last_grid', 'dps_slice_last_lanes']
    declared = re.findall(r'\b(dps_\w+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    assert sorted(declared) == sorted(set(declared)) == sorted(sigs), 'every entry point is declared once'
    # the exports of the library with this prefix are exactly the header's (its .dynsym, read without binutils)
    data = open(hip.LIB_PATH, 'rb').read()
    shoff, = struct.unpack_from('<Q', data, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', data, 0x3A)
    sections = [struct.unpack_from('<IIQQQQIIQQ', data, shoff + i * shentsize) for i in range(shnum)]
    exported = set()
    for _, sh_type, _, _, offset, size, link, _, _, entsize in sections:
        if sh_type != 11:
            continue
        str_off = sections[link][4]
        for k in range(size // entsize):
            st_name, st_info, _, st_shndx = struct.unpack_from('<IBBH', data, offset + k * entsize)
            if st_shndx != 0 and (st_info & 0xF) == 2:
                end = data.index(b'\0', str_off + st_name)
                exported.add(data[str_off + st_name:end].decode())
    assert {n for n in exported if n.startswith('dps_')} == set(sigs)
    assert (sl.DPS_LANES_MAX, sl.DPS_AUTO_LANES_MAX, sl.DPS_AUTO_STREAK, sl.DPS_AUTO_RECHECK) == (15, 4, 4, 8)
    assert sl.DPS_LANES_MAX == hip.DPK_FLAG_SLICE_LANES_MASK >> hip.DPK_FLAG_SLICE_LANES_SHIFT


def test_grid_sweep():
    from deeprob.hip import slice as sl
    fn = sl.load_library().dps_slice_grid
    for cus in (256, 304):
        for np_ in (0, 13):
            for lanes in range(1, 9):
                share = cus // lanes
                for ntiles in range(1, 4097):
                    g = fn(ntiles, cus, lanes, np_)
                    if lanes == 1:
                        assert g == min(ntiles, cus), (ntiles, cus, np_)
                        continue
                    gmax = max(share, min(np_, ntiles))
                    ok = (1 <= g <= gmax and _cdiv(ntiles, g) == _cdiv(ntiles, gmax) and g >= min(np_, ntiles)
                          and (share < np_ or g * lanes <= cus))
                    assert ok, (ntiles, cus, lanes, np_, g)


def test_grid_examples_and_edges():
    from deeprob.hip import slice as sl
    # three chains of 85 compute units: 1024 blocks -> 13 rounds -> 79 work-groups; 256 blocks -> 4 rounds -> 64
    assert sl.grid(1024, 256, 3) == 79 and sl.grid(256, 256, 3) == 64
    # the headline batch on two streams: 2048 blocks, 16 rounds on half the chip
    assert sl.grid(2048, 256, 2) == 128 and sl.grid(2048, 256, 2, 13) == 128
    # a share smaller than the hashing work-groups of an in-launch table check: those come first
    assert sl.grid(14, 64, 8, 13) == 13 and sl.grid(5, 64, 8, 13) == 5 and sl.grid(14, 64, 8, 0) == 7
    # nothing to do, no device, more lanes than compute units, lane counts below 1
    assert sl.grid(0, 256, 2) == 0 and sl.grid(8, 0, 2) == 0 and sl.grid(-3, 256, 1) == 0
    assert sl.grid(100, 4, 8) == 1 and sl.grid(100, 256, 0) == 100 and sl.grid(1000, 256, -2) == 256
    # the largest launch: 64 blocks per work-group (the kernel's mask of blocks left to the exact evaluation)
    for lanes in (1, 2, 3, 8):
        gmax = 256 // lanes
        assert _cdiv(64 * gmax, sl.grid(64 * gmax, 256, lanes)) == 64


def test_lane_count_round_trips_through_the_flags():
    from deeprob import hip
    from deeprob.hip import ops
    assert (hip.DPK_FLAG_SLICE_LANES_SHIFT, hip.DPK_FLAG_SLICE_LANES_MASK) == (8, 3840)
    others = (hip.DPK_FLAG_STRUCT_CACHED | hip.DPK_FLAG_UNIT_SCALE | hip.DPK_FLAG_PARAMS_CACHED | hip.DPK_FLAG_PARAMS_VERIFY |
              hip.DPK_FLAG_IN_PIXEL_MAJOR | hip.DPK_FLAG_OUT_PIXEL_MAJOR | hip.DPK_FLAG_LL_SUM_SPREAD)
    assert others & hip.DPK_FLAG_SLICE_LANES_MASK == 0 and ops.slice_lanes_flag(None) == 0
    for lanes in range(1, 16):
        f = ops.slice_lanes_flag(lanes)
        assert f & others == 0 and ops.slice_lanes_of(f | others) == lanes and (f | others) & others == others
    assert ops.slice_lanes_of(others) == 0
    for bad in (0, -1, 16):
        with pytest.raises(ValueError):
            ops.slice_lanes_flag(bad)


def test_lanes_knob_returns_the_previous_setting():
    from deeprob.hip import slice as sl
    first = sl.lanes(2)
    try:
        assert sl.lanes(1) == 2 and sl.lanes(0) == 1 and sl.lanes(99) == 0 and sl.lanes(-1) == sl.DPS_LANES_MAX
        assert sl.lanes(0) == min(max(int(os.environ.get('DPK_SLICE_LANES', '0')), 0), sl.DPS_LANES_MAX)   # (the initial value)
    finally:
        sl.lanes(first)
