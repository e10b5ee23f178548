"""ctypes binding of the grid choice of the RAT-SPN slice mapping (the C ABI declared in ``include/deeprob_slice.h``,
prefix ``dps_``; the entry points live in ``libdeeprob_hip.so``).  The prototypes and the ``DPS_*`` constants are read from
the header with the parser of ``deeprob.hip``; nothing of them is written down a second time.  Host side only: no call
here touches the device.
"""
from deeprob import hip

BINDING = hip.SLICE
SIGNATURES, CONSTANTS = BINDING.signatures, BINDING.constants
globals().update(CONSTANTS)
load_library = BINDING.load           # ``libdeeprob_hip.so`` with the ``dps_`` entry points bound
hip.bound_module(__name__)         # HEADER_PATH and LIB_PATH are views of BINDING


def grid(ntiles: int, cus: int, lanes: int = 1, np: int = 0) -> int:
    """Work-groups of a slice launch over ``ntiles`` blocks of 32 samples on ``lanes`` lanes (``dps_slice_grid``)."""
    return load_library().dps_slice_grid(int(ntiles), int(cus), int(lanes), int(np))


def lanes(n: int) -> int:
    """Process-wide lane count (``dps_slice_lanes``): 0 = as stated / auto, 1 = always the whole chip, n = fixed, negative =
    back to the initial value.  Returns the previous setting."""
    return load_library().dps_slice_lanes(int(n))


def last_grid() -> int:
    """Grid of the most recent slice launch of the process (0 before the first)."""
    return load_library().dps_slice_last_grid()


def last_lanes() -> int:
    """Lane count of the most recent slice launch of the process (0 before the first)."""
    return load_library().dps_slice_last_lanes()
