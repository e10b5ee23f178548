"""ctypes binding of the grid choice of the RAT-SPN slice mapping (the C ABI declared in ``include/deeprob_slice.h``,
prefix ``dps_``; the entry points live in ``libdeeprob_hip.so``).  The prototypes and the ``DPS_*`` constants are read from
the header with the parser of ``deeprob.hip``; nothing of them is written down a second time.  Host side only: no call
here touches the device.
"""
import os

from deeprob import hip
from deeprob.hip import HipError

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', '..', 'include', 'deeprob_slice.h'))


def _read_header():
    if not os.path.isfile(HEADER_PATH):
        raise HipError("deeprob_slice.h not found at {} -- it is the declaration of the C ABI this binding is built "
                       "from".format(HEADER_PATH))
    with open(HEADER_PATH) as f:
        return hip.parse_header(f.read(), prefix='dps', header='deeprob_slice.h')


SIGNATURES, CONSTANTS, _ = _read_header()
globals().update(CONSTANTS)

_bound = False


def load_library():
    """``libdeeprob_hip.so`` with the ``dps_`` entry points bound."""
    global _bound
    lib = hip.load_library()
    if not _bound:
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError if the .so and the header disagree
            fn.restype = restype
            fn.argtypes = argtypes
        _bound = True
    return lib


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
