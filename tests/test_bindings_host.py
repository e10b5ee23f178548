"""The registry of native libraries (``deeprob.hip.BINDINGS``) without a device: every shared object exports exactly the
entry points of the headers bound onto it and no name of any other library's prefix, and every library keeps an error text
of its own, per thread."""
import os
import subprocess
import threading

import pytest

from deeprob import hip

LIBRARIES = sorted({b.lib_path for b in hip.BINDINGS})


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], check=True, capture_output=True, text=True).stdout
    return [l.split()[-1] for l in out.splitlines() if l.split()]


def test_registry_is_seven_headers_on_six_libraries():
    assert [b.prefix for b in hip.BINDINGS] == ['dpk', 'dps', 'dpl', 'dpc', 'dpg', 'dpq', 'dpr']
    assert [os.path.basename(p) for p in LIBRARIES] == ['libdeeprob_clt.so', 'libdeeprob_dgc.so', 'libdeeprob_hip.so',
                                                        'libdeeprob_learn.so', 'libdeeprob_rat.so', 'libdeeprob_spnq.so']
    assert hip.SLICE.onto is hip.MAIN and hip.SLICE.lib_path == hip.MAIN.lib_path == hip.LIB_PATH
    for b in hip.BINDINGS:
        if b.onto is None:
            assert b.abi_version() >= 1, b.name


@pytest.mark.parametrize('b', hip.BINDINGS, ids=lambda b: b.name)
def test_library_exports_its_header_and_no_name_of_another_library(b):
    """The defined dynamic symbols of a binding's library with its prefix are exactly its header's names, and the library
    exports no name with the prefix of a binding of another library (all thirty ordered pairs of libraries; the main
    library exports ``dpk_`` and ``dps_`` and nothing of the others)."""
    exported = _exports(b.lib_path)
    mine = sorted(n for n in exported if n.startswith(b.prefix + '_'))
    assert mine == sorted(b.signatures), set(mine) ^ set(b.signatures)
    for other in hip.BINDINGS:
        if other.lib_path != b.lib_path:
            theirs = [n for n in exported if n.startswith(other.prefix + '_')]
            assert not theirs, '{} exports {} of deeprob_{}.h'.format(os.path.basename(b.lib_path), theirs, other.name)


def test_error_text_is_per_library_and_per_thread():
    """Two libraries fail in turn on sizes that are rejected before anything touches the device; each ``*_last_error()``
    still holds its own text after the other has failed, and a thread that has called nothing sees an empty text."""
    from deeprob.hip import rat, spnq
    rlib, qlib = rat.load_library(), spnq.load_library()

    def rat_fails():
        return rlib.dpr_ratspn_moments(0, -1, 15, 2, 3, 3, 5, 1, 4, None, None, 0, None, None, None, None, None, None, None,
                                       None, None)

    def spnq_fails():
        return qlib.dpq_flat_spn_posterior_workspace_bytes(4, None, 0)

    assert rat_fails() == rat.DPR_EINVAL
    rtext = rlib.dpr_last_error()
    assert b'ratspn_moments' in rtext
    assert spnq_fails() == spnq.DPQ_EINVAL
    qtext = qlib.dpq_last_error()
    assert b'bad sizes' in qtext and qtext != rtext
    assert rlib.dpr_last_error() == rtext, 'the failure of libdeeprob_spnq.so overwrote the text of libdeeprob_rat.so'
    assert rat_fails() == rat.DPR_EINVAL
    assert qlib.dpq_last_error() == qtext, 'the failure of libdeeprob_rat.so overwrote the text of libdeeprob_spnq.so'
    seen = []
    t = threading.Thread(target=lambda: seen.extend([rlib.dpr_last_error(), qlib.dpq_last_error()]))
    t.start()
    t.join()
    assert seen == [b'', b''], seen
    assert rlib.dpr_last_error() == rtext and qlib.dpq_last_error() == qtext
