"""Body of tests/test_flows2d_envelope_gpu.py::test_routes_behind_the_environment_switches, run as a child process
(``python -X faulthandler -m tests._conv2d_route_cases``): dpk_conv2d_forward reads DPK_CONV_MFMA3, DPK_CONV_VALU and
DPK_CONV_LDS once per process, so each switch needs a process of its own.  The child finds the one switch set in its
environment, evaluates that switch's rows of tests/flows2d_cases.py::SWITCH_ROWS against the float64 reference and prints
one line: MARK + json of {'switch': name, 'errors': {row: [error, bound]}}.  The parent asserts the bounds."""
import json
import os

import torch

from tests import flows2d_cases as fc

MARK = 'CONV2D-ROUTE-CASES '


def main():
    mine = [var for var, (value, _, _) in fc.SWITCH_ROWS.items() if os.environ.get(var, '')[:1] == value]
    assert len(mine) == 1, 'exactly one of {} must be set, got {}'.format(sorted(fc.SWITCH_ROWS), mine)
    var = mine[0]
    value, want, names = fc.SWITCH_ROWS[var]
    dev = torch.device('cuda', 0)
    errors = {}
    for name in names:
        case = fc.BY_NAME[name]
        assert fc.route(case.B, case.Cin, case.Cout, case.H, case.W, case.ks, case.mask, os.environ)['route'] == want, name
        inp = fc.make_inputs(case)
        got, whole = fc.run(case, inp, dev)
        err, bound, _ = fc.check_row(case, inp, got)
        assert whole is None or fc.outside_untouched(case, whole), name + ': wrote outside the output slice'
        errors[name] = [err, bound]
    print(MARK + json.dumps(dict(switch=var, errors=errors)), flush=True)


if __name__ == '__main__':
    main()
