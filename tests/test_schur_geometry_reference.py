"""The cases of tests/schur_geometry_cases.py on the CPU: the fp64 oracle against the extended-precision reference of tests/schur_cases.py (the reduced system
entry by entry on the scale A).  The errors measured here are e(oracle) of schur_geometry_cases.TABLE: the bounds of tests/test_gpu_schur_geometry.py derive
from them."""
import numpy as np
import pytest

import schur_geometry_cases as gc


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_oracle_against_the_extended_reference(name):
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    e = gc.measure(name)
    print("e(oracle) %s: %s" % (name, ", ".join("%s=%.3g" % kv for kv in e.items())))
    t = gc.TABLE[name]
    assert e["n_terms"] == t["n_terms"]
    for k in ("S", "b"):
        assert e[k] < 1e-9, (k, e[k])
        assert e[k] <= 2.0 * t[k] and t[k] <= 2.0 * max(e[k], 2.0 ** -60), "schur_geometry_cases.TABLE[%r][%r] = %.3g, measured %.3g: measure again and update the table" % (name, k, t[k], e[k])
