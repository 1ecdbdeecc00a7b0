"""The reference I-slice fixtures against the reference's own code, live (oracle/_ref/libpcamv_ref.so, built from the reference tree by
oracle/Makefile): every fixture of tests/islice_cases.py is made again by the recipe of oracle/gen_golden.py and must be, array for
array and byte for byte, what is committed under tests/golden/.  Skipped where the reference library is absent, or is a prebuilt one from
a harness without refh_code_iframe in a place where the reference tree is not there to build it again."""
import os
import sys

import numpy as np
import pytest

import islice_cases as isc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import refh  # noqa: E402

pytestmark = pytest.mark.skipif(not refh.has("refh_code_iframe"), reason="oracle/_ref/libpcamv_ref.so not built from this harness (needs the reference tree)")


@pytest.mark.parametrize("case", isc.CASES, ids=[isc.name(c)[len("islice_ref_"):] for c in isc.CASES])
def test_fixture_is_what_the_reference_codes(case):
    import gen_golden
    new, old = gen_golden.islice_fixture_data(case), isc.load(case)
    assert sorted(new) == sorted(old)
    for k in new:
        a, b = np.asarray(new[k]), old[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
