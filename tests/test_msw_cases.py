"""Host logic (no GPU): under every option set of tests/msw_cases.py the library's ksw_align2, in both forms, equals the compiled
reference's on the generated mate-rescue requests, and the reference's own results reach what the requests are there for — before any
kernel is involved."""
import numpy as np
import pytest

import msw_cases as mc
from oracle import pyoracle as po


@pytest.mark.parametrize("name", list(mc.OPTION_SETS))
def test_host_align2_equals_reference_and_cases_reach_their_branches(built, name):
    if not po.ref_available():
        pytest.skip("the reference library is not built")
    from mpibwa_amd import api
    lib = api.load_library()
    cs = mc.cases(name)
    ref = mc.reference_results(po.ref_lib(), cs)
    for portable in (0, 1):
        got = mc.host_results(lib, cs, portable)
        bad = np.nonzero((got != ref).any(axis=1))[0]
        assert len(bad) == 0, (name, portable, [(int(i), cs.kind[i], list(got[i]), list(ref[i])) for i in bad[:5]])
    want = mc.Want(cs, ref, mc.host_results(lib, cs, full_width=True))
    mc.check_coverage(name, cs, mc.coverage(want))


def test_generated_cases_hold_what_they_promise():
    """what needs no alignment: l_pac, window bounds, the packed reference, the work list (what a case set must contain is asserted per
    option set by msw_cases.check_coverage)"""
    assert mc.L_PAC % 4 != 0
    for name in ("default", "a5"):
        cs = mc.cases(name)
        dref, pac = cs.dref, cs.pac
        assert len(pac) == mc.L_PAC // 4 + 1
        for p in (0, 1, 2, 3, 4, mc.L_PAC - 1, mc.L_PAC - 2, 12345):
            assert (pac[p >> 2] >> ((~p & 3) << 1)) & 3 == dref[p]
        for i in range(len(cs)):
            assert 0 <= cs.rb[i] <= cs.re[i] <= 2 * mc.L_PAC and (cs.re[i] <= mc.L_PAC or cs.rb[i] >= mc.L_PAC)
        items, word = mc.work_list(cs)
        assert sorted([k for it in items for k in it if k >= 0] + word) == list(range(len(cs)))
