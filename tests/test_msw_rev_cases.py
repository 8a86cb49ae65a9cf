"""Host logic (no GPU): by the compiled reference's ksw_align2 alone, every family of tests/msw_rev_cases.py reaches what it is there
for — the class of every hit, who shares a quad under the pairing rule, where the reverse passes stop — before any kernel is involved."""
import numpy as np
import pytest

import msw_cases as mc
import msw_rev_cases as rv
from oracle import pyoracle as po


def expected(lib, family, name):
    cs = rv.cases(family, name)
    return cs, mc.Want(cs, mc.reference_results(po.ref_lib(), cs), mc.host_results(lib, cs, full_width=True))


@pytest.fixture(scope="module")
def lib(built):
    if not po.ref_available():
        pytest.skip("the reference library is not built")
    from mpibwa_amd import api
    return api.load_library()


def stop_rows(want, pl):
    """rows the reverse pass of a classed request walks before KSW_XSTOP: te - tb + 1"""
    return {i: int(want.res[i][1] - want.res[i][5] + 1) for m in pl["members"].values() for i in m}


def no_silent_start_miss(name, want, pl):
    """tb = -1 on a hit that did not saturate: the reverse pass missed the forward score.  Printed, and none may exist."""
    n = sum(1 for m in pl["members"].values() for i in m if want.res[i][5] < 0 or want.res[i][6] < 0)
    print("msw rev %s: classed hits whose reference record has tb = -1: %d" % (name, n))
    # (under o_ins = 0 the reference has such records: its lazy-F loop ends early, tests/msw_model.py — and mate rescue is the host's)
    assert n == 0 or name in mc.GATED, name


@pytest.mark.parametrize("name", rv.FAMILY_SETS["borders"])
def test_borders_reach_both_ends_of_every_segment_length(lib, name):
    cs, want = expected(lib, "borders", name)
    pl = rv.plan(want)
    o = cs.o
    no_silent_start_miss(name, want, pl)
    # by the reference's own qe: every (read length, s, border) the builder could construct has a classed hit ending exactly there
    got = {(cs.tag[i][1], int(want.res[i][2])) for m in pl["members"].values() for i in m if i in cs.tag}
    built = {(t[1], t[3]) for t in cs.tag.values()}
    assert built <= got, (name, sorted(built - got))
    # what it could not: exactly the stretches shorter than min_seed_len (s = 1 only where min_seed_len <= 16; qe = 0 and 1 never)
    for _, L, s, qe in cs.unreachable:
        assert qe + 1 < o["min_seed_len"] and (qe + 1) * o["a"] < o["min_seed_len"] * o["a"], (name, L, s, qe)
    ss = {(c - 1) // 3 + 1 for c in pl["members"]}
    top = (max(t[1] for t in cs.tag.values()) + 15) // 16
    assert set(range(2, top + 1)) <= ss and ((1 in ss) == (o["min_seed_len"] <= 16)), (name, sorted(ss))
    # partners come from different reads and, somewhere, from different orientations and from behind l_pac
    assert pl["pairs"] and all(cs.rd[x] != cs.rd[y] for x, y in pl["pairs"]), name
    assert any(cs.rev[x] != cs.rev[y] for x, y in pl["pairs"]) and any(cs.rb[x] >= mc.L_PAC for x, y in pl["pairs"]), name
    assert len({(c - 1) % 3 for c in pl["members"]}) >= (3 if max(t[1] for t in cs.tag.values()) >= 86 else 2), name
    print("msw rev borders/%s: requests %d, classes %d, pairs %d, alone %d" % (name, len(cs), len(pl["members"]), len(pl["pairs"]), len(pl["alone"])))


@pytest.mark.parametrize("name", rv.FAMILY_SETS["unequal"])
def test_unequal_partners_share_a_quad(lib, name):
    cs, want = expected(lib, "unequal", name)
    pl = rv.plan(want)
    no_silent_start_miss(name, want, pl)
    rows = stop_rows(want, pl)
    if name in mc.GATED:
        return
    for x, y in cs.partners:
        assert (x, y) in pl["pairs"], (name, x, y, list(want.res[x]), list(want.res[y]))
        short, long_ = (x, y) if rows[x] < rows[y] else (y, x)
        L = cs.tag[long_][1]
        # one stops at the edge of the score class, the other walks the whole read; both have the same segment length
        assert rows[long_] == L and rows[short] == L - cs.tag[short][2] and rows[short] < rows[long_], (name, rows[short], rows[long_])
        if cs.tag[short][3] == 0:   # at the very start of its window: te + 1 rows and not one more
            assert want.res[short][1] + 1 == rows[short] and want.res[short][5] == 0, (name, list(want.res[short]))
    assert max(abs(rows[x] - rows[y]) for x, y in cs.partners) >= 8, name   # (how far apart: by the edge of the read's score class)
    assert any(cs.tag[x][3] == 0 or cs.tag[y][3] == 0 for x, y in cs.partners) and {x < y for x, y in cs.partners} == {True}
    assert {cs.tag[x][2] > 0 for x, y in cs.partners} == {True, False}, "the short one first, and second"
    # te = 0 cannot carry a hit: one row scores at most max(mat)
    assert ("unequal", "te = 0") in cs.unreachable and cs.o["a"] < cs.o["min_seed_len"] * cs.o["a"]
    assert all(want.res[i][1] > 0 for i in rows), name
    # rows past the stop that reach the maximum again: a read that is its unit twice over, one unit in the window
    units = [i for i in rows if cs.unit[i] > 0]
    assert len(cs.reads[cs.rd[0]]) < 2 * cs.o["min_seed_len"] + 3 or units, name


@pytest.mark.parametrize("name", rv.FAMILY_SETS["quirks"])
def test_quirks_hold_gaps_both_ways_and_n(lib, name):
    cs, want = expected(lib, "quirks", name)
    pl = rv.plan(want)
    no_silent_start_miss(name, want, pl)
    res = want.res
    gap = {i: int((res[i][1] - res[i][5]) - (res[i][2] - res[i][6])) for m in pl["members"].values() for i in m}
    s = (len(cs.reads[0]) + 15) // 16
    ins = {cs.tag[i][1] % s for i, g in gap.items() if cs.tag[i][0] == "ins" and g < 0}
    dele = {cs.tag[i][1] % s for i, g in gap.items() if cs.tag[i][0] == "del" and g > 0}
    assert len(ins) >= s - 2 and len(dele) >= s - 2, (name, sorted(ins), sorted(dele))   # gaps at (nearly) every offset of a segment
    assert {cs.tag[i][1] for i in gap if cs.tag[i][0] == "N"} == {0, 1}, name
    assert any((cs.reads[cs.rd[i]] == 4).any() for i, g in gap.items() if cs.tag[i][0] == "ins"), name


@pytest.mark.parametrize("name", rv.FAMILY_SETS["ceiling"])
def test_ceiling_family_never_mixes_saturation_into_a_quad(lib, name):
    cs, want = expected(lib, "ceiling", name)
    pl = rv.plan(want)
    no_silent_start_miss(name, want, pl)
    shift = max(-int(cs.mat.min()), 0)
    tops = [i for i, t in cs.tag.items() if t[0] == "top"]
    assert tops and all(want.res[i][0] == 255 - shift - 1 - (255 - shift - 1) % cs.o["a"] and pl["cls"][i] > 0 for i in tops), name
    assert want.sat.sum() >= 8 and all(pl["cls"][i] == 0 for i in np.nonzero(want.sat)[0]), name
    assert any(x in tops or y in tops for x, y in pl["pairs"]), name


def test_sizes_single_and_mixed(lib):
    cs, want = expected(lib, "sizes", "default")
    pl = rv.plan(want)
    assert sorted(len(m) for m in pl["members"].values()) == sorted(rv.SIZES.values()), {c: len(m) for c, m in pl["members"].items()}
    assert {((c - 1) // 3, (c - 1) % 3): len(m) for c, m in pl["members"].items()} == rv.SIZES
    assert pl["counts"] == [49, 4, 0, 53] and len(pl["members"]) + 42 == rv.N_CLASSES   # classes of 0 members: the other 42
    assert any(m != list(range(m[0], m[0] + len(m))) for m in pl["members"].values()), "the classes are interleaved"
    cs, want = expected(lib, "single", "default")
    assert len(cs) == 1 and rv.plan(want)["counts"] == [0, 1, 0, 1]
    cs, want = expected(lib, "mixed", "default")
    pl = rv.plan(want)
    assert len({len(cs.reads[cs.rd[i]]) for m in pl["members"].values() for i in m}) == 3 and pl["counts"][0] >= 16, pl["counts"]
