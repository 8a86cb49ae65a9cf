"""Host logic (no GPU): the families of tests/msw_regs_cases.py contain what they claim — by their construction, by the library's host
ksw_align2 and, where it is built, by the compiled reference's, which the host's must equal on every request."""
import numpy as np
import pytest

import msw_cases as mc
import msw_regs_cases as rc
from oracle import pyoracle as po


@pytest.fixture(scope="module")
def lib(built):
    from mpibwa_amd import api
    return api.load_library()


def expected(lib, cs):
    """-> (Want by the host's ksw_align2, its coverage); the reference's results are the same where it is built"""
    res = mc.host_results(lib, cs)
    if po.ref_available():
        ref = mc.reference_results(po.ref_lib(), cs)
        bad = np.nonzero((res != ref).any(axis=1))[0]
        assert len(bad) == 0, (cs.name, [(int(i), cs.kind[i], list(res[i]), list(ref[i])) for i in bad[:5]])
    want = mc.want_from_host(lib, cs, res)
    return want, mc.coverage(want)


def qlen(cs, i):
    return len(cs.reads[cs.rd[i]])


def runs(cs):
    out = [1]
    for i in range(1, len(cs)):
        if cs.rd[i] == cs.rd[i - 1]:
            out[-1] += 1
        else:
            out.append(1)
    return out


def check_bounds(cs):
    assert 100 <= len(cs) <= 600, len(cs)
    for i in range(len(cs)):
        assert 0 <= cs.rb[i] <= cs.re[i] <= 2 * mc.L_PAC and (cs.re[i] <= mc.L_PAC or cs.rb[i] >= mc.L_PAC)
        assert cs.re[i] - cs.rb[i] <= qlen(cs, i) + mc.MAX_EXTRA
    items, word = mc.work_list(cs)
    assert sorted([k for it in items for k in it if k >= 0] + word) == list(range(len(cs)))


@pytest.mark.parametrize("name", rc.OPTION_SETS)
def test_boundary_lengths(lib, name):
    cs = rc.cases("boundary", name)
    check_bounds(cs)
    want, st = expected(lib, cs)
    a = cs.o["a"]
    Lb = (250 + a - 1) // a - 1
    lens = {qlen(cs, i) for i in range(len(cs))}
    reach = [s for s in rc.REGS_SLEN if 16 * s - 15 <= Lb]
    assert reach[:3] == [5, 7, 8] and (a > 1 or reach == list(rc.REGS_SLEN))
    for s in reach:
        # the shortest length of the segment length (15 padding positions), the longest the byte flavour has (none, or 256 - 249), one between
        assert {16 * s - 15, min(16 * s, Lb)} <= lens and any(16 * s - 15 < L < min(16 * s, Lb) for L in lens) or 16 * s - 7 >= Lb, (name, s, sorted(lens))
        for L in (16 * s - 15, min(16 * s, Lb)):
            mine = [i for i in range(len(cs)) if qlen(cs, i) == L and not want.sat[i]]
            # an exact hit that ends on the read's last base, right before the padding (or the end of the last segment)
            assert any(want.res[i][0] == L * a and want.res[i][2] == L - 1 for i in mine) or all(want.sat[i] for i in range(len(cs)) if qlen(cs, i) == L and cs.kind[i] == "clean"), (name, L)
            assert sum(1 for i in mine if want.res[i][0] >= cs.o["min_seed_len"] * a) >= 4, (name, L)
    assert any(rc.launch_of(L, a) == 0 for L in lens), (name, sorted(lens))
    assert all(rc.launch_of(L, a) != "word" for L in lens)
    assert st["hit"] >= 0.4 * st["n"] and st["miss"] >= 10 and st["second"] >= 5, (name, st)


@pytest.mark.parametrize("name", rc.OPTION_SETS)
def test_quad_shapes(lib, name):
    cs = rc.cases("quads", name)
    check_bounds(cs)
    want, st = expected(lib, cs)
    assert {1, 2, 3, 50} <= set(runs(cs)), sorted(set(runs(cs)))
    items, word = mc.work_list(cs)
    assert not word
    full = sum(1 for _, b in items if b >= 0)
    alone = sum(1 for _, b in items if b < 0)
    assert full >= 80 and alone >= 8, (full, alone)       # (three runs of 50 are 75 full quads)
    tl = lambda k: cs.re[k] - cs.rb[k]
    shapes = {(tl(x) == 1, tl(x) < qlen(cs, x), tl(x) == qlen(cs, x) + mc.MAX_EXTRA, tl(y) == 1, tl(y) < qlen(cs, y), tl(y) == qlen(cs, y) + mc.MAX_EXTRA)
              for x, y in items if y >= 0}
    one, short, longest = (lambda t: t[0] or t[3]), (lambda t: t[1] or t[4]), (lambda t: t[2] or t[5])
    assert any(t[0] and t[5] for t in shapes) and any(t[2] and t[3] for t in shapes) and any(t[0] and t[3] for t in shapes), shapes
    assert any(t[1] and not t[0] and t[5] for t in shapes) and any(t[2] and t[4] and not t[3] for t in shapes), shapes
    assert any(one(t) for t in shapes) and any(short(t) for t in shapes) and any(longest(t) for t in shapes)
    # an empty window rides alone and so does the real one next to it
    empties = [k for k in range(len(cs)) if tl(k) == 0]
    assert len(empties) >= 3 and all((k, -1) in items for k in empties)
    assert any((k + 1, -1) in items and cs.rd[k] == cs.rd[k + 1] and tl(k + 1) > 0 for k in empties if k + 1 < len(cs))
    assert all(want.res[k][0] == 0 for k in empties)
    # two segment lengths, both instantiated: two launches, the items of a launch are a multiple of 16 plus an odd tail somewhere
    plan, order = rc.launch_plan(cs)
    assert set(plan) == set(order) and len(order) == 2 and any(len(plan[s]) % 16 for s in order), {s: len(v) for s, v in plan.items()}
    assert st["hit"] >= 0.3 * st["n"], st


@pytest.mark.parametrize("name", rc.OPTION_SETS)
def test_mixed_lengths_and_their_launches(lib, name):
    cs = rc.cases("mixed", name)
    check_bounds(cs)
    want, st = expected(lib, cs)
    a = cs.o["a"]
    # three lengths, run after run: no two runs next to each other have one length
    first = [i for i in range(len(cs)) if i == 0 or cs.rd[i] != cs.rd[i - 1]]
    lens = [qlen(cs, i) for i in first]
    assert len(set(lens)) == 3 and all(x != y for x, y in zip(lens, lens[1:]))
    where = {L: rc.launch_of(L, a) for L in set(lens)}
    assert sorted(where.values(), key=str) == sorted([0, 7, max(s for s in rc.REGS_SLEN if 16 * s - 15 <= (250 + a - 1) // a - 1)], key=str), where
    # from the lengths alone: every request is in the launch of its read's length, whole work items, each launch with pairs and lone items
    plan, order = rc.launch_plan(cs)
    assert set(plan) == set(where.values()) and len(order) == 2
    seen = []
    for s, items in plan.items():
        assert all(where[qlen(cs, k)] == s for it in items for k in it if k >= 0)
        assert any(b >= 0 for _, b in items) and any(b < 0 for _, b in items), s
        assert len(items) > 16, (s, len(items))          # more than one wave per launch
        seen += [k for it in items for k in it if k >= 0]
    assert sorted(seen) == list(range(len(cs)))
    # every launch appends to the same tail lists: each of the three has alignments that need the second pass
    minsc = cs.o["min_seed_len"] * a
    for s, items in plan.items():
        assert sum(1 for it in items for k in it if k >= 0 and not want.sat[k] and want.res[k][0] >= minsc) >= 10, s
    assert st["hit"] >= 0.4 * st["n"], st


@pytest.mark.parametrize("name", rc.OPTION_SETS)
def test_scores(lib, name):
    cs = rc.cases("scores", name)
    check_bounds(cs)
    want, st = expected(lib, cs)
    o = cs.o
    a, minsc = o["a"], o["min_seed_len"] * o["a"]
    shift = max(-int(cs.mat.min()), 0)
    res = want.res
    clean = [i for i in range(len(cs)) if cs.kind[i] == "clean" and not want.sat[i]]
    assert len(clean) >= 20 and all(res[i][0] == qlen(cs, i) * a for i in clean)
    miss = [i for i in range(len(cs)) if cs.kind[i] == "miss"]
    assert len(miss) >= 20 and sum(1 for i in miss if res[i][0] < minsc) >= 0.8 * len(miss)
    # the 8-bit ceiling: in reach exactly where the longest byte-flavour read's exact score is 255 - shift or more
    Lb = (250 + a - 1) // a - 1
    assert (st["sat"] > 0) == (Lb * a >= 255 - shift), (name, st["sat"], Lb, shift)
    if name == "b9":
        assert st["sat"] >= 4
    # long gaps are bridged: the score is beyond what either side of the gap gives alone
    for i in range(len(cs)):
        k, _, g = cs.kind[i].partition(":")
        if k in ("ins", "del") and int(g) >= 12 and not want.sat[i]:
            assert res[i][0] >= minsc, (name, i, cs.kind[i], list(res[i]))
    assert sum(1 for i in range(len(cs)) if cs.kind[i].split(":")[0] in ("ins", "del")) >= 16
    assert st["tie"] >= 3 and "lowcx" in cs.kind, st
    # insertion runs across the end of a segment: laid where they claim, and the alignment goes through them (it beats the longer flank)
    assert len(cs.border) >= 40
    through = 0
    for i, (c, g, s) in cs.border.items():
        L = qlen(cs, i)
        assert s == rc.slen_of(L) and c <= (c + g - 1) // s * s - 1 < c + g - 1 and (c // s) != ((c + g - 1) // s), (i, c, g, s)
        if not want.sat[i] and res[i][0] > max(c, L - c - g) * a:
            through += 1
            assert res[i][0] <= (L - g) * a - (o["o_ins"] + g * o["e_ins"])
    assert through >= 0.75 * len(cs.border), (name, through, len(cs.border))
    assert {rc.slen_of(qlen(cs, i)) for i in cs.border} >= {7, rc.slen_of(Lb)}
