"""CPU: the cases of tests/pair_lines_cases.py are worth running — seen through the reference alone (mem_align1_core, mem_pestat,
mem_sort_dedup_patch and mem_sam_pe of oracle/_ref/libbwaref.so) sets (a) and (b) hold hundreds of pairs that mem_sam_pe reports end by
end within the caps of the device path, of every kind the path has a branch for, and every hand-built family of (c) reaches the branch
it is built for.  The floors are the issue's; the counts are printed.  No GPU involved.

Counts of the reference alone (printed below).  (a): 360 pairs, 270 leave the paired branch, all 270 eligible — both ends unmapped 45,
one end unmapped 90, one line each without 0x2 45, a two-line end 135 (both ends two-line 45), a chimeric end beside an unmapped mate 45,
an XA tag 24.  (b): supp_cases.CHIMERA_PLAN lists 70 + 80 + 120 = 270 reads in its three 150-base classes, but one four-segment read
(ch4_149_109) lost a base to the indels of its segments and is 149 bases long, so "the reads of 150 bases" are 269 — the recipe selects by
length and the count is asserted as 269.  All 269 pairs leave the paired branch; 260 are eligible and 9 are not: each of the 9 holds more
than 64 regions on an end (none has more than four lines on an end) — longest end of 2 / 3 / 4 lines 79 / 97 / 82, four lines on both ends 9, an XA tag 43, an unmapped end 65, a rescue attempt in all
260."""
import numpy as np
import pytest

from mpibwa_amd import abi
from oracle import pyoracle as po

import pair_lines_cases as plc
import pair_wave_cases as pw
import supp_cases as spc

pytestmark = pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref/libbwaref.so not built")


@pytest.fixture(scope="module")
def side(tmp_path_factory, built):
    g = pw.build_index(tmp_path_factory.mktemp("pair_lines"))
    g["ref"] = po.RefIndex(g["prefix"])
    return g


def _pairs(side, reads, name="default", n_processed=0):
    from mpibwa_amd import simulate
    ropt = side["ref"].opt(**plc.option_fields(name))
    reads = simulate.reads_to_ascii(reads)
    codes, lists, pes = plc.phase1(side["ref"], ropt, reads)
    return plc.reference_pairs(side["ref"], ropt, [r[0] for r in reads], codes, lists, pes, n_processed), pes


def test_set_a_holds_every_kind(side):
    pairs, _ = _pairs(side, plc.set_a(side))
    c = plc.census(pairs)
    print("(a)", c)
    assert c["pairs"] == 360
    assert c["eligible"] >= 250 and c["both_unmapped"] >= 40 and c["one_unmapped"] >= 80 and c["multi"] >= 120, c


def test_set_a_is_what_pair_wave_cases_reference_side_sees(side):
    """the same pairs through pair_wave_cases.reference_side (id = the pair's number): the two reference sides agree"""
    from mpibwa_amd import simulate
    reads = simulate.reads_to_ascii(plc.set_a(side)[:80])
    theirs, _ = pw.reference_side(side["ref"], side["ref"].opt(flag=abi.MEM_F_PE), reads)
    mine, _ = _pairs(side, plc.set_a(side)[:80])
    assert [P.text for P in theirs] == [P.text for P in mine]
    assert all((a == b).all() for P, Q in zip(theirs, mine) for a, b in zip(P.after, Q.after))


def test_set_b_holds_long_ends(side):
    reads, n_ch = plc.set_b(side)
    assert n_ch == 269 and len(reads) == plc.B_N_PLAIN + 269   # (the 270 of supp_cases.CHIMERA_PLAN's 150-base classes but one of 149 bases)
    pairs, _ = _pairs(side, reads)
    c = plc.census(pairs[plc.B_N_PLAIN:])
    print("(b)", c)
    assert c["pairs"] == 269
    assert c["over_lines"] == 0 and c["over_regions"] == 9 and c["over_other"] == 0, c   # (why the nine are not eligible: more than 64 regions on an end)
    assert c["eligible"] >= 240, c
    assert min(c["longest2"], c["longest3"], c["longest4"]) >= 60, c
    assert c["four_both"] >= 5 and c["with_xa"] >= 30 and c["an_end_unmapped"] >= 40, c


def _rlen(cigar):
    import re
    return sum(int(n) for n, op in re.findall(rb"(\d+)([MIDSH])", cigar) if op in b"MD")


@pytest.mark.parametrize("name", ["default", "M", "q"])
def test_every_family_of_c_reaches_its_branch(side, name):
    ref = side["ref"]
    _, pes = _pairs(side, plc.set_a(side))
    ropt = ref.opt(**plc.option_fields(name))
    o = ropt.contents
    ix = spc.Index(side["prefix"], ref.bns)
    cases = plc.build_cases(ix, o, pes)
    codes, lists = plc.lists_of_cases(ref, ropt, cases)
    pairs = plc.reference_pairs(ref, ropt, [cs["name"] for cs in cases], codes, lists, pes, 4000)
    seen = {}
    for cs, P in zip(cases, pairs):
        fam = cs["family"]
        seen[fam] = seen.get(fam, 0) + 1
        nl, fl, um = plc.n_lines(P), plc.flags(P), plc.unmapped(P)
        F = [[l.split(b"\t") for l in x] for x in P.lines]
        long_end = 0 if nl[0] >= nl[1] else 1
        assert plc.eligible(P) == (cs["expect"] == plc.PW_DECIDED_LINES), (fam, cs["tag"], P.text)
        if fam == "five":
            assert max(nl) == 5, (fam, P.text)
            continue
        if fam in ("two_lines", "cap_mapq", "top_lead_del", "proper", "improper"):
            assert sorted(nl) == [1, 2], (fam, nl, P.text)
        if fam in ("supp_lead_del", "chimeric_alone"):
            assert sorted(nl) == [0, 2], (fam, nl, P.text)
        if fam == "two_lines":
            supp = fl[long_end][1]
            assert bool(supp & 0x100) == (name == "M") and bool(supp & 0x800) == (name != "M"), (fam, name, supp)
        if fam == "cap_mapq":
            q0, q1 = int(F[long_end][0][4]), int(F[long_end][1][4])
            assert q0 < 60 and (q1 > q0 if name == "q" else q1 == q0), (fam, name, q0, q1)
        if fam == "supp_lead_del":
            g = int(cs["tag"][1])
            r = P.after[long_end][spc.line_regions(o, P.after[long_end])[1]]
            assert _rlen(F[long_end][1][5]) == int(r["re"] - r["rb"]) - g, (fam, cs["tag"], F[long_end][1][5], r)
            assert all(f[6] == b"=" and f[7] == f[3] and f[8] == b"0" and int(f[1]) & 0x8 for f in F[long_end]), (fam, P.text)   # every line lends its own POS
            assert F[1 - long_end][0][3] == F[long_end][0][3] and int(F[1 - long_end][0][1]) & 0x4, (fam, P.text)
        if fam == "top_lead_del":
            g = int(cs["tag"][1])
            r = P.after[long_end][0]
            assert _rlen(F[long_end][0][5]) == int(r["re"] - r["rb"]) - g, (fam, cs["tag"], F[long_end][0][5], r)
            mate = F[1 - long_end][0]
            assert mate[7] == F[long_end][0][3] and b"MC:Z:" + F[long_end][0][5] in mate, (fam, P.text)
        if fam == "unmapped_rev":
            e = um.index(True)
            assert nl[1 - e] == 1 and fl[e][0] & 0x34 == 0x34 and fl[1 - e][0] & 0x18 == 0x18, (fam, fl)
            want = bytes(np.frombuffer(b"TGCAN", dtype=np.uint8)[P.reads[e][::-1]])
            assert F[e][0][9] == want and F[e][0][5] == b"*" and F[e][0][3] == F[1 - e][0][3], (fam, P.text)
        if fam == "chimeric_alone":
            assert um[1 - long_end] and all(f & 0x8 for f in fl[long_end]), (fam, fl)
        if fam == "proper":
            assert all(f & 0x2 for x in fl for f in x), (fam, fl)
        if fam == "improper":
            assert not any(f & 0x2 for x in fl for f in x), (fam, fl)
    print(name, "families", seen)
    assert set(seen) == {"five", "two_lines", "cap_mapq", "supp_lead_del", "top_lead_del", "unmapped_rev", "chimeric_alone", "proper", "improper"}
