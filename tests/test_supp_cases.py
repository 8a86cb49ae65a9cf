"""CPU: the cases of tests/supp_cases.py are what that file says they are — shown on the reference's own text and lists
(oracle/_ref/libbwaref.so: mem_align1_core, mem_sort_dedup_patch, mem_mark_primary_se and mem_reg2sam as the single-end branch of
worker2 calls them), without any kernel.

Per option set every synthetic family reaches its branch: the line counts; flag 0x800 on the lines behind the first (0x100 under -M,
with SEQ and an SA tag all the same); H for the clips of those lines and a SEQ cut to the aligned part, S and the whole read under -Y;
SA:Z on every line naming exactly the other lines with their POS, strand, CIGAR (clips as S), MAPQ and NM; the tag order NM MD AS XS RG
SA XA; cap_mapq's second line carries line 0's MAPQ, below 60, and its own higher one under -q; lead_del / trail_del have a line whose
window starts / ends g bases off its POS / end; the xa families carry their entry counts on their lines and xa_over none; five has
five lines; below_T_second one; either hit of tie is line 0 in a good share of the reads and not the same one under both ids; row_over
has a line of which the others' SA tags say more than SA_STAGE bytes.

The census of the realistic chimeras (a) under the default options, as printed by this test, with its floors (at least 30 eligible
reads in each of the 2-, 3- and 4-line classes):
  reads 282: 2 lines 79, 3 lines 112, 4 lines 89, one line 2, more than four 0; a list past 64 regions 5, a tag past 8 entries 0;
  eligible 275 — 2 lines 79, 3 lines 111, 4 lines 85 — of which 29 carry an XA tag on a line.
Lines with a squeezed deletion among the 6 + 6 reads of lead_del / trail_del: 6 / 3 (elsewhere a base outside the deletion matches by
chance and the global alignment keeps it).
"""
import collections
import re

import pytest

import supp_cases as spc
from oracle import pyoracle as po

pytestmark = pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref/libbwaref.so not present")

N_PROCESSED = (4000, (1 << 32) + 5)


@pytest.fixture(scope="module")
def ref(genome):
    return po.RefIndex(genome["prefix"])


def _opts(ref, name):
    kw, with_qual, rg = spc.OPTION_SETS[name]
    ropt = ref.opt(**kw)
    if kw:
        ref.lib.bwa_fill_scmat(ropt.contents.a, ropt.contents.b, ropt.contents.mat)
    return ropt, with_qual, rg


def _clip_s(cigar):
    return cigar.replace(b"H", b"S")


def _query_len(cigar, ops="MIS"):
    n, tot = 0, 0
    for ch in cigar.decode():
        if ch.isdigit():
            n = n * 10 + int(ch)
        else:
            tot += n if ch in ops else 0
            n = 0
    return tot


def check_record(name, cs, text, after, o, ix, with_qual, rg):
    """what mem_aln2sam promises of a record of several lines, on the reference's own text"""
    from mpibwa_amd import abi
    soft, no_multi = bool(o.flag & abi.MEM_F_SOFTCLIP), bool(o.flag & abi.MEM_F_NO_MULTI)
    lines = [spc.parse_line(x) for x in text.splitlines()]
    L = len(cs["read"])
    for j, P in enumerate(lines):
        assert (P["flag"] & ~0x10) == (0 if j == 0 else 0x100 if no_multi else 0x800), (name, cs["family"], j, P["flag"])
        assert P["seq"] != b"*" and (P["qual"] != b"*") == with_qual
        if j and not soft:
            assert b"S" not in P["cigar"] and len(P["seq"]) == _query_len(P["cigar"], "MI"), (name, cs["family"], P["cigar"])
        else:
            assert b"H" not in P["cigar"] and len(P["seq"]) == L == _query_len(P["cigar"]), (name, cs["family"], P["cigar"])
        others = [Q for i, Q in enumerate(lines) if i != j]
        assert [(e[0], e[1], e[2], e[3], e[4], e[5]) for e in P["sa"]] == \
               [(Q["rname"], Q["pos"], b"-" if Q["flag"] & 0x10 else b"+", _clip_s(Q["cigar"]), Q["mapq"], int(Q["tags"][b"NM"])) for Q in others], (name, cs["family"], j, text)
        want_order = [t for t in (b"NM", b"MD", b"AS", b"XS", b"RG", b"SA", b"XA") if t in P["tags"]]
        assert P["order"] == want_order and (b"RG" in P["tags"]) == bool(rg), (name, P["order"])
    return lines


@pytest.mark.parametrize("name", list(spc.OPTION_SETS))
def test_families_reach_their_branches(ref, genome, name):
    from mpibwa_amd import abi
    ropt, with_qual, rg = _opts(ref, name)
    o = ropt.contents
    M = spc.n_xa_max(o)
    ix = spc.Index(genome["prefix"], ref.bns)
    ref.set_rg(rg)
    try:
        order = spc.shuffled(spc.build_cases(ix, o, 3), 4)
        read_no = spc.read_numbers(len(order), 5)
        wants = [spc.reference_side(ref, ropt, order, with_qual, npr, read_no) for npr in N_PROCESSED]
    finally:
        ref.set_rg(None)
    n = collections.Counter()
    tie_first, tie_flips, over = [0, 0], 0, 0
    squeezed = collections.Counter()
    for i, cs in enumerate(order):
        fam = cs["family"]
        n[fam] += 1
        for w, want in enumerate(wants):
            text, after = want[i]
            n_lines = len(text.splitlines())
            if cs["expect"] == "lines":
                assert n_lines == cs["n_lines"] and len(spc.line_regions(o, after)) == n_lines, (name, fam, cs["tag"], text)
                lines = check_record(name, cs, text, after, o, ix, with_qual, rg)
                assert spc.eligible(cs, text) == all(len(P["xa"]) <= spc.PW_XA_CAP for P in lines)
                if "n_xa" in cs:
                    assert [len(P["xa"]) for P in lines] == cs["n_xa"], (name, fam, cs["tag"], text)
                    for z, P in zip(spc.line_regions(o, after), lines):
                        assert len(spc.listed(o, after, z)) == len(P["xa"])
                if cs.get("has_xa"):
                    assert spc.has_xa(text), (name, fam, text)
                elif fam not in ("cap_mapq",):
                    assert not spc.has_xa(text), (name, fam, text)
            elif cs["expect"] == "plain":
                assert n_lines == 1 and b"\tSA:Z:" not in text, (name, fam, text)
                assert sum(r["secondary"] < 0 for r in after) == 2 and sum(r["secondary"] < 0 and r["score"] >= o.T for r in after) == 1
            if fam == "five":
                assert n_lines == 5 and not spc.eligible(cs, text), (name, text)
            if fam == "three":
                mid = [P for P in lines if P["cigar"].count(b"H") + P["cigar"].count(b"S") == 2]   # (S when it is line 0 or under -Y)
                assert mid, (name, text)
            if fam == "cap_mapq":
                assert lines[0]["mapq"] < 60, (name, text)
                if o.flag & abi.MEM_F_KEEP_SUPP_MAPQ:
                    assert lines[1]["mapq"] > lines[0]["mapq"], (name, text)
                else:
                    assert lines[1]["mapq"] == lines[0]["mapq"], (name, text)
            if fam in ("lead_del", "trail_del"):
                g = int(cs["tag"][1:].split("/")[0])
                r = [r for r in after if r["qe"] - r["qb"] == 60][0]
                P = [P for P in lines if len(P["seq"]) in (60, 150) and _query_len(P["cigar"], "MI") == 60][0]
                ref_len = _query_len(P["cigar"], "MD")
                ops = [x for x in re.findall(rb"\d+([MIDSH])", P["cigar"]) if x not in (b"S", b"H")]
                assert ops[0] != b"D" and ops[-1] != b"D", (name, fam, P["cigar"], r)
                # (the global alignment may keep a base that matches by chance outside the deletion: then nothing is squeezed)
                if int(r["re"] - r["rb"]) == ref_len + g:
                    squeezed[fam] += w == 0
                    rev = r["rb"] >= ix.l_pac
                    first = (2 * ix.l_pac - int(r["re"]) if rev else int(r["rb"])) - ix.off[int(r["rid"])] + 1
                    # (the window is longer at its front in forward coordinates on either strand: the squeezed deletion moves POS)
                    assert P["pos"] == first + (g if fam == "lead_del" else 0), (name, fam, cs["tag"], P["pos"], first)
            if fam == "tie":
                z = spc.line_regions(o, after)[0]
                assert len(spc.listed(o, after, z)) == 1 and int(after[spc.listed(o, after, z)[0]]["score"]) == int(after[z]["score"])
                tie_first[w] += int(after[z]["rb"]) == cs["regs"][0]["rb"]
            if fam == "row_over" and w == 0:
                over += any(spc.sa_bytes(x) > spc.SA_STAGE or spc.row_bytes(x, with_qual, rg) > spc.LINES_ROW for x in text.splitlines())
        if fam == "tie":
            tie_flips += int(wants[0][i][1][0]["rb"]) != int(wants[1][i][1][0]["rb"])
    assert n["two"] == 8 and n["three"] == 4 and n["four"] == 4 and n["five"] == 3 and n["lead_del"] == 6 and n["trail_del"] == 6 and n["cap_mapq"] == 6
    assert n["xa_on_0"] == n["xa_on_1"] == n["xa_on_both"] == M and n["xa_over"] == 3 and n["below_T_second"] == 4 and n["tie"] == 24 and n["row_over"] == 4
    print(name, "families", dict(n), "tie: the list's first hit is line 0 in", tie_first, "of 24; the winner changes with n_processed in", tie_flips,
          "; row_over reads beyond the staging:", over)
    assert all(4 <= t <= 20 for t in tie_first) and tie_flips >= 4, (tie_first, tie_flips)
    assert over == n["row_over"], over
    print(name, "lines with a squeezed deletion:", dict(squeezed))
    assert squeezed["lead_del"] >= 2 and squeezed["trail_del"] >= 2, squeezed


def test_realistic_chimeras_hold_enough_reads_of_every_class(tmp_path_factory, built):
    import pair_wave_cases as pw
    g = pw.build_index(tmp_path_factory.mktemp("supp"))
    wref = po.RefIndex(g["prefix"])
    ropt = wref.opt()
    ix = spc.Index(g["prefix"], wref.bns)
    cases = spc.realistic_cases(g)
    want = spc.reference_side(wref, ropt, cases, True, 4000, spc.read_numbers(len(cases), 5))
    c = spc.census(cases, want)
    print("census", c)
    for k in (2, 3, 4):
        assert c.get("eligible%d" % k, 0) >= 30, c
    assert cases[0]["n_seg"] == 2 and len(cases[0]["read"]) == 150 and any(len(cs["read"]) == 250 and cs["n_seg"] == 3 for cs in cases)
    for cs, (text, after) in zip(cases, want):
        if spc.eligible(cs, text):
            check_record("real", cs, text, after, ropt.contents, ix, True, None)
    # the 75 + 75 read on the reverse strand
    assert spc.eligible(cases[0], want[0][0]) and all(spc.parse_line(x)["flag"] & 0x10 for x in want[0][0].splitlines()), want[0][0]
