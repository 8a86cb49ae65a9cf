"""CPU: the cases of tests/se_wave_cases.py are what that file says they are — shown on the reference's own text and lists
(oracle/_ref/libbwaref.so: mem_align1_core, mem_sort_dedup_patch, mem_mark_primary_se and mem_reg2sam as the single-end branch of
worker2 calls them), without any kernel.

Per option set every synthetic family reaches its branch: the n-families keep exactly their number of regions and end in one plain
line (the unmapped one for n0), n65 holds 65 regions, all_below_T ends in the unmapped record with 9 .. 30 regions, xa_k carries a tag
of k entries naming the close hits in list order, xa_over and xa_under_other carry none, xa_edge lists the hit of 121 and not the one of
120, tie ends in a tag of one entry with either hit as the line (and the winner changes with n_processed), supp has a supplementary
line, long a region beyond the per-length table of a 150-base launch, alt a region on an ALT contig.

The census of the realistic reads (a) under the default options, with its floors (at least 50 eligible reads in each of "plain, more
than eight regions" and "XA", at least one tag of every entry count 1 .. max_XA_hits = 5), as printed by this test:
  reads 4750, eligible 4750 (no list past 64 regions, no second line, no tag past 8 entries), plain with more than eight regions 805,
  XA 330 (tags of 1 / 2 / 3 / 4 / 5 entries: 179 / 48 / 38 / 33 / 32), the rest 3615; unmapped records among them 293.
The recipe of tests/pair_wave_cases.py yields enough: no read is added."""
import collections

import pytest

import se_wave_cases as swc
from oracle import pyoracle as po

pytestmark = pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref/libbwaref.so not present")

N_PROCESSED = (4000, (1 << 32) + 5)


@pytest.fixture(scope="module")
def ref(genome):
    return po.RefIndex(genome["prefix"])


def _opts(ref, name):
    kw, with_qual, rg = swc.OPTION_SETS[name]
    ropt = ref.opt(**kw)
    if kw:
        ref.lib.bwa_fill_scmat(ropt.contents.a, ropt.contents.b, ropt.contents.mat)
    return ropt, with_qual, rg


def _line_hit(ix, text, after, T):
    """the place in `after` of the hit the record's line reports"""
    f = text.split(b"\t")
    rev = bool(int(f[1]) & 0x10)
    pri = [j for j, r in enumerate(after) if r["secondary"] < 0 and r["score"] >= T and (r["rb"] >= ix.l_pac) == rev and ix.names[r["rid"]] == f[2]]
    assert len(pri) == 1, (text, after)
    return pri[0]


def _listed(ropt, after, z):
    """mem_gen_alt's hits under z, in list order (src/bwamem_extra.c:91-118): the ratio is a float, the product a double"""
    import numpy as np
    ratio = float(np.float32(ropt.XA_drop_ratio))
    return [j for j, r in enumerate(after) if r["secondary_all"] == z and int(r["score"]) >= int(after[z]["score"]) * ratio]


@pytest.mark.parametrize("name", list(swc.OPTION_SETS))
def test_families_reach_their_branches(ref, genome, name):
    ropt, with_qual, rg = _opts(ref, name)
    o = ropt.contents
    M = swc.n_xa_max(o)
    ix = swc.Index(genome["prefix"], ref.bns)
    rgid = ref.set_rg(rg)
    try:
        order = swc.shuffled(swc.build_cases(ix, o, 3), 4)
        read_no = swc.read_numbers(len(order), 5)
        wants = [swc.reference_side(ref, ropt, order, with_qual, npr, read_no) for npr in N_PROCESSED]
    finally:
        ref.set_rg(None)
    n = collections.Counter()
    tie_first = [0, 0]
    tie_flips = 0
    for i, cs in enumerate(order):
        fam, before = cs["family"], cs["before"]
        n[fam] += 1
        for w, want in enumerate(wants):
            text, after = want[i]
            lines = text.splitlines()
            entries = swc.xa_entries(text)
            flag = int(lines[0].split(b"\t")[1])
            if "n_after" in cs:
                assert len(before) == cs["n_after"], (fam, len(before))
            if cs["expect"] == "plain":
                assert len(lines) == 1 and not entries and b"\tSA:Z:" not in text and swc.eligible(cs, text), (fam, cs["tag"], text)
                assert bool(flag & 4) == (fam in ("n0", "all_below_T")), (fam, text)
            if fam == "n65":
                assert len(before) == 65 and not swc.eligible(cs, text)
            if fam == "all_below_T":
                assert 9 <= len(before) <= 30 and all(r["score"] < o.T for r in before)
            if cs["expect"] == "xa":
                assert len(lines) == 1 and len(entries) == cs["n_xa"] and b"\tSA:Z:" not in text, (fam, cs["tag"], text)
                z = _line_hit(ix, text, after, o.T)
                listed = _listed(o, after, z)
                assert len(listed) == len(entries), (fam, listed, entries)
                for j, e in zip(listed, entries):   # in list order
                    assert e[0] == ix.names[after[j]["rid"]] and (e[1] == b"-") == bool(after[j]["rb"] >= ix.l_pac), (fam, j, e)
                assert swc.eligible(cs, text) == (len(entries) <= swc.PW_XA_CAP)
                if fam == "xa_edge":
                    assert [int(after[j]["score"]) for j in listed] == [121] and sorted(int(r["score"]) for r in after)[-3:] == [120, 121, 150]
                if fam == "tie":
                    assert int(after[listed[0]]["score"]) == int(after[z]["score"])
                    first = cs["regs"][0]
                    tie_first[w] += int(after[z]["rb"]) == first["rb"]
            if fam == "xa_over":
                assert len(_listed(o, after, _line_hit(ix, text, after, o.T))) == M + 1
            if fam == "xa_under_other":
                z = _line_hit(ix, text, after, o.T)
                if cs["tag"] == "below_T":   # hits close to their parent, which is a primary hit below T
                    close = [j for j, r in enumerate(after) if r["secondary_all"] >= 0 and r["secondary_all"] != z and
                             after[r["secondary_all"]]["score"] < o.T and r["score"] >= after[r["secondary_all"]]["score"] * 0.8]
                else:                        # hits close to another secondary hit, not to their parent
                    close = [j for j, r in enumerate(after) if r["secondary_all"] == z and
                             any(q["secondary_all"] == z and r["score"] < q["score"] and r["score"] >= q["score"] * 0.8 for q in after)]
                assert close and not _listed(o, after, z), (cs["tag"], after)
            if fam == "supp":
                assert len(lines) == 2 and b"\tSA:Z:" in text and not swc.eligible(cs, text)
            if fam == "long":
                assert max(max(int(r["qe"] - r["qb"]), int(r["re"] - r["rb"])) for r in before) >= 4 * 150 + 256
        if fam == "tie":
            tie_flips += int(wants[0][i][1][0]["rb"]) != int(wants[1][i][1][0]["rb"])
    for k in (0, 1, 2, 8, 9, 63, 64, 65):
        assert n["n%d" % k] >= 4, (k, n)
    for k in range(1, M + 1):
        assert n["xa_%d" % k] == 4
    assert n["xa_over"] == 4 and n["xa_edge"] == 6 and n["xa_under_other"] == 12 and n["tie"] == 40 and n["supp"] == 12 and n["long"] == 6 and n["all_below_T"] == 10
    print(name, "families", dict(n), "tie: the list's first hit is the line in", tie_first, "of 40; the winner changes with n_processed in", tie_flips)
    # the hash decides, and it depends on the id: either hit wins in a good share of the reads, and not the same one under both ids
    assert all(8 <= t <= 32 for t in tie_first) and tie_flips >= 8, (tie_first, tie_flips)


def test_alt_family(ref, genome_alt):
    aref = po.RefIndex(genome_alt["prefix"])
    ropt = aref.opt()
    ix = swc.Index(genome_alt["prefix"], aref.bns)
    is_alt = [int(aref.bns.contents.anns[c].is_alt) for c in range(ix.n_seqs)]
    assert sum(is_alt) == len(genome_alt["alt"])
    cases = swc.build_alt_cases(ix, is_alt, ropt.contents, 6)
    swc.reference_side(aref, ropt, cases, True, 4000, swc.read_numbers(len(cases), 5))
    for cs in cases:
        assert any(is_alt[int(r["rid"])] for r in cs["before"]) and len(cs["before"]) <= swc.PW_MAXREG


def test_realistic_reads_hold_what_se_wave_kernel_is_for(tmp_path_factory, built):
    import pair_wave_cases as pw
    g = pw.build_index(tmp_path_factory.mktemp("se_wave"))
    wref = po.RefIndex(g["prefix"])
    ropt = wref.opt()
    cases = swc.realistic_cases(g)
    want = swc.reference_side(wref, ropt, cases, True, 4000, swc.read_numbers(len(cases), 5))
    c = swc.census(cases, want)
    print("census", c)
    assert c["plain_gt8"] >= 50 and c["xa"] >= 50, c
    for k in range(1, swc.n_xa_max(ropt.contents) + 1):
        assert c["xa_%d" % k] >= 1, (k, c)
