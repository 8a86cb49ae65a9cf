"""CPU: the cases of the single-end stage test are what tests/se_stage_cases.py says they are — shown on the reference's own text
(oracle/_ref/libbwaref.so: mem_sort_dedup_patch, mem_mark_primary_se and mem_reg2sam as the single-end branch of worker2 calls them),
without any kernel.  Per option set: the families built to be plain end in ONE line without XA / SA (flag 4 where no region reaches T),
the families built to be the host's end in something else or hold more regions than the kernel looks at; `shadow` sets XS and lowers
MAPQ, `frac_rep` lowers MAPQ, `dup` is left with one region, `lengths` has every length, the `row` ladder puts the length of the short
fields on every value from 256 to 265.  The thresholds are the counts measured when the cases were written (at most that, at least
half of it)."""
import collections

import pytest

import se_stage_cases as sec
from oracle import pyoracle as po

pytestmark = pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref/libbwaref.so not present")

# reads per family (measured: exactly these)
N_READS = dict(plain=120, clip=150, lead_del=150, trail_del=150, none=60, below_T=60, shadow=120, xa=80, supp=80, maxreg=60, dup=80, tie=80,
               tie_low=80, frac_rep=80, lengths=120, row=405)


@pytest.fixture(scope="module")
def ref(genome):
    return po.RefIndex(genome["prefix"])


@pytest.fixture(scope="module")
def maxreg():
    """regions per read the kernels look at (PR_MAXREG of the library, not a number of this file)"""
    from mpibwa_amd import api
    return int(api.load_library().mi355x_pair_maxreg())


def reference_text(ref, prefix, name, seed=1):
    kw, with_qual, rg = sec.OPTION_SETS[name]
    ropt = ref.opt(**kw)
    if kw:
        ref.lib.bwa_fill_scmat(ropt.contents.a, ropt.contents.b, ropt.contents.mat)
    rgid = ref.set_rg(rg)
    try:
        ix = sec.Index(prefix, ref.bns)
        order = sec.shuffled(sec.build_cases(ix, ropt.contents, seed), seed + 1)
        out = sec.reference_side(ref, ropt, order, with_qual, n_processed=1000)
    finally:
        ref.set_rg(None)
    return ix, ropt, order, out, rgid


@pytest.mark.parametrize("name", list(sec.OPTION_SETS))
def test_families_reach_their_branches(ref, genome, maxreg, name):
    ix, ropt, order, out, rgid = reference_text(ref, genome["prefix"], name)
    n = collections.Counter()
    row_short, row_dev = collections.Counter(), collections.Counter()
    for cs, (text, after) in zip(order, out):
        fam = cs["family"]
        n[fam] += 1
        lines = text.splitlines(keepends=True)
        P = sec.parse(lines[0], rgid)
        f = P["fields"]
        assert f[0] == cs["name"] and (f[10] == b"*") == (not sec.OPTION_SETS[name][1]) and P["tags"].get(b"RG", b"") == rgid
        assert not (P["flag"] & 0xe9) and f[6:9] == [b"*", b"0", b"0"] and b"MC" not in P["tags"]   # never a mate
        n[fam, "lines%d" % len(lines)] += 1
        n[fam, "XA"] += b"\tXA:Z:" in text
        n[fam, "SA"] += b"\tSA:Z:" in text
        n[fam, "flag4"] += bool(P["flag"] & 4)
        n[fam, "XS>0"] += int(P["tags"].get(b"XS", b"0")) > 0
        n[fam, "rev" if P["flag"] & 0x10 else "fwd"] += 1
        n[fam, "mapq60"] += int(f[4]) == 60
        n[fam, "N"] += b"N" in f[9]
        n[fam, "len%d" % len(f[9])] += 1
        n[fam, "clip5"] += P["cigar"].split(b"S")[0].isdigit()
        n[fam, "clip3"] += P["cigar"].endswith(b"S")
        if cs["expect"] == "plain":
            assert sec.is_plain(text), (fam, cs["tag"], text)
            assert b"XS" in P["tags"] and b"AS" in P["tags"]
            if fam in ("none", "below_T"):
                assert P["flag"] == 4 and P["rname"] == b"*" and P["cigar"] == b"*" and f[11:13] == [b"AS:i:0", b"XS:i:0"], text
            else:
                region, flag, mapq, score, sub = sec.the_line(ropt.contents, text, after)
                assert region is not None and flag == 0 and score == region["score"] and sub == region["sub"]
                assert bool(P["flag"] & 0x10) == (region["rb"] >= ix.l_pac) and P["rname"] == ix.names[region["rid"]]
        elif cs["expect"] == "host":
            assert not sec.is_plain(text) or len(cs["regs"]) > maxreg, (fam, cs["tag"], text)
        if fam == "maxreg":
            assert len(cs["regs"]) > maxreg, (cs["tag"], maxreg)
        if fam == "dup":
            assert len(after) == 1 and len(cs["regs"]) == 2
        if fam == "row":
            row_short[P["short"]] += 1
            if sum(P["cigar"].count(c) for c in b"MID") <= 96:   # (the CIGARs aln_kernel computes itself)
                row_dev[P["short"]] += 1
        elif cs["expect"] == "plain":
            assert P["short"] <= 130, (fam, cs["tag"], P["short"], text)
    for fam, want in N_READS.items():
        assert n[fam] == want, (fam, n[fam])
    print(name, "short fields of the row ladder:", min(row_short), "..", max(row_short), "bytes,", sum(c for v, c in row_short.items() if v > sec.SAM_ROW), "beyond the row;",
          "with at most 96 operations at 260 / 261:", row_dev[sec.SAM_ROW], row_dev[sec.SAM_ROW + 1], "beyond:", sum(c for v, c in row_dev.items() if v > sec.SAM_ROW))
    # one line everywhere in the plain families, on either strand (measured: plain 60 / 60, clip 75 / 75)
    for fam in sec.PLAIN_FAMILIES:
        assert n[fam, "lines1"] == n[fam] and n[fam, "XA"] == 0 and n[fam, "SA"] == 0, (fam, n)
    assert n["plain", "fwd"] >= 60 and n["plain", "rev"] >= 60
    assert n["clip", "clip5"] >= 75 and n["clip", "clip3"] >= 75 and n["clip", "fwd"] >= 60 and n["clip", "rev"] >= 60
    # flag 4: no region, or none that reaches T
    assert n["none", "flag4"] == 60 and n["below_T", "flag4"] == 60
    assert sum(n[fam, "flag4"] for fam in sec.FAMILIES if fam not in ("none", "below_T")) == 0
    # shadow and tie_low: XS present with the secondary hit's score, a lower MAPQ; XS:i:0 in the plain family
    assert n["shadow", "XS>0"] == 120 and n["tie_low", "XS>0"] == 80 and n["plain", "XS>0"] == 0
    assert n["shadow", "mapq60"] <= 80 and n["plain", "mapq60"] == 120   # (measured: 80 of 120, the 40 short reads are below 60)
    assert n["frac_rep", "mapq60"] == 0
    # the host's families: XA (one line with the tag), a supplementary line with SA, the hash tie with XA
    assert n["xa", "XA"] == 80 and n["xa", "lines1"] == 80
    assert n["supp", "lines2"] == 80 and n["supp", "SA"] == 80
    assert n["tie", "XA"] == 80
    # lengths: every length, 20 reads each, N in some
    for L in sec.LENGTHS:
        assert n["lengths", "len%d" % L] == 20, (L, n)
    assert n["lengths", "N"] >= 10
    # row: every length of the short fields from 256 to 265, a good number on either side of the row
    for v in range(256, 266):
        assert row_short[v] >= 1, (v, sorted(row_short.items()))
    # ... and on either side of the boundary a CIGAR of at most 96 operations, the most aln_kernel returns
    assert row_dev[sec.SAM_ROW] >= 1 and row_dev[sec.SAM_ROW + 1] >= 1, sorted(row_dev.items())
    assert sum(c for v, c in row_short.items() if v > sec.SAM_ROW) >= 50 and sum(c for v, c in row_short.items() if v <= sec.SAM_ROW) >= 50
