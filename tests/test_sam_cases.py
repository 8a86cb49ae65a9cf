"""CPU: the cases of the SAM stage test are what tests/sam_stage_cases.py says they are — shown on the reference's own text
(oracle/_ref/libbwaref.so: mem_reg2aln + mem_aln2sam as mem_sam_pe's paired branch calls them), without any kernel.  Per option set:
every record parses as 11 fields + tags, every family is there in its numbers, the deletion families show the squeeze in POS / CIGAR,
the `row` ladder puts the length of the short fields on every value from 256 to 265, and outside `row` the short fields stay far
below the 260 bytes of a lane's staging row.  The thresholds are the counts measured when the cases were written (at most that, at
least half of it); where the issue of this test names a number (20), that number is a floor under them."""
import collections

import pytest

import sam_stage_cases as sc
from oracle import pyoracle as po

pytestmark = pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref/libbwaref.so not present")

# records per family in the shuffled launch (measured: plain 400, contigs 372, clip 300, lead_del 300, trail_del 300, lengths 264, row 1378,
# declined 24, unmapped 120; not_mine 326 reads without a record)
MIN_RECORDS = dict(plain=400, contigs=372, clip=300, lead_del=300, trail_del=300, lengths=264, row=1300, declined=24, unmapped=120)


@pytest.fixture(scope="module")
def ref(genome):
    return po.RefIndex(genome["prefix"])


def reference_text(ref, prefix, name, seed=1):
    kw, with_qual, rg = sc.OPTION_SETS[name]
    ropt = ref.opt(**kw)
    if kw:
        ref.lib.bwa_fill_scmat(ropt.contents.a, ropt.contents.b, ropt.contents.mat)
    rgid = ref.set_rg(rg)
    try:
        ix = sc.Index(prefix, ref.bns)
        cases = sc.build_cases(ix, ropt.contents, seed)
        order = sc.shuffled_launch(cases, seed + 1)
        text = sc.reference_side(ref, ropt, order, with_qual)
    finally:
        ref.set_rg(None)
    return ix, cases, order, text, rgid


@pytest.mark.parametrize("name", list(sc.OPTION_SETS))
def test_families_reach_their_branches(ref, genome, name):
    ix, cases, order, text, rgid = reference_text(ref, genome["prefix"], name)
    assert len(rgid) == {"rg7": 7, "rg255": 255}.get(name, 0)
    n = collections.Counter()
    row_short = collections.Counter()
    for k, cs in enumerate(order):
        fam = cs["family"]
        for e in range(2):
            rec = text[2 * k + e]
            if fam == "not_mine":
                assert rec is None
                n["not_mine"] += 1
                continue
            P = sc.parse(rec, rgid)
            f = P["fields"]
            n[fam] += 1
            assert f[0] == cs["name"] and len(f[9]) == len(cs["reads"][e]) and P["flag"] & (0x40 << e)
            assert (f[10] == b"*") == (not sc.OPTION_SETS[name][1]) and (P["tags"].get(b"RG", b"") == rgid)
            if fam == "unmapped":
                assert P["flag"] == (77, 141)[e] and P["rname"] == b"*" and P["cigar"] == b"*" and f[11:13] == [b"AS:i:0", b"XS:i:0"]
                continue
            r = cs["regs"][e]
            rev = r["rb"] >= ix.l_pac
            assert bool(P["flag"] & 0x10) == rev and P["rname"] == ix.names[r["rid"]]
            assert (b"XS" in P["tags"]) == (r["sub"] >= 0) and int(P["tags"][b"AS"]) == r["score"]
            n[fam, "rev" if rev else "fwd"] += 1
            n[fam, "tlen>0" if P["tlen"] > 0 else "tlen<0" if P["tlen"] < 0 else "tlen=0"] += 1
            n[fam, "rnext_name"] += P["rnext"] not in (b"=", b"*")
            n[fam, "clip5"] += P["cigar"].split(b"S")[0].isdigit()
            n[fam, "clip3"] += P["cigar"].endswith(b"S")
            n[fam, "N"] += b"N" in f[9]
            n[fam, "name%d" % len(f[0])] += 1
            if sc.cigar_ref_len(P["cigar"]) < r["re"] - r["rb"]:   # a deletion at the front or the back was squeezed out
                fwd_start = (r["rb"] if not rev else 2 * ix.l_pac - r["re"]) - ix.off[r["rid"]]
                n[fam, "lead" if P["pos"] - 1 != fwd_start else "trail", "rev" if rev else "fwd"] += 1
            if fam == "row":
                row_short[P["short"]] += 1
            else:
                assert P["short"] <= 130, (fam, cs["tag"], P["short"], rec)   # (measured: at most 94)
    for fam, want in MIN_RECORDS.items():
        assert n[fam] >= want, (fam, n[fam])
    assert n["not_mine"] >= 2 * (3 * 32 + 50)
    # plain: TLEN of either sign and 0 (measured 159 / 159 / 82), every strand combination
    assert n["plain", "tlen>0"] >= 100 and n["plain", "tlen<0"] >= 100 and n["plain", "tlen=0"] >= 60, n
    assert n["plain", "rev"] >= 100 and n["plain", "fwd"] >= 100
    # contigs: RNEXT is a name, TLEN 0, in every record of the family
    assert n["contigs", "rnext_name"] == n["contigs"] == n["contigs", "tlen=0"]
    assert sum(n[f, "rnext_name"] for f in sc.FAMILIES if f != "contigs") == 0
    # clip: on either end (measured 200 / 200 of 300 records)
    assert n["clip", "clip5"] >= 150 and n["clip", "clip3"] >= 150 and n["clip", "rev"] >= 100 and n["clip", "fwd"] >= 100
    # the squeeze, on each strand (measured: leading 75 / 75, trailing 59 / 50; one base of a trailing window sometimes matches)
    for strand in ("fwd", "rev"):
        assert n["lead_del", "lead", strand] >= 60 and n["trail_del", "trail", strand] >= 40, n
    # lengths: N in reads (measured 100), the names
    assert n["lengths", "N"] >= 50 and n["lengths", "rev"] >= 60 and n["lengths", "fwd"] >= 60
    for ln in (1, 63, 64, 65, 200, 254):
        assert n["lengths", "name%d" % ln] >= 30, (ln, n["lengths", "name%d" % ln])
    # row: every length of the short fields from 256 to 265
    for v in range(256, 266):
        assert row_short[v] >= 1, (v, sorted(row_short.items()))
    assert sum(c for v, c in row_short.items() if v > sc.SAM_ROW) >= 40 and sum(c for v, c in row_short.items() if v <= sc.SAM_ROW) >= 600


def test_contig_names_of_the_second_index(tmp_path_factory, built):
    prefix = sc.build_named_index(tmp_path_factory.mktemp("named"))
    ref2 = po.RefIndex(prefix)
    ix, cases, order, text, _ = reference_text(ref2, prefix, "default", seed=5)
    assert [len(x) for x in ix.names] == [1, 64, 65, 120]
    seen = collections.Counter()
    for rec in text:
        if rec is not None:
            P = sc.parse(rec)
            seen["r", len(P["rname"])] += 1
            seen["m", len(P["rnext"])] += P["rnext"] not in (b"=", b"*")
    for ln in (1, 64, 65, 120):
        assert seen["r", ln] >= 300 and seen["m", ln] >= 30, seen   # (measured: >= 700 / >= 78)


def test_the_pipeline_arena_is_too_small_for_long_names_and_a_read_group(ref, genome):
    """the launch the GPU test runs with the pipeline's own arena size: 254-byte names and a 255-byte read group on 150-bp reads —
    by the reference's record lengths the records need more than reads x (2 x 150 + 320) + 1 MB, by more than a wave's worth"""
    from mpibwa_amd import api
    kw, with_qual, rg = sc.OPTION_SETS["rg255"]
    ropt = ref.opt()
    rgid = ref.set_rg(rg)
    try:
        ix = sc.Index(genome["prefix"], ref.bns)
        order = sc.arena_launch(sc.build_cases(ix, ropt.contents, 1), 3)
        text = sc.reference_side(ref, ropt, order, with_qual)
    finally:
        ref.set_rg(None)
    assert all(len(r) == 150 for cs in order for r in cs["reads"]) and all(len(cs["name"]) == 254 for cs in order)
    need = sum(len(t) for t in text)
    have = int(api.load_library().mi355x_sam_arena_bytes(len(text), 150))
    assert have == len(text) * (2 * 150 + 320) + (1 << 20)
    assert need > have + 64 * 1200 and have > 64 * 1200, (need, have)
