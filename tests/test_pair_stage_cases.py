"""CPU: the cases of the designed pairing stage test are what tests/pair_stage_cases.py says they are — shown on the reference's OWN
mem_sam_pe (oracle/pair_inject.c through pyoracle.ref_pair: its rescue loop, primary marking, mem_pair, MAPQ and XA test), without any
kernel.  Per option set and case, `expect` against the reference:

    1   its paired branch wrote two lines, mem_matesw aligned nothing, no hit got an XA entry (the pair without any hit: the ends are
        reported independently, nothing is looked at)
    7   mem_matesw aligned
    11  a hit got an XA entry
    8, 9, 10   the ends are reported independently, and mem_matesw aligned nothing
    2   the ends are reported independently (mem_matesw does align for the hit of a pair whose other end is empty)
    4   mem_sort_dedup_patch gives another list with the sequences than without (the `patch` lists, as tests/dedup_cases.py does it); the
        lists marked cheap_only have no sequence behind them: the reference, which never patches without one, reports two primary hits
    3, 6   limits of the kernel alone (PR_MAXREG / PR_MAXPAIR, the per-length table): the reference has none

Neighbouring steps of a ladder fall on different sides in the reference exactly where they were built to, and a case that names the
sub-optimal score it was built for gets it.  Every non-default option set changes the reference's answer on at least one case of every
family it is listed for — except where the option is read by the kernel alone (max_len) or by the cheap tests of mem_patch_reg, which
the reference reaches only with sequences (max_chain_gap and -w on `dedup`): there the designed codes must differ from the default's.
The `tie` family is run at pair numbers on both sides of 2^23 and 2^31 and compared with the Python restatement of the hash tie-breaks
that tests/test_pairmath.py pins pairmath.h to.  The census is printed."""
import collections

import pytest

import pair_stage_cases as psc
from oracle import pyoracle as po
from ref_band import reg2aln_band

pytestmark = pytest.mark.skipif(not (po.ref_available() and po.pair_inject_available()), reason="oracle/_ref/libbwaref.so, libpairinj.so not present")

ID0 = 1234
KERNEL_ONLY = {("maxlen250", "length"), ("gap50", "dedup"), ("w3", "dedup")}
_CACHE = {}


@pytest.fixture(scope="module")
def ref(genome):
    return po.RefIndex(genome["prefix"])


@pytest.fixture(scope="module")
def maxreg():
    from mpibwa_amd import api
    return int(api.load_library().mi355x_pair_maxreg())


def option_set(ref, genome, maxreg, name):
    """-> (geometry, the reference's options, cases in launch order, the reference's answers): computed once per set and left unchanged"""
    if name not in _CACHE:
        ix = psc.Geometry(ref.bns)
        ropt = psc.set_options(ref.lib, ref.opt(**psc.OPTION_SETS[name]["kw"]), name)
        fams = psc.OPTION_SETS[name]["families"] or psc.FAMILIES
        lists = psc.patch_lists(ref, ropt, genome["seqs"], maxreg) if "dedup" in fams else ()
        order = psc.shuffled(psc.build_cases(ix, ropt.contents, name, lists))
        _CACHE[name] = (ix, ropt, order, psc.reference_side(ref, ropt, order, ID0))
    return _CACHE[name]


def answer(o, w):
    """everything of the reference's answer the stage test compares, with the band of its lines' regions under the options o"""
    return (w["paired"], w["n_align"] > 0, w["n_xa"], w["n_lines"],
            tuple((L["rb"], L["re"], L["qb"], L["qe"], L["score"], L["sub"], L["flag"], L["mapq"],
                   reg2aln_band(o, L["qe"] - L["qb"], L["re"] - L["rb"], L["truesc"], L["w"])) for L in w["lines"]))


def candidate_pairs(ix, cs):
    """hit pairs of the two ends in a live orientation and inside its window (opposite strands: the distance of mem_infer_dir is the
    one mem_pair computes)"""
    st = psc.STATS[cs["pes"]]
    n = 0
    for r0 in cs["regs0"]:
        for r1 in cs["regs1"]:
            d, dist = psc.infer_dir(ix.l_pac, int(r0["rb"]), int(r1["rb"]))
            n += d in st and d in (1, 2) and st[d][0] <= dist <= st[d][1]
    return n


def ladder_answer(cs, w):
    if not psc.is_plain(w):
        return ("not plain", w["paired"])
    f = psc.LADDER_FIELD[cs["family"]]
    return tuple(L[f] for L in w["lines"])


@pytest.mark.parametrize("name", list(psc.OPTION_SETS))
def test_cases_fall_where_they_were_built_to(ref, genome, maxreg, name):
    ix, ropt, order, want = option_set(ref, genome, maxreg, name)
    o = ropt.contents
    n = collections.Counter()
    ladders = collections.defaultdict(list)
    for cs, w in zip(order, want):
        e, fam = cs["expect"], cs["family"]
        n[fam] += 1
        n["code", e] += 1
        what = (name, fam, cs["tag"], e, {k: v for k, v in w.items() if k != "lines"}, [(L["score"], L["sub"], L["flag"], L["mapq"]) for L in w["lines"]])
        if fam == "nohit" and cs["tag"] == "00":
            assert e == 1 and not w["paired"] and w["n_align"] == 0 and w["n_reg2aln"] == 0 and w["n_lines"] == 0, what
        elif e == 1:
            assert psc.is_plain(w), what
            flags = tuple(L["flag"] for L in w["lines"])
            assert flags in ((67, 131), (65, 129)), what
            n[fam, "improper"] += flags == (65, 129)
            if cs.get("improper"):
                assert flags == (65, 129), what
            if "want_sub" in cs:
                assert w["lines"][cs["anchor"]]["sub"] == cs["want_sub"], what
        elif e == 7:
            assert w["n_align"] > 0, what
        elif e == 11:
            assert w["n_align"] == 0 and sum(w["n_xa"]) > 0, what
        elif e in (8, 9, 10):
            assert not w["paired"] and w["n_align"] == 0, what
        elif e == 2:
            assert not w["paired"] and min(len(cs["regs0"]), len(cs["regs1"])) == 0, what
        elif e == 4:
            if cs.get("cheap_only"):
                assert not w["paired"] and w["n_align"] == 0, what
            else:
                assert "read" in cs     # (psc.patch_lists kept it because the reference merges it with the sequences, and only then)
        elif e == 3:
            assert max(len(cs["regs0"]), len(cs["regs1"])) > maxreg or candidate_pairs(ix, cs) > 16, what
            assert min(len(cs["regs0"]), len(cs["regs1"])) > 0
        elif e == 6:
            assert psc.is_plain(w), what
        else:
            assert e is None, what
        if fam == "maxreg" and e == 1:
            assert candidate_pairs(ix, cs) == len(cs["regs0"]) * len(cs["regs1"]) <= 16, what
        if cs.get("ladder"):
            ladders[fam, cs["ladder"][0]].append((cs["ladder"][1], cs["designed"], ladder_answer(cs, w), cs["tag"]))
    # the ladders: the reference's answer changes between neighbouring steps exactly where the family says
    n_flip = collections.Counter()
    for (fam, lad), steps in ladders.items():
        steps.sort(key=lambda s: s[0])
        assert len(steps) >= 2 and all(b[0] == a[0] + 1 for a, b in zip(steps, steps[1:])), (name, fam, lad, [s[0] for s in steps])
        changes = [a[2] != b[2] for a, b in zip(steps, steps[1:])]
        if steps[0][1] is None:      # the reference alone says where: once (with pen_unpaired 0 no pair beats its two ends: never)
            assert sum(changes) == (0 if o.pen_unpaired == 0 else 1), (name, fam, lad, sum(changes))
            if sum(changes):
                at = changes.index(True)
                assert 0 < at < len(changes) - 1, (name, fam, lad, at)      # both neighbours of the step are in the ladder
                print(name, fam, lad, "the reference's flags change between distance", steps[at][0], "and", steps[at + 1][0], ":", steps[at][2], "->", steps[at + 1][2])
        else:
            assert changes == [a[1] != b[1] for a, b in zip(steps, steps[1:])], (name, fam, lad, steps)
        n_flip[fam] += sum(changes)
    for fam in psc.LADDER_FIELD:
        if n[fam] and not (fam == "improper" and o.pen_unpaired == 0):
            assert n_flip[fam] >= (2 if fam == "improper" else 4), (name, fam, n_flip)
    # the census
    print(name, "cases", len(order), "per family", {f: n[f] for f in psc.FAMILIES if n[f]}, "per expected code", {str(c): n["code", c] for c in (1, 2, 3, 4, 6, 7, 8, 9, 10, 11, None) if n["code", c]},
          "improper decided", n["improper", "improper"], "ladder steps at which the reference's answer changes", dict(n_flip))
    if name == "default":
        assert all(n[f] for f in psc.FAMILIES)
        for c in (1, 2, 3, 4, 6, 7, 8, 9, 10, 11):
            assert n["code", c] >= 8, (c, n["code", c])
    if n["improper"]:
        assert n["improper", "improper"] >= 40, n["improper", "improper"]


@pytest.mark.parametrize("name", [s for s in psc.OPTION_SETS if s != "default"])
def test_every_option_set_moves_every_family_it_lists(ref, genome, maxreg, name):
    ix, ropt, order, want = option_set(ref, genome, maxreg, name)
    dopt = ref.opt()
    plain = psc.reference_side(ref, dopt, order, ID0)     # the same pairs under the default options
    moved = collections.Counter()
    for cs, w, p in zip(order, want, plain):
        moved[cs["family"]] += answer(ropt.contents, w) != answer(dopt.contents, p)
    # the designed codes of the same tags under the default options
    codes = collections.defaultdict(set)
    for cs in psc.build_cases(ix, dopt.contents, "default"):
        codes[cs["family"], cs["tag"]].add(cs["expect"])
    for fam in psc.OPTION_SETS[name]["families"]:
        if (name, fam) in KERNEL_ONLY:
            other = sum(1 for cs in order if cs["family"] == fam and (fam, cs["tag"]) in codes and cs["expect"] not in codes[fam, cs["tag"]])
            print(name, fam, "cases whose designed code differs from the default's", other)
            assert other >= 4, (name, fam, other)
        else:
            print(name, fam, "cases on which the reference answers otherwise than under the default options", moved[fam])
            assert moved[fam] >= 1, (name, fam)


@pytest.mark.parametrize("id0", [0, ID0, (1 << 23) - 40, (1 << 31) - 40])
def test_tie_family_against_the_pinned_hash_arithmetic(ref, genome, maxreg, id0):
    """The reference, compiled as it is, at pair numbers where its `id << 8` on an int is undefined (2^23 .. ) and where the int itself
    wraps (2^31 ..): it names the hit that hash_64 and the two's-complement shift of tests/test_pairmath.py name."""
    ix, ropt, order, _ = option_set(ref, genome, maxreg, "default")
    ties = [cs for cs in order if cs["family"] == "tie"]
    assert len(ties) >= 80      # (the launch straddles the boundary 40 pairs in)
    want = psc.reference_side(ref, ropt, ties, id0)
    seen = collections.Counter()
    for k, (cs, w) in enumerate(zip(ties, want)):
        assert psc.is_plain(w), (id0, k, cs["tag"], w)
        got = w["lines"][1 - cs["anchor"]]["qb"]
        assert got == psc.tie_prediction(ix, cs, id0 + k, ropt.contents.a), (id0, k, cs["tag"], got)
        seen[cs["tag"].split("/")[0], got, id0 + k >= 1 << 23 if id0 < 1 << 30 else id0 + k >= 1 << 31] += 1
    print("pair numbers from", id0, "(kind, reported query start, beyond the boundary): pairs", dict(seen))
    for kind in ("pair", "end"):      # either hit wins some, on either side of the boundary
        for qb in (0, 75):
            assert seen[kind, qb, False] + seen[kind, qb, True] >= 5, (id0, kind, qb, seen)
