"""Designed cases of the pairing stage test (pair_simple_kernel through mi355x_pair_stage_batch): pairs given by the region lists of their
two ends as mem_chain2aln could leave them, every family built round ONE threshold or option the kernel reads (mpibwa_amd/csrc/
pair_kernel.hip, pair_common.cuh, pairmath.h).  tests/test_pair_stage_cases.py proves on the CPU, from the reference's own mem_sam_pe
(oracle/pair_inject.c through pyoracle.ref_pair), that every case falls on the side its `expect` names; tests/test_gpu_pair_stage.py
holds the kernel to the same codes and, for the decided pairs, to the reference's fields.

A case is a dict: family, tag, pes (a name of STATS: a launch has one set of insert-size statistics), regs0 / regs1 (ALNREG_DT arrays on
the session genome: 3 contigs of 120 000, l_pac 360 000, no ALT), expect (a status code of device.h, or None: only the invariant "a
decided pair is the reference's plain pair, field by field" holds) and, where the threshold moves a FIELD and not the code, `ladder`:
(name, step) with `designed`, the side of the threshold the step was built for — the CPU test asks that the reference's answer
(LADDER_FIELD says which field) changes between neighbouring steps exactly where `designed` does; designed None: the reference alone
says where (the `improper` ladders: once along each).

Mates are placed with test_pairmath.infer_dir, in the doubled coordinate, so that the distance named in a tag is the one the REFERENCE
computes (for opposite strands |2 l_pac - 1 - b2 - b1|, not a difference of forward coordinates).  Every family comes with the anchor
hit on either strand (`rev`) and with the ends swapped (`swap`), and in an FR and an RF library where orientation matters.

Where an expectation follows from arithmetic (the pair score of `score`, the float products of `mask`, `xa`, `dedup`) it is computed
here in the reference's types, only to CHOOSE the neighbours of the threshold; what decides is the reference, in the CPU test.

Seeds: SEED for the places of the hits (one generator per family: SEED + its index in FAMILIES), SHUFFLE_SEED for the launch order,
PATCH_SEED for the reads of the patch lists (dedup_cases.patch_cases)."""
import math

import numpy as np

from mpibwa_amd import abi
from oracle import pyoracle as po
from pair_cases import _reg
from test_pair_stage import PES_SETS, _pes
from test_pairmath import hash_64, id_mix, infer_dir

SEED = 4100
SHUFFLE_SEED = 4177
PATCH_SEED = 4190
LQ = 150
FAMILIES = ("window", "improper", "score", "T", "mask", "xa", "sub_n", "dedup", "maxreg", "length", "nohit", "tie", "band", "no_rescue")
FORMS = ((0, 0), (0, 1), (1, 0), (1, 1))   # (the anchor hit on the reverse strand, the ends swapped)

# status codes (mpibwa_amd/csrc/device.h)
PR_DECIDED, PR_HOST_NO_HIT, PR_HOST_MAXREG, PR_HOST_PATCH, PR_HOST_LENGTH = 1, 2, 3, 4, 6
PR_HOST_RESCUE, PR_HOST_NO_PAIR, PR_HOST_SCORE, PR_HOST_SUPP, PR_HOST_XA = 7, 8, 9, 10, 11

# insert-size statistics per orientation (0 FF, 1 FR, 2 RF, 3 RR): (low, high, avg, std); the others failed
STATS = {
    "FR": PES_SETS[0][0],
    "RF": PES_SETS[1][0],
    "ALL": PES_SETS[2][0],                       # all four alive: mem_matesw always finds an orientation to align for
    "FRt": {1: (160, 640, 400.0, 20.0)},         # narrow: the ends of the window lie 12 sigma out, where a pair loses to its two ends unpaired
    "RFt": {2: (120, 800, 460.0, 28.5)},
    "FRw": {1: (100, 6000, 3000.0, 800.0)},      # wide: room for 8 x 8 hits 300 apart, all of them candidate pairs; a flat score term
    "RFw": {2: (100, 6000, 3000.0, 800.0)},
}
LIBS = (("FR", 1), ("RF", 2))
TAILS = (("FRt", 1), ("RFt", 2))
WIDE = (("FRw", 1), ("RFw", 2))

# option sets: each moves ONE option from the default (kw: mem_opt_t fields), and names the families it can change (None: all);
# max_len is the launch's longest read (PairParams::ltab_n = 4 max_len + 256)
F_PE = abi.MEM_F_PE
OPTION_SETS = {
    "default": dict(kw={}, families=None),
    "pen0": dict(kw=dict(pen_unpaired=0), families=("improper", "sub_n")),
    "pen5": dict(kw=dict(pen_unpaired=5), families=("improper", "sub_n")),
    "pen40": dict(kw=dict(pen_unpaired=40), families=("improper", "sub_n")),
    "T20": dict(kw=dict(T=20), families=("T", "mask")),
    "T40": dict(kw=dict(T=40), families=("T", "mask")),
    "mask03": dict(kw=dict(mask_level=0.3), families=("mask",)),
    "mask09": dict(kw=dict(mask_level=0.9), families=("mask",)),
    "redun05": dict(kw=dict(mask_level_redun=0.5), families=("dedup",)),
    "xa05": dict(kw=dict(XA_drop_ratio=0.5), families=("xa",)),
    "xa09": dict(kw=dict(XA_drop_ratio=0.9), families=("xa",)),
    "gap50": dict(kw=dict(max_chain_gap=50), families=("dedup",)),
    "seed10": dict(kw=dict(min_seed_len=10), families=("improper",)),      # (read where a hit has no sub-optimal score: sub = min_seed_len * a)
    "seed30": dict(kw=dict(min_seed_len=30), families=("improper",)),
    "w3": dict(kw=dict(w=3), families=("band", "dedup")),
    "ins82": dict(kw=dict(o_ins=8, e_ins=2), families=("sub_n",)),          # (tmp = o_ins + e_ins = 10)
    "ins31": dict(kw=dict(o_ins=3, e_ins=1), families=("band",)),           # (the insertion's inferred band is the wider one)
    "a2b3": dict(kw=dict(a=2, b=3), families=("improper", "score", "sub_n", "band")),
    "coef70": dict(kw=dict(mapQ_coef_len=70, mapQ_coef_fac=4), families=("improper", "length")),
    "matesw0": dict(kw=dict(max_matesw=0), families=("window", "no_rescue")),
    "matesw1": dict(kw=dict(max_matesw=1), families=("no_rescue",)),
    "matesw2": dict(kw=dict(max_matesw=2), families=("no_rescue",)),
    "norescue": dict(kw=dict(flag=F_PE | abi.MEM_F_NO_RESCUE), families=("window", "no_rescue")),
    "maxlen250": dict(kw={}, max_len=250, families=("length",)),
}
# what of the reference's answer a family's ladders move (the lines' field), as answer() reads it
LADDER_FIELD = dict(improper="flag", sub_n="mapq", mask="sub", dedup="sub")


def max_len_of(name):
    return OPTION_SETS[name].get("max_len", LQ)


def set_options(lib, opt, name):
    """the option set's fields on an mem_opt_t made by mem_opt_init of `lib` (kw already applied by the caller's opt(**kw)): the score
    matrix follows a and b"""
    kw = OPTION_SETS[name]["kw"]
    if "a" in kw or "b" in kw:
        lib.bwa_fill_scmat(opt.contents.a, opt.contents.b, opt.contents.mat)
    return opt


class Geometry:
    """what the generator needs of the index: the contig table (se_stage_cases.Index without the bases)"""

    def __init__(self, bns):
        b = bns.contents
        self.l_pac = int(b.l_pac)
        self.n_seqs = int(b.n_seqs)
        self.off = [int(b.anns[k].offset) for k in range(self.n_seqs)]
        self.len = [int(b.anns[k].len) for k in range(self.n_seqs)]

    def fwd_start(self, rb, ln):
        return rb if rb < self.l_pac else 2 * self.l_pac - rb - ln

    def rid_of(self, rb, ln):
        p = self.fwd_start(rb, ln)
        for c in range(self.n_seqs):
            if self.off[c] <= p and p + ln <= self.off[c] + self.len[c]:
                return c
        raise AssertionError("a hit across a contig boundary: %d + %d" % (rb, ln))


def mate_rb(l_pac, b1, d, dist):
    """rb of a mate that the reference's mem_infer_dir puts in orientation d at distance dist of a hit starting at b1"""
    p2 = b1 + dist if d in (0, 1) else b1 - dist
    b2 = p2 if d in (0, 3) else 2 * l_pac - 1 - p2
    assert infer_dir(l_pac, b1, b2) == (d, dist), (b1, d, dist, infer_dir(l_pac, b1, b2))
    return b2


def pair_term(stats, d, dist, a):
    """the double term of a candidate pair's score, as src/bwamem_pair.c:217-218 evaluates it"""
    _, _, avg, std = stats[d]
    ns = (dist - avg) / std
    return .721 * math.log(2. * math.erfc(math.fabs(ns) * math.sqrt(.5))) * a


def pair_score(stats, d, dist, s0, s1, a):
    q = int(float(s0 + s1) + pair_term(stats, d, dist, a) + .499)
    return q if q > 0 else 0


def f32_ge(v, n, level):
    """v >= n * level with level a float option: the comparison of src/bwamem.c:507 in its types"""
    return bool(np.float32(v) >= np.float32(n) * np.float32(level))


def f32_gt(v, n, level):
    """v > level * n (src/bwamem.c:455)"""
    return bool(np.float32(v) > np.float32(level) * np.float32(n))


def xa_product(p, ratio):
    """score * XA_drop_ratio of src/bwamem_extra.c:90-93: the float option widened to double, times the int score"""
    return float(p) * float(np.float32(ratio))


class Builder:
    def __init__(self, ix, o, name):
        self.ix, self.o, self.name = ix, o, name
        self.L = ix.l_pac
        self.cases = []
        self.norescue = bool(o.flag & abi.MEM_F_NO_RESCUE) or o.max_matesw <= 0
        self.tmp = max(o.a + o.b, o.o_del + o.e_del, o.o_ins + o.e_ins)
        self.rng = None

    def family(self, fam):
        self.fam = fam
        self.rng = np.random.default_rng(SEED + FAMILIES.index(fam))

    def add(self, tag, pes, anchor_end, mate_end, swap, expect, **extra):
        e0, e1 = (mate_end, anchor_end) if swap else (anchor_end, mate_end)
        cs = dict(family=self.fam, tag=tag, pes=pes, regs0=np.array(e0, dtype=po.ALNREG_DT), regs1=np.array(e1, dtype=po.ALNREG_DT), expect=expect,
                  anchor=1 if swap else 0)
        cs.update(extra)
        self.cases.append(cs)

    # -- places --
    def at(self, rb, ln=LQ, qb=0, qe=LQ, score=LQ, **kw):
        """a hit on reference [rb, rb + ln) of the doubled coordinate, well inside its contig"""
        c = self.ix.rid_of(rb, ln)
        p = self.ix.fwd_start(rb, ln) - self.ix.off[c]
        edge = kw.pop("edge", False)   # (edge: the family wants a hit at the end of a contig; otherwise every rescue window fits into it)
        assert edge or (4000 <= p and p + ln <= self.ix.len[c] - 4000), (rb, ln, p)
        return _reg(rb, rb + ln, qb, qe, c, score, **kw)

    def spot(self, rev, ln=LQ, c=None):
        """rb of an anchor hit: a random place 30 000 .. 80 000 into a contig, on the strand asked for"""
        c = int(self.rng.integers(self.ix.n_seqs)) if c is None else c
        p = self.ix.off[c] + int(self.rng.integers(30000, 80000))
        return (2 * self.L - p - ln) if rev else p

    def other(self, rb, k=1, rev=None):
        """rb of a hit elsewhere: on another contig than rb's, either strand"""
        c = (self.ix.rid_of(rb, 1) + 1 + (k & 1)) % self.ix.n_seqs
        return self.spot(int(self.rng.integers(2)) if rev is None else rev, c=c) + 1000 * (k >> 1)

    def mate(self, rb, d, dist):
        return mate_rb(self.L, rb, d, dist)


def _window(B):
    """The insert-size window dist >= low && dist <= high, which stands in mem_matesw's "is this orientation explained?" (no_rescue_needed)
    and in mem_pair's scan (pair_candidates_of).  one: a full-length hit per end at low - 1 .. high + 1 — outside, mem_matesw aligns (7; with
    the rescue loop off no pair is found: 8), inside the pair is plain (1).  second: the best mate hit lies 6 000 away and a SECOND,
    weaker mate hit stands at the distance; a weak hit of the anchor's end explains the far one, so that only the anchor's call depends on
    the window.  The same pairs under the statistics with all four orientations alive: mem_matesw aligns for the three others whatever the
    distance (7), and with the rescue loop off they are the one-orientation pairs again.  contig: two hits whose doubled coordinates are
    in the window but which lie on different contigs — mem_matesw's test does not look at the contig (explained: no alignment), mem_pair's
    does (no pair): 8, the one way to that code with the rescue loop on."""
    for pes, d in LIBS + (("ALL", 1), ("ALL", 2)):
        low, high = STATS[pes][d][:2]
        for dist in (low - 1, low, low + 1, high - 1, high, high + 1):
            inside = low <= dist <= high
            where = "%s%+d" % (("low", dist - low) if dist <= low + 1 else ("high", dist - high))
            for rev, swap in FORMS:
                a = B.spot(rev)
                if pes == "ALL":
                    exp = (PR_DECIDED if inside else PR_HOST_NO_PAIR) if B.norescue else PR_HOST_RESCUE
                else:
                    exp = PR_DECIDED if inside else PR_HOST_NO_PAIR if B.norescue else PR_HOST_RESCUE
                B.add("%s/%d/one/%s" % (pes, d, where), pes, [B.at(a)], [B.at(B.mate(a, d, dist))], swap, exp)
                if pes == "ALL":
                    continue
                a2 = a + 6000
                far = B.mate(a2, d, (low + high) // 2)
                B.add("%s/%d/second/%s" % (pes, d, where), pes, [B.at(a), B.at(a2, score=100)], [B.at(far), B.at(B.mate(a, d, dist), score=100)], swap,
                      PR_DECIDED if inside or B.norescue else PR_HOST_RESCUE)
    ix = B.ix
    for pes, d in LIBS:
        low, high = STATS[pes][d][:2]
        for c in (0, 1):
            for dist in ((low + high) // 2, high - 40):
                for swap in (0, 1):
                    # FR: a forward hit at the end of contig c, its mate reverse at the start of c + 1; RF: the reverse hit on c, the forward one on c + 1
                    edge = ix.off[c + 1]
                    a = edge - LQ - 5 if d == 1 else edge + 10
                    m = B.mate(a, d, dist)
                    ra, rm = B.at(a, edge=True), B.at(m, edge=True)
                    assert ra["rid"] != rm["rid"]
                    B.add("%s/%d/contig/%d/%d" % (pes, d, c, dist), pes, [ra], [rm], swap, PR_HOST_NO_PAIR)


def _improper(B):
    """o <= score_un: the pair is in the window but so far in the tail that the two best hits unpaired score more; z[0] = z[1] = 0, the
    MAPQs are mem_approx_mapq_se's alone, flag 0x2 stays off (65 / 129).  ladder: every distance from the mean to either end of the
    window — somewhere the reference's flag changes (the CPU test finds where, nothing here computes it); with pen_unpaired 0 it never
    does, since no pair beats its ends by the half point the score term can add.  low: scores 30 / 30 and 40 / 40 at the ends of the window.
    z: two hits on the mate's end, the weaker one at the mean — mem_pair's best pair names hit 1, and the fall-back reports hit 0."""
    for pes, d in TAILS:
        low, high, avg, _ = STATS[pes][d]
        avg = int(avg)
        for k, (lo, hi, form) in enumerate(((avg, high, FORMS[0 if d == 1 else 1]), (low, avg, FORMS[3 if d == 1 else 2]))):
            a = B.spot(form[0])
            for dist in range(lo, hi + 1):
                B.add("%s/ladder%d/%d" % (pes, k, dist), pes, [B.at(a)], [B.at(B.mate(a, d, dist))], form[1], PR_DECIDED, ladder=("%s/%d" % (pes, k), dist), designed=None)
        for dist in (low, low + 1, low + 30, high - 30, high - 1, high):
            for rev, swap in FORMS:
                for s in (30 * B.o.a, 40 * B.o.a, 150 * B.o.a):
                    a = B.spot(rev)
                    B.add("%s/low/%d/%d" % (pes, s, dist), pes, [B.at(a, score=s)], [B.at(B.mate(a, d, dist), score=s)], swap, PR_DECIDED, improper=True)
                a = B.spot(rev)
                B.add("%s/z/%d" % (pes, dist), pes, [B.at(a)], [B.at(B.mate(a, d, dist)), B.at(B.mate(a, d, avg), score=110)], swap, PR_DECIDED, improper=True)


def _score(B):
    """o <= 0: at the end of the narrow window the score term is about -54 a, and a pair of weak hits scores nothing (mem_pair returns 0:
    the ends are reported independently, 9).  The sum of the two scores climbs one by one through the value at which the pair score
    becomes 1 (decided, improper)."""
    a_ = B.o.a
    for pes, d in TAILS:
        low, high = STATS[pes][d][:2]
        for dist in (low, high):
            zero = max(s for s in range(38, 400) if pair_score(STATS[pes], d, dist, 19, s - 19, a_) == 0)
            for rev, swap in FORMS:
                for tot in range(zero - 3, zero + 4):
                    s0 = 19 + (tot - 38) // 3
                    a = B.spot(rev)
                    B.add("%s/%d/%+d" % (pes, dist, tot - zero), pes, [B.at(a, score=s0)], [B.at(B.mate(a, d, dist), score=tot - s0)], swap,
                          PR_DECIDED if tot > zero else PR_HOST_SCORE)


def _T(B):
    """score >= T of a second primary hit: a primary on query [0, 100) and a hit on [100, 150) elsewhere, of score T - 1 (paired, plain), T and
    T + 1 (the single-end logic's case: 10), on either end."""
    T = B.o.T
    for pes, d in LIBS:
        for s in (T - 1, T, T + 1):
            for rev, swap in FORMS:
                for on_mate in (0, 1):
                    a = B.spot(rev)
                    m = B.mate(a, d, 400)
                    x = B.at(B.other(a), ln=50, qb=100, qe=150, score=s)
                    ea, em = [B.at(a, ln=100, qe=100, score=100)], [B.at(m)]
                    if on_mate:
                        ea, em = [B.at(a)], [B.at(m, ln=100, qe=100, score=100)]
                    (em if on_mate else ea).append(x)
                    B.add("%s/%+d/%s" % (pes, s - T, "mate" if on_mate else "anchor"), pes, ea, em, swap, PR_DECIDED if s < T else PR_HOST_SUPP)


def _mask(B):
    """e_min - b_max >= min_l * mask_level (float): a primary on query [0, 100) and a second hit elsewhere of span n that overlaps it by v, for
    v just below, at and just above n * mask_level.  Below, the hit is a second primary: with a score under T the pair is plain and sub
    stays 0, at T it is the single-end logic's (10); from the limit on it is secondary and sub is its score."""
    T, lvl = B.o.T, B.o.mask_level
    for n in (30, 40, 49, 50, 60, 70):
        c = math.ceil(round(float(np.float32(lvl)) * n, 4))
        for v in (c - 1, c, c + 1):
            if not 0 < v < n:
                continue
            sec = f32_ge(v, n, lvl)
            for s in (T - 1, T):
                for rev, swap in FORMS[::2] if n % 20 else FORMS:
                    a = B.spot(rev)
                    x = B.at(B.other(a), ln=n, qb=100 - v, qe=100 - v + n, score=s)
                    B.add("n%d/v%d/%s/%d" % (n, v, "sec" if sec else "pri", s - T), "FR", [B.at(a, ln=100, qe=100, score=100), x], [B.at(B.mate(a, 1, 400))], swap,
                          PR_DECIDED if sec or s < T else PR_HOST_SUPP, want_sub=s if sec else 0, ladder=("n%d/s%d/%d%d" % (n, s - T, rev, swap), v), designed=sec)


def _xa(B):
    """score >= primary's score * XA_drop_ratio: a secondary hit of score s under a primary of score p, s on both sides of the product, p such
    that the product is an integer (150, 100) and such that it is not (147, 77).  The secondary has a weak mate hit of its own, so that
    mem_matesw has nothing to align for it.  other: the secondary stands under a second primary below T, which is not reported — the
    reference writes no XA on the lines it reports, the kernel's test looks at every primary and leaves the pair (expect None)."""
    ratio = B.o.XA_drop_ratio
    for p in (150, 147, 100, 77):
        exact = xa_product(p, ratio)
        for s in sorted({math.floor(exact) - 1, math.floor(exact), math.floor(exact) + 1, math.ceil(exact)}):
            for rev, swap in FORMS:
                a = B.spot(rev)
                x = B.other(a)
                B.add("p%d/s%d" % (p, s), "FR", [B.at(a, score=p), B.at(x, score=s)], [B.at(B.mate(a, 1, 400)), B.at(B.mate(x, 1, 400), score=40)], swap,
                      PR_HOST_XA if s >= exact else PR_DECIDED)
    for rev, swap in FORMS:
        for s in (27, 24, 23):
            a = B.spot(rev)
            x = B.other(a)
            B.add("other/%d" % s, "FR", [B.at(a, ln=100, qe=100, score=100), B.at(x, ln=50, qb=100, qe=150, score=29), B.at(B.other(a, 2), ln=50, qb=100, qe=150, score=s)],
                  [B.at(B.mate(a, 1, 400))], swap, None)


def _sub_n(B):
    """score difference <= tmp = max(a + b, o_del + e_del, o_ins + e_ins).  se: under a weak primary (score 30: its secondaries stay
    below the XA product) one secondary tmp - 1 below and 0 .. 6 more at tmp - 1, tmp or tmp + 1 below, each shifted by a few bases (not redundant);
    the mate stands in the tail of the narrow window, where the MAPQ is mem_approx_mapq_se's alone and moves with sub_n.  pe: one hit
    against a primary and 1 .. 4 weaker mate hits 8 bases apart, under the wide statistics (one score term for all of them); the third
    best candidate pair scores tmp - 1, tmp or tmp + 1 below the second, and q_pe moves with n_sub."""
    tmp = B.tmp
    ratio = B.o.XA_drop_ratio
    pa = max(p for p in range(20, 150) if p - (tmp - 1) < xa_product(p, ratio))   # (30 by default: 24 < 30 * (double)0.8f)
    span = pa // B.o.a       # (as long as a hit of that score without a mismatch: its identity is 1 and the MAPQ is far from 0)
    for pes, d in TAILS:
        high = STATS[pes][d][1]
        for n in range(0, 7):
            for k, diff in enumerate((tmp - 1, tmp, tmp + 1)):
                for rev, swap in FORMS[::3] if n % 2 else FORMS[1:3]:
                    a = B.spot(rev)
                    step = (span // 20 + 2) * (1 if d == 1 else -1)   # (towards the mate, a few bases: not redundant, and every pair stays in the tail)
                    hit = lambda j, sc: B.at(a + step * j, ln=span, qe=span, score=sc)
                    hits = [hit(0, pa), hit(1, pa - (tmp - 1))] + [hit(j + 2, pa - diff) for j in range(n)]
                    B.add("se/%s/n%d/%+d" % (pes, n, diff - tmp), pes, hits, [B.at(B.mate(a, d, high))], swap, PR_DECIDED, improper=True,
                          ladder=("se/%s/n%d/%d%d" % (pes, n, rev, swap), k) if n else None, designed=diff <= tmp)
        # chosen: the pair with a SECONDARY hit at the mean is the best pair; whether it beats the two primaries unpaired is pen_unpaired's
        # matter (it does from 36 on) — then the secondary hit is reported, with its primary's score as sub
        for rev, swap in FORMS:
            a = B.spot(rev)
            m = B.mate(a, d, high)
            avg = int(STATS[pes][d][2])
            proper = pair_score(STATS[pes], d, avg, 115 * B.o.a, 150 * B.o.a, B.o.a) > 300 * B.o.a - B.o.pen_unpaired
            # (once it is reported, the former primary is ITS secondary, and close enough for an XA entry)
            B.add("chosen/%s" % pes, pes, [B.at(a, score=150 * B.o.a), B.at(B.mate(m, d, avg), score=115 * B.o.a)], [B.at(m, score=150 * B.o.a)], swap,
                  PR_HOST_XA if proper else PR_DECIDED)
    s = max(p for p in range(20, 150) if p - tmp < xa_product(p, ratio))   # (34 by default)
    for pes, d in WIDE:      # (the wide statistics: the score term is the same for hits a few bases apart)
        for n in range(1, 5):
            for k, diff in enumerate((tmp - 1, tmp, tmp + 1)):
                for rev, swap in FORMS:
                    a = B.spot(rev)
                    m = B.mate(a, d, 3000)
                    hits = [B.at(m, score=s), B.at(m + 8, score=s - tmp)] + [B.at(m + 8 * (j + 2), score=s - tmp - diff) for j in range(n)]
                    B.add("pe/%s/n%d/%+d" % (pes, n, diff - tmp), pes, [B.at(a, score=s)], hits, swap, PR_DECIDED, ladder=("pe/%s/n%d/%d%d" % (pes, n, rev, swap), k),
                          designed=diff <= tmp or B.o.pen_unpaired == 0)   # (pen_unpaired 0: the pair never beats its ends, q_pe is not read)


def _dedup(B, patch_lists):
    """mem_sort_dedup_patch on the two hits of an end.  ref / query: their overlap on the reference, or on the query, just below and just
    above mask_level_redun x the shorter one (the weaker hit goes, or stays as a secondary whose score is sub), with the weaker and with
    the stronger hit ending first.  gap: a second hit max_chain_gap - 1, max_chain_gap and max_chain_gap + 1 beyond the end of the first
    and colinear with it: within reach the two pass the cheap tests of mem_patch_reg when the gap is small against -w (max_chain_gap 50: 4),
    at 10 000 no band is that wide and all three are two primary hits (10).  cheap: two pieces a 7- or 5-base deletion apart (4 while the gap is at most 2 w, else two primary hits; no sequence
    stands behind them, the CPU test can only show that the reference, which never patches without one, is indifferent).  twin: equal
    (score, rb, qb).  patch: raw lists of dedup_cases.patch_cases that the reference merges when it has the sequences (4)."""
    lvl, gap = B.o.mask_level_redun, B.o.max_chain_gap
    cut = next(dl for dl in range(1, 150) if not f32_gt(150 - dl, 150, lvl))   # the first shift at which 150 - shift is no longer > lvl * 150
    for dl in (cut - 1, cut, cut + 1):
        for strong_first in (0, 1):
            for rev, swap in FORMS:
                a = B.spot(rev)
                x, y = B.at(a, score=100 if strong_first else 150), B.at(a - dl, score=150 if strong_first else 100)   # (y ends first)
                best = y if strong_first else x
                B.add("ref/%+d/%d" % (dl - cut, strong_first), "FR", [x, y], [B.at(B.mate(int(best["rb"]), 1, 400))], swap, PR_DECIDED,
                      want_sub=0 if dl < cut else 100, ladder=("ref/%d/%d%d" % (strong_first, rev, swap), dl), designed=dl < cut)
    cutq = next(q for q in range(1, 80) if not f32_gt(80 - q, 80, lvl))
    for q in (cutq - 1, cutq, cutq + 1):
        for rev, swap in FORMS:
            a = B.spot(rev)
            sub = 0 if q < cutq or not f32_ge(80 - q, 80, B.o.mask_level) else 29   # (gone; or kept as a second primary below T; or secondary)
            B.add("query/%+d" % (q - cutq), "FR", [B.at(a, ln=80, qe=80, score=80), B.at(a, ln=80, qb=q, qe=q + 80, score=29)], [B.at(B.mate(a, 1, 400))], swap,
                  PR_DECIDED, want_sub=sub, ladder=("query/%d%d" % (rev, swap), q), designed=sub)
    for g in (gap - 1, gap, gap + 1):
        for rev, swap in FORMS:
            a = B.spot(rev)
            x, y = B.at(a, ln=50, qe=50, score=50), B.at(a + 50 + g, ln=55, qb=95, qe=150, score=55)
            reach = g < gap and abs(g - 45) <= 2 * B.o.w
            mates = [B.at(B.mate(a, 1, 400))] + ([B.at(B.mate(a + 50 + g, 1, 400), score=40)] if g > 150 else [])   # (a weak mate hit explains a far y)
            B.add("gap/%+d" % (g - gap), "FR", [x, y], mates, swap, PR_HOST_PATCH if reach else PR_HOST_SUPP, cheap_only=reach)
    for rev, swap in FORMS:
        for gdel in (7, 5):
            a = B.spot(rev)
            x, y = B.at(a, ln=70, qe=70, score=70), B.at(a + 70 + gdel, ln=80, qb=70, qe=150, score=80)
            B.add("cheap/%d" % gdel, "FR", [y, x], [B.at(B.mate(a, 1, 400))], swap, PR_HOST_PATCH if gdel <= 2 * B.o.w else PR_HOST_SUPP, cheap_only=gdel <= 2 * B.o.w)
        a = B.spot(rev)
        B.add("twin/same", "FR", [B.at(a), B.at(a)], [B.at(B.mate(a, 1, 400))], swap, PR_DECIDED, want_sub=0)
        a = B.spot(rev)
        B.add("twin/shorter", "FR", [B.at(a), B.at(a, ln=140, qe=140, score=150)], [B.at(B.mate(a, 1, 400))], swap, PR_DECIDED, want_sub=0)
    for k, (regs, read) in enumerate(patch_lists):
        c = int(regs["rid"][0])
        m = B.at(B.spot(k & 1, c=c))
        B.add("patch/%d" % k, "FR", list(regs), [m], (k >> 1) & 1, PR_HOST_PATCH, read=read)


def _maxreg(B):
    """PR_MAXREG = 8 regions on an end and PR_MAXPAIR = 16 candidate pairs.  The hits of an end share the query span, lie 300 apart and
    score 150 then 100 (below the XA product); under the wide statistics every hit pair is a candidate (distances 900 .. 5 100).  8 x 1 and 4 x 4: decided; 9 x 1,
    4 x 5 and 8 x 8: 3."""
    low = min(100, math.floor(xa_product(150, B.o.XA_drop_ratio)) - 5)
    for na, nm, exp in ((8, 1, PR_DECIDED), (9, 1, PR_HOST_MAXREG), (4, 4, PR_DECIDED), (4, 5, PR_HOST_MAXREG), (8, 8, PR_HOST_MAXREG), (1, 9, PR_HOST_MAXREG),
                        (2, 8, PR_DECIDED), (3, 6, PR_HOST_MAXREG)):
        for rev, swap in FORMS:
            a = B.spot(rev)
            m = B.mate(a, 1, 3000)
            B.add("%dx%d" % (na, nm), "FRw", [B.at(a + 300 * j, score=low if j else 150) for j in range(na)],
                  [B.at(m + 300 * j, score=low if j else 150) for j in range(nm)], swap, exp)


def _length(B, max_len):
    """l >= ltab_n = 4 max_len + 256: a region whose longer span, on the reference or on the query, is the last entry of the per-length
    table (decided) and one beyond it (6).  The reference has no such table: both are plain pairs to it.  The mate stands in the tail of the
    narrow window: the MAPQ is mem_approx_mapq_se's alone, and shows the table's last entry (mapQ_coef_fac / log(l))."""
    for lmax in sorted({4 * LQ + 255, 4 * max_len + 255}):
        for l in (lmax, lmax + 1):
            for on_query in (0, 1):
                for rev, swap in FORMS:
                    a = B.spot(rev)
                    r = B.at(a, ln=LQ if on_query else l, qe=l if on_query else LQ, score=100)
                    B.add("%d/%s" % (l, "query" if on_query else "ref"), "FRt", [r], [B.at(B.mate(a, 1, 620))], swap,
                          PR_DECIDED if l < 4 * max_len + 256 else PR_HOST_LENGTH)


def _nohit(B):
    """(0, 0): the two unmapped records, decided without a look at anything (flags 77 / 141, req -3, rid -1).  One empty end: 2 — also with 9
    regions on the other, since the test for an empty end comes before the one for PR_MAXREG."""
    for rev, swap in FORMS:
        a = B.spot(rev)
        B.add("00", "FR", [], [], swap, PR_DECIDED)
        B.add("01", "FR", [], [B.at(a)], swap, PR_HOST_NO_HIT)
        B.add("08", "FR", [], [B.at(a + 300 * j, score=100 if j else 150) for j in range(8)], swap, PR_HOST_NO_HIT)
        B.add("09", "FR", [], [B.at(a + 300 * j, score=100 if j else 150) for j in range(9)], swap, PR_HOST_NO_HIT)


def _tie(B):
    """Equal keys, where hash_64 decides.  pair: the mate's end has two primaries below T on query [0, 75) and [75, 150), 40 bases apart
    and of one score: two candidate pairs of one score, and hash_64(y ^ id << 8) names the hit that is reported (`id << 8` on the
    reference's int: undefined from pair number 2^23 on).  end: the same in the tail of the narrow window — the pair loses, hit 0 of the
    end is reported, and mem_mark_primary_se's hash_64(id + i) says which of the two that is."""
    for rep in range(20):
        for rev, swap in FORMS:
            for kind, pes in (("pair", "FR"), ("end", "FRt")):
                a = B.spot(rev)
                m = B.mate(a, 1, 400 if kind == "pair" else 620)
                B.add("%s/%d" % (kind, rep), pes, [B.at(a)], [B.at(m, ln=75, qe=75, score=29), B.at(m + 40, ln=75, qb=75, qe=150, score=29)], swap, PR_DECIDED)


def _band(B):
    """The band of mem_reg2aln's first global alignment: max of the two infer_bw, capped by the region's own w only where it passes -w.
    One hit per end with unequal spans, truesc below score, and a region band of 0 (a rescued hit), below and above the inferred one."""
    for dl in (0, 1, -2, 5, 12):
        for drop in (0, 4, 11, 30, 60):
            for w_reg in (0, 2, 5, 100, 400):
                rev, swap = FORMS[(dl + drop + w_reg) % 4]
                a = B.spot(rev)
                B.add("dl%d/-%d/w%d" % (dl, drop, w_reg), "FR", [B.at(a, ln=LQ + dl, score=B.o.a * 140, truesc=B.o.a * 140 - drop, w=w_reg)],
                      [B.at(B.mate(a, 1, 400), ln=LQ - dl, score=B.o.a * 140 - drop, truesc=B.o.a * 140 - 2 * drop, w=w_reg)], swap, PR_DECIDED)


def _no_rescue(B):
    """MEM_F_NO_RESCUE, max_matesw <= 0 (PairParams::no_rescue) and the cut of the candidate list at max_matesw.  third: three hits of
    an end that are candidates for rescue (within pen_unpaired of the best, below its XA product: 80, 63, 63), 300 apart, the k-th of
    them out of the mate's window: mem_matesw aligns for it (7) only while k <= max_matesw and the loop runs at all.  two: under the
    statistics with four orientations alive an FR pair and, from the same anchor, an FF hit: 7 with the loop, a decided pair without."""
    mm = B.o.max_matesw
    for pes, d in LIBS:
        low, high = STATS[pes][d][:2]
        for k in (1, 2, 3):
            for rev, swap in FORMS:
                a = B.spot(rev)
                # two of the hits 300 apart and both in the mate's window, one 3 000 away on either side; which of them is the k-th in mem_sort_dedup_patch's
                # order (score, then rb) follows from where they stand
                for offs in [o for far in (3000, -3000) for o in ((0, 300, far), (0, far, 300), (far, 0, 300), (300, far, 0), (far, 300, 0), (300, 0, far))]:
                    hits = [B.at(a + offs[j], score=80 if j == 0 else 63) for j in range(3)]
                    order = sorted(range(3), key=lambda j: (-int(hits[j]["score"]), int(hits[j]["rb"])))
                    if abs(offs[order[k - 1]]) == 3000:
                        break
                else:
                    raise AssertionError((pes, k, rev))
                m = B.mate(a, d, 500 if d == 1 else 450)
                for j in range(3):
                    dd, dist = infer_dir(B.L, a + offs[j], m)
                    assert (dd == d and low <= dist <= high) == (abs(offs[j]) != 3000)
                B.add("third/%s/k%d" % (pes, k), pes, hits, [B.at(m)], swap, PR_HOST_RESCUE if not B.norescue and k <= mm else PR_DECIDED)
    for rev, swap in FORMS:
        for dist0 in (50, 300, 900):
            a = B.spot(rev)
            B.add("two/%d" % dist0, "ALL", [B.at(a)], [B.at(B.mate(a, 1, 400)), B.at(B.mate(a, 0, dist0), score=100)], swap, PR_DECIDED if B.norescue else PR_HOST_RESCUE)


def build_cases(ix, o, name="default", patch_lists=()):
    """All the families of an option set -> list of case dicts (not shuffled).  ix: Geometry; o: mem_opt_t contents WITH the set's
    fields; patch_lists: patch_lists() for the `dedup` family (needs the reference and the genome's sequences)"""
    fams = OPTION_SETS[name]["families"] or FAMILIES
    B = Builder(ix, o, name)
    for fam in FAMILIES:
        if fam not in fams:
            continue
        B.family(fam)
        if fam == "dedup":
            _dedup(B, patch_lists)
        elif fam == "length":
            _length(B, max_len_of(name))
        else:
            globals()["_" + fam](B)
    return B.cases


def patch_lists(ref, ropt, seqs, maxreg, n_reads=40):
    """raw region lists (at most maxreg regions) that the reference's mem_sort_dedup_patch MERGES when it has the sequences and leaves
    alone without: they pass the cheap tests of mem_patch_reg -> [(regs, read)]"""
    import dedup_cases as dc
    cases = dc.patch_cases(ref, ropt, seqs, n_reads, PATCH_SEED)
    with_seq, bare = dc.reference_results(ref, ropt, cases, True), dc.reference_results(ref, ropt, cases, False)
    return [(cs["regs"], cs["read"]) for cs, w, b in zip(cases, with_seq, bare) if not dc.same_lists(w, b) and 2 <= len(cs["regs"]) <= maxreg]


def by_stats(cases):
    """the cases of an option set by the statistics they run under -> {pes name: [case]}"""
    out = {}
    for cs in cases:
        out.setdefault(cs["pes"], []).append(cs)
    return out


def shuffled(cases, seed=SHUFFLE_SEED, last=None):
    """the launch order: shuffled; the family `last` behind the others (in its own shuffled order)"""
    rng = np.random.default_rng(seed)
    order = [cases[i] for i in rng.permutation(len(cases))]
    if last:
        order = [cs for cs in order if cs["family"] != last] + [cs for cs in order if cs["family"] == last]
    return order


def device_regions(order, reg_dt, maxreg):
    """-> regs (2 n, maxreg) of reg_dt and n_regs (2 n,) for Engine.pairs_stage; of a longer list only the count goes up"""
    regs = np.zeros((2 * len(order), maxreg), dtype=reg_dt)
    n_regs = np.zeros(2 * len(order), dtype=np.int32)
    for k, cs in enumerate(order):
        for e, r in enumerate((cs["regs0"], cs["regs1"])):
            n_regs[2 * k + e] = len(r)
            if 0 < len(r) <= maxreg:
                for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep"):
                    regs[2 * k + e, :len(r)][f] = r[f]
    return regs, n_regs


def reference_side(ref, ropt, order, id0):
    """the reference's mem_sam_pe on every pair of a launch; pair k has the number id0 + k"""
    pes = {}
    out = []
    for k, cs in enumerate(order):
        if cs["pes"] not in pes:
            pes[cs["pes"]] = _pes(STATS[cs["pes"]])
        out.append(po.ref_pair(ropt, ref.bns, ref.pac, pes[cs["pes"]], id0 + k, LQ, cs["regs0"], cs["regs1"]))
    return out


def is_plain(w):
    return w["paired"] and w["n_align"] == 0 and w["n_xa"] == (0, 0) and w["n_lines"] == 2


def tie_prediction(ix, cs, pair_id, a=1):
    """for a `tie` case: query start (0 or 75) of the mate-end hit that is reported for pair number pair_id, from the Python restatements
    tests/test_pairmath.py pins pairmath.h to: hash_64, and `id << 8` as two's-complement arithmetic on a 32-bit int.  kind end: hit 0
    after mem_mark_primary_se's sort by (score, hash_64(id + i)); kind pair: the hit named by the best candidate pair of mem_pair
    (src/bwamem_pair.c:182-243), equal pair scores ordered by hash_64(y ^ id << 8)"""
    M64 = (1 << 64) - 1
    e_m = 1 - cs["anchor"]
    regs = cs["regs1"] if e_m else cs["regs0"]
    anchor = (cs["regs0"] if e_m else cs["regs1"])[0]
    first = sorted(range(2), key=lambda j: int(regs[j]["rb"]))   # mem_sort_dedup_patch: equal scores by rb
    id_e = (pair_id << 1 | e_m) & M64
    lst = [regs[first[i]] for i in sorted(range(2), key=lambda i: hash_64((id_e + i) & M64))]
    if cs["tag"].startswith("end"):
        return int(lst[0]["qb"])
    stats = STATS[cs["pes"]]
    v = []
    for e, hits in ((cs["anchor"], [anchor]), (e_m, lst)):
        for i, r in enumerate(hits):
            rb, rid = int(r["rb"]), int(r["rid"])
            x = rb if rb < ix.l_pac else 2 * ix.l_pac - 1 - rb
            v.append((rid << 32 | (x - ix.off[rid]), int(r["score"]) << 32 | i << 2 | (rb >= ix.l_pac) << 1 | e))
    v.sort()
    u = []
    for i, (x, y) in enumerate(v):
        for r in (0, 1):
            d = r << 1 | (y >> 1 & 1)
            if d not in stats:
                continue
            which = r << 1 | ((y & 1) ^ 1)
            for k in range(i - 1, -1, -1):
                if v[k][1] & 3 != which:
                    continue
                dist = x - v[k][0]
                if dist > stats[d][1]:
                    break
                if dist < stats[d][0]:
                    continue
                py = k << 32 | i
                u.append((pair_score(stats, d, dist, y >> 32, v[k][1] >> 32, a) << 32 | (hash_64(py ^ (id_mix(pair_id) & M64)) & 0xffffffff), py))
    assert len(u) == 2 and u[0][0] >> 32 == u[1][0] >> 32, u
    best = max(u)[1]
    z = [(v[j][1] & 0xffffffff) >> 2 for j in (best >> 32, best & 0xffffffff) if v[j][1] & 1 == e_m]
    return int(lst[z[0]]["qb"])
