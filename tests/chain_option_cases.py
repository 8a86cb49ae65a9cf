"""Seed sets on which the options of the chaining stage decide the outcome, and what the reference's own mem_chain + mem_chain_flt
(oracle/chain_inject.c) make of them under every option set.  Shared by tests/test_chain_option_cases.py (CPU: the inputs reach the
branches they are there for, the library's host chaining equals the reference) and tests/test_gpu_chain_options.py (chain_kernel and
chain_heavy_kernel against the reference).

The seven options chain_params hands to the kernels: w and max_chain_gap (test_and_merge, src/bwamem.c:202; max_chain_gap also in the
mask test, :355), min_chain_weight (:337), mask_level (:355), drop_ratio and min_seed_len (:358), max_chain_extend (:373-378).

No read here has two seeds at one reference position (the device may decline such a read) and every read is 151 bases long, a length at
which mem_flt_chained_seeds returns at once under every set of OPTION_SETS."""
import numpy as np

import chain_cases as cc
from oracle import pyoracle as po

LQ = 151
MAX_HITS = 400          # hits per interval, below max_occ = 500: every hit is a seed and l_rep = 0

OPTION_SETS = {
    "default": dict(),
    "extend1": dict(max_chain_extend=1),
    "extend3": dict(max_chain_extend=3),
    "extend40": dict(max_chain_extend=40),
    "weight30": dict(min_chain_weight=30),
    "weight45": dict(min_chain_weight=45),
    "gap40": dict(max_chain_gap=40),
    "gap100": dict(max_chain_gap=100),
    "w0": dict(w=0),
    "w2": dict(w=2),
    "w130": dict(w=130),
    "seedlen10": dict(min_seed_len=10),
    "seedlen30": dict(min_seed_len=30),
    "mask.1_drop.9": dict(mask_level=0.1, drop_ratio=0.9),
    "mask.95_drop.1": dict(mask_level=0.95, drop_ratio=0.1),
    # mask_level alone (with drop_ratio 0.1 nothing is dropped, with 0.9 nearly everything that overlaps: only next to the default
    # drop_ratio does the overlap threshold decide a chain's fate)
    "mask.1": dict(mask_level=0.1),
    "mask.9": dict(mask_level=0.9),
    "combined": dict(w=2, max_chain_gap=40, min_chain_weight=30, max_chain_extend=3, mask_level=0.3, drop_ratio=0.8),
}

LANE = ("lane16x4", "lane64x9", "lane255x9")             # chain_kernel<16, 4>, <64, 9>, <255, 9>
HEAVY = ("heavy256", "heavy1024", "heavy2048", "heavy4096")   # chain_heavy_kernel<256 / 1024 / 2048 / 4096>
CLASSES = LANE + HEAVY
LANE_FLOOR, HEAVY_FLOOR, FAMILY_FLOOR = 10, 4, 5
# (option set, class) pairs on which the option cannot change the outcome of these reads: a lane's read has at most 9 chains, fewer
# than max_chain_extend = 40; under mask_level 0.1 / drop_ratio 0.9 the many-seed reads of <255, 9> end as under the defaults
NO_FLOOR = {("extend40", k) for k in LANE} | {("mask.1_drop.9", "lane255x9")} | {("default", k) for k in CLASSES}
# min_seed_len only moves the `w_j - w_i >= min_seed_len << 1` test of the filter: a floor per kernel family
FAMILY_SETS = ("seedlen10", "seedlen30")
# the sets that change test_and_merge's condition.  No floor on merges for max_chain_gap = 100 in <255, 9>: a gap of 100 between two
# consecutive seeds of a chain leaves 51 bases of a read of 151 for the seeds, too few for 65 seeds on at most 9 chains
MERGE_SETS = ("gap40", "gap100", "w0", "w2", "w130")
NO_MERGE_FLOOR = {("gap100", "lane255x9")}


def launch_class(n_seeds, n_chains_before_filter):
    """launch_chain's rule (chain_kernel.hip): the first lane-per-read launch whose seed and chain bounds hold the read, else the
    wavefront-per-read class by seed count; None: the host.  The chain count is the one mem_chain ends with: chains are only added."""
    for name, s_hi, c_hi in (("lane16x4", 16, 4), ("lane64x9", 64, 9), ("lane255x9", 255, 9)):
        if n_seeds <= s_hi and n_chains_before_filter <= c_hi:
            return name
    for name, s_hi in (("heavy256", 255), ("heavy1024", 1024), ("heavy2048", 2048), ("heavy4096", 4096)):
        if n_seeds <= s_hi:
            return name
    return None


def floor(set_name, klass):
    if (set_name, klass) in NO_FLOOR or set_name in FAMILY_SETS:
        return 0
    return LANE_FLOOR if klass in LANE else HEAVY_FLOOR


class Geometry:
    """the contigs of an index as the generators need them"""

    def __init__(self, bns):
        self.l_pac = int(bns.contents.l_pac)
        self.n_seqs = int(bns.contents.n_seqs)
        self.offs = [int(bns.contents.anns[k].offset) for k in range(self.n_seqs)] + [self.l_pac]
        self.alt = [int(bns.contents.anns[k].is_alt) != 0 for k in range(self.n_seqs)]

    def slots(self, step, contigs=None, room=LQ):
        """ascending positions `step` apart on both strands of the contigs, 500 bases and `room` clear of contig ends and of the strand
        boundary"""
        spans = []
        for k in (range(self.n_seqs) if contigs is None else contigs):
            lo, hi = self.offs[k], self.offs[k + 1]
            spans.append((lo + 500, hi - 500 - room))
            spans.append((2 * self.l_pac - hi + 500, 2 * self.l_pac - lo - 500 - room))
        spans.sort()
        return [p for lo, hi in spans for p in range(lo, hi, step)]


# ---- the lane-per-read launches: a few chains of many seeds ----
FEW_ROOM = LQ + 230 + 400     # a read's hits lie within LQ + 223 of their anchor


def few_chains_many_seeds(rng, slots, n_seeds, n_anchor=None, n_light=None, windows=0.3):
    """One read of lo <= seeds <= hi on 2-5 anchors and 0-3 light anchors taken from `slots` (400 apart).  Every interval (qb, qb + len),
    len 19-60, puts a hit on each anchor with probability 0.8, at anchor + qb + off(anchor, qb); off is non-decreasing in qb (0-3
    breakpoints per anchor, each adds 1, 2 or 3 — small indels, merged while w allows; one in four anchors has one of 120, merged
    only under w = 130, one in four one of 60 or 100, merged under the default w unless max_chain_gap forbids the step on the
    reference), so a later seed is never left of an earlier one, and an anchor takes one hit per qb: all positions differ.
    One read in four has a hole in its query, 45-60 bases without a seed (101-106 in some reads of up to 64 seeds): the chains go on
    across it unless max_chain_gap is smaller.  In three reads in ten (`windows`) every anchor takes seeds from a window of 40-110
    bases of the query only: chains that overlap by any fraction of the shorter one, on either side of every mask_level.
    A light anchor has one or two seeds of 19-25 bases that cover less than 30 together: min_chain_weight = 30 drops its chain.
    -> (lq, [(qb, qe, hits)])"""
    lo, hi = n_seeds
    target = int(rng.integers(lo, hi + 1))
    n_anchor = int(rng.integers(2, 6)) if n_anchor is None else n_anchor
    n_light = int(rng.integers(0, 4)) if n_light is None else n_light
    pick = [slots[i] for i in rng.choice(len(slots), n_anchor + n_light, replace=False)]
    anchors, lights = pick[:n_anchor], pick[n_anchor:]
    brk = []
    for _ in anchors:
        nb = int(rng.integers(0, 4))
        pts = sorted(int(x) for x in rng.integers(1, LQ - 19, nb))
        adds = [int(rng.choice([1, 2, 3])) for _ in pts]
        if nb and rng.random() < 0.25:
            adds[int(rng.integers(nb))] = 120
        if nb and rng.random() < 0.25:
            adds[int(rng.integers(nb))] = int(rng.choice([60, 100]))
        brk.append(list(zip(pts, adds)))
    hole, win = None, [(0, LQ)] * n_anchor
    shape = rng.random() if anchors else 1.0
    if 0.25 <= shape < 0.25 + windows:
        cand = []
        for _ in anchors:
            width = int(rng.integers(40, 111))
            a0 = int(rng.integers(0, LQ - width + 1))
            cand.append((a0, a0 + width))
        n_qb = sum(a1 - a0 - 18 for a0, a1 in cand)
        if n_qb // 2 >= lo:
            win, target = cand, min(target, n_qb // 2)
    if shape < 0.25:
        width = int(rng.integers(101, 107)) if hi <= 64 and rng.random() < 0.4 else int(rng.integers(45, 61))
        h0 = int(rng.integers(22, LQ - 22 - width + 1))
        n_qb = (h0 - 18) + (LQ - 18 - h0 - width)           # query starts that leave room for a seed of 19 on either side
        if n_qb * n_anchor * 6 // 10 >= lo:
            hole, target = (h0, h0 + width), min(target, n_qb * n_anchor * 6 // 10)
    ivs, used, n = {}, set(), 0
    for p in lights:
        q = int(rng.integers(0, LQ - 30))
        ivs.setdefault((q, q + int(rng.integers(19, 26))), []).append(p + q)
        n += 1
        if rng.random() < 0.5 and n < hi:
            d = int(rng.integers(1, 4))
            ivs.setdefault((q + d, q + d + int(rng.integers(19, 26))), []).append(p + q + d)
            n += 1
    for _ in range(20000):
        if n >= target or not anchors:
            break
        qb = int(rng.integers(0, LQ - 19))
        ln = int(rng.integers(19, min(LQ - qb, 60) + 1))
        if (qb, qb + ln) in ivs or (hole and qb < hole[1] and qb + ln > hole[0]):
            continue
        hits = []
        for a, p in enumerate(anchors):
            if n + len(hits) < hi and (a, qb) not in used and win[a][0] <= qb and qb + ln <= win[a][1] and rng.random() < 0.8:
                used.add((a, qb))
                hits.append(p + qb + sum(d for at, d in brk[a] if qb >= at))
        if hits:
            ivs[(qb, qb + ln)] = [hits[i] for i in rng.permutation(len(hits))]
            n += len(hits)
    assert lo <= n <= hi or not anchors, (n, n_seeds, hole)
    return LQ, [(qb, qe, h) for (qb, qe), h in ivs.items()]


# ---- the wavefront-per-read classes: many chains, most of two seeds ----
PAIR_KINDS = 12
PAIR_OFF = (0, 2, 50, 130)     # the second seed's distance from the first one's diagonal, by kind % 4
FLAT_OFF = 300                 # ... in a flat read: beyond every w of OPTION_SETS, the second seed is a chain of its own


def paired_seed_read(rng, step, slots, n_slots, flavour="paired", second_on=None):
    """One read of n_slots first seeds at distinct slots (as test_gpu_chain_heavy_classes.single_seed_read: at least 8 groups, group g
    has the interval (g, g + len_g) with distinct len_g in 25-60, at most MAX_HITS hits each, positions shuffled; a first seed never
    merges into another slot's chain while step - groups > w), three in four with a second seed of one of 12 kinds: kind k is the
    interval (75 + k, 95 + 3 k) and lies PAIR_OFF[k % 4] off the first seed's diagonal, so whether it merges depends on w (through that
    distance) and on max_chain_gap (through 75 + k - g - len_g).  The intervals are visited in (qbeg, qend) order: every first seed
    before any second one.
    flat: len_g in 25-62 with one in 25-29 and one in 58-62, and no second seed merges (FLAT_OFF; step 400 only): no chain weighs more
    than 62, so the chains of 25-29 are lighter than half the heaviest by 29-37, on either side of `w_j - w_i >= min_seed_len << 1`
    for min_seed_len 10 and 19 (in the other reads a chain of two seeds, 65 or more heavier, drops them whatever min_seed_len is).
    offset: len_g in 25-45, under 30 in the first two and the last two groups, and the last two begin at 13 and 14; kind k is the
    interval (15 + 2 k, 75 + 4 k) and never merges (FLAT_OFF; step 400 only): chains of 60-82 that begin at 15-37, inside the first
    seeds' chains (which end at 25-55) by anything from nothing to nearly all of them.  The light chains of the first groups lie under
    them by less than half, those of the last groups by more: whether the heavier chain drops the lighter one is decided by mask_level,
    nowhere else (in the other reads every light chain lies inside a heavier one altogether).
    second_on: the slots that may get a second seed (default: all).
    -> (lq, [(qb, qe, hits)])"""
    flat = flavour != "paired"
    pick = [slots[i] for i in rng.choice(len(slots), n_slots, replace=False)]
    n_groups = max((n_slots + MAX_HITS - 1) // MAX_HITS, 8)
    assert n_groups <= 11 and step - n_groups > 130 and (not flat or step >= 400), (n_slots, step, n_groups)
    if flavour == "offset":
        short = [int(v) for v in rng.choice(np.arange(25, 30), 4, replace=False)]
        lens = short[:2] + [int(v) for v in rng.choice(np.arange(30, 46), n_groups - 4, replace=False)] + short[2:]
    elif flat:
        lens = [int(rng.integers(25, 30)), int(rng.integers(58, 63))]
        lens += [int(v) for v in rng.choice(np.arange(30, 58), n_groups - 2, replace=False)]
        lens = [lens[i] for i in rng.permutation(n_groups)]
    else:
        lens = [int(v) for v in rng.choice(np.arange(25, 61), n_groups, replace=False)]
    kind = (lambda k: (15 + 2 * k, 75 + 4 * k)) if flavour == "offset" else (lambda k: (75 + k, 95 + 3 * k))
    q0 = list(range(n_groups))       # where a group's interval begins
    if flavour == "offset":
        q0[-2:] = [13, 14]
    ivs, second, at = [], {}, 0
    for g in range(n_groups):
        m = n_slots // n_groups + (1 if g < n_slots % n_groups else 0)
        assert 0 < m <= MAX_HITS
        ivs.append((q0[g], q0[g] + lens[g], pick[at:at + m]))
        for p in pick[at:at + m]:
            if rng.random() < 0.75 and (second_on is None or p in second_on):
                k = int(rng.integers(PAIR_KINDS))
                second.setdefault(k, []).append(p + kind(k)[0] - q0[g] + (FLAT_OFF if flat else PAIR_OFF[k % 4]))
        at += m
    for k, hits in sorted(second.items()):
        assert len(hits) <= MAX_HITS
        ivs.append(kind(k) + (hits,))
    return LQ, ivs


def light_chains_read(rng, slots, n_light):
    """n_light > 9 light anchors and nothing else: a read of chain_heavy_kernel<256> that min_chain_weight >= 30 leaves without a chain"""
    return few_chains_many_seeds(rng, slots, (n_light, 2 * n_light), n_anchor=0, n_light=n_light)


# reads per family of the set every option is run on
N_FEW = ((5, 16, 260), (17, 64, 150), (65, 255, 220))     # (seeds from, to, reads)
N_NARROW = 220                                             # reads of 5-16 seeds on 2-3 anchors: chain_kernel<16, 4>
N_MANY = 40                                                # reads of 12-90 anchors, up to 255 seeds: chain_heavy_kernel<256>
N_LIGHT_ONLY = 12                                          # reads of 2-4 light anchors
N_LIGHT_HEAVY = 6                                          # reads of 12-40 light anchors
N_PAIRED = ((150, 170, 8), (600, 700, 7), (1100, 1200, 7), (1500, 1700, 6))   # (slots from, to, reads): 257-300, ~1 100, ~2 000, ~2 800 seeds
N_FLAT = ((150, 170, 5), (600, 700, 3), (1500, 1650, 3))
N_OFFSET = ((150, 170, 8), (600, 700, 5), (1100, 1200, 4), (1500, 1650, 6))
CASE_SEED = 4101


def option_cases(geo, seed=CASE_SEED):
    """The reads every option set is run on -> [(family, (lq, [(qb, qe, hits)]))]"""
    rng = np.random.default_rng(seed)
    few = geo.slots(400, room=FEW_ROOM)
    grid = geo.slots(400)
    cases = []
    for lo, hi, n in N_FEW:
        cases += [("few%d" % hi, few_chains_many_seeds(rng, few, (lo, hi), windows=0.3 if hi < 255 else 0.6)) for _ in range(n)]
    for _ in range(N_NARROW):
        cases.append(("narrow", few_chains_many_seeds(rng, few, (5, 16), n_anchor=int(rng.integers(2, 4)), n_light=int(rng.integers(0, 2)))))
    for _ in range(N_MANY):
        na = int(rng.integers(12, 91))
        cases.append(("many", few_chains_many_seeds(rng, few, (min(3 * na, 250), 255), n_anchor=na, n_light=int(rng.integers(0, 4)), windows=0.6)))
    cases += [("light", few_chains_many_seeds(rng, few, (2, 8), n_anchor=0, n_light=int(rng.integers(2, 5)))) for _ in range(N_LIGHT_ONLY)]
    cases += [("light_heavy", light_chains_read(rng, few, int(rng.integers(12, 41)))) for _ in range(N_LIGHT_HEAVY)]
    for lo, hi, n in N_PAIRED:
        cases += [("paired", paired_seed_read(rng, 400, grid, int(rng.integers(lo, hi + 1)))) for _ in range(n)]
    for lo, hi, n in N_FLAT:
        cases += [("flat", paired_seed_read(rng, 400, grid, int(rng.integers(lo, hi + 1)), "flat")) for _ in range(n)]
    for lo, hi, n in N_OFFSET:
        cases += [("offset", paired_seed_read(rng, 400, grid, int(rng.integers(lo, hi + 1)), "offset")) for _ in range(n)]
    return cases


def alt_cases(geo, seed=CASE_SEED + 1):
    """Reads on an index with ALT contigs, about half of them with half of their anchors / slots on the ALT contigs (whose slots are
    172 apart where a read needs more of them than lie 400 apart); in every other such heavy read only the ALT slots get a second seed,
    so that a light primary chain has nothing heavier above it than ALT chains: it is kept only because `!ALT(j) || ALT(i)` is false
    -> [(family, case)]"""
    rng = np.random.default_rng(seed)
    alt = [k for k in range(geo.n_seqs) if geo.alt[k]]
    pri = [k for k in range(geo.n_seqs) if not geo.alt[k]]
    assert alt and pri
    few_alt, few_pri = geo.slots(400, alt, room=FEW_ROOM), geo.slots(400, pri, room=FEW_ROOM)
    cases = []

    def mixed(a, p, n):   # n slots, half of them from a
        na = min(n // 2, len(a))
        return sorted([a[i] for i in rng.choice(len(a), na, replace=False)] + [p[i] for i in rng.choice(len(p), n - na, replace=False)])

    for lo, hi, n in ((5, 16, 280), (17, 64, 200), (65, 255, 120)):
        for it in range(n):
            pool = mixed(few_alt, few_pri, 16) if it % 2 == 0 else few_pri
            cases.append(("few%d" % hi, few_chains_many_seeds(rng, pool, (lo, hi))))
    for lo, hi, n in ((150, 170, 24), (600, 700, 12)):
        for it in range(n):
            n_slots = int(rng.integers(lo, hi + 1))
            step = 400 if n_slots // 2 <= len(geo.slots(400, alt)) else 172
            a_slots = geo.slots(step, alt)
            pool = mixed(a_slots, geo.slots(step, pri), n_slots) if it % 2 == 0 else geo.slots(step, pri)
            cases.append(("paired", paired_seed_read(rng, step, pool, n_slots, second_on=set(a_slots) if it % 4 == 0 else None)))
    return cases


# ---- reads whose reference window is cut: every other read here lies 500 bases clear of contig ends and of the strand boundary ----
EDGE_FAMILIES = ("first_fwd", "first_rev", "last_fwd", "last_rev", "boundary_fwd", "boundary_rev")
EDGE_DIST = (0, 37, 90)       # bases between the read and the edge
EDGE_EXTRA = 12               # single-seed chains elsewhere that take a read to chain_heavy_kernel<256>


def edge_cases(geo, seed=CASE_SEED + 2):
    """Per family and distance of EDGE_DIST two reads with ONE chain of two seeds, (10, 50) and (100, 140) on one diagonal, the read that
    far from the first or the last base of an inner contig (on either strand) or from l_pac (on either side of it): under the default
    options the seeds reach 95 and 96 bases beyond the read (cal_max_gap of the 100 and 101 bases before and behind them), so the window
    is cut at the contig's edge, in the boundary families also at the strand boundary.  The second read has EDGE_EXTRA chains of one
    seed of 25-36 bases elsewhere as well: more than 9 chains, a read of chain_heavy_kernel<256>.
    -> [(family, case)]"""
    rng = np.random.default_rng(seed)
    assert geo.n_seqs >= 3
    grid = geo.slots(400)
    l2 = 2 * geo.l_pac
    cases = []
    for fam in EDGE_FAMILIES:
        for d in EDGE_DIST:
            k = int(rng.integers(1, geo.n_seqs - 1))
            lo, hi = geo.offs[k], geo.offs[k + 1]
            at = {"first_fwd": lo + d, "last_fwd": hi - LQ - d, "first_rev": l2 - lo - LQ - d, "last_rev": l2 - hi + d,
                  "boundary_fwd": geo.l_pac - LQ - d, "boundary_rev": geo.l_pac + d}[fam]
            chain = [(10, 50, [at + 10]), (100, 140, [at + 100])]
            cases.append((fam, (LQ, chain)))
            lens = rng.choice(np.arange(25, 37), EDGE_EXTRA, replace=False)
            far = [grid[i] for i in rng.choice(len(grid), EDGE_EXTRA, replace=False)]
            cases.append((fam, (LQ, chain + [(1 + g, 1 + g + int(lens[g]), [far[g]]) for g in range(EDGE_EXTRA)])))
    return cases


# ---- the reference's answer ----
def kept_intervals(case, min_seed_len):
    """mem_collect_intv drops the intervals shorter than min_seed_len (src/bwamem.c:127): they are no seeds, for nobody"""
    lq, ivs = case
    return lq, [iv for iv in ivs if iv[1] - iv[0] >= min_seed_len]


def reference_chains(ref, ropt, cases):
    """chain_cases.reference_chains on the intervals that are seeds under ropt"""
    msl = int(ropt.contents.min_seed_len)
    return cc.reference_chains(ref, ropt, [kept_intervals(c, msl) for c in cases])


def chains_before_filter(ref, ropt, case):
    """mem_chain's chains as it leaves them, in position order -> [seeds of a chain]"""
    lq, ivs = kept_intervals(case, int(ropt.contents.min_seed_len))
    return [c[5] for c in po.ref_chains(ropt, ref.bns, lq, sorted(ivs, key=lambda t: (t[0] << 32) | t[1]), do_flt=False)]


class Evaluated:
    """a set of reads under one option set: what the stage is handed, the reference's chains, the launch class of every read"""

    def __init__(self, ref, kw, cases):
        ropt = ref.opt(**kw)
        self.kw = kw
        self.lens, self.seedsets, self.want = reference_chains(ref, ropt, cases)
        self.pre = [chains_before_filter(ref, ropt, c) for c in cases]
        self.klass = [launch_class(len(sd), len(pre)) for sd, pre in zip(self.seedsets, self.pre)]

    def count(self, flags=None):
        """reads per class (of those flagged)"""
        n = dict.fromkeys(CLASSES, 0)
        for k, c in enumerate(self.klass):
            if flags is None or flags[k]:
                n[c] += 1
        return n


def sensitive(ev, base):
    """per read: the reference's answer under ev's options is not its answer under base's (the defaults)"""
    return [a != b for a, b in zip(ev.want, base.want)]


def merge_sensitive(ev, base):
    """per read: mem_chain itself (test_and_merge: w, max_chain_gap) leaves other chains than under base's options"""
    return [a != b for a, b in zip(ev.pre, base.pre)]


_CACHE = {}


def evaluated(ref, prefix, name, cases_fn=option_cases, kw=None):
    """Evaluated(cases_fn(...), OPTION_SETS[name]) once per process, index and option set -> (cases, Evaluated)"""
    key = (prefix, cases_fn.__name__)
    if key not in _CACHE:
        _CACHE[key] = (cases_fn(Geometry(ref.bns)), {})
    cases, evs = _CACHE[key]
    if name not in evs:
        evs[name] = Evaluated(ref, OPTION_SETS[name] if kw is None else kw, [c for _, c in cases])
    return cases, evs[name]


def check_floors(name, ev, base):
    """the sensitive reads per class under one option set against the floors; -> (reads per class, sensitive per class)"""
    n_class, n_sens = ev.count(), ev.count(sensitive(ev, base))
    low = {k: n_sens[k] for k in CLASSES if n_sens[k] < floor(name, k)}
    assert not low, (name, "too few reads on which the option changes the reference's answer", low, n_sens)
    if name in FAMILY_SETS:
        assert sum(n_sens[k] for k in LANE) >= FAMILY_FLOOR and sum(n_sens[k] for k in HEAVY) >= FAMILY_FLOOR, (name, n_sens)
    if name in MERGE_SETS:   # max_chain_gap is also read by the mask test: the merges themselves must differ on enough reads
        n_merge = ev.count(merge_sensitive(ev, base))
        low = {k: n_merge[k] for k in CLASSES if n_merge[k] < floor(name, k) and (name, k) not in NO_MERGE_FLOOR}
        assert not low, (name, "too few reads on which the option changes what mem_chain merges", low, n_merge)
    return n_class, n_sens


# ---- ALT contigs in the mask test ----
def alt_nestings(chains, mask_level, max_chain_gap, drop_ratio=0.5, min_seed_len=19):
    """chains: po.ref_chains' output after the filter (the kept chains, heavier first) -> (a kept primary chain is overlapped on the query,
    beyond mask_level, by a heavier kept ALT chain: the pair `!ALT(j) || ALT(i)` takes out of the mask test; the same with a kept ALT
    chain under a heavier primary one; a pair of the first kind in which the ALT chain would have dropped the primary one, by
    drop_ratio and min_seed_len, had the mask test looked at it)"""
    if len(chains) < 2:
        return False, False, False
    beg = np.array([c[5][0][1] for c in chains])
    end = np.array([c[5][-1][1] + c[5][-1][2] for c in chains])
    w = np.array([c[1] for c in chains])
    alt = np.array([c[3] for c in chains]) != 0
    found = [False, False, False]
    for i in range(1, len(chains)):
        ov = np.minimum(end[:i], end[i]) - np.maximum(beg[:i], beg[i])
        min_l = np.minimum(end[:i] - beg[:i], end[i] - beg[i])
        sig = (ov > 0) & (ov.astype(np.float32) >= min_l.astype(np.float32) * np.float32(mask_level)) & (min_l < max_chain_gap) & (w[:i] > w[i])
        if not alt[i] and (sig & alt[:i]).any():
            found[0] = True
        if alt[i] and (sig & ~alt[:i]).any():
            found[1] = True
        drop = sig & alt[:i] & (np.float32(w[i]) < w[:i].astype(np.float32) * np.float32(drop_ratio)) & (w[:i] - w[i] >= min_seed_len << 1)
        if not alt[i] and drop.any():
            found[2] = True
        if all(found):
            break
    return tuple(found)


ALT_SETS = ("default", "combined")


def alt_coverage(ref, prefix, name):
    """alt_cases under OPTION_SETS[name] -> reads per kernel family with a primary chain under an ALT one, with the opposite nesting, and
    with a primary chain that owes its place to the ALT term, from the reference's own w, is_alt and seeds"""
    cases, ev = evaluated(ref, prefix, name, alt_cases)
    ropt = ref.opt(**OPTION_SETS[name])
    o = ropt.contents
    n = {"lane": [0, 0, 0], "heavy": [0, 0, 0], "reads": ev.count()}
    for (_, case), klass in zip(cases, ev.klass):
        lq, ivs = kept_intervals(case, int(o.min_seed_len))
        chains = po.ref_chains(ropt, ref.bns, lq, sorted(ivs, key=lambda t: (t[0] << 32) | t[1]))
        got = alt_nestings(chains, o.mask_level, o.max_chain_gap, o.drop_ratio, o.min_seed_len)
        fam = n["lane" if klass in LANE else "heavy"]
        for k in range(3):
            fam[k] += got[k]
    return n


def check_alt_coverage(name, n):
    """at least LANE_FLOOR / HEAVY_FLOOR reads of each of the three kinds of alt_coverage in the lanes' launches / in chain_heavy_kernel"""
    assert min(n["lane"]) >= LANE_FLOOR and min(n["heavy"]) >= HEAVY_FLOOR, (name, "too few reads with a chain under a heavier one of the other kind", n)
