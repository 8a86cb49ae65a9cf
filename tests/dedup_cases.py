"""Cases of the stage test of the redundancy pass on the device (dedup_kernel.hip through mi355x_dedup_batch): raw region lists as
mem_chain2aln could leave them, BEFORE mem_sort_dedup_patch, every family built to reach one branch of the pass
(tests/test_dedup_cases.py shows on the reference alone that it does).

A case is a dict: family, tag, regs (an oracle.pyoracle.ALNREG_DT array: the raw list), read (nt4 codes the spans of the list lie in),
expect ("taken", "maxreg", "patch", or None: only the invariant of the stage test applies).

  same_span  every region of a list has the same (qb, qe), so mem_patch_reg's co-linearity test fails by construction and no list
             reaches its alignment.  Hits sit at 1-5 loci with jitter 0, +-1, 3, 10, 60 in rb, reference spans that differ by 0, +-1, 2
             (many equal `re`), scores from a handful of values (many equal), both strands, two contigs, loci closer and farther apart
             than max_chain_gap (any of the option sets').  The regions of a locus overlap almost completely, so the redundancy scan
             removes most of them.  Exact (score, rb, qb) twins with different `re` that the scan can compare are removed by it as
             well (same rb and same span: always redundant); the SECOND removal, of adjacent equal elements after the second sort
             (src/bwamem.c:482-484), only fires for twins the scan cannot bring together.  Half of the lists carry such twins: two
             regions equal in (score, rb, qb) with a region of ANOTHER rid between them in `re` order, where the scan from the later
             twin stops (:451), or, in a list of two, twins that differ in rid.  No aligner produces such a list; the reference's code
             does not look at what a rid means, and neither may the kernel.  Which twin survives is the second sort's order of equal keys.
  far        regions that are never compared: another contig or strand, or farther apart than any max_chain_gap in use
  junction   hits on the last contig close to l_pac on both strands: the same rid and neighbouring doubled coordinates, where
             mem_patch_reg's first test (:411) is the one that says no
  patch      reads of two long pieces a deletion apart that is wider than the band (kind 0 of tests/test_host_pair.py), their regions
             from the reference's own mem_chain -> mem_chain_flt -> mem_flt_chained_seeds -> mem_chain2aln: two co-linear regions
             that mem_patch_reg joins.  expect = "patch" where the reference's results with and without the sequences differ
             (it merged), set by full_set()
  mixed      the clusters of same_span with a span of its own for every region: about half of these lists reach the patch tests
  random     the ends of pair_cases.adversarial_pairs, as in se_stage_cases.random_cases
  sorted_re, sorted_score   lists that arrive in the order that takes the first (by `re`) or the second sort (by score, rb, qb) out of
             its depth budget and into ks_introsort's comb sort, with equal keys whose order shows in the result (sorted_cases(), apart
             from build_cases(): no other family gets there)
"""
import ctypes as C

import numpy as np

from mpibwa_amd import abi
from oracle import pyoracle as po
from sam_stage_cases import Index   # noqa: F401  (re-exported for the tests)

FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep")
CAP = 512                  # DD_MAXREG; the stage test compares it with mi355x_dedup_maxreg()
SMALL = 8                  # PR_MAXREG: up to here a lane per read, above a wavefront per read
SAME_SPAN_SIZES = (2, 3, 8, 9, 16, 17, 18, 33, 63, 64, 65, 127, 128, 129, CAP - 1, CAP, CAP + 1)
MIXED_SIZES = (2, 3, 5, 8, 9, 12, 17, 40, 70, 130)
FAR_SIZES = (2, 3, 5, 8, 9, 12, 20)
MAX_GAP = 10000            # the largest max_chain_gap of the option sets
OPTION_SETS = {
    "default": dict(),
    "redun08_w40": dict(mask_level_redun=0.8, w=40),
    "gap300": dict(max_chain_gap=300),
}
LQ = 150


def _regs(rows):
    a = np.zeros(len(rows), dtype=po.ALNREG_DT)
    for j, (rb, re, qb, qe, rid, score) in enumerate(rows):
        a[j]["rb"], a[j]["re"], a[j]["qb"], a[j]["qe"], a[j]["rid"], a[j]["score"] = rb, re, qb, qe, rid, score
    a["truesc"] = a["score"]
    a["w"] = 100
    a["seedcov"] = (a["qe"] - a["qb"]) // 2
    a["seedlen0"] = 19
    a["secondary"] = a["secondary_all"] = -1
    return a


def _strand_range(ix, c, rev):
    """[lo, hi) of contig c on a strand, in the doubled coordinate"""
    if not rev:
        return ix.off[c], ix.off[c] + ix.len[c]
    return 2 * ix.l_pac - ix.off[c] - ix.len[c], 2 * ix.l_pac - ix.off[c]


def _loci(ix, rng, n_loci):
    """1-5 places (contig, start in the doubled coordinate): the first anywhere, the others next to it (closer than the smallest and
    than the largest max_chain_gap, farther than the largest), on its other strand or on another contig"""
    c0, rev0 = int(rng.integers(ix.n_seqs)), int(rng.integers(2))
    lo, hi = _strand_range(ix, c0, rev0)
    p0 = int(rng.integers(lo + 400, hi - 45000))
    loci = [(c0, p0)]
    steps = [170, 700, 2500, 15000, 31000]
    for k in range(1, n_loci):
        kind = int(rng.integers(4))
        if kind < 2:
            loci.append((c0, p0 + steps[int(rng.integers(len(steps)))] + 3 * k))
        elif kind == 2:
            l2, h2 = _strand_range(ix, c0, 1 - rev0)
            loci.append((c0, int(rng.integers(l2 + 400, h2 - 400 - LQ))))
        else:
            c1 = (c0 + 1 + int(rng.integers(ix.n_seqs - 1))) % ix.n_seqs
            l2, h2 = _strand_range(ix, c1, int(rng.integers(2)))
            loci.append((c1, int(rng.integers(l2 + 400, h2 - 400 - LQ))))
    return loci


def _cluster_rows(ix, rng, n, free_span, loci=None):
    if loci is None:
        loci = _loci(ix, rng, int(rng.integers(1, min(5, max(1, n // 2)) + 1)))
    qb0, qe0 = [(0, LQ), (5, 140), (30, 110), (0, 75)][int(rng.integers(4))]
    s0 = int(rng.choice([qe0 - qb0, qe0 - qb0 - 10, 60]))
    rows = []
    for j in range(n):
        c, p = loci[int(rng.integers(len(loci)))]
        if free_span:
            qb = int(rng.integers(0, 80))
            qe = int(rng.integers(qb + 25, LQ + 1))
            p += qb   # (roughly where that part of the read would lie)
        else:
            qb, qe = qb0, qe0
        rb = p + int(rng.choice([0, 0, 0, 1, -1, 3, 10, 60]))
        re = rb + (qe - qb) + int(rng.choice([0, 0, 0, 1, -1, 2]))
        score = max(19, min(s0, qe - qb) - int(rng.choice([0, 0, 0, 1, 5, 20])))
        rows.append((rb, re, qb, qe, c, score))
    return rows


def _with_twins(ix, rng, rows, n):
    """the last 3 (2 in a list of two) rows replaced by twins the scan cannot bring together -> rows, (rb, score) of the twins"""
    qb, qe, c = rows[0][2], rows[0][3], rows[0][4]
    other = (c + 1) % ix.n_seqs
    top = max(r[1] for r in rows[:max(1, n - 3)] if r[4] == c)
    t = top + int(rng.choice([40, 900, 20000]))
    sc = int(rng.choice([qe - qb, 50]))
    ln = qe - qb
    if n == 2:
        return [(t, t + ln, qb, qe, c, sc), (t, t + ln + int(rng.integers(0, 3)), qb, qe, other, sc)], (t, sc)
    return rows[:n - 3] + [(t, t + ln, qb, qe, c, sc), (t + 7, t + ln + 1, qb, qe, other, sc - 3), (t, t + ln + 2, qb, qe, c, sc)], (t, sc)


def _read(rng):
    return rng.integers(0, 4, LQ).astype(np.uint8)


def build_cases(ix, seed):
    """the synthetic families on one index (not shuffled; the same for every option set)"""
    rng = np.random.default_rng(seed)
    cases = []

    def add(family, tag, rows, expect, **kw):
        rows = [rows[i] for i in rng.permutation(len(rows))]
        cases.append(dict(family=family, tag=tag, regs=_regs(rows), read=_read(rng), expect=expect, **kw))

    for n in SAME_SPAN_SIZES:
        for rep in range(8 if n <= 18 else 4 if n < CAP - 1 else 2):
            rows, twins = _cluster_rows(ix, rng, n, False), None
            if rep % 2 == 1:
                rows, twins = _with_twins(ix, rng, rows, n)
            add("same_span", "n%d" % n, rows, "maxreg" if n > CAP else "taken", twins=twins)
    for n in MIXED_SIZES:
        for rep in range(12 if n <= 17 else 4):
            add("mixed", "n%d" % n, _cluster_rows(ix, rng, n, True), None)
    # far: one region per slot, the slots 12 000 apart on every contig and strand
    slots = []
    for c in range(ix.n_seqs):
        for rev in (0, 1):
            lo, hi = _strand_range(ix, c, rev)
            slots += [(c, lo + 1000 + 12000 * k) for k in range((hi - lo - 2000) // 12000)]
    for n in FAR_SIZES:
        for rep in range(4):
            rows = []
            for s in rng.choice(len(slots), n, replace=False):
                c, p = slots[int(s)]
                qb = int(rng.integers(0, 60))
                qe = int(rng.integers(qb + 30, LQ + 1))
                rows.append((p + int(rng.integers(0, 500)), 0, qb, qe, c, int(rng.integers(19, qe - qb + 1))))
            rows = [(rb, rb + qe - qb + int(rng.integers(-2, 3)), qb, qe, c, sc) for rb, _, qb, qe, c, sc in rows]
            add("far", "n%d" % n, rows, "taken")
    # junction: the end of the last contig on the forward strand and its beginning on the reverse strand meet at l_pac
    last = ix.n_seqs - 1
    for rep in range(60):
        n = int(rng.integers(2, 7))
        rows = []
        for j in range(n):
            qb = int(rng.integers(0, 70))
            qe = int(rng.integers(qb + 30, LQ + 1))
            ln = qe - qb
            near = int(rng.choice([0, 1, 5, 40, 250, 900]))
            if (j + rep) % 2:
                rb = ix.l_pac - ln - near                      # forward strand, ends `near` bases before l_pac
            else:
                rb = ix.l_pac + near                           # reverse strand, starts `near` bases behind it
            rows.append((rb, rb + ln, qb, qe, last, int(rng.choice([ln, ln - 4, 40]))))
        add("junction", "n%d" % n, rows, None)
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# The families of the comb sort.  ks_introsort falls back to a comb sort of the range in hand when its depth budget 2 * ceil(log2 n) is
# spent; an input that is already in order loses one element per partition and gets there from 26 elements on, shuffled or random
# lists practically never do (tests/test_introsort_model.py counts it).  These lists arrive in the order that spends the budget —
# they are NOT shuffled — and are built with the model of the sort (tests/introsort_model.py) in the loop.
# ---------------------------------------------------------------------------------------------------------------------
SORTED_SIZES = (25, 26, 27, 40, 64, 65, 130, 511, 512)
SORTED_SEED = 2606         # list number s of a family (0: sorted_re, 1: sorted_score) and size n is drawn from the seed (SORTED_SEED, family, n, s)
SORTED_PER_SIZE = 4
# found by find_sorted_seeds() on the index of the suite's `genome` fixture (three contigs of 120 000)
SORTED_SEEDS = {
    ("sorted_re", 25): [0, 1, 2, 3], ("sorted_re", 26): [8, 15, 23, 46], ("sorted_re", 27): [0, 32, 37, 43],
    ("sorted_re", 40): [0, 1, 19, 22], ("sorted_re", 64): [7, 12, 36, 46], ("sorted_re", 65): [4, 8, 14, 28],
    ("sorted_re", 130): [24, 36, 39, 43], ("sorted_re", 511): [303, 596, 634, 847], ("sorted_re", 512): [55, 536, 732, 979],
    ("sorted_score", 25): [0, 1, 2, 3], ("sorted_score", 26): [0, 1, 2, 3], ("sorted_score", 27): [0, 2, 4, 5],
    ("sorted_score", 40): [0, 1, 2, 3], ("sorted_score", 64): [0, 1, 2, 3], ("sorted_score", 65): [0, 1, 2, 3],
    ("sorted_score", 130): [0, 1, 2, 3], ("sorted_score", 511): [0, 1, 2, 3], ("sorted_score", 512): [0, 1, 2, 3],
}
_SORTED = {}               # the lists are built once per index geometry and left unchanged


def can_run_out_of_depth(n):
    """every partition takes at least one element off the range and ranges of 16 or fewer are left to the final insertion sort, so the
    budget of n elements can only be spent on a range of 17 or more from n = 26 on (25: a budget of 10, 16 left after 9 partitions)"""
    import introsort_model as im
    return n - (im.budget(n) - 1) >= 17


def model_pass(regs, max_chain_gap=MAX_GAP, mask_level_redun=0.95, comb=(True, True)):
    """mem_sort_dedup_patch (src/bwamem.c:437-489) without mem_patch_reg — for lists whose regions all have one query span, which its
    co-linearity test turns away — with the sorts of introsort_model, either with its fallback as comb[k] says
    -> dict(kept: raw places in final order, first / second: the Stats of the two sorts, sorted: the survivors after the second sort)"""
    import introsort_model as im
    rb, re, qb, qe, rid, sc = (regs[f].tolist() for f in ("rb", "re", "qb", "qe", "rid", "score"))
    n = len(rb)
    o = list(range(n))
    st1 = im.introsort(o, lambda x, y: re[x] < re[y], comb[0])
    alive = [qe[k] > qb[k] for k in range(n)]
    f, prod = np.float32(mask_level_redun), {}

    def over(x, m):   # x > mask_level_redun * m in the reference's types: the int64 m goes to float, the product is a float, x goes to float
        if m not in prod:
            prod[m] = float(f * np.float32(m))
        return float(np.float32(x)) > prod[m] if abs(x) >= 1 << 24 else x > prod[m]

    for i in range(1, n):
        p, j = o[i], i - 1
        while j >= 0 and rid[p] == rid[o[j]] and rb[p] < re[o[j]] + max_chain_gap:
            q = o[j]
            j -= 1
            if not alive[q]:
                continue
            orr = re[q] - rb[p]
            oq = qe[q] - qb[p] if qb[q] < qb[p] else qe[p] - qb[q]
            mr = min(re[q] - rb[q], re[p] - rb[p])
            mq = min(qe[q] - qb[q], qe[p] - qb[p])
            if over(orr, mr) and over(oq, mq):
                if sc[p] < sc[q]:
                    alive[p] = False
                    break
                alive[q] = False
    surv = [k for k in o if alive[k]]
    st2 = im.introsort(surv, lambda x, y: sc[x] > sc[y] or (sc[x] == sc[y] and (rb[x] < rb[y] or (rb[x] == rb[y] and qb[x] < qb[y]))), comb[1])
    kept = [k for i, k in enumerate(surv) if i == 0 or (sc[k], rb[k], qb[k]) != (sc[surv[i - 1]], rb[surv[i - 1]], qb[surv[i - 1]])]
    return dict(kept=kept, first=st1, second=st2, sorted=surv)


def kept_rows(regs, kept):
    return [tuple(int(regs[k][f]) for f in FIELDS) for k in kept]


def twin_order(sorted_places, twins):
    """per twin pair (a, b): does a stand before b?"""
    at = {k: i for i, k in enumerate(sorted_places)}
    return [at[a] < at[b] for a, b in twins]


def _sorted_re_rows(ix, rng, n):
    """first sort, by `re`: the least `re` first, a body of the same_span kind at one to three loci of one contig and strand, then
    2 * ceil(log2 n) regions with strictly ascending `re` farther along the contig than any max_chain_gap"""
    import introsort_model as im
    t = im.budget(n)
    c, rev = int(rng.integers(ix.n_seqs)), int(rng.integers(2))
    lo, hi = _strand_range(ix, c, rev)
    p0 = int(rng.integers(lo + 1000, hi - 60000))
    steps = [170, 700, 2500, 15000]
    loci = [(c, p0)] + [(c, p0 + steps[int(rng.integers(len(steps)))] + 3 * k) for k in range(1, int(rng.integers(1, 4)))]
    body = _cluster_rows(ix, rng, n - 1 - t, False, loci)
    qb, qe = body[0][2], body[0][3]
    scores = [r[5] for r in body]
    rows = [(p0 - 400, p0 - 400 + qe - qb, qb, qe, c, scores[int(rng.integers(len(scores)))])] + body
    p = max(r[1] for r in body) + MAX_GAP + 5000 + int(rng.integers(0, 5000))
    for k in range(t):
        p += int(rng.choice([3, 40, 400]))
        rows.append((p, p + qe - qb, qb, qe, c, scores[int(rng.integers(len(scores)))]))
    assert rows[-1][1] < hi - 400
    return rows


def _sorted_score_rows(ix, rng, n):
    """second sort, by score descending, then rb, then qb: regions nothing removes — one per slot, in ascending position, all with one
    query span (so mem_patch_reg's co-linearity test turns every pair away where the slots are closer than max_chain_gap: the slots
    of `far` are 12 000 apart, these as far as n of them fit, 800 or more) — with the highest score first, a body of scores from 2-6
    values, and 2 * ceil(log2 n) strictly descending scores below the body's at the end.  The keys are unique but for the twins: body
    regions followed by a copy equal in (score, rb, qb) under another rid and with a later `re`, which no scan reaches (it stops at
    the other rid) and the removal of adjacent equal elements takes one of.  -> rows, [(raw place of a twin, of its copy)]"""
    import introsort_model as im
    t = im.budget(n)
    n_tw = max(2, n // 10)
    base = n - n_tw
    spans = sorted(_strand_range(ix, c, rev) + (c,) for c in range(ix.n_seqs) for rev in (0, 1))
    step = min(12000, sum(hi - lo - 2000 - LQ for lo, hi, c in spans) // (base + len(spans)))
    assert step >= 1200
    slots = [(c, p) for lo, hi, c in spans for p in range(lo + 1000, hi - 1000 - LQ - step // 3, step)]
    assert len(slots) >= base
    qb, qe = [(0, LQ), (5, 140), (30, 110), (0, 75)][int(rng.integers(4))]
    ln = qe - qb
    top = int(rng.integers(18 + t, min(ln - 8, 30 + t) + 1))
    tail = sorted((int(v) for v in rng.choice(np.arange(19, top + 1), t, replace=False)), reverse=True)
    vals = rng.choice(np.arange(top + 1, ln), int(rng.integers(2, 7)), replace=False)
    score = [ln] + [int(v) for v in rng.choice(vals, base - 1 - t)] + tail
    twin_at = set(int(k) for k in rng.choice(np.arange(1, base - t), n_tw, replace=False))
    rows, twins = [], []
    for j, s in enumerate(np.sort(rng.choice(len(slots), base, replace=False))):
        c, p = slots[int(s)]
        rb = p + int(rng.integers(0, step // 3))
        rows.append((rb, rb + ln + int(rng.integers(-2, 3)), qb, qe, c, score[j]))
        if j in twin_at:
            twins.append((len(rows) - 1, len(rows)))
            rows.append((rb, rows[-1][1] + 1 + int(rng.integers(0, 2)), qb, qe, (c + 1) % ix.n_seqs, score[j]))
    return rows, twins


def sorted_list(ix, family, n, s):
    """list number s of a family and size -> a case, or None where the model turns it down: from 26 regions on a list counts only if
    the sort it is built for hands a range of at least 17 to the comb sort, which swaps, and an insertion sort in the comb sort's
    place would have changed the result — for sorted_re the regions the pass keeps, for sorted_score the relative order of a twin
    pair.  Lists of 25 cannot spend the budget (can_run_out_of_depth): they are the edge and all count."""
    k = ("sorted_re", "sorted_score").index(family)
    rng = np.random.default_rng((SORTED_SEED, k, n, s))
    rows, twins = (_sorted_re_rows(ix, rng, n), None) if k == 0 else _sorted_score_rows(ix, rng, n)
    regs = _regs(rows)
    if can_run_out_of_depth(n):
        real = model_pass(regs)
        st = real["second" if k else "first"]
        if st.widest < 17 or not st.comb_swaps:
            return None
        mut = model_pass(regs, comb=(k == 1, k == 0))
        if k == 0 and kept_rows(regs, mut["kept"]) == kept_rows(regs, real["kept"]):
            return None
        if k == 1 and (len(real["sorted"]) != n or twin_order(mut["sorted"], twins) == twin_order(real["sorted"], twins)):
            return None
    return dict(family=family, tag="n%d" % n, regs=regs, read=_read(rng), expect="taken", twins=twins)


def find_sorted_seeds(ix, per_size=SORTED_PER_SIZE):
    """the generation rule: per family and size the first per_size list numbers the model lets through -> what SORTED_SEEDS states"""
    import itertools
    found = {}
    for family in ("sorted_re", "sorted_score"):
        for n in SORTED_SIZES:
            ok = (s for s in itertools.count() if sorted_list(ix, family, n, s) is not None)
            found[family, n] = list(itertools.islice(ok, per_size))
    return found


def sorted_cases(ix):
    """sorted_re and sorted_score: the lists SORTED_SEEDS names, SORTED_PER_SIZE per size and family, in the order of their
    construction.  A list the model turns down on this index is an error, not a list left out."""
    key = (tuple(ix.off), tuple(ix.len))
    if key not in _SORTED:
        cases = []
        for n in SORTED_SIZES:
            for family in ("sorted_re", "sorted_score"):
                assert len(SORTED_SEEDS[family, n]) == SORTED_PER_SIZE
                for s in SORTED_SEEDS[family, n]:
                    cs = sorted_list(ix, family, n, s)
                    assert cs is not None, (family, n, s, "the model turns this list down")
                    cases.append(cs)
        _SORTED[key] = cases
    return _SORTED[key]


def random_cases(ix, n_pairs, seed):
    """the ends of pair_cases.adversarial_pairs, each as one raw list"""
    from pair_cases import adversarial_pairs
    rng = np.random.default_rng(seed)
    offs = np.array(ix.off + [ix.l_pac])
    out = []
    for ends in adversarial_pairs(rng, n_pairs, ix.l_pac, offs):
        for e in range(2):
            out.append(dict(family="random", tag="r", regs=np.array(ends[e], dtype=po.ALNREG_DT), read=_read(rng), expect=None))
    return out


def patch_cases(ref, ropt, seqs, n_reads, seed):
    """kind 0 of tests/test_host_pair.py:207-211 on the genome `seqs`: two pieces a deletion wider than the band apart; the raw regions
    are the reference's own (mem_chain -> mem_chain_flt -> mem_flt_chained_seeds -> mem_chain2aln)"""
    from c2a_cases import CHAIN_T_BYTES, _alnreg_v, _chain_v, _ref_handle, _regs_copy
    R = _ref_handle()
    P_opt, P_bwt, P_bns, P_u8 = C.POINTER(abi.mem_opt_t), C.POINTER(abi.bwt_t), C.POINTER(abi.bntseq_t), C.POINTER(C.c_uint8)
    R.mem_chain.restype = _chain_v
    R.mem_chain.argtypes = [P_opt, P_bwt, P_bns, C.c_int, C.c_char_p, C.c_void_p]
    R.mem_chain_flt.restype = C.c_int
    R.mem_chain_flt.argtypes = [P_opt, C.c_int, C.c_void_p]
    R.mem_flt_chained_seeds.restype = None
    R.mem_flt_chained_seeds.argtypes = [P_opt, P_bns, P_u8, C.c_int, C.c_char_p, C.c_int, C.c_void_p]
    R.mem_chain2aln.restype = None
    R.mem_chain2aln.argtypes = [P_opt, P_bns, P_u8, C.c_int, C.c_char_p, C.c_void_p, C.POINTER(_alnreg_v)]
    rng = np.random.default_rng(seed)
    comp = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
    w_opt = int(ropt.contents.w)
    out = []
    for r in range(n_reads):
        c = int(rng.integers(0, len(seqs)))
        gap = w_opt + 1 + int(rng.integers(0, w_opt // 2))
        ln = int(gap * (11 + 3 * rng.random()))
        pos = int(rng.integers(0, len(seqs[c]) - 2 * ln - gap - 10))
        read = np.concatenate([seqs[c][pos:pos + ln], seqs[c][pos + ln + gap:pos + 2 * ln + gap]])
        read = np.where(read > 3, 0, read).astype(np.uint8)
        m = rng.random(len(read)) < 0.003
        read[m] = (read[m] + 1) & 3
        if rng.random() < 0.5:
            read = comp[read[::-1]]
        buf = C.create_string_buffer(read.tobytes(), len(read) + 1)   # nt4 codes, as mem_align1_core makes them (src/bwamem.c:1057-1058)
        chn = R.mem_chain(ropt, ref.bwt, ref.bns, len(read), buf, None)
        chn.n = R.mem_chain_flt(ropt, chn.n, chn.a)
        R.mem_flt_chained_seeds(ropt, ref.bns, ref.pac, len(read), buf, chn.n, chn.a)
        regs = _alnreg_v()
        for i in range(chn.n):
            R.mem_chain2aln(ropt, ref.bns, ref.pac, len(read), buf, chn.a + i * CHAIN_T_BYTES, C.byref(regs))
        raw = _regs_copy(regs)
        if regs.a:
            po.libc.free(C.c_void_p(regs.a))
        out.append(dict(family="patch", tag="g%d" % gap, regs=raw, read=np.ascontiguousarray(read), expect=None))
    return out


def shuffled(cases, seed):
    rng = np.random.default_rng(seed)
    return [cases[i] for i in rng.permutation(len(cases))]


def reference_results(ref, ropt, cases, with_seq=True):
    """per case: the reference's list after mem_sort_dedup_patch (ALNREG_DT), called as tests/se_stage_cases.py calls it — with the
    sequences, or with bns = pac = query = 0, where mem_patch_reg returns at once and nothing is merged"""
    R = ref.lib
    P = C.POINTER
    R.mem_sort_dedup_patch.restype = C.c_int
    R.mem_sort_dedup_patch.argtypes = [P(abi.mem_opt_t), P(abi.bntseq_t), P(C.c_uint8), C.c_void_p, C.c_int, C.c_void_p]
    out = []
    for cs in cases:
        a = np.array(cs["regs"], dtype=po.ALNREG_DT, copy=True)
        sq = np.array(cs["read"], dtype=np.uint8, copy=True)   # (mem_patch_reg's alignment may reverse the query in place and back)
        if len(a):
            n = R.mem_sort_dedup_patch(ropt, ref.bns if with_seq else None, ref.pac if with_seq else None, sq.ctypes.data if with_seq else None,
                                       len(a), a.ctypes.data)
        else:
            n = 0
        out.append(a[:n].copy())
    return out


def same_lists(x, y):
    return len(x) == len(y) and all((x[f] == y[f]).all() for f in FIELDS)


def full_set(ref, ropt, ix, seqs, seed=5, n_random=1500, n_patch=60):
    """everything the stage test runs under one option set -> (cases in launch order, the reference's results with the sequences);
    expect = "patch" is set on the reads of the `patch` family the reference merged"""
    cases = shuffled(build_cases(ix, seed) + patch_cases(ref, ropt, seqs, n_patch, seed + 1), seed + 2) + random_cases(ix, n_random, seed + 3)
    want = reference_results(ref, ropt, cases, True)
    bare = reference_results(ref, ropt, [cs for cs in cases if cs["family"] == "patch"], False)
    k = 0
    for cs, w in zip(cases, want):
        if cs["family"] == "patch":
            cs["merged"] = not same_lists(w, bare[k])
            if cs["merged"]:
                cs["expect"] = "patch"
            k += 1
    return cases, want
