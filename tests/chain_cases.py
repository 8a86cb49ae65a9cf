"""Adversarial seed sets for the chaining stage and what the reference's own mem_chain + mem_chain_flt make of them
(oracle/chain_inject.c).  Shared by the CPU test of the library's host chaining and the GPU test of chain_kernel."""
import numpy as np

from oracle import pyoracle as po


def adversarial_interval_sets(rng, n_cases, l_pac, offs, n_seqs):
    """Seed sets as mem_chain sees them: intervals with distinct (qbeg, qend), each with its suffix-array hits."""
    cases = []
    for it in range(n_cases):
        lq = int(rng.choice([100, 150, 151, 250]))
        mode = rng.random()
        n_anchor = int(rng.integers(1, 4)) if mode < 0.6 else int(rng.integers(3, 14))
        if mode > 0.96:
            n_anchor = int(rng.integers(15, 90))            # dozens of chains: the ordered map grows past one node, then past two levels
        anchors = []
        for _ in range(n_anchor):
            k = int(rng.integers(0, n_seqs))
            p = int(rng.integers(offs[k], max(offs[k] + 1, offs[k + 1] - lq - 1)))
            if rng.random() < 0.5:
                p = max(2 * l_pac - 1 - p - lq, l_pac)      # reverse strand
            anchors.append(p)
        if rng.random() < 0.15 and len(anchors) > 1:
            anchors[1] = anchors[0]                          # two chains anchored at the same position
        if rng.random() < 0.05 and n_seqs > 1:
            anchors[0] = offs[int(rng.integers(1, n_seqs))] - 10   # seeds bridging two contigs
        n_iv = int(rng.integers(1, 16)) if mode < 0.9 else int(rng.integers(30, 50))
        if mode > 0.96:
            n_iv = int(rng.integers(60, 110))
        ivs = {}
        for _ in range(n_iv):
            qb = int(rng.integers(0, lq - 19))
            ln = int(rng.integers(19, min(lq - qb, 80) + 1))
            hits = []
            for _ in range(int(rng.choice([1, 1, 1, 2, 3]))):
                a = anchors[int(rng.integers(0, len(anchors)))]
                shift = int(rng.choice([0, 0, 0, 1, -1, 3, 120, 20000]))
                hits.append(min(max(a + qb + shift, 0), 2 * l_pac - ln - 1))
            ivs[(qb, qb + ln)] = hits
        if rng.random() < 0.3 and mode <= 0.96:              # equal weights: disjoint seeds of the same length
            ivs = {((30 * j) % (lq - 25), (30 * j) % (lq - 25) + 25): [min(max(anchors[j % len(anchors)] + 30 * j + (0 if j % 2 else 7), 0), 2 * l_pac - 26)]
                   for j in range(int(rng.integers(3, 9)))}
        cases.append((lq, [(qb, qe, h) for (qb, qe), h in ivs.items()]))
    return cases




def repeat_like_interval_sets(rng, n_cases, l_pac, offs, n_seqs, n_copies=(100, 400), n_ivs=(2, 4)):
    """Reads of a high-copy repeat: two or three intervals with 100 to 400 hits each at unrelated positions, so mem_chain_flt
    sees hundreds of chains of (nearly) equal weight that overlap completely on the query and mostly all survive — the quadratic
    case of its kept-list scan."""
    cases = []
    for it in range(n_cases):
        lq = int(rng.choice([100, 150, 250]))
        n_copy = int(rng.integers(n_copies[0], n_copies[1]))
        copies = []
        for _ in range(n_copy):
            k = int(rng.integers(0, n_seqs))
            p = int(rng.integers(offs[k], max(offs[k] + 1, offs[k + 1] - lq - 1)))
            if rng.random() < 0.5:
                p = max(2 * l_pac - 1 - p - lq, l_pac)
            copies.append(p)
        ivs = {}
        for j in range(int(rng.integers(n_ivs[0], n_ivs[1]))):
            qb = int(rng.integers(0, lq - 40))
            ln = int(rng.integers(19, min(lq - qb, 60) + 1))
            # most copies carry the interval at its place, some a little off (a gap in the copy), some not at all
            hits = sorted(min(max(c + qb + int(rng.choice([0, 0, 0, 0, 2, -3])), 0), 2 * l_pac - ln - 1) for c in copies if rng.random() < 0.9)
            ivs[(qb, qb + ln)] = hits
        cases.append((lq, [(qb, qe, h) for (qb, qe), h in ivs.items()]))
    return cases


SORTED_TAIL_SIZES = (25, 26, 27, 40, 64, 130, 255, 300, 700, 1100, 2000)
SORTED_TAIL_SEED = 2605     # the families of the comb sort are generated under this seed
SORTED_TAIL_LQ = 151


def sorted_tail_weights(rng, n):
    """n weights of single-seed chains (seed lengths 76 ... 150: all within the default drop_ratio of one another) that take
    mem_chain_flt's sort (heavier first) out of its depth budget: the heaviest first, a body from 2-6 values in random order, then
    2 * ceil(log2 n) strictly lighter and lighter ones below the body.  Every partition of the quicksort takes the range's last
    element for its pivot and splits off nothing else, so the range that is left when the budget is spent goes to the comb sort.
    Drawn again until the model (tests/introsort_model.py) says so, for a range of at least 17, and says that an insertion sort in
    the comb sort's place would have left another order."""
    import introsort_model as im
    t = im.budget(n)
    heavier = lambda x, y: x > y
    while True:
        top = int(rng.integers(75 + t, 121))
        tail = sorted((int(v) for v in rng.choice(np.arange(76, top + 1), t, replace=False)), reverse=True)
        vals = rng.choice(np.arange(top + 1, 150), int(rng.integers(2, 7)), replace=False)
        w = [150] + [int(v) for v in rng.choice(vals, n - 1 - t)] + tail
        if n - (t - 1) < 17:     # 25 chains: 16 are left when the budget is down to its last partition, and the final insertion sort takes them
            return w
        o, st = im.sort_keys(w, heavier)
        if st.widest >= 17 and st.comb_swaps and im.sort_keys(w, heavier, comb=False)[0] != o:
            return w


def sorted_tail_chain_sets(rng, sizes, l_pac, offs, n_seqs, max_hits=400):
    """Reads whose chains reach mem_chain_flt's sort in an order that ends in its comb sort (sorted_tail_weights): n single-seed chains
    per read, so a chain's weight is its seed's length and its place among the chains is its position's.  Positions ascend through both
    strands of every contig, 500 bases clear of contig ends and of the strand boundary, 400 or more apart (300 where n chains would
    not fit otherwise): no seed is within w of another chain's diagonal, none is contained in another, all positions differ.  At most
    max_hits (< max_occ) chains share one query interval.  Four reads per size up to 255 chains, two per larger size; the order of the
    rows is the construction's and is not shuffled.  -> [(lq, [(qb, qe, hits)])] as reference_chains takes them"""
    lq = SORTED_TAIL_LQ
    spans = []
    for k in range(n_seqs):
        spans.append((offs[k] + 500, offs[k + 1] - 500 - lq))
        spans.append((2 * l_pac - offs[k + 1] + 500, 2 * l_pac - offs[k] - 500 - lq))
    spans.sort()
    cases = []
    for n in sizes:
        for rep in range(4 if n <= 255 else 2):
            step, jit = 500, 100
            slots = [p for lo, hi in spans for p in range(lo, hi - jit, step)]
            if len(slots) < n:
                step, jit = 340, 40
                slots = [p for lo, hi in spans for p in range(lo, hi - jit, step)]
            assert len(slots) >= n, (n, len(slots))
            first = int(rng.integers(0, len(slots) - n + 1)) if n <= 255 else 0
            pick = slots[first:first + n] if n <= 255 else [slots[i] for i in np.sort(rng.choice(len(slots), n, replace=False))]
            pos = [p + int(rng.integers(0, jit + 1)) for p in pick]
            ivs, full = {}, lambda qb, ln: len(ivs.get((qb, qb + ln), ())) >= max_hits
            for p, ln in zip(pos, sorted_tail_weights(rng, n)):
                qb = int(rng.integers(0, lq - ln + 1))
                while full(qb, ln):
                    qb = (qb + 1) % (lq - ln + 1)
                ivs.setdefault((qb, qb + ln), []).append(p)
            cases.append((lq, [(qb, qe, h) for (qb, qe), h in ivs.items()]))
    return cases


def single_seed_weights(case):
    """the weights of the chains of a read whose chains have one seed each, in the order mem_chain_flt's sort meets them (ascending
    position)"""
    lq, ivs = case
    return [ln for _, ln in sorted((rb, qe - qb) for qb, qe, hits in ivs for rb in hits)]


def reference_chains(ref, ropt, cases):
    """-> (read lengths, seeds per read in mem_chain's visiting order, expected chains [(rid, frac_rep bits, seeds)])"""
    lens, seedsets, want = [], [], []
    for lq, ivs in cases:
        # mem_chain visits the intervals in info order (mem_collect_intv sorts them, src/bwamem.c:161) and the hits of one
        # interval in suffix-array order (:273-283); every interval here has at most max_occ hits, so l_rep = 0
        ivs = sorted(ivs, key=lambda t: (t[0] << 32) | t[1])
        seedsets.append([(rb, qb, qe - qb) for qb, qe, hits in ivs for rb in hits])
        lens.append(lq)
        exp = []
        for rid, w, kept, is_alt, fb, sd in po.ref_chains(ropt, ref.bns, lq, ivs):
            # mem_chain2aln sorts the seeds of a chain by (score << 32 | index) and walks that array from its end
            # (src/bwamem.c:663-668); the stage hook returns the sorted array
            order = sorted(range(len(sd)), key=lambda i: (sd[i][2] << 32) | i)
            exp.append((rid, fb, [sd[i] for i in order]))
        want.append(exp)
    return lens, seedsets, want


TIED_SMALL_SEED = 2611
TIED_SMALL_PER_LAUNCH = 32
# (seeds, chains) a read may have for each of the three lane-per-read launches: chain_kernel<16, 4>, <64, 9>, <255, 9>
TIED_SMALL_LAUNCHES = (((3, 16), (3, 4)), ((17, 64), (3, 9)), ((65, 255), (3, 9)))


def tied_small_launch(n_seeds, n_chains):
    """which of the three launches takes a read with so many seeds and chains: the first whose UPPER bounds fit, as the kernels decide
    it (a read of 5 seeds and 6 chains is the second launch's); None: none of them"""
    for k, ((_, s_hi), (_, c_hi)) in enumerate(TIED_SMALL_LAUNCHES):
        if n_seeds <= s_hi and n_chains <= c_hi:
            return k
    return None


def tied_small_chain_sets(rng, l_pac, offs, n_seqs, per_launch=TIED_SMALL_PER_LAUNCH):
    """Reads whose 3-9 chains reach mem_chain_flt's sort with TIES among their weights, not in sorted order: the sort of the one-node
    path (chain_read: ks_introsort's small form).  A chain is m co-linear seeds (q0 + j, length L) at positions p + q0 + j, j < m: each
    merges into the chain the first one opened, none is contained in it, and the chain weighs L + m - 1 on the query and on the
    reference; m brings the read's seed count into its launch's range.  Chains lie 500 or more apart in ascending position on one
    strand of one contig (so the sort meets them in the order built), weights are drawn from 2-3 values in 76...150 (all within the
    default drop_ratio of one another; every seed at least min_seed_len long).  per_launch reads for each of TIED_SMALL_LAUNCHES.
    -> ([(lq, [(qb, qe, hits)])], [(launch, weights in the order the sort meets them)])"""
    lq = SORTED_TAIL_LQ
    spans = [(offs[k] + 500, offs[k + 1] - 500 - lq) for k in range(n_seqs)]
    cases, meta = [], []
    for launch, ((s_lo, s_hi), (c_lo, c_hi)) in enumerate(TIED_SMALL_LAUNCHES):
        for it in range(per_launch):
            n = int(rng.integers(c_lo, c_hi + 1))
            ns = int(rng.integers(max(s_lo, n), s_hi + 1))
            m = [ns // n + (1 if c < ns % n else 0) for c in range(n)]            # seeds per chain, at most 85
            while True:   # (every seed keeps min_seed_len = 19 bases: L = weight - m + 1)
                vals = rng.choice(np.arange(max(76, m[0] + 18), 151), int(rng.integers(2, 4)), replace=False)
                w = [int(v) for v in rng.choice(vals, n)]
                if len(set(w)) < n and w != sorted(w, reverse=True):
                    break
            lo, hi = spans[int(rng.integers(0, len(spans)))]
            first = int(rng.integers(lo, hi - 600 * n))
            ivs = {}
            for c in range(n):
                p = first + 600 * c + int(rng.integers(0, 100))
                L = w[c] - m[c] + 1
                q0 = int(rng.integers(0, lq - w[c] + 1))
                for j in range(m[c]):
                    ivs.setdefault((q0 + j, q0 + j + L), []).append(p + q0 + j)
            cases.append((lq, [(qb, qe, sorted(h)) for (qb, qe), h in ivs.items()]))
            meta.append((launch, w))
    return cases, meta
