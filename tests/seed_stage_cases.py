"""Cases of the seed enumeration stage test (seed_prep_kernel / seed_enum_kernel through mi355x_seed_batch) and the plain restatement
they are compared with: src/bwamem.c:161 (the sort of the intervals by info), :265-272 (l_rep) and :273-283 (the seeds of an interval
larger than max_occ are taken at a stride).  Integers only, so the comparison is exact.  tests/test_gpu_seed_stage.py pins the
restatement itself against the reference's mem_chain (oracle/chain_inject.c) on the CPU."""
import numpy as np

MAX_OCCS = (1, 2, 50, 500, 10000)


def info(qb, qe):
    return (qb << 32) | qe


def expected(intv, cap, max_occ):
    """-> (intervals sorted by info, l_rep, (rows, qbeg, len) of the seeds in mem_chain's order) for the first `cap` intervals of a read"""
    a = sorted((tuple(int(x) for x in t) for t in np.asarray(intv, dtype=np.uint64).reshape(-1, 4)[:cap]), key=lambda t: t[3])
    b = e = l_rep = 0
    rows, qbeg, slen = [], [], []
    for x0, x1, size, inf in a:
        sb, se = inf >> 32, inf & 0xffffffff
        if size > max_occ:
            if sb > e:
                l_rep += e - b
                b, e = sb, se
            else:
                e = max(e, se)
        # for (k = count = 0; k < size && count < max_occ; k += step, ++count): k = 0, step, 2 step, ... below size, at most max_occ of them
        step = size // max_occ if size > max_occ else 1
        count = min(max_occ, (size + step - 1) // step)
        rows.append(np.uint64(x0) + np.arange(count, dtype=np.uint64) * np.uint64(step))
        qbeg.append(np.full(count, sb, dtype=np.int32))
        slen.append(np.full(count, se - sb, dtype=np.int32))
    l_rep += e - b
    cat = lambda v, t: np.concatenate(v) if v else np.zeros(0, dtype=t)
    return a, l_rep, (cat(rows, np.uint64), cat(qbeg, np.int32), cat(slen, np.int32))


def sizes_for(max_occ):
    s = {1, max_occ - 1, max_occ, max_occ + 1, 2 * max_occ - 1, 2 * max_occ, 2 * max_occ + 1, 10 * max_occ + 3, (1 << 32) + 5, (1 << 40) + 12345}
    return sorted(x for x in s if x >= 1)


def crafted_reads(max_occ, cap, seed):
    """per read a list of (x0, x1, size, info); the families of the issue: every size around max_occ, repetitive intervals that are
    disjoint, touch, overlap, nest, arrive in descending order, none / all repetitive, 0 / 1 / cap / more than cap intervals, equal keys"""
    rng = np.random.default_rng(seed)
    big, small = 3 * max_occ + 1, 1
    x = lambda: int(rng.integers(0, 1 << 33))
    rd = []
    for s in sizes_for(max_occ):                                   # one interval of every size, alone and between two others
        rd.append([(x(), x(), s, info(10, 40))])
        rd.append([(x(), x(), 1, info(0, 30)), (x(), x(), s, info(10, 40)), (x(), x(), max_occ + 1, info(50, 90))])
    geo = {
        "disjoint": [(0, 30), (40, 70), (100, 150)],
        "touch": [(0, 30), (30, 60), (60, 61), (61, 100)],           # sb == e: merged (the test is sb > e)
        "touch+1": [(0, 30), (31, 60)],
        "overlap": [(0, 50), (20, 80), (79, 120)],
        "nest": [(0, 100), (10, 40), (50, 60), (99, 130)],
        "same_start": [(5, 30), (5, 60), (5, 45)],
        "from_zero": [(0, 19)],
        "late": [(120, 150)],
    }
    for pts in geo.values():
        for order in (pts, pts[::-1], [pts[i] for i in rng.permutation(len(pts))]):
            rd.append([(x(), x(), big, info(qb, qe)) for qb, qe in order])                                   # all repetitive
            rd.append([(x(), x(), big if j % 2 == 0 else small, info(qb, qe)) for j, (qb, qe) in enumerate(order)])   # every other one
            rd.append([(x(), x(), small, info(qb, qe)) for qb, qe in order])                                 # none repetitive
    rd.append([])                                                  # no interval
    rd.append([(x(), x(), max_occ, info(3, 33))])
    same = (x(), x(), 2 * max_occ + 1, info(20, 60))               # one interval found twice: identical records
    rd.append([(x(), x(), 1, info(70, 100)), same, (x(), x(), 3, info(0, 25)), same])
    for n in (cap - 1, cap, cap + 1, cap + 5):                     # exactly cap, more than cap (the kernels look at the first cap)
        rd.append([(x(), x(), int(rng.choice(sizes_for(max_occ)[:8])), info(int(q), int(q) + int(rng.integers(19, 60))))
                   for q in rng.permutation(200)[:n]])
    for _ in range(60 if max_occ <= 500 else 8):                    # random mixtures
        n = int(rng.integers(0, cap + 1))
        rd.append([(x(), x(), int(rng.choice(sizes_for(max_occ)[:8])), info(int(q), int(q) + int(rng.integers(19, 90))))
                   for q in rng.integers(0, 120, n)])
    # equal keys must be identical records (the sort is not stable in the reference): drop accidental clashes of the random reads
    out = []
    for r in rd:
        seen, keep = {}, []
        for t in r:
            if seen.setdefault(t[3], t) == t:
                keep.append(t)
        out.append(keep)
    return out
