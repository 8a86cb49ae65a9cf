"""Inputs of the stage tests of the seeding kernels (smem_kernel in csrc/fm_kernels.hip, smem_p3_kernel in csrc/smem_kernels.hip):
tests/test_smem_cases.py (CPU: the oracle against the reference under every option set, and the conditions that make the cases bite)
and tests/test_gpu_smem_options.py (the kernels against the oracle).  CPU only: nothing here touches the GPU.

What the kernels branch on, and so what the cases are placed around:
  * launch_smem picks smem_kernel<QLDS, LC, QS, COUNT, KMT> from the longest read of the batch: <= QSLOT_S, <= QSLOT, longer;
  * SmemParams: min_seed_len (the third pass's jump table switches off at min_seed_len <= P3_K; the k-mer tables hand out results of
    up to kmt_depth() bases, shorter than a seed when min_seed_len is larger), split_len, split_width, max_mem_intv;
  * the interval list of a forward sweep lives in LDS up to LCAP_S / LCAP entries and in HBM beyond;
  * smem_p3_kernel keeps two 8-base windows per lane and builds its k-mer from P3_K + 1 bases; a workgroup has P3_BLOCK lanes;
    smem_kernel deals reads SMEM_FETCH at a time."""
import numpy as np

# csrc/fm_kernels.hip, csrc/smem_kernels.hip, csrc/device.hip (tests/test_smem_cases.py reads the sources and compares)
LCAP_S, LCAP, QSLOT_S, QSLOT, SMEM_FETCH, P3_BLOCK = 20, 23, 160, 256, 16, 256
P3_K = 12                       # maybe_build_p3: extensions folded into the third pass's jump table


def kmt_depth(seq_len):
    """maybe_build_kmt's default: the shortest k with 4^k >= rows of the index (at most 14)"""
    k = 1
    while k < 14 and (1 << (2 * k)) < seq_len:
        k += 1
    return k


DEFAULTS = dict(min_seed_len=19, split_factor=1.5, split_width=10, max_mem_intv=20)
REPEAT_GENOME = dict(total_len=240_000, n_contigs=3, seed=17, repeat_frac=0.35)     # the genome of tests/test_gpu_seed_stage.py
REPEAT_KMT = kmt_depth(2 * REPEAT_GENOME["total_len"])                             # 10: the text is the genome and its reverse complement
CORNER = dict(min_seed_len=10, split_factor=0.5, split_width=200, max_mem_intv=500)


def _option_sets():
    sets = [("default", {})]
    # 12: the jump table is off; 13: on, at the edge; REPEAT_KMT and one below: the k-mer tables answer up to a whole seed / all but its last base
    for v in sorted({10, P3_K, P3_K + 1, 25, REPEAT_KMT, REPEAT_KMT - 1}):
        sets.append(("min_seed_len=%d" % v, dict(min_seed_len=v)))
    for v in (0.5, 1.0, 4.0):   # 0.5: split_len is shorter than a seed, so every rare SMEM re-seeds
        sets.append(("split_factor=%g" % v, dict(split_factor=v)))
    for v in (0, 1, 200):
        sets.append(("split_width=%d" % v, dict(split_width=v)))
    for v in (0, 1, 2, 500):
        sets.append(("max_mem_intv=%d" % v, dict(max_mem_intv=v)))
    sets.append(("corner", dict(CORNER)))
    return sets


OPTION_SETS = _option_sets()
OPTION_IDS = [n for n, _ in OPTION_SETS]


def oracle_args(kw):
    """the arguments of OracleFM.collect_intv for an option set"""
    o = dict(DEFAULTS)
    o.update(kw)
    return o["min_seed_len"], o["split_factor"], o["split_width"], o["max_mem_intv"]


def write_index(directory, name, names, seqs):
    """FASTA and bwa-format index of a case genome, built by the product's own indexer on the CPU -> the prefix"""
    import os
    from mpibwa_amd import api, simulate
    fa = os.path.join(str(directory), name + ".fa")
    simulate.write_fasta(fa, names, seqs)
    api.build_index(fa, fa)
    return fa


def rc(a):
    a = np.asarray(a, np.uint8)
    return np.where(a > 3, 4, 3 - a)[::-1].astype(np.uint8)


def length_class(reads):
    """0 / 1 / 2: the instantiation family launch_smem picks for this batch"""
    m = max(len(r) for r in reads)
    return 0 if m <= QSLOT_S else 1 if m <= QSLOT else 2


# ---------------------------------------------------------------------------------------------------------------------------------
# staircases: reads whose forward sweep changes its interval size some thirty times, so the list outgrows LDS
# ---------------------------------------------------------------------------------------------------------------------------------
STAIR_LENS = (150, 150, 250, 250, 300, 300)
N_STEPS = 30


def _other(rng, b):
    return np.uint8((int(b) + int(rng.integers(1, 4))) & 3)


def staircase_genome(seed=5):
    """-> (names, seqs, reads): one contig of random bases, some 41 kb, and two families of reads planted in it.

    `stair`: a read S, held once in full, and for k = 1..30 a copy of S[:12 + 4k] followed by a base that differs from S[12 + 4k].  The
    sweep from position 0 sees the interval shrink at thirty lengths; the list's last entry, beyond LDS, is the one reported.  The
    reverse complement has the staircase on its left: a backward extension loses a copy every fourth step.

    `hill`: a read A + B of two halves, held once in full, and for k = 1..30 a copy of A[-a_k:] + B[:8 + 2k] between two differing
    bases.  The whole read occurs once, so re-seeding starts a sweep at its middle with min_intv 2: thirty entries going forward,
    and going backward entry k dies after a_k steps.  a_k falls with k in the first read of a length (every row loses its first entry
    alone, every survivor differs from its neighbour) and is random in the second (survivors of equal size are dropped, some of
    them across two groups of four)."""
    rng = np.random.default_rng(seed)
    sp = lambda: rng.integers(0, 4, size=20, dtype=np.uint8)
    pieces, reads = [rng.integers(0, 4, size=1500, dtype=np.uint8)], []
    for n, L in enumerate(STAIR_LENS):
        S = rng.integers(0, 4, size=L, dtype=np.uint8)
        pieces += [S, sp()]
        for k in range(1, N_STEPS + 1):
            b = 12 + 4 * k
            pieces += [S[:b], [_other(rng, S[b])], sp()]
        reads.append(("stair%d_%d" % (L, n % 2), S))
    for n, L in enumerate(STAIR_LENS):
        R = rng.integers(0, 4, size=L, dtype=np.uint8)
        mid = L >> 1
        A, B = R[:mid], R[mid:]
        if n % 2 == 0:
            a = [70 - 2 * k for k in range(1, N_STEPS + 1)]
        else:
            a = [int(v) for v in rng.integers(4, 71, size=N_STEPS)]
        pieces += [R, sp()]
        for k in range(1, N_STEPS + 1):
            b = 8 + 2 * k
            pieces += [[_other(rng, A[-a[k - 1] - 1])], A[-a[k - 1]:], B[:b], [_other(rng, B[b])], sp()]
        reads.append(("hill%d_%d" % (L, n % 2), R))
    pieces.append(rng.integers(0, 4, size=1500, dtype=np.uint8))
    text = np.concatenate([np.asarray(p, np.uint8) for p in pieces])
    check_staircases(text, reads)
    reads += [(t + "_rc", rc(r)) for t, r in reads]
    return ["stairs"], [text], reads


def list_entries(text, read, x):
    """Brute force on the text itself (the forward strand followed by its reverse complement, as the index holds it): the number of
    distinct occurrence counts of read[x:x+l] for l = 1, 2, ... while it occurs at all.  A forward sweep from x pushes one list entry
    per change of that count."""
    T = np.concatenate([np.asarray(text, np.uint8), rc(text)])
    pos = np.arange(len(T))
    counts = set()
    for l in range(1, len(read) - x + 1):
        c = read[x + l - 1]
        if c > 3:
            break
        pos = pos[pos + l - 1 < len(T)]
        pos = pos[T[pos + l - 1] == c]
        if len(pos) == 0:
            break
        counts.add(len(pos))
    return len(counts)


def staircase_sweep_start(tag, read):
    """where the long sweep of a staircase read starts: position 0, or for a hill the middle, where re-seeding starts it"""
    return len(read) >> 1 if tag.startswith("hill") and not tag.endswith("_rc") else 0


def check_staircases(text, reads):
    """the condition on the staircase reads: the list of the long sweep outgrows LDS by at least three entries"""
    for tag, r in reads:
        if tag.endswith("_rc"):
            continue
        n = list_entries(text, r, staircase_sweep_start(tag, r))
        assert n >= LCAP + 3, (tag, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# reads of a repeat-rich genome: re-seeding and the third pass have something to find
# ---------------------------------------------------------------------------------------------------------------------------------
def repeat_genome():
    from mpibwa_amd import simulate
    return simulate.make_genome(REPEAT_GENOME["total_len"], REPEAT_GENOME["n_contigs"], seed=REPEAT_GENOME["seed"],
                                repeat_frac=REPEAT_GENOME["repeat_frac"])


def repeat_reads(seqs=None):
    """-> (reads150, reads_var, reads_long): 300 reads of 150 bp, 300 of 30-250 bp, 24 of 257-400 bp, all from `seqs` (repeat_genome()'s
    when not given)"""
    from mpibwa_amd import simulate
    if seqs is None:
        seqs = repeat_genome()[1]
    take = lambda rd: [np.asarray(r[1], np.uint8) for r in rd]
    r150 = take(simulate.simulate_reads(seqs, 300, 150, paired=False, seed=3))
    rvar = take(simulate.simulate_reads(seqs, 300, 150, paired=False, seed=4, var_len=(30, 250)))
    rlong = take(simulate.simulate_reads(seqs, 24, 150, paired=False, seed=5, var_len=(257, 400)))
    return r150, rvar, rlong


def class_batches(r150, rvar, rlong):
    """three batches, one per length class of launch_smem; the last has reads on either side of QSLOT (the per-read q_lds)"""
    small = r150 + [r for r in rvar if len(r) <= QSLOT_S]
    mid = list(rvar)
    large = rlong + rvar[:100] + r150[:100]
    assert length_class(small) == 0 and length_class(mid) == 1 and length_class(large) == 2
    assert max(len(r) for r in mid) > QSLOT_S and sum(len(r) <= QSLOT for r in large) >= 100 and sum(len(r) > QSLOT for r in large) >= 20
    return small, mid, large


# ---------------------------------------------------------------------------------------------------------------------------------
# lengths, ambiguous bases on the kernels' own boundaries
# ---------------------------------------------------------------------------------------------------------------------------------
def edge_reads(seqs, p3_k=P3_K, min_seed_lens=(19, 12, 13)):
    """-> [(tag, read)] cut from an N-free stretch of the genome `seqs`"""
    g = None
    for s in seqs:
        s = np.asarray(s, np.uint8)
        bad = np.flatnonzero(s > 3)
        start = 2000 if len(bad) == 0 or bad[0] > 3000 else int(bad[-1]) + 1000
        if start + 1000 <= len(s) and (s[start:start + 1000] < 4).all():
            g = s[start:start + 1000]
            break
    assert g is not None
    out = []
    lens = {7, 8, 9, 15, 16, 17, 159, 160, 161, 255, 256, 257, p3_k, p3_k + 1, p3_k + 2}
    for m in min_seed_lens:
        lens |= {m - 1, m, m + 1}
    for k, L in enumerate(sorted(lens)):
        out.append(("len%d" % L, g[3 * k:3 * k + L].copy()))
        out.append(("len%d_rc" % L, rc(g[3 * k + 100:3 * k + 100 + L])))

    def with_n(base, at, tag):
        r = base.copy()
        r[list(at)] = 4
        out.append((tag, r))
    for L in (150, 40, 257):
        base = g[300:300 + L]
        for p in sorted({0, 7, 8, p3_k - 1, p3_k, p3_k + 1, L - 1, L - 8, L - 9, L - p3_k - 1, L - p3_k - 2}):
            with_n(base, [p], "N@%d/%d" % (p, L))
        for p in (0, 7, 8, 20, L - 9):
            with_n(base, [p, p + 8], "N@%d+8/%d" % (p, L))
        with_n(base, range(0, L, 13), "N/13/%d" % L)
        with_n(base, range(p3_k, L, p3_k + 1), "N/%d@%d/%d" % (p3_k + 1, p3_k, L))
        with_n(base, range(L), "allN/%d" % L)
        with_n(base, range(1, L), "oneBase/%d" % L)
    for L in (150, 256, 300):
        for b in range(4):
            out.append(("homo%d/%d" % (b, L), np.full(L, b, np.uint8)))
        for a, b in ((0, 1), (0, 3), (1, 2), (2, 0)):
            out.append(("di%d%d/%d" % (a, b, L), np.array([a, b] * (L // 2), np.uint8)))
        out.append(("tri/%d" % L, np.array([0, 2, 3] * (L // 3), np.uint8)))
    assert len({t for t, _ in out}) == len(out)
    return out
