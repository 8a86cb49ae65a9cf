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


def _cluster_rows(ix, rng, n, free_span):
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
