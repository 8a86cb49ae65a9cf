"""Chains and what the reference's own mem_chain2aln makes of them (oracle/_ref/libbwaref.so), for the stage test of c2a_kernel and its chain
groups (tests/test_gpu_c2a_stage.py) and its CPU companion (tests/test_c2a_cases.py).

Two sources of chains.  (A) natural ones: designed reads on a repeat-rich genome through the reference's mem_chain -> mem_chain_flt ->
mem_flt_chained_seeds, as mem_align1_core runs them.  (B) hand-built ones at the exact thresholds of mem_chain2aln, built to the invariants
mem_chain guarantees (one strand and one contig per chain, rid = the contig of seeds[0], seeds inside the read, score = len unless
rescored), so that the reference's assert(c->rid == rid) holds.  Either way the reference side is mem_chain2aln per chain, in chain order,
into one mem_alnreg_v."""
import ctypes as C
import math
import os

import numpy as np

import window_model
from oracle import pyoracle as po


def _ref_handle():
    """a ctypes handle of our own on the reference's library: the prototypes set here must not change those of oracle/pyoracle.py's handle"""
    po.ref_lib()
    h = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(po.__file__)), "_ref", "libbwaref.so"))
    h.bwa_fill_scmat.argtypes = [C.c_int, C.c_int, C.c_void_p]
    return h


class _alnreg_v(C.Structure):   # mem_alnreg_v (src/bwamem.h:79)
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.c_void_p)]


class _chain_v(C.Structure):   # mem_chain_v (src/bwamem.c:180)
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.c_void_p)]


CHAIN_T_BYTES = 40   # mem_chain_t (src/bwamem.c:174-179): n, m, first, rid, w:29|kept:2|is_alt:1, frac_rep, pos, seeds*


class _seed_t(C.Structure):    # mem_seed_t (src/bwamem.c:168-172)
    _fields_ = [("rbeg", C.c_int64), ("qbeg", C.c_int32), ("len", C.c_int32), ("score", C.c_int32)]


class _chain_t(C.Structure):   # mem_chain_t
    _fields_ = [("n", C.c_int), ("m", C.c_int), ("first", C.c_int), ("rid", C.c_int), ("bits", C.c_uint32), ("frac_rep", C.c_float),
                ("pos", C.c_int64), ("seeds", C.POINTER(_seed_t))]


assert C.sizeof(_chain_t) == CHAIN_T_BYTES and C.sizeof(_seed_t) == 24


def _regs_copy(v):
    if not v.n:
        return np.zeros(0, dtype=po.ALNREG_DT)
    return np.ctypeslib.as_array(C.cast(v.a, C.POINTER(C.c_uint8)), shape=(v.n * 88,)).view(po.ALNREG_DT).copy()


FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep")

# mem_opt_t settings of the stage test (never e_del or e_ins = 0: cal_max_gap divides by them)
OPTION_SETS = {
    "default": dict(),
    "w20": dict(w=20),
    "w300": dict(w=300),
    "a2b5": dict(a=2, b=5, o_del=8, e_del=2, o_ins=7, e_ins=3),
    "b9": dict(a=1, b=9, o_del=2, e_del=1, o_ins=2, e_ins=1),   # a + b >= min(o) + min(e): a flank with one mismatch goes to the DP
    "clip5_0": dict(pen_clip5=0, pen_clip3=100),
    "clip3_0": dict(pen_clip5=100, pen_clip3=0),
    "zdrop1": dict(zdrop=1),
    "zdrop0": dict(zdrop=0),
    "maxocc20": dict(max_occ=20),
    "minseed30": dict(min_seed_len=30),
}


class Reference:
    """the reference's index, options and stage functions"""

    def __init__(self, prefix, kw):
        from mpibwa_amd import abi
        self.R = R = _ref_handle()
        self.ref = po.RefIndex(prefix)
        self.opt = self.ref.opt(**kw)
        if "a" in kw or "b" in kw:
            R.bwa_fill_scmat(self.opt.contents.a, self.opt.contents.b, self.opt.contents.mat)
        P_opt, P_bwt, P_bns, P_u8 = C.POINTER(abi.mem_opt_t), C.POINTER(abi.bwt_t), C.POINTER(abi.bntseq_t), C.POINTER(C.c_uint8)
        R.mem_chain.restype = _chain_v
        R.mem_chain.argtypes = [P_opt, P_bwt, P_bns, C.c_int, C.c_char_p, C.c_void_p]
        R.mem_chain_flt.restype = C.c_int
        R.mem_chain_flt.argtypes = [P_opt, C.c_int, C.c_void_p]
        R.mem_flt_chained_seeds.restype = None
        R.mem_flt_chained_seeds.argtypes = [P_opt, P_bns, P_u8, C.c_int, C.c_char_p, C.c_int, C.c_void_p]
        R.mem_chain2aln.restype = None
        R.mem_chain2aln.argtypes = [P_opt, P_bns, P_u8, C.c_int, C.c_char_p, C.c_void_p, C.POINTER(_alnreg_v)]
        bns = self.ref.bns.contents
        self.l_pac = int(bns.l_pac)
        self.contigs = [(int(bns.anns[i].offset), int(bns.anns[i].len)) for i in range(bns.n_seqs)]

    def chains(self, read):
        """mem_chain -> mem_chain_flt -> mem_flt_chained_seeds on a read (nt4 codes) -> ([(rid, frac_rep, [(rbeg, qbeg, len, score)])],
        chains that mem_flt_chained_seeds emptied)"""
        buf = C.create_string_buffer(bytes(read.astype(np.uint8)), len(read) + 1)
        chn = self.R.mem_chain(self.opt, self.ref.bwt, self.ref.bns, len(read), buf, None)
        chn.n = self.R.mem_chain_flt(self.opt, chn.n, chn.a)
        before = [C.cast(chn.a + i * CHAIN_T_BYTES, C.POINTER(_chain_t)).contents.n for i in range(chn.n)]
        self.R.mem_flt_chained_seeds(self.opt, self.ref.bns, self.ref.pac, len(read), buf, chn.n, chn.a)
        out, emptied = [], 0
        for i in range(chn.n):
            c = C.cast(chn.a + i * CHAIN_T_BYTES, C.POINTER(_chain_t)).contents
            out.append((int(c.rid), float(c.frac_rep), [(int(c.seeds[j].rbeg), int(c.seeds[j].qbeg), int(c.seeds[j].len), int(c.seeds[j].score))
                                                         for j in range(c.n)]))
            emptied += before[i] > 0 and c.n == 0
        return out, emptied

    def chain2aln(self, read, chains, alone=False):
        """mem_chain2aln on every chain in order into one region list (mem_align1_core) -> ALNREG_DT array; alone: every chain into a
        list of its own -> [region count per chain]"""
        buf = C.create_string_buffer(bytes(read.astype(np.uint8)), len(read) + 1)
        keep = []
        regs = _alnreg_v()
        counts = []
        for rid, frac, sd in chains:
            arr = (_seed_t * max(len(sd), 1))()
            for j, (rb, qb, ln, sc) in enumerate(sd):
                arr[j].rbeg, arr[j].qbeg, arr[j].len, arr[j].score = rb, qb, ln, sc
            ch = _chain_t(n=len(sd), m=len(sd), first=-1, rid=rid, bits=0, frac_rep=frac, pos=sd[0][0] if sd else 0, seeds=arr)
            keep.append((arr, ch))
            if alone:
                one = _alnreg_v()
                self.R.mem_chain2aln(self.opt, self.ref.bns, self.ref.pac, len(read), buf, C.addressof(ch), C.byref(one))
                counts.append(int(one.n))
                po.libc.free(C.c_void_p(one.a))
            else:
                self.R.mem_chain2aln(self.opt, self.ref.bns, self.ref.pac, len(read), buf, C.addressof(ch), C.byref(regs))
        if alone:
            return counts
        got = _regs_copy(regs)
        po.libc.free(C.c_void_p(regs.a))
        return got

    def cal_max_gap(self, qlen):   # src/bwamem.c:621-628
        return window_model.cal_max_gap(self.opt.contents, qlen)

    def window(self, lq, chain):
        """(rmax0, rmax1 before clamping, after clamping) of mem_chain2aln (src/bwamem.c:642-661)"""
        rid, _, sd = chain
        before, _, after = window_model.chain_window(self.l_pac, self.contigs, self.cal_max_gap, lq, rid, sd)
        return before, after


# ---------------------------------------------------------------------------------------------------------------------------------
# (A) natural chains of designed reads
# ---------------------------------------------------------------------------------------------------------------------------------
_COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


def _clean(s, rng):
    s = np.array(s, dtype=np.uint8)
    m = s > 3
    s[m] = rng.integers(0, 4, int(m.sum()))
    return s


def _sub(s, pos):
    s = s.copy()
    for p in pos:
        s[p] = (s[p] + 1 + (p % 3)) & 3
    return s


def natural_reads(seqs, w, rng, scale=1):
    """-> [(family, read)]: reads (nt4 codes) designed to reach the branches of mem_chain2aln; w = the option set's band"""
    out = []
    L = len(seqs)

    def piece(ln, c=None, edge=0):
        c = int(rng.integers(0, L)) if c is None else c
        p = int(rng.integers(edge, len(seqs[c]) - ln - edge))
        return c, p, _clean(seqs[c][p:p + ln], rng)

    def strand(r):
        return _COMP[r[::-1]] if rng.random() < 0.5 else r

    # no-DP closed form: 0-3 substitutions at chosen distances from the seed ends, flank position 0 and the last base included
    for k in range(24 * scale):
        ln = int(rng.choice([100, 126, 150]))
        _, _, r = piece(ln)
        nsub = k % 4
        choices = [0, 1, ln - 1, ln - 2, 20, 21, 40, 60, ln - 21, ln - 30]
        pos = sorted(set(int(x) for x in rng.choice(choices, nsub, replace=False))) if nsub else []
        out.append(("closed", strand(_sub(r, pos))))
    # exactly one mismatch per flank: the seed in the middle, one substitution on either side
    for k in range(16 * scale):
        _, _, r = piece(150)
        out.append(("one_mm", strand(_sub(r, [int(rng.integers(5, 50)), int(rng.integers(100, 145))]))))
    # an ambiguous base in a flank
    for k in range(8 * scale):
        _, _, r = piece(150)
        r = r.copy()
        r[int(rng.choice([2, 10, 140, 147]))] = 4
        out.append(("ambig", strand(r)))
    # band doubling: indels near both ends, deletions just under, at and over w and 0.75 w
    for k in range(10 * scale):
        c, p, r = piece(600)
        ln = 150
        if k % 2 == 0:   # an indel near an end
            cut = int(rng.choice([3, 6, 10, ln - 10, ln - 6]))
            if rng.random() < 0.5:
                read = np.concatenate([r[:cut], r[cut + int(rng.integers(1, 6)):cut + ln]])
            else:
                read = np.concatenate([r[:cut], rng.integers(0, 4, int(rng.integers(1, 5))).astype(np.uint8), r[cut:ln]])[:ln]
            out.append(("indel_end", strand(read)))
    for d in sorted({w - 1, w, w + 1, (3 * w) // 4 - 1, (3 * w) // 4, (3 * w) // 4 + 1, 2 * w - 1}):
        for _ in range(2 * scale):
            c, p, r = piece(3 * d + 200)
            out.append(("deletion", strand(np.concatenate([r[:d + 100], r[2 * d + 100:]]))))
    # two long pieces a deletion wider than w apart: two chains, the second one's seeds may fall inside the first one's region
    for k in range(6 * scale):
        gap = w + 1 + int(rng.integers(0, max(w // 2, 1)))
        ln = min(int(gap * (11 + 3 * rng.random())), 1800)
        c, p, r = piece(2 * ln + gap)
        out.append(("two_piece", strand(np.concatenate([r[:ln], r[ln + gap:]]))))
    # tandem duplications of a 2-40 base unit (seeds on diagonals a period apart) and low-complexity stretches
    for k in range(12 * scale):
        per = int(rng.choice([2, 3, 5, 8, 13, 21, 40]))
        c, p, r = piece(200)
        a = int(rng.integers(40, 110))
        copies = int(rng.integers(1, 4))
        read = np.concatenate([r[:a]] + [r[a - per:a]] * copies + [r[a:]])[:150]
        out.append(("tandem", strand(read)))
    # reads of repeat families: many chains; some with the deletion construction as well
    for k in range(120 * scale):
        c, p, r = piece(150)
        out.append(("repeat?", strand(r)))
    for k in range(6 * scale):
        gap = w + 1 + int(rng.integers(0, max(w // 2, 1)))
        c, p, r = piece(300 + gap)
        out.append(("repeat_del?", strand(np.concatenate([r[:150], r[150 + gap:300 + gap]]))))
    # window clamping: reads over contig starts and ends, at the forward/reverse boundary, next to N runs
    for k in range(4 * scale):
        c = int(rng.integers(0, L))
        h = int(rng.integers(5, 40))
        out.append(("edge", strand(np.concatenate([rng.integers(0, 4, h).astype(np.uint8), _clean(seqs[c][:150 - h], rng)]))))
        out.append(("edge", strand(np.concatenate([_clean(seqs[c][len(seqs[c]) - 150 + h:], rng), rng.integers(0, 4, h).astype(np.uint8)]))))
    last = seqs[L - 1]
    for k in range(2 * scale):
        r = _clean(last[len(last) - 150 + k:], rng)
        out.append(("edge", r))
        out.append(("edge", _COMP[r[::-1]]))
    for c in range(L):
        nz = np.flatnonzero(seqs[c] == 4)
        if len(nz):
            a, b = int(nz[0]), int(nz[-1]) + 1
            if a > 200:
                out.append(("n_run", _clean(seqs[c][a - 140:a + 10], rng)))
            if b + 200 < len(seqs[c]):
                out.append(("n_run", strand(_clean(seqs[c][b - 10:b + 140], rng))))
    # long reads: mem_flt_chained_seeds rescores and drops seeds, chains can end up empty; the longest one takes c2a's LDS beyond 64 KB
    for k, ln in enumerate([1500, 2200, 3000, 4000, 5000][:2 + 3 * scale]):
        c, p, r = piece(ln + 40)
        r = r[:ln].copy()
        m = rng.random(ln) < 0.01
        r[m] = (r[m] + 1) & 3
        if k % 2:
            r = np.concatenate([r[:ln // 2], r[ln // 2 + 12:]])
        out.append(("long", strand(r)))
    # long reads with a 30-base piece from elsewhere at an end: a chain of its own that mem_flt_chained_seeds empties
    for k in range(2 * scale):
        c, p, r = piece(1600)
        _, _, f = piece(30)
        out.append(("long", strand(np.concatenate([r[:1570], f]) if k % 2 else np.concatenate([f, r[30:]]))))
    return out


def natural_cases(ref, seqs, rng, scale=1):
    """-> [(family, read, chains)] with the reference's chains; the repeat families keep only reads with more than 8 chains"""
    res = []
    w = int(ref.opt.contents.w)
    emptied = 0
    for fam, read in natural_reads(seqs, w, rng, scale):
        chains, e = ref.chains(read)
        emptied += e
        if fam.endswith("?"):
            if len(chains) <= 8:
                continue
            fam = fam[:-1]
        res.append((fam, read, chains))
    return res, emptied


# ---------------------------------------------------------------------------------------------------------------------------------
# (B) hand-built chains at exact thresholds
# ---------------------------------------------------------------------------------------------------------------------------------
def built_cases(ref, seqs, rng):
    """-> [(family, read, chains)]: chains built by hand at the thresholds of mem_chain2aln (src/bwamem.c:671-706) and of the chain
    groups (c2a_groups.hip), every seed matching the read exactly on the forward strand of one contig"""
    o = ref.opt.contents
    w, a = int(o.w), int(o.a)
    out = []

    def place(ln, c=None, lo=1000):
        c = int(rng.integers(0, len(seqs))) if c is None else c
        p = int(rng.integers(lo, len(seqs[c]) - ln - 1000))
        return c, p

    def seed(c, p, q, ln, sc=None):
        return (ref.contigs[c][0] + p + q, q, ln, a * ln if sc is None else sc)

    # containment with s.len - seedlen0 at floor(.1 l_query) and one more: a long seed first, a longer one inside its region next
    for lq in (100, 150, 151, 250):
        for extra in (0, 1):
            c, p = place(lq)
            read = _clean(seqs[c][p:p + lq], rng)
            read = _sub(read, [lq // 2 - 30, lq // 2 + 40])
            t = int(math.floor(.1 * lq)) + extra
            l1 = 20
            s1 = seed(c, p, lq // 2 - 25, l1, sc=1000)            # visited first (highest score)
            s2 = seed(c, p, lq // 2 - 25, min(l1 + t, 60), sc=900)
            out.append(("thr10", read, [(c, 0.0, [s2, s1])]))
    # the overlap test with t.len at ceil(.95 s.len) and one less: seed s inside an earlier region, t overlapping it on another diagonal
    for sl in (20, 37, 40, 59):
        for extra in (0, -1):
            lq = 150
            c, p = place(lq + 10)
            read = _clean(seqs[c][p:p + lq], rng)
            tl = int(math.ceil(sl * .95)) + extra
            big = seed(c, p, 10, 120, sc=5000)                     # its region covers the read
            s = seed(c, p, 40, sl, sc=100)
            t = (ref.contigs[c][0] + p + 40 + 3, 40 + sl // 4, tl, 200)   # visited between them, 3 bases off s's diagonal, inside s
            out.append(("ceil95", read, [(c, 0.0, [t, s, big])]))
    # qd - rd at +-w and +-(w - 1): a seed inside a region that covers the read, that far off its diagonal (far enough from the read start
    # that cal_max_gap does not bound the band below w)
    for d in (w, w - 1, -w, -(w - 1)):
        qs = w + 10 + max(d, 0)
        while ref.cal_max_gap(qs - max(d, 0)) < w:
            qs += 8
        lq = qs + abs(d) + 40
        c, p = place(lq + 10)
        read = _clean(seqs[c][p:p + lq], rng)
        big = seed(c, p, 0, min(100, lq), sc=10 ** 6)
        s = (ref.contigs[c][0] + p + qs - d, qs, 30, 30 * a)
        out.append(("band_edge", read, [(c, 0.0, [s, big])]))
    # one chain with more than 64 seeds, and a read with <= 8 chains but more than 8 regions (seeds on diagonals 1-3 apart, overlapping
    # on the query)
    for k in range(3):
        lq = 300
        c, p = place(lq + 200)
        read = _clean(seqs[c][p:p + lq], rng)
        sds = []
        for j in range(70 + 10 * k):
            q = (j * 7) % (lq - 25)
            sds.append(seed(c, p, q, 20 + (j % 5)))
        out.append(("many_seeds", read, [(c, 0.0, sds)]))
    for k in range(4):
        lq = 150
        c, p = place(lq + 40)
        read = _clean(seqs[c][p:p + lq], rng)
        chains = []
        for ci in range(2 + k % 2):
            sds = []
            for j in range(10 if ci == 0 else 4):
                q = 5 + 12 * j + 3 * ci
                sds.append((ref.contigs[c][0] + p + q + (j % 3) + ci, q, 30, 30 * a))
            chains.append((c, 0.0, sds))
        out.append(("many_regions", read, chains))
    # chain groups: windows that touch exactly (rmax0 = the previous rmax1) and windows that overlap by one base; every third chain sits
    # inside the one before it, so that a component of several chains holds real cross-chain containment
    for ov in (0, 1, 0, 1):
        lq = 150
        c, p = place(lq + 12000)
        read = _clean(seqs[c][p:p + lq], rng)
        wd = 150 + ref.cal_max_gap(40) + ref.cal_max_gap(60)   # the window of a seed of 50 bases at 40 in a read of 150
        rb = ref.contigs[c][0] + p
        chains = []
        for ci in range(10):
            if ci % 3 == 2:
                chains.append((c, 0.0, [(chains[-1][2][0][0] + 5, 45, 30, 30 * a)]))
                rb = chains[-2][2][0][0] + wd - ov
            else:
                chains.append((c, 0.0, [(rb, 40, 50, 50 * a)]))
                rb += wd - ov
        out.append(("groups_touch", read, chains))
    # a seed at a contig's first base with qbeg > 0 (the left flank meets an empty window), the mirror case on the right, windows of 1-3
    # bases
    for c in range(len(seqs)):
        off, ln = ref.contigs[c]
        for h in (1, 2, 3, 20):
            lq = 120
            read = np.concatenate([rng.integers(0, 4, h).astype(np.uint8), _clean(seqs[c][:lq - h], rng)])
            out.append(("contig_start", read, [(c, 0.0, [(off, h, 40, 40 * a)])]))
            read = np.concatenate([_clean(seqs[c][ln - (lq - h):], rng), rng.integers(0, 4, h).astype(np.uint8)])
            out.append(("contig_end", read, [(c, 0.0, [(off + ln - 40, lq - h - 40, 40, 40 * a)])]))
            for wl in (1, 2, 3):   # a seed wl bases from the contig start: the left window is wl bases
                read = np.concatenate([rng.integers(0, 4, 30).astype(np.uint8), _clean(seqs[c][wl:wl + 90], rng)])
                out.append(("contig_start", read, [(c, 0.0, [(off + wl, 30, 40, 40 * a)])]))
    # drifted chains in a launch of short reads only: the window is longer than c2a_win_cap(max_len)
    for k in range(4):
        lq = 100
        c, p = place(lq + 14000)
        read = _clean(seqs[c][p:p + lq], rng)
        base = ref.contigs[c][0] + p
        sds = [(base + 0, 0, 30, 30 * a), (base + 40 + 1500 * (k + 1), 40, 25, 25 * a), (base + 70 + 3000 * (k + 1), 70, 30, 30 * a)]
        out.append(("drift", read, [(c, 0.0, sds)]))
    for fam, read, chains in out:
        for rid, _, sd in chains:
            for rb, qb, ln, _ in sd:
                assert 0 <= qb and qb + ln <= len(read) and ref.contigs[rid][0] <= rb and rb + ln <= sum(ref.contigs[rid]), (fam, rb, qb, ln)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
def win_cap(max_len):   # c2a_kernel.hip: c2a_win_cap
    return (3 * max_len + 128 + 15) & ~15


def reference_side(ref, cases, alone=True):
    """the reference's regions per case, and coverage counts that say which branches the cases reach"""
    o = ref.opt.contents
    want, cov = [], dict(skipped_seed=0, cross_chain=0, cross_chain_heavy=0, doubled=0, left_local=0, left_to_end=0, right_local=0,
                         right_to_end=0, clamped=0, regs_gt8=0, seeds_gt64=0, win_gt_cap=0, frac_rep=0, reads=len(cases), regions=0)
    cap = win_cap(max(len(r) for _, r, _ in cases))
    for fam, read, chains in cases:
        got = ref.chain2aln(read, chains)
        want.append(got)
        lq = len(read)
        n_seeds = sum(len(sd) for _, _, sd in chains)
        cov["regions"] += len(got)
        cov["skipped_seed"] += len(got) < n_seeds
        if alone and len(chains) > 1:
            per = ref.chain2aln(read, chains, alone=True)
            more = sum(per) > len(got)
            cov["cross_chain"] += more
            cov["cross_chain_heavy"] += more and len(chains) > 8
        cov["doubled"] += int((got["w"] == 2 * o.w).sum())
        cov["left_local"] += int((got["qb"] > 0).sum())
        cov["left_to_end"] += int(((got["qb"] == 0) & (got["seedlen0"] < lq)).sum())
        cov["right_local"] += int((got["qe"] < lq).sum())
        cov["right_to_end"] += int(((got["qe"] == lq) & (got["seedlen0"] < lq)).sum())
        cov["regs_gt8"] += len(got) > 8
        cov["seeds_gt64"] += n_seeds > 64
        cov["frac_rep"] += any(fr > 0 for _, fr, sd in chains if sd)
        for ch in chains:
            if ch[2]:
                (lo, hi), (a, b) = ref.window(lq, ch)
                cov["clamped"] += (a, b) != (max(lo, 0), min(hi, 2 * ref.l_pac))
                cov["win_gt_cap"] += b - a > cap
    return want, cov


def compare(fam_reads, want, got, tag):
    """region lists of the stage against the reference's, field by field -> list of messages (empty: equal)"""
    bad = []
    for i, ((fam, read, chains), w, g) in enumerate(zip(fam_reads, want, got)):
        if len(g) != len(w):
            bad.append("%s read %d (%s, %d chains, %d bases): %d regions, the reference %d" % (tag, i, fam, len(chains), len(read), len(g), len(w)))
            continue
        for k in range(len(w)):
            for f, name in enumerate(FIELDS):
                want_v = int(np.float32(w[name][k]).view(np.uint32)) if name == "frac_rep" else int(w[name][k])
                if int(g[k][f]) != want_v:
                    bad.append("%s read %d (%s, %d chains, %d bases) region %d (seedlen0 %d): %s = %d, the reference %d" %
                               (tag, i, fam, len(chains), len(read), k, int(w["seedlen0"][k]), name, int(g[k][f]), want_v))
                    break
    return bad
