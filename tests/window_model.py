"""The reference window of mem_chain2aln (src/bwamem.c:621-628, 642-661) in exact Python integers: a model shared by the stage tests of
c2a (tests/c2a_cases.py), of the chaining stage (test_gpu_chain_options.py, test_gpu_chain_heavy_classes.py, test_host_chain.py,
test_chain_option_cases.py) and by the test of mpibwa_amd/csrc/chainmath.h (test_chainmath.py)."""


def cal_max_gap(o, qlen):   # src/bwamem.c:621-628; o: a, o_del, e_del, o_ins, e_ins, w
    l_del = int((qlen * o.a - o.o_del) / o.e_del + 1.)
    l_ins = int((qlen * o.a - o.o_ins) / o.e_ins + 1.)
    return min(max(l_del, l_ins, 1), o.w << 1)


def strand_span(l_pac, off, ln, is_rev):
    """a contig on the strand of a chain, in the doubled coordinate (bns_fetch_seq, src/bntseq.c:413-418)"""
    return (2 * l_pac - off - ln, 2 * l_pac - off) if is_rev else (off, off + ln)


def seed_reach(rb, qb, ln, lq, gap):   # :646-655 for one seed
    return rb - (qb + gap(qb)), rb + ln + (lq - qb - ln) + gap(lq - qb - ln)


def clamp(l_pac, lo, hi, first_r, far_beg, far_end):
    """:656-661 and bns_fetch_seq's clamp to the contig -> (rmax0, rmax1)"""
    a, b = max(lo, 0), min(hi, 2 * l_pac)
    if a < l_pac < b:
        if first_r < l_pac:
            b = l_pac
        else:
            a = l_pac
    return max(a, far_beg), min(b, far_end)


def chain_window(l_pac, contigs, gap, lq, rid, seeds):
    """contigs: [(offset, len)]; gap(q): cal_max_gap; seeds: [(rbeg, qbeg, len, ...)] in the chain's order
    -> ((lo, hi) before clamping, (far_beg, far_end), (rmax0, rmax1))"""
    reach = [seed_reach(s[0], s[1], s[2], lq, gap) for s in seeds]
    lo, hi = min(b for b, _ in reach), max(e for _, e in reach)
    fb, fe = strand_span(l_pac, contigs[rid][0], contigs[rid][1], seeds[0][0] >= l_pac)
    return (lo, hi), (fb, fe), clamp(l_pac, lo, hi, seeds[0][0], fb, fe)


class ChainWindows:
    """(far_beg, far_end, rmax0, rmax1) of the reference's chains under one option set, for the chaining stage tests"""

    def __init__(self, bns, opt):
        b = bns.contents
        self.l_pac = int(b.l_pac)
        self.contigs = [(int(b.anns[i].offset), int(b.anns[i].len)) for i in range(b.n_seqs)]
        self.o = opt.contents
        self._gap = {}

    def gap(self, q):
        if q not in self._gap:
            self._gap[q] = cal_max_gap(self.o, q)
        return self._gap[q]

    def of(self, lq, rid, seeds):
        _, far, rmax = chain_window(self.l_pac, self.contigs, self.gap, lq, rid, seeds)
        return far + rmax

    def check(self, lens, want, got, what):
        """got: per read the stage's chains (rid, far_beg, far_end, rmax0, rmax1, frac_bits, seeds), already shown to be the reference's
        chains `want` (rid, frac_bits, seeds) in its order: the four window fields of every chain are the model's"""
        for k, (lq, w, g) in enumerate(zip(lens, want, got)):
            assert len(g) == len(w), (what, k)
            for j, ((rid, _, seeds), c) in enumerate(zip(w, g)):
                assert tuple(c[1:5]) == self.of(lq, rid, seeds), (what, "read", k, "chain", j, c[:5], self.of(lq, rid, seeds))

    def clamps(self, lq, rid, seeds):
        """-> (the window is cut at a contig edge, at the strand boundary)"""
        (lo, hi), (fb, fe), _ = chain_window(self.l_pac, self.contigs, self.gap, lq, rid, seeds)
        a, b = max(lo, 0), min(hi, 2 * self.l_pac)
        return lo < fb or hi > fe, a < self.l_pac < b
