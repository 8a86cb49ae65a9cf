"""The band mem_reg2aln starts its global alignment with (src/bwamem.c:792-800, 1094-1099), restated once for the stage tests: the
pairing test checks the kernel's CIGAR requests against it, the SAM stage test builds its requests with it, so that the device and
the reference align with the same band."""


def infer_bw(l1, l2, score, a, q, r):   # src/bwamem.c:792-800
    if l1 == l2 and l1 * a - score < (q + r - a) << 1:
        return 0
    w = int(float((l1 if l1 < l2 else l2) * a - score - q) / r + 2.)
    return max(w, abs(l1 - l2))


def reg2aln_band(opt, l_query, l_ref, truesc, w_reg):
    """opt: mem_opt_t (contents); the first band of mem_reg2aln's loop for a region of l_query x l_ref with local score truesc and band w_reg"""
    w2 = max(infer_bw(l_query, l_ref, truesc, opt.a, opt.o_del, opt.e_del), infer_bw(l_query, l_ref, truesc, opt.a, opt.o_ins, opt.e_ins))
    if w2 > opt.w:
        w2 = min(w2, w_reg)
    return w2
