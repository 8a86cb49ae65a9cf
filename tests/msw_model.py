"""The recurrence of the header comment of mpibwa_amd/csrc/msw_kernel.hip in plain Python: what msw_pass, msw2_kernel's forward pass and
the second pass (the b[] rule, the reverse pass with its stop score) compute for one request, cell by cell, without lanes, quads or LDS.

It is there to say where the closed form — two F values per cell, Fseg restarting at every segment border of the striped layout and
Ffull never — equals what Farrar's striped loop leaves behind and where it does not (tests/test_msw_model.py): it does for every gap
penalty with o_ins > 0 and does not for o_ins = 0, where the reference's lazy-F loop ends after the first position of every segment
(its exit test `f - e_ins <= max(h, f) - (o_ins + e_ins)` is always true) and a carry across a border raises only that position while
Ffull carries it on.  The expected results of every test still come from the reference's own ksw_align2."""
PAD = 7


def _pass(codes, slen, target, mat, o_del, e_del, o_ins, e_ins, endsc, rows=None):
    """codes: the query padded to slen * P positions (PAD scores 0 against everything); target: the rows in the order they are read.
    -> (score, te, qe); rows: the row maxima are appended"""
    n = len(codes)
    oe_del, oe_ins = o_del + e_del, o_ins + e_ins
    H, E = [0] * n, [0] * n
    gmax, te, qe = 0, -1, -1
    for i, t in enumerate(target):
        srow = [mat[t * 5 + c] if c < 5 else 0 for c in range(8)]
        diag = fseg = ffull = 0
        imax, ipos = 0, -1
        for k in range(n):
            e = E[k]
            h = max(diag + srow[codes[k]], e, fseg)          # Hpre(i, k)
            if h > imax or ipos < 0:
                imax, ipos = h, k
            diag = H[k]
            H[k] = max(h, ffull)                             # H(i, k) after the lazy-F pass
            E[k] = max(e - e_del, h - oe_del, 0)
            fseg = max(fseg - e_ins, h - oe_ins, 0)
            ffull = max(ffull - e_ins, h - oe_ins, 0)
            if (k + 1) % slen == 0:
                fseg = 0
        if rows is not None:
            rows.append(imax)
        if imax > gmax:
            gmax, te, qe = imax, i, ipos
            if gmax >= endsc:
                break
    return gmax, te, qe


def _padded(q, P):
    slen = (len(q) + P - 1) // P
    return [min(int(c), 4) for c in q] + [PAD] * (slen * P - len(q)), slen


def align2(q, target, mat, a, o_del, e_del, o_ins, e_ins, min_seed_len):
    """ksw_align2 as mem_matesw calls it (KSW_XSUBO | KSW_XSTART | min_seed_len * a, KSW_XBYTE when qlen * a < 250), by the kernels'
    recurrence -> [score, te, qe, score2, te2, tb, qb], or None where the byte flavour would reach its ceiling"""
    mat = [int(v) for v in mat]
    P = 16 if len(q) * a < 250 else 8
    shift, max_sc = max(-min(mat), 0), max(max(mat), 1)
    sat_limit = 255 - shift if P == 16 else 0x10000
    minsc = min_seed_len * a
    target = [int(t) for t in target]
    codes, slen = _padded(q, P)
    rows = []
    score, te, qe = _pass(codes, slen, target, mat, o_del, e_del, o_ins, e_ins, 0x10000, rows)
    if score >= sat_limit:
        return None
    out = [score, te, qe, -1, -1, -1, -1]
    if score < minsc or te < 0:
        return out
    # b[]: runs of rows that reach minsc, a run's entry is its first best row; a row continues the run whose ENTRY is the row before
    d = (score + max_sc - 1) // max_sc
    b = []
    for i, im in enumerate(rows):
        if im < minsc:
            continue
        if not b or b[-1][1] + 1 != i:
            b.append([im, i])
        elif b[-1][0] < im:
            b[-1] = [im, i]
    for im, i in b:
        if (i < te - d or i > te + d) and im > out[3]:
            out[3], out[4] = im, i
    # the reverse pass over the reversed prefixes, until the forward score is reached
    codes2, slen2 = _padded(list(q[:qe + 1])[::-1], P)
    g, gte, gqe = _pass(codes2, slen2, target[:te + 1][::-1], mat, o_del, e_del, o_ins, e_ins, score)
    if g >= sat_limit:
        return None
    if g == score:
        out[5], out[6] = te - gte, qe - gqe
    return out
