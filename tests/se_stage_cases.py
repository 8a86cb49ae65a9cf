"""Cases of the single-end stage test (se_simple_kernel through mi355x_se_batch, then aln_kernel and the single-end instantiation of
sam_emit_kernel through mi355x_sam_se_batch): single-end reads planted on an index with the helpers of tests/sam_stage_cases.py, every
family built to reach one branch of the decision (tests/test_se_cases.py proves from the reference's own text that it does).

A case is a read (nt4 codes), a name and the read's region list as mem_chain2aln could leave it, BEFORE mem_sort_dedup_patch: the first
region is a true alignment of the read (sam_stage_cases.plant), the others are hits elsewhere that overlap it on the query — what they
align to does not matter as long as they stay secondary or the read is the host's.  `expect` says what the family is built to be:
"plain" (one record without XA / SA: the kernel has to take it), "host" (the kernel must leave it) or None.

The reference's side is its own mem_sort_dedup_patch, mem_mark_primary_se (id = n_processed + i) and mem_reg2sam from
oracle/_ref/libbwaref.so, called the way the single-end branch of worker2 calls them."""
import ctypes as C

import numpy as np

from mpibwa_amd import abi
from oracle import pyoracle as po
from sam_stage_cases import OPTION_SETS, SAM_ROW, Index, parse, plant   # noqa: F401  (re-exported for the tests)

PLAIN_FAMILIES = ("plain", "clip", "lead_del", "trail_del", "none", "below_T", "shadow", "dup", "tie_low", "frac_rep", "lengths", "row")
HOST_FAMILIES = ("xa", "supp", "maxreg", "tie")
FAMILIES = PLAIN_FAMILIES + HOST_FAMILIES
LENGTHS = (30, 63, 64, 65, 150, 300)
ROW_LEN = 800            # reads of the `row` ladder
MAX_LEN = ROW_LEN


def _full(reg, frac_rep=0.0):
    r = dict(reg)
    r.pop("sub", None)
    r.setdefault("seedcov", (r["qe"] - r["qb"]) // 2)
    r.setdefault("seedlen0", 19)
    r["frac_rep"] = frac_rep
    return r


def _elsewhere(ix, rng, like, score, qb=None, qe=None, avoid=()):
    """a hit of `score` on query [qb, qe) (default: the span of `like`) somewhere else: another position, either strand"""
    qb = like["qb"] if qb is None else qb
    qe = like["qe"] if qe is None else qe
    ln = qe - qb
    while True:
        c = int(rng.integers(ix.n_seqs))
        p = ix.off[c] + int(rng.integers(400, ix.len[c] - 400 - ln))
        fwd_like = [like] + list(avoid)
        far = True
        for o in fwd_like:
            s = o["rb"] if o["rb"] < ix.l_pac else 2 * ix.l_pac - o["re"]
            if abs(s - p) < 11000:   # (beyond max_chain_gap: mem_sort_dedup_patch never compares the two)
                far = False
        if far:
            break
    rb, re = (p, p + ln) if rng.integers(2) else (2 * ix.l_pac - p - ln, 2 * ix.l_pac - p)
    return _full(dict(rb=rb, re=re, qb=qb, qe=qe, rid=c, truesc=score, score=score, w=100))


def _name(rng, k):
    return b"s%05d" % k + b":" + bytes(rng.choice(np.frombuffer(b"ACGT0123456789_/", np.uint8), int(rng.integers(0, 12))))


def build_cases(ix, opt, seed):
    """All families on one index -> list of case dicts (not shuffled).  opt: mem_opt_t contents."""
    rng = np.random.default_rng(seed)
    cases = []
    spot = lambda c, room: int(rng.integers(400, ix.len[c] - 400 - room))

    def add(family, tag, read, regs, expect):
        cases.append(dict(family=family, tag=tag, name=_name(rng, len(cases)), read=read, regs=regs, expect=expect))

    def one(length=150, rev=None, frac_rep=0.0, **kw):
        c = int(rng.integers(ix.n_seqs))
        rev = int(rng.integers(2)) if rev is None else rev
        read, reg = plant(ix, rng, opt, c, spot(c, 2 * length + 100) + 50, length, rev, **kw)
        return read, _full(reg, frac_rep)

    for rep in range(60):
        for rev in (0, 1):
            read, reg = one(rev=rev, n_mm=int(rng.integers(0, 4)))
            add("plain", "s%d" % rev, read, [reg], "plain")
    for rep in range(25):
        for cl, cr in ((int(rng.integers(1, 60)), 0), (0, int(rng.integers(1, 60))), (int(rng.integers(1, 40)), int(rng.integers(1, 40)))):
            for rev in (0, 1):
                read, reg = one(rev=rev, cl=cl, cr=cr)
                add("clip", "%d/%d/%d" % (cl > 0, cr > 0, rev), read, [reg], "plain")
    for fam, key in (("lead_del", "lead"), ("trail_del", "trail")):
        for rep in range(25):
            for g in (1, 2, 9):
                for rev in (0, 1):
                    read, reg = one(rev=rev, n_mm=int(rng.integers(0, 3)), **{key: g})
                    add(fam, "g%d/%d" % (g, rev), read, [reg], "plain")
    # none: no region at all; below_T: one or two regions, none of which reaches T
    for rep in range(60):
        L = int(rng.choice([30, 64, 150, 151]))
        add("none", "u", rng.integers(0, 5 if rep % 4 == 0 else 4, L).astype(np.uint8), [], "plain")
    for rep in range(60):
        read, reg = one(score=int(rng.integers(19, opt.T)))
        regs = [reg]
        if rep % 2:
            regs.append(_elsewhere(ix, rng, reg, int(rng.integers(19, opt.T)), qb=10, qe=60))
        add("below_T", "n%d" % len(regs), read, regs, "plain")
    # shadow: a secondary hit far below the primary: XS, a lower MAPQ, no XA
    # (MAPQ leaves 60 only where score - sub is small: a 40-base read whose secondary hit is just outside XA_drop_ratio)
    for rep in range(120):
        if rep % 3 == 0:
            read, reg = one(length=40, n_mm=0)
            sec = _elsewhere(ix, rng, reg, int(reg["score"] * 0.78))
        else:
            read, reg = one()
            sec = _elsewhere(ix, rng, reg, max(20, int(reg["score"] * rng.uniform(0.2, 0.75))), qb=int(rng.integers(0, 30)), qe=150 - int(rng.integers(0, 30)))
        add("shadow", "x", read, [reg, sec] if rep % 2 else [sec, reg], "plain")
    # xa: a secondary hit within XA_drop_ratio of its primary
    for rep in range(80):
        read, reg = one()
        sec = _elsewhere(ix, rng, reg, int(reg["score"] * rng.uniform(0.85, 0.99)))
        add("xa", "x", read, [reg, sec] if rep % 2 else [sec, reg], "host")
    # supp: two primary hits on the two halves of the read
    for rep in range(80):
        h = int(rng.integers(60, 91))
        read, reg = one(cr=150 - h, rev=0) if rep % 2 else one(cl=150 - h, rev=1)   # (either way the aligned part is query [0, h))
        assert (reg["qb"], reg["qe"]) == (0, h)
        other = _elsewhere(ix, rng, reg, (150 - h) * opt.a - 5, qb=h, qe=150)
        add("supp", "h%d" % h, read, [reg, other], "host")
    # maxreg: more regions than the kernel looks at
    for rep in range(60):
        read, reg = one()
        regs = [reg]
        for j in range(int(rng.integers(8, 12))):
            regs.append(_elsewhere(ix, rng, reg, 20 + j, qb=int(rng.integers(0, 40)), qe=int(rng.integers(100, 151)), avoid=regs[1:]))
        add("maxreg", "n%d" % len(regs), read, [regs[i] for i in rng.permutation(len(regs))], "host")
    # dup: two regions at one place (identical, or the same place with a lower score): mem_sort_dedup_patch leaves one
    for rep in range(80):
        read, reg = one()
        twin = dict(reg)
        if rep % 2:
            twin["score"] = twin["truesc"] = reg["score"] - int(rng.integers(1, 30))
        add("dup", "t%d" % (rep % 2), read, [reg, twin] if rep % 4 < 2 else [twin, reg], "plain")
    # tie: two hits of equal score on the same query span (the hash decides which one is primary; the other gets an XA entry);
    # tie_low: two secondary hits of equal score far below the primary (the hash orders them, the record does not change).
    # Neither makes the hash order of the device observable, and no case can: in `tie` the read is the host's (status 11) whichever hit
    # the hash puts first, and for a read the kernel takes, a tie of the primary would put the loser within XA_drop_ratio <= 1 of it
    # (an XA entry: the host's), while the order of tied secondary hits changes nothing in the one record.  The families show that
    # equal scores lead to the right decision, not that hash_64 / id0 are right; those are compared by the end-to-end test, where
    # the host path marks the primary hits of the same chunk's other reads with the same ids.
    for rep in range(80):
        read, reg = one()
        add("tie", "e", read, [reg, _elsewhere(ix, rng, reg, reg["score"])][::1 if rep % 2 else -1], "host")
    for rep in range(80):
        read, reg = one()
        sc2 = max(20, int(reg["score"] * rng.uniform(0.2, 0.7)))
        s1 = _elsewhere(ix, rng, reg, sc2, qb=5, qe=140)
        s2 = _elsewhere(ix, rng, reg, sc2, qb=5, qe=140, avoid=[s1])
        regs = [reg, s1, s2]
        add("tie_low", "e", read, [regs[i] for i in rng.permutation(3)], "plain")
    for rep in range(80):
        read, reg = one(frac_rep=float(rng.choice([0.1, 0.25, 0.5, 0.9])))
        add("frac_rep", "f", read, [reg], "plain")
    for rep in range(10):
        for L in LENGTHS:
            for rev in (0, 1):
                read, reg = one(length=L, rev=rev, n_mm=0 if L <= 65 else 2, n_codes=(rep % 3 == 0) * min(3, L // 40))
                add("lengths", "L%d/%d" % (L, rev), read, [reg], "plain")
    # row: k single-base indels in 800 bases, with and without clips: the short fields (FLAG POS MAPQ CIGAR * 0 0 NM AS XS) pass 260
    # bytes at ~90 operations, most of them with a two-digit length (aln_kernel hands a CIGAR of more than 96 operations to the host, so
    # the ladder has to get there with fewer; measured on the reference's text: 231 .. 299 bytes, 8 to 14 reads at 260 and at 261 bytes with a CIGAR of at most 96 operations)
    for rep in range(45):
        for k in range(42, 51):
            cl, cr = int(rng.choice([0, 0, 12, 105])), int(rng.choice([0, 0, 15]))
            read, reg = one(length=ROW_LEN, k_indel=k, n_mm=0, loss=opt.o_del + 8 * opt.e_del, cl=cl, cr=cr)
            add("row", "k%d" % k, read, [reg], "plain")
    return cases


def random_cases(ix, n_pairs, seed):
    """the ends of pair_cases.adversarial_pairs, each as a single-end read of 150 random bases"""
    from pair_cases import adversarial_pairs
    rng = np.random.default_rng(seed)
    offs = np.array(ix.off + [ix.l_pac])
    out = []
    for k, ends in enumerate(adversarial_pairs(rng, n_pairs, ix.l_pac, offs)):
        for e in range(2):
            regs = [{f: (float(r[f]) if f == "frac_rep" else int(r[f])) for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep")}
                    for r in ends[e]]
            out.append(dict(family="random", tag="r", name=b"a%d_%d" % (k, e), read=rng.integers(0, 4, 150).astype(np.uint8), regs=regs, expect=None))
    return out


def shuffled(cases, seed):
    rng = np.random.default_rng(seed)
    return [cases[i] for i in rng.permutation(len(cases))]


def small_launch(cases, n, seed):
    """n reads, one of every family as far as they go"""
    rng = np.random.default_rng(seed)
    by_fam = {}
    for cs in cases:
        by_fam.setdefault(cs["family"], []).append(cs)
    fams = [f for f in FAMILIES if f in by_fam]
    return [by_fam[fams[(seed + j) % len(fams)]][int(rng.integers(len(by_fam[fams[(seed + j) % len(fams)]])))] for j in range(n)]


def _qual(n, k):
    return (33 + (np.arange(n) * 7 + k) % 41).astype(np.uint8).tobytes()


def read_inputs(order, with_qual):
    """reads, qualities and names as Engine.sam_records_se and the reference take them"""
    return dict(reads=[cs["read"] for cs in order], quals=[_qual(len(cs["read"]), k) for k, cs in enumerate(order)] if with_qual else None,
                names=[cs["name"] for cs in order])


def device_regions(order, reg_dt, maxreg):
    """the inputs of Engine.singles: the first maxreg regions of every read and the true region counts"""
    regs = np.zeros((len(order), maxreg), dtype=reg_dt)
    n_regs = np.zeros(len(order), dtype=np.int32)
    for i, cs in enumerate(order):
        n_regs[i] = len(cs["regs"])
        for j, r in enumerate(cs["regs"][:maxreg]):
            for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep"):
                regs[i, j][f] = r[f]
    return regs, n_regs


def reference_side(ref, ropt, order, with_qual, n_processed=0):
    """per read of `order`: (the reference's text, its region list after mem_sort_dedup_patch and mem_mark_primary_se as ALNREG_DT)"""
    R = ref.lib
    P = C.POINTER
    R.mem_sort_dedup_patch.restype = C.c_int
    R.mem_sort_dedup_patch.argtypes = [P(abi.mem_opt_t), P(abi.bntseq_t), P(C.c_uint8), C.c_void_p, C.c_int, C.c_void_p]
    R.mem_mark_primary_se.restype = C.c_int
    R.mem_mark_primary_se.argtypes = [P(abi.mem_opt_t), C.c_int, C.c_void_p, C.c_int64]
    R.mem_reg2sam.restype = None
    R.mem_reg2sam.argtypes = [P(abi.mem_opt_t), P(abi.bntseq_t), P(C.c_uint8), P(abi.bseq1_t), P(po._alnreg_v), C.c_int, C.c_void_p]
    libc = po.libc
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    inp = read_inputs(order, with_qual)
    out = []
    for i, cs in enumerate(order):
        a = np.zeros(len(cs["regs"]), dtype=po.ALNREG_DT)
        for j, r in enumerate(cs["regs"]):
            for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep"):
                a[j][f] = r[f]
            a[j]["secondary"] = a[j]["secondary_all"] = -1
        sq = np.ascontiguousarray(cs["read"], dtype=np.uint8)
        p = libc.malloc(max(1, a.nbytes))   # (mem_sort_dedup_patch may realloc nothing, but mem_reg2sam's callers own a malloc'ed list)
        C.memmove(p, a.ctypes.data, a.nbytes)
        v = po._alnreg_v(len(a), len(a), p)
        v.n = R.mem_sort_dedup_patch(ropt, ref.bns, ref.pac, sq.ctypes.data, v.n, v.a)
        R.mem_mark_primary_se(ropt, v.n, v.a, n_processed + i)
        after = np.zeros(v.n, dtype=po.ALNREG_DT)
        if v.n:
            C.memmove(after.ctypes.data, v.a, after.nbytes)
        nm = C.create_string_buffer(bytes(cs["name"]))
        ql = C.create_string_buffer(bytes(inp["quals"][i])) if with_qual else None
        s = abi.bseq1_t()
        s.l_seq = len(sq); s.name = C.addressof(nm); s.seq = sq.ctypes.data; s.qual = C.addressof(ql) if ql is not None else None
        R.mem_reg2sam(ropt, ref.bns, ref.pac, C.byref(s), C.byref(v), 0, None)
        out.append((C.string_at(s.sam), after))
        libc.free(C.c_void_p(s.sam))
        libc.free(C.c_void_p(v.a))
    return out


def is_plain(text):
    """one line, neither XA nor SA: the kind of record the device may write"""
    return text.count(b"\n") == 1 and b"\tXA:Z:" not in text and b"\tSA:Z:" not in text


def the_line(ropt, text, after):
    """what the reference's single line says: (region or None for the unmapped record, flag without the strand bit, MAPQ, AS, XS)"""
    P = parse(text)
    f = P["fields"]
    xs = int(P["tags"][b"XS"]) if b"XS" in P["tags"] else -1
    if P["flag"] & 4:
        return None, P["flag"], int(f[4]), int(P["tags"][b"AS"]), xs
    pri = [r for r in after if r["secondary"] < 0 and r["score"] >= ropt.T]
    assert len(pri) == 1
    return pri[0], P["flag"] & ~0x10, int(f[4]), int(P["tags"][b"AS"]), xs
