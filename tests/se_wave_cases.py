"""Single-end reads for se_wave_kernel (mpibwa_amd/csrc/se_wave_kernel.hip) and what the reference alone makes of them, for the stage test
(tests/test_gpu_se_wave_stage.py), the end-to-end test (tests/test_gpu_se_wave_e2e.py) and their CPU companion
(tests/test_se_wave_cases.py).

(a) Realistic reads.  The index and the pairs are those of tests/pair_wave_cases.py (build_index, make_reads clean and damaged); every
mate is taken as a single-end read: both mates of the clean pairs, and the damaged mate 2 of every second pair (the other reads of the
damaged set are the clean ones again).  The regions are the reference's own mem_align1_core (which ends in its mem_sort_dedup_patch),
then its mem_mark_primary_se with id = n_processed + read number and its mem_reg2sam, the way the single-end branch of worker2 calls
them.  A read is ELIGIBLE, from the reference alone, when its list holds at most 64 regions, its text is one line without SA:Z / pa:f,
and an XA tag, if there is one, has at most PW_XA_CAP = 8 entries.  Eligible reads divide into "plain_gt8" (no XA, more than eight
regions), "xa" and "rest".

(b) Synthetic families on the session genome, built with the helpers of tests/se_stage_cases.py / tests/sam_stage_cases.py: a read
planted at a place of the genome (its first region is a true alignment) and hits elsewhere on the same query span, which stay secondary
(what they align to does not matter).  `expect` says what the family is built to be: "plain" (status 1), "xa" (status 16 with the tag
the reference writes; 11 where the call has no XA listing), or the status code that leaves the read to the host.  The lists go through
the reference's own mem_sort_dedup_patch first: what the device is handed is the reference's list between that and
mem_mark_primary_se.

  n0 n1 n2 n8 n9 n63 n64   exactly that many regions, one primary at or above T             plain
  n65                      65 regions                                                        13
  all_below_T              9 .. 30 regions, none reaches T                                   plain (the unmapped record)
  xa_k, k = 1 .. M         k secondaries within XA_drop_ratio (M = max_XA_hits)              xa, k entries in list order
  xa_over                  M + 1 of them                                                     plain, no tag
  xa_edge                  120 and 121 under a primary of 150 at the ratio 0.8f              xa, one entry: the hit of 121
  xa_under_other           close hits whose parent is a primary below T; a hit close to a
                           secondary hit but not to the primary                              plain
  tie                      two hits of equal score on one span                               xa, one entry: the hash says which
  supp                     two primary hits on the two halves of the read                    10
  long                     a region beyond the per-length table                              5
  alt (genome_alt)         a region on an ALT contig                                         6
"""
import ctypes as C

import numpy as np

from mpibwa_amd import abi
from oracle import pyoracle as po

import pair_wave_cases as pw
import se_stage_cases as sec
from c2a_cases import _alnreg_v, _ref_handle, _regs_copy
from se_stage_cases import Index, parse, plant   # noqa: F401  (re-exported for the tests)

PW_MAXREG = 64
PW_XA_CAP = 8
XA_STAGE = 64                 # bytes of ",+-pos,CIGAR,NM;" sam_emit_kernel stages per XA entry
SAM_ROW = sec.SAM_ROW
SE_DECIDED, SE_HOST_LENGTH, SE_HOST_ALT, SE_HOST_SUPP, SE_HOST_XA, SE_HOST_FULL, SE_HOST_TIE, SE_DECIDED_XA = 1, 5, 6, 10, 11, 13, 14, 16

OPTION_SETS = dict(sec.OPTION_SETS)           # name -> (mem_opt_t fields, with qualities, @RG line)
OPTION_SETS["xa8"] = (dict(max_XA_hits=8), True, None)     # the cap of the kernel's side array itself
OPTION_SETS["xa9"] = (dict(max_XA_hits=9), True, None)     # beyond it: no listing, XA reads get 11, plain long lists are still taken

FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep")
_ASCII = np.frombuffer(b"ACGTN", dtype=np.uint8)


# ---- (a) ----
def realistic_cases(g):
    """g: pair_wave_cases.build_index's dict -> list of case dicts (name, read)"""
    clean = pw.make_reads(g["seqs"], g["copies"], False)
    damaged = pw.make_reads(g["seqs"], g["copies"], True)
    out = []
    for k, (name, a, b) in enumerate(clean):
        out.append(dict(family="real", tag="m1", name=("%s_1" % name).encode(), read=np.ascontiguousarray(a, dtype=np.uint8), expect=None))
        out.append(dict(family="real", tag="m2", name=("%s_2" % name).encode(), read=np.ascontiguousarray(b, dtype=np.uint8), expect=None))
    for k, (name, a, b) in enumerate(damaged):
        if k % 2:
            out.append(dict(family="real", tag="m2d", name=("%s_2d" % name).encode(), read=np.ascontiguousarray(b, dtype=np.uint8), expect=None))
    return out


# ---- (b) ----
def _spread(ix, rng, like, scores, avoid=()):
    """hits of the given scores on the query span of `like`, at places of their own 400 bases apart and away from `like` and `avoid`:
    mem_sort_dedup_patch finds no two of them redundant (no overlap on the reference) and patches none (equal query starts)"""
    ln = like["qe"] - like["qb"]
    taken = set()
    for o in [like] + list(avoid):
        s = o["rb"] if o["rb"] < ix.l_pac else 2 * ix.l_pac - o["re"]
        for d in (-1, 0, 1, 2, 3):
            taken.add(s // 400 + d)
    out = []
    for sc in scores:
        while True:
            c = int(rng.integers(ix.n_seqs))
            slot = (ix.off[c] + int(rng.integers(400, ix.len[c] - 800 - ln))) // 400
            if slot not in taken and slot * 400 >= ix.off[c] + 400 and slot * 400 + ln + 400 < ix.off[c] + ix.len[c]:
                break
        taken.add(slot)
        p = slot * 400
        rb, re = (p, p + ln) if rng.integers(2) else (2 * ix.l_pac - p - ln, 2 * ix.l_pac - p)
        out.append(sec._full(dict(rb=rb, re=re, qb=like["qb"], qe=like["qe"], rid=c, truesc=int(sc), score=int(sc), w=100)))
    return out


def n_xa_max(opt):
    return min(int(opt.max_XA_hits), int(opt.max_XA_hits_alt))


def build_cases(ix, opt, seed):
    """The families on the session genome -> list of case dicts (not shuffled).  opt: mem_opt_t contents."""
    rng = np.random.default_rng(seed)
    cases = []
    spot = lambda c, room: int(rng.integers(400, ix.len[c] - 400 - room))
    M = n_xa_max(opt)

    def add(family, tag, read, regs, expect, **kw):
        cases.append(dict(family=family, tag=tag, name=sec._name(rng, len(cases)), read=read, regs=regs, expect=expect, **kw))

    def one(length=150, rev=None, **kw):
        c = int(rng.integers(ix.n_seqs))
        rev = int(rng.integers(2)) if rev is None else rev
        read, reg = plant(ix, rng, opt, c, spot(c, 2 * length + 100) + 50, length, rev, **kw)
        return read, sec._full(reg)

    def mixed(regs):
        return [regs[i] for i in rng.permutation(len(regs))]

    for k, reps in ((0, 6), (1, 6), (2, 6), (8, 6), (9, 8), (63, 4), (64, 4)):
        for rep in range(reps):
            if k == 0:
                add("n0", "n0", rng.integers(0, 4, 150).astype(np.uint8), [], "plain", n_after=0)
                continue
            read, reg = one(n_mm=int(rng.integers(0, 3)))
            low = _spread(ix, rng, reg, [int(rng.integers(19, max(20, int(reg["score"] * 0.6)))) for _ in range(k - 1)])
            add("n%d" % k, "n%d" % k, read, mixed([reg] + low), "plain", n_after=k)
    for rep in range(4):
        read, reg = one()
        low = _spread(ix, rng, reg, [int(rng.integers(19, max(20, int(reg["score"] * 0.6)))) for _ in range(64)])
        add("n65", "n65", read, mixed([reg] + low), SE_HOST_FULL, n_after=65)
    for rep in range(10):
        k = int(rng.integers(9, 31)) if rep > 1 else (9, 30)[rep]
        read, reg = one(score=int(rng.integers(19, opt.T)))
        low = _spread(ix, rng, reg, [int(rng.integers(19, opt.T)) for _ in range(k - 1)])
        add("all_below_T", "b%d" % k, read, mixed([reg] + low), "plain", n_after=k)
    for k in range(1, M + 2):
        for rep in range(4):
            read, reg = one(n_mm=0)
            S = reg["score"]
            close = _spread(ix, rng, reg, [int(rng.integers(int(S * 0.85), S)) for _ in range(k)])
            low = _spread(ix, rng, reg, [int(S * 0.3) + j for j in range(int(rng.integers(0, 9)))], avoid=close)
            fam = "xa_over" if k == M + 1 else "xa_%d" % k
            add(fam, fam, read, mixed([reg] + close + low), "plain" if k == M + 1 else "xa", n_xa=0 if k == M + 1 else k)
    for rep in range(6):
        read, reg = one(n_mm=0, score=150)
        two = _spread(ix, rng, reg, [120, 121])
        low = _spread(ix, rng, reg, [int(rng.integers(20, 100)) for _ in range(int(rng.integers(0, 8)))], avoid=two)
        add("xa_edge", "e", read, mixed([reg] + two + low), "xa", n_xa=1, xa_scores=[121])
    for rep in range(12):
        if rep % 2 == 0:   # a primary below T on the other half of the read, and hits close to it under it
            h = int(rng.integers(80, 101))
            read, reg = one(cr=150 - h, rev=0) if rep % 4 else one(cl=150 - h, rev=1)   # (either way the aligned part is query [0, h))
            assert (reg["qb"], reg["qe"]) == (0, h)
            b_sc = opt.T - 2
            other = sec._elsewhere(ix, rng, reg, b_sc, qb=h, qe=150)
            under = _spread(ix, rng, other, [b_sc - 1, b_sc - 2, b_sc - 2], avoid=[reg])
            add("xa_under_other", "below_T", read, mixed([reg, other] + under), "plain", n_xa=0)
        else:              # a hit close to a secondary hit, far from the primary
            read, reg = one(n_mm=0)
            S = reg["score"]
            chain = _spread(ix, rng, reg, [int(S * 0.66), int(S * 0.6), int(S * 0.55)])
            add("xa_under_other", "secondary", read, mixed([reg] + chain), "plain", n_xa=0)
    for rep in range(40):
        read, reg = one()
        twin = _spread(ix, rng, reg, [reg["score"]])
        low = _spread(ix, rng, reg, [int(reg["score"] * 0.4)] * int(rng.integers(0, 3)), avoid=twin)
        add("tie", "t", read, ([reg] + twin if rep % 2 else twin + [reg]) + low, "xa", n_xa=1)
    for rep in range(12):
        h = int(rng.integers(60, 91))
        read, reg = one(cr=150 - h, rev=0) if rep % 2 else one(cl=150 - h, rev=1)
        assert (reg["qb"], reg["qe"]) == (0, h)
        other = sec._elsewhere(ix, rng, reg, (150 - h) * opt.a - 5, qb=h, qe=150)
        low = _spread(ix, rng, reg, [20 + j for j in range(int(rng.integers(0, 10)))], avoid=[other])
        add("supp", "h%d" % h, read, mixed([reg, other] + low), SE_HOST_SUPP)
    for rep in range(6):   # a reference span of 4 * 150 + 256 bases and more (the table of a launch whose longest read has 150 bases)
        read, reg = one()
        span = 4 * 150 + 256 + int(rng.integers(0, 40))
        while True:
            c = int(rng.integers(ix.n_seqs))
            p = ix.off[c] + int(rng.integers(2000, ix.len[c] - 4000))
            s = reg["rb"] if reg["rb"] < ix.l_pac else 2 * ix.l_pac - reg["re"]
            if abs(s - p) > 12000:
                break
        rb, re = (p, p + span) if rep % 2 else (2 * ix.l_pac - p - span, 2 * ix.l_pac - p)
        far = sec._full(dict(rb=rb, re=re, qb=reg["qb"], qe=reg["qe"], rid=c, truesc=40, score=40, w=100))
        add("long", "l", read, mixed([reg, far]), SE_HOST_LENGTH)
    return cases


def build_alt_cases(ix, is_alt, opt, seed):
    """`alt` on the genome with ALT contigs: a read of a primary contig with a secondary hit on an ALT contig"""
    rng = np.random.default_rng(seed)
    pri = [c for c in range(ix.n_seqs) if not is_alt[c]]
    alt = [c for c in range(ix.n_seqs) if is_alt[c]]
    assert pri and alt
    cases = []
    for rep in range(8):
        c = pri[int(rng.integers(len(pri)))]
        read, reg = plant(ix, rng, opt, c, int(rng.integers(400, ix.len[c] - 800)), 150, int(rng.integers(2)))
        reg = sec._full(reg)
        ca = alt[int(rng.integers(len(alt)))]
        p = ix.off[ca] + int(rng.integers(200, ix.len[ca] - 400))
        hit = sec._full(dict(rb=p, re=p + 150, qb=0, qe=150, rid=ca, truesc=50, score=50, w=100))
        low = _spread(ix, rng, reg, [20 + j for j in range(int(rng.integers(0, 10)))], avoid=[hit])
        regs = [reg, hit] + [r for r in low if not is_alt[r["rid"]]]
        cases.append(dict(family="alt", tag="a", name=sec._name(rng, rep), read=read, regs=regs, expect=SE_HOST_ALT))
    return cases


def shuffled(cases, seed):
    return sec.shuffled(cases, seed)


def read_numbers(n, seed):
    """read numbers in the chunk that are not 0 .. n-1: ascending, with gaps"""
    rng = np.random.default_rng(seed)
    return (17 + np.cumsum(rng.integers(1, 5, n))).astype(np.int32)


def quality(n, k):
    return sec._qual(n, k)


# ---- the reference's side ----
def reference_side(ref, ropt, cases, with_qual, n_processed, read_no):
    """Per case: cs["before"] = the read's list after mem_sort_dedup_patch (ALNREG_DT: what the device is handed), and
    -> [(the reference's text, the list after mem_mark_primary_se)].  A case with "regs" (synthetic) starts from that list and the
    reference's mem_sort_dedup_patch, one without from its mem_align1_core on the read."""
    R = _ref_handle()
    P = C.POINTER
    R.mem_align1_core.restype = _alnreg_v
    R.mem_align1_core.argtypes = [P(abi.mem_opt_t), P(abi.bwt_t), P(abi.bntseq_t), P(C.c_uint8), C.c_int, C.c_char_p, C.c_void_p]
    R.mem_sort_dedup_patch.restype = C.c_int
    R.mem_sort_dedup_patch.argtypes = [P(abi.mem_opt_t), P(abi.bntseq_t), P(C.c_uint8), C.c_void_p, C.c_int, C.c_void_p]
    R.mem_mark_primary_se.restype = C.c_int
    R.mem_mark_primary_se.argtypes = [P(abi.mem_opt_t), C.c_int, C.c_void_p, C.c_int64]
    R.mem_reg2sam.restype = None
    R.mem_reg2sam.argtypes = [P(abi.mem_opt_t), P(abi.bntseq_t), P(C.c_uint8), P(abi.bseq1_t), P(_alnreg_v), C.c_int, C.c_void_p]
    libc = po.libc
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    out = []
    for i, cs in enumerate(cases):
        codes = np.ascontiguousarray(cs["read"], dtype=np.uint8)
        if "regs" in cs:
            a = np.zeros(len(cs["regs"]), dtype=po.ALNREG_DT)
            for j, r in enumerate(cs["regs"]):
                for f in FIELDS:
                    a[j][f] = r[f]
                a[j]["secondary"] = a[j]["secondary_all"] = -1
            p = libc.malloc(max(1, a.nbytes))
            C.memmove(p, a.ctypes.data, a.nbytes)
            v = _alnreg_v(len(a), len(a), p)
            v.n = R.mem_sort_dedup_patch(ropt, ref.bns, ref.pac, codes.ctypes.data, v.n, v.a)
            seq_ptr, keep = codes.ctypes.data, codes
        else:
            keep = C.create_string_buffer(_ASCII[codes].tobytes(), len(codes) + 1)   # ASCII in, nt4 codes out (src/bwamem.c:1057-1058)
            v = R.mem_align1_core(ropt, ref.bwt, ref.bns, ref.pac, len(codes), keep, None)
            seq_ptr = C.addressof(keep)
        cs["before"] = _regs_copy(v)
        R.mem_mark_primary_se(ropt, v.n, v.a, int(n_processed) + int(read_no[i]))
        after = _regs_copy(v)
        nm = C.create_string_buffer(bytes(cs["name"]))
        ql = C.create_string_buffer(bytes(quality(len(codes), i))) if with_qual else None
        s = abi.bseq1_t()
        s.l_seq = len(codes); s.name = C.addressof(nm); s.seq = seq_ptr; s.qual = C.addressof(ql) if ql is not None else None
        R.mem_reg2sam(ropt, ref.bns, ref.pac, C.byref(s), C.byref(v), 0, None)
        out.append((C.string_at(s.sam), after))
        libc.free(C.c_void_p(s.sam))
        libc.free(C.c_void_p(v.a))
    return out


def xa_entries(text):
    """the entries of the record's XA tag as (contig name, strand, position, CIGAR, NM) — empty without a tag"""
    if b"\tXA:Z:" not in text:
        return []
    tag = text[:-1].split(b"\tXA:Z:")[1].split(b"\t")[0]
    out = []
    for e in tag.split(b";")[:-1]:
        name, pos, cig, nm = e.rsplit(b",", 3)
        out.append((name, pos[:1], int(pos[1:]), cig, int(nm)))
    return out


def without_xa(text):
    """the record without its XA tag (the last tag of a line): what sam_emit_kernel stages in its row"""
    return text[:-1].split(b"\tXA:Z:")[0] + b"\n" if b"\tXA:Z:" in text else text


def xa_entry_bytes(entry):
    """the bytes of an entry sam_emit_kernel stages: ",+-pos,CIGAR,NM;" """
    name, strand, pos, cig, nm = entry
    return len(b",%s%d,%s,%d;" % (strand, pos, cig, nm))


def eligible(cs, text):
    """from the reference alone: at most 64 regions, one line without SA / pa, an XA tag of at most PW_XA_CAP entries"""
    if len(cs["before"]) > PW_MAXREG or text.count(b"\n") != 1 or b"\tSA:Z:" in text or b"\tpa:f:" in text:
        return False
    return len(xa_entries(text)) <= PW_XA_CAP


def klass(cs, text):
    """of an eligible read: "xa", "plain_gt8" or "rest" """
    if xa_entries(text):
        return "xa"
    return "plain_gt8" if len(cs["before"]) > 8 else "rest"


def census(cases, want):
    c = dict(reads=len(cases), eligible=0, plain_gt8=0, xa=0, rest=0, unmapped=0, gt64=0, lines2=0, xa_over_cap=0)
    for k in range(1, PW_XA_CAP + 1):
        c["xa_%d" % k] = 0
    for cs, (text, after) in zip(cases, want):
        if len(cs["before"]) > PW_MAXREG:
            c["gt64"] += 1
        if text.count(b"\n") != 1:
            c["lines2"] += 1
        if len(xa_entries(text)) > PW_XA_CAP:
            c["xa_over_cap"] += 1
        if not eligible(cs, text):
            continue
        c["eligible"] += 1
        c[klass(cs, text)] += 1
        c["unmapped"] += bool(int(text.split(b"\t")[1]) & 4)
        if xa_entries(text):
            c["xa_%d" % len(xa_entries(text))] += 1
    return c


def device_lists(cases, reg_dt):
    """the inputs of Engine.singles_wave: per read its list after mem_sort_dedup_patch"""
    out = []
    for cs in cases:
        a = np.zeros(len(cs["before"]), dtype=reg_dt)
        for f in FIELDS:
            a[f] = cs["before"][f]
        out.append(a)
    return out
