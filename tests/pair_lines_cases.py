"""Pairs that mem_sam_pe reports end by end through no_pairing: (src/bwamem_pair.c:371-392) — an unmapped end, two unmapped ends, no pair
of hits in a proper orientation and distance, a best pair that scores nothing, a chimeric end — and what the reference alone makes of
them, for the stage test of pair_wave_kernel's no_pairing tail and of the paired instantiation of sam_lines_kernel
(tests/test_gpu_pair_lines_stage.py) and their CPU companion (tests/test_pair_lines_cases.py).  Everything lives on the index of
tests/pair_wave_cases.py, which is imported and left alone, as are tests/supp_cases.py and tests/test_sampost.py.

(a) test_sampost._pairs_of_every_kind(g, n=360, seed=40): ordinary pairs, mates from two places, one or two random mates, chimeric mates
with and without a mapping partner.

(b) The chimeric reads of 150 bases of supp_cases.realistic_cases(g) (2, 3 and 4 segments; the 250-base class is left out, and so is the
one read of the 270 in the three 150-base classes that its indels left 149 bases long: 269 reads) as one end.  rng = default_rng(97); the
other end by k % 4: 0 or 3 — 150 clean bases cut from a random place; 1 — 150 random bases; 2 — the next chimera, reverse-complemented.
The ends are swapped when k % 8 >= 4.  The pairs are appended to simulate_reads(seqs, 400, 150, paired=True, seed=98, frac_random=0.0),
so that mem_pestat has its pairs.

(c) Hand-built pairs whose lists are planted (supp_cases._segments, se_stage_cases.plant: every region is a true alignment) and go
through the reference's own mem_sort_dedup_patch; the insert-size statistics are those of set (a).  `expect`: 17 (PW_DECIDED_LINES), or
the code that leaves the pair to the host.
  five            five lines on one end                                                                          10
  two_lines       80 + 70 against a mate of one line elsewhere (the pair -M is looked at on)                      17
  cap_mapq        80 + 70, the 80 with a secondary hit at 0.78 of its score (a low MAPQ), the 70 unique: its MAPQ is
                  lowered to line 0's (src/bwamem.c:1029), and is not under -q                                    17
  supp_lead_del   90 + 60 whose 60 starts with a deletion mem_reg2aln squeezes out, the mate unmapped: the
                  supplementary line's POS moves, and with it the PNEXT it lends its mate                         17
  top_lead_del    the same on the 90 of a 90 + 60 end with a mapped mate: the mate's PNEXT and MC move with it    17
  unmapped_rev    an end without a hit whose mate's only hit is on the reverse strand (both orders of the ends)   17
  chimeric_alone  80 + 70 beside an end without a hit                                                             17
  proper          80 + 70 whose 80 and the mate's hit lie on one contig at a proper distance: 0x2 on every line   17
  improper        the same pair 3 000 bases apart: no 0x2                                                         17

The reference's side: mem_align1_core regions per read and the chunk's mem_pestat (sets (a), (b)) or the planted lists through
mem_sort_dedup_patch (set (c)), then the reference's own mem_sam_pe per pair with id = (n_processed >> 1) + the pair's number.

ELIGIBLE, from the reference's text and lists alone: some line lacks 0x2, or an end has several lines or is unmapped; at most
SE_LINES_CAP = 4 lines per end; at most PW_XA_CAP = 8 XA entries per line; no pa:f; at most 64 regions per end before and after
mem_sam_pe."""
import ctypes as C

import numpy as np

from mpibwa_amd import abi
from oracle import pyoracle as po

import pair_wave_cases as pw
import se_stage_cases as sec
import se_wave_cases as swc
import supp_cases as spc
from c2a_cases import _alnreg_v, _ref_handle, _regs_copy

SE_LINES_CAP = spc.SE_LINES_CAP
PW_XA_CAP = spc.PW_XA_CAP
PW_MAXREG = spc.PW_MAXREG
PW_DECIDED, PW_HOST_LENGTH, PW_HOST_NO_PAIR, PW_HOST_SCORE, PW_HOST_SUPP, PW_HOST_XA, PW_HOST_NO_RESULT, PW_HOST_TIE, PW_DECIDED_XA = 1, 6, 8, 9, 10, 11, 12, 14, 16
PW_DECIDED_LINES = 17
WRITER_BITS = 0x4 | 0x8 | 0x10 | 0x20   # of a line's flag: mem_aln2sam's (0x1 is in the decision's extra_flag as well)

OPTION_SETS = dict(spc.OPTION_SETS)     # name -> (mem_opt_t fields, with qualities, @RG line); MEM_F_PE is added by flags_of
OPTION_SETS["no_rescue"] = (dict(flag=abi.MEM_F_NO_RESCUE), True, None)
PATH_OFF = {"a": abi.MEM_F_ALL, "5": abi.MEM_F_PRIMARY5, "P": abi.MEM_F_NOPAIRING}

B_SEED, B_PAIRS_SEED, B_N_PLAIN = 97, 98, 400
_COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


def option_fields(name):
    """the mem_opt_t fields of an option set of OPTION_SETS or PATH_OFF, MEM_F_PE included"""
    kw = dict(OPTION_SETS[name][0]) if name in OPTION_SETS else dict(flag=PATH_OFF[name])
    kw["flag"] = kw.get("flag", 0) | abi.MEM_F_PE
    return kw


# ---- (a), (b) ----
def set_a(g):
    from test_sampost import _pairs_of_every_kind
    return _pairs_of_every_kind(g, n=360, seed=40)


def set_b(g):
    """-> (the pairs [(name, mate 1, mate 2)] as code arrays: B_N_PLAIN ordinary pairs, then the chimeric ones; the chimeras' number)"""
    from mpibwa_amd import simulate
    rng = np.random.default_rng(B_SEED)
    seqs = g["seqs"]

    def piece(n):
        while True:
            c = int(rng.integers(0, len(seqs)))
            p = int(rng.integers(0, len(seqs[c]) - n))
            s = seqs[c][p:p + n]
            if (s < 4).all():
                return s.copy()
    ch = [c for c in spc.realistic_cases(g) if len(c["read"]) == 150]
    reads = simulate.simulate_reads(seqs, B_N_PLAIN, 150, paired=True, seed=B_PAIRS_SEED, frac_random=0.0)
    for k, c in enumerate(ch):
        kind = k % 4
        a = c["read"]
        if kind == 1:
            b = rng.integers(0, 4, 150).astype(np.uint8)
        elif kind == 2:
            b = _COMP[ch[(k + 1) % len(ch)]["read"][::-1]].copy()
        else:
            b = piece(150)
        if k % 8 >= 4:
            a, b = b, a
        reads.append(("x%d" % k, a, b))
    return reads, len(ch)


# ---- (c) ----
def _fwd(ix, reg):
    """(contig, forward start on the contig, forward end) of a region"""
    s, e = (reg["rb"], reg["re"]) if reg["rb"] < ix.l_pac else (2 * ix.l_pac - reg["re"], 2 * ix.l_pac - reg["rb"])
    return int(reg["rid"]), int(s - ix.off[reg["rid"]]), int(e - ix.off[reg["rid"]])


def build_cases(ix, opt, pes, seed=5):
    """The families of (c) -> list of case dicts(family, tag, name, reads [end 0, end 1], regs [list, list], expect).  opt: mem_opt_t
    contents; pes: the statistics the pairs are judged under (the FR orientation must not have failed)."""
    rng = np.random.default_rng(seed)
    cases = []
    assert not pes[1].failed
    mid = (int(pes[1].low) + int(pes[1].high)) // 2

    def add(family, tag, ends, expect, swap=False):
        ends = ends[::-1] if swap else ends
        cases.append(dict(family=family, tag=tag, name=sec._name(rng, len(cases)), reads=[e[0] for e in ends], regs=[e[1] for e in ends], expect=expect))

    def nothing():
        return rng.integers(0, 4, 150).astype(np.uint8), []

    def one(rev=None, far_from=()):
        while True:
            c = int(rng.integers(ix.n_seqs))
            p = int(rng.integers(600, ix.len[c] - 1000))
            if all(abs(ix.off[c] + p - (ix.off[f[0]] + f[1])) >= 20000 for f in far_from):
                break
        read, reg = sec.plant(ix, rng, opt, c, p, 150, int(rng.integers(2)) if rev is None else rev, n_mm=int(rng.integers(0, 3)))
        return read, [sec._full(reg)]

    def chimera(lens, **kw):
        read, regs = spc._segments(ix, rng, opt, lens, **kw)
        return read, regs

    def mate_at(reg, dist):
        """a reverse-strand mate of the forward hit `reg` at insert distance `dist` as mem_infer_dir measures it"""
        c, s, _ = _fwd(ix, reg)
        read, m = sec.plant(ix, rng, opt, c, s + dist + 1 - 150, 150, 1, n_mm=1)
        return read, [sec._full(m)]

    def room(reg, dist):
        c, s, _ = _fwd(ix, reg)
        return s + dist + 400 < ix.len[c]

    for rep in range(3):
        add("five", "v", [chimera((30,) * 5), one()], PW_HOST_SUPP, swap=rep == 1)
    for rep in range(4):
        add("two_lines", "t", [chimera((80, 70)), one()], PW_DECIDED_LINES, swap=rep % 2 == 1)
    for rep in range(4):
        read, regs = chimera((80, 70))
        sub = swc._spread(ix, rng, regs[0], [int(regs[0]["score"] * 0.78)])
        add("cap_mapq", "c", [(read, regs + sub), one()], PW_DECIDED_LINES, swap=rep % 2 == 1)
    for g in (1, 2, 9):
        for rev in (0, 1):
            add("supp_lead_del", "g%d/%d" % (g, rev), [chimera((90, 60), revs=(int(rng.integers(2)), rev), kws={1: dict(lead=g)}), nothing()], PW_DECIDED_LINES,
                swap=rev == 1)
            add("top_lead_del", "g%d/%d" % (g, rev), [chimera((90, 60), revs=(rev, int(rng.integers(2))), kws={0: dict(lead=g)}), one()], PW_DECIDED_LINES,
                swap=rev == 1)
    for rep in range(4):
        add("unmapped_rev", "u", [nothing(), one(rev=1)], PW_DECIDED_LINES, swap=rep % 2 == 1)
    for rep in range(4):
        add("chimeric_alone", "a", [chimera((80, 70)), nothing()], PW_DECIDED_LINES, swap=rep % 2 == 1)
    for family, dist in (("proper", mid), ("improper", 3000)):
        for rep in range(4):
            while True:
                read, regs = chimera((80, 70), revs=(0, int(rng.integers(2))))
                if room(regs[0], dist):
                    break
            add(family, "d%d" % dist, [(read, regs), mate_at(regs[0], dist)], PW_DECIDED_LINES)
    return cases


# ---- the reference's side ----
def _handle():
    R = _ref_handle()
    P = C.POINTER
    R.mem_sam_pe.restype = C.c_int
    R.mem_sam_pe.argtypes = [P(abi.mem_opt_t), P(abi.bntseq_t), P(C.c_uint8), P(abi.mem_pestat_t), C.c_uint64, P(abi.bseq1_t), P(_alnreg_v)]
    R.mem_sort_dedup_patch.restype = C.c_int
    R.mem_sort_dedup_patch.argtypes = [P(abi.mem_opt_t), P(abi.bntseq_t), P(C.c_uint8), C.c_void_p, C.c_int, C.c_void_p]
    po.libc.malloc.restype = C.c_void_p
    po.libc.malloc.argtypes = [C.c_size_t]
    return R


def _alloc(a):
    """a malloc()ed mem_alnreg_v holding the ALNREG_DT array a (mem_sam_pe grows and the caller frees it)"""
    p = po.libc.malloc(max(1, a.nbytes))
    C.memmove(p, a.ctypes.data, a.nbytes)
    return _alnreg_v(len(a), len(a), p)


def phase1(ref, ropt, reads):
    """reads: [(name, mate 1, mate 2)] as ACGT byte strings -> (per read its nt4 codes, per read its mem_align1_core list, the chunk's
    mem_pestat): what does not depend on n_processed"""
    from test_host_pair import _batch
    R = _handle()
    regs, seqs, pes = _batch(ref, R, ropt, reads)
    codes = [np.frombuffer(s.raw[:-1], dtype=np.uint8).copy() for s in seqs]
    lists = [_regs_copy(regs[r]) for r in range(len(seqs))]
    for r in range(len(seqs)):
        po.libc.free(C.c_void_p(regs[r].a))
    return codes, lists, pes


def lists_of_cases(ref, ropt, cases):
    """set (c): per read its codes and its planted list after the reference's mem_sort_dedup_patch"""
    R = _handle()
    codes, lists = [], []
    for cs in cases:
        for e in range(2):
            sq = np.ascontiguousarray(cs["reads"][e], dtype=np.uint8)
            a = np.zeros(len(cs["regs"][e]), dtype=po.ALNREG_DT)
            for j, r in enumerate(cs["regs"][e]):
                for f in swc.FIELDS:
                    a[j][f] = r[f]
                a[j]["secondary"] = a[j]["secondary_all"] = -1
            v = _alloc(a)
            v.n = R.mem_sort_dedup_patch(ropt, ref.bns, ref.pac, sq.ctypes.data, v.n, v.a)
            codes.append(sq)
            lists.append(_regs_copy(v))
            po.libc.free(C.c_void_p(v.a))
    return codes, lists


def reference_pairs(ref, ropt, names, codes, lists, pes, n_processed=0, with_qual=True):
    """the reference's own mem_sam_pe on every pair, id = (n_processed >> 1) + the pair's number -> list of pair_wave_cases.Pair
    (before: the lists handed in, which are what the device is handed)"""
    R = _handle()
    out = []
    for p, name in enumerate(names):
        P = pw.Pair()
        P.name = name.encode() if isinstance(name, str) else bytes(name)
        nm = C.create_string_buffer(P.name)
        P.reads = [np.ascontiguousarray(codes[2 * p + k], dtype=np.uint8).copy() for k in range(2)]
        qual = [C.create_string_buffer(pw.quality(len(P.reads[k]), p)) for k in range(2)]
        P.before = [lists[2 * p + k] for k in range(2)]
        s = (abi.bseq1_t * 2)()
        for k in range(2):
            s[k].l_seq = len(P.reads[k])
            s[k].name = C.addressof(nm)
            s[k].seq = P.reads[k].ctypes.data
            s[k].qual = C.addressof(qual[k]) if with_qual else None
        a = (_alnreg_v * 2)(_alloc(P.before[0]), _alloc(P.before[1]))
        P.n_rescue = R.mem_sam_pe(ropt, ref.bns, ref.pac, pes, (int(n_processed) >> 1) + p, s, a)
        P.after = [_regs_copy(a[k]) for k in range(2)]
        P.text = []
        for k in range(2):
            P.text.append(C.string_at(s[k].sam))
            po.libc.free(C.c_void_p(s[k].sam))
            po.libc.free(C.c_void_p(a[k].a))
        out.append(P)
    return out


# ---- what the reference's text and lists say ----
def n_xa_of(line):
    return len(swc.xa_entries(line + b"\n"))


def flags(P):
    return [[int(l.split(b"\t")[1]) for l in x] for x in P.lines]


def unmapped(P):
    return [bool(f[0] & 4) for f in flags(P)]


def n_lines(P):
    """the lines of each end as the kernel counts them: 0 for the unaligned record"""
    return [0 if u else len(x) for u, x in zip(unmapped(P), P.lines)]


def leaves_the_paired_branch(P):
    return any(not f & 2 for x in flags(P) for f in x) or max(len(x) for x in P.lines) > 1 or any(unmapped(P))


def eligible(P):
    if not leaves_the_paired_branch(P):
        return False
    if max(len(x) for x in P.lines) > SE_LINES_CAP or any(n_xa_of(l) > PW_XA_CAP for x in P.lines for l in x) or any(b"\tpa:f:" in t for t in P.text):
        return False
    return max(P.n_before) <= PW_MAXREG and max(len(P.after[0]), len(P.after[1])) <= PW_MAXREG


def has_xa(P):
    return any(b"\tXA:Z:" in t for t in P.text)


def reference_lines(o, ix, P, e):
    """per line of end e, in order: supp_cases.reference_lines' dict with the flag without the writer's bits; [] for an unmapped end"""
    if unmapped(P)[e]:
        return []
    out = spc.reference_lines(o, ix, P.text[e], P.after[e])
    for R, line in zip(out, P.lines[e]):
        R["flag"] = int(line.split(b"\t")[1]) & ~WRITER_BITS
    return out


def census(pairs):
    """the counts the CPU test puts floors under"""
    c = dict(pairs=len(pairs), leave=0, eligible=0, both_unmapped=0, one_unmapped=0, one_line_each=0, multi=0, both_multi=0, chimeric_unmapped_mate=0,
             with_xa=0, an_end_unmapped=0, over_lines=0, over_regions=0, over_other=0, longest2=0, longest3=0, longest4=0, four_both=0, rescue_attempt=0)
    for P in pairs:
        if not leaves_the_paired_branch(P):
            continue
        c["leave"] += 1
        nl = [len(x) for x in P.lines]
        if not eligible(P):
            over_regions = max(P.n_before) > PW_MAXREG or max(len(P.after[0]), len(P.after[1])) > PW_MAXREG
            c["over_lines" if max(nl) > SE_LINES_CAP else "over_regions" if over_regions else "over_other"] += 1
            continue
        um = unmapped(P)
        c["eligible"] += 1
        c["both_unmapped"] += sum(um) == 2
        c["one_unmapped"] += sum(um) == 1
        c["an_end_unmapped"] += any(um)
        c["one_line_each"] += max(nl) == 1 and not any(um)
        c["multi"] += max(nl) > 1
        c["both_multi"] += min(nl) > 1
        c["chimeric_unmapped_mate"] += max(nl) > 1 and any(um)
        c["with_xa"] += has_xa(P)
        c["rescue_attempt"] += P.n_rescue > 0
        if max(nl) > 1:
            c["longest%d" % max(nl)] += 1
        c["four_both"] += min(nl) == SE_LINES_CAP
    return c


def device_regs(pairs, reg_dt):
    """the inputs of Engine.pairs_wave_lines: per read its list before mem_sam_pe"""
    out = []
    for P in pairs:
        for e in range(2):
            a = np.zeros(len(P.before[e]), dtype=reg_dt)
            for f in swc.FIELDS:
                a[f] = P.before[e][f]
            out.append(a)
    return out
