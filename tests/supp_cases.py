"""Single-end reads whose record has several lines — a primary line and supplementary lines with SA tags — and what the reference
alone makes of them, for the stage test of se_wave_kernel's multi-line branch and of sam_lines_kernel
(tests/test_gpu_supp_stage.py) and their CPU companion (tests/test_supp_cases.py).  Built on tests/se_wave_cases.py, which is imported
and left alone: the reference's side is its reference_side() (mem_align1_core or mem_sort_dedup_patch, then mem_mark_primary_se with
id = n_processed + read number and mem_reg2sam, the way the single-end branch of worker2 calls them).

(a) Realistic reads on the index of tests/pair_wave_cases.py: chimeric reads of 2, 3 and 4 segments cut from different places and
strands of its genome, clean or with substitutions at 2 % and an occasional indel; 150 bases (75+75 / 50+50+50 / 38+37+38+37), some
3-segment reads of 250 bases.  Their regions are the reference's own mem_align1_core.

(b) Synthetic families on the session genome: every segment is planted with se_stage_cases.plant (its region is a true alignment),
further hits come from se_wave_cases._spread / se_stage_cases._elsewhere.  `expect`:
  "lines"  the kernel decides the read with SE_DECIDED_LINES (17) and n_lines lines; with has_xa and the XA listing off: 11
  "plain"  one line: status 1 or 16 as before
  a code   the host's read

  two             75 + 75 on two places, the four strand combinations, on one contig and on two            lines, 2
  three           50 + 50 + 50: the middle line is clipped on both sides                                     lines, 3
  four            40 + 40 + 35 + 35: the cap                                                                 lines, 4
  five            5 x 30 without a mismatch, each scoring >= T                                               10
  lead_del / trail_del   90 + 60, the window of the 60 is g bases longer at its front / back: its CIGAR starts / ends with a
                  deletion mem_reg2aln squeezes out, which moves the POS the other line's SA tag quotes    lines, 2
  cap_mapq        80 + 70; the 80 has a secondary hit at 0.78 of its score (a low MAPQ, no XA entry at the default ratio), the 70
                  is unique: its MAPQ is lowered to line 0's (src/bwamem.c:1029), and is not under -q       lines, 2
  xa_on_0 / xa_on_1 / xa_on_both   k = 1 .. max_XA_hits hits within XA_drop_ratio under line 0 / 1 / both   lines, 2, has_xa
  xa_over         max_XA_hits + 1 of them under line 1: no tag on that line                                  lines, 2
  below_T_second  100 + a second primary hit of T - 2 on the other 50                                        plain
  tie             80 + 70, the 80 with a twin of equal score on its span: hash_64(id + place) says which of the two is line 0, the
                  other is its XA entry                                                                      lines, 2, has_xa
  row_over        250 bases, 200 + 50: the 200 with 30 single-base indels; what the other line's SA tag says of it outgrows the
                  kernel's staging, so the read is decided and its text handed back                          lines, 2

Code 14 (two hits equal under (score, hash)) cannot be reached by any list: hash_64 is a bijection and the keys id + place differ, so
the `tie` family shows instead that the hash is followed in a read of several lines.

ELIGIBLE, from the reference alone: at most 64 regions, 2 to SE_LINES_CAP lines, no pa:f, every line's XA tag at most PW_XA_CAP entries.
"""
import numpy as np

from mpibwa_amd import abi

import se_stage_cases as sec
import se_wave_cases as swc
from ref_band import reg2aln_band
from se_wave_cases import Index, device_lists, n_xa_max, quality, read_numbers, reference_side, shuffled   # noqa: F401  (re-exported)

SE_LINES_CAP = 4
PW_XA_CAP = swc.PW_XA_CAP
PW_MAXREG = swc.PW_MAXREG
LINES_ROW = 512               # bytes sam_lines_kernel stages per line for its short fields
SA_STAGE = 96                 # ... and for what the other lines' SA tags say of a line behind its contig name
XA_STAGE = swc.XA_STAGE
SE_DECIDED, SE_HOST_SUPP, SE_HOST_XA, SE_HOST_TIE, SE_DECIDED_XA, SE_DECIDED_LINES = 1, 10, 11, 14, 16, 17
MAX_LEN = 250                 # the longest read of either set

OPTION_SETS = {               # name -> (mem_opt_t fields, with qualities, @RG line)
    "default": ({}, True, None),
    "Y": (dict(flag=abi.MEM_F_SOFTCLIP), True, None),
    "M": (dict(flag=abi.MEM_F_NO_MULTI), True, None),
    "q": (dict(flag=abi.MEM_F_KEEP_SUPP_MAPQ), True, None),
    "noqual": ({}, False, None),
    "rg": ({}, True, b"@RG\\tID:grp0007\\tSM:s"),
    "xa_ratio": (dict(XA_drop_ratio=0.5), True, None),
    "xa9": (dict(max_XA_hits=9), True, None),          # beyond the cap: no listing; reads with a tag on any line get 11
    "scoring": (dict(a=2, b=5), True, None),
}

_COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


# ---- (a) ----
CHIMERA_SEED = 71
CHIMERA_PLAN = (              # (segment lengths, reads)
    ((75, 75), 70), ((50, 50, 50), 80), ((38, 37, 38, 37), 120), ((90, 80, 80), 12),
)


def realistic_cases(g, seed=CHIMERA_SEED, plan=CHIMERA_PLAN):
    """g: pair_wave_cases.build_index's dict -> case dicts (name, read, n_seg); every second read clean, the others with
    substitutions at 2 % and indels at 0.2 % per segment"""
    from mpibwa_amd import simulate
    rng = np.random.default_rng(seed)
    seqs = g["seqs"]
    out = []
    for lens, n in plan:
        for k in range(n):
            parts = []
            for j, ln in enumerate(lens):
                c = int(rng.integers(len(seqs)))
                p = int(rng.integers(1000, len(seqs[c]) - 1000 - ln))
                seg = seqs[c][p:p + ln + 4].copy()
                m = seg > 3
                seg[m] = rng.integers(0, 4, int(m.sum())).astype(np.uint8)
                if k % 2:
                    seg = simulate._mutate(seg, rng, 0.02, 0.002)
                seg = seg[:ln]
                # (the first read of the two-segment class is the 75 + 75 read on the reverse strand)
                rev = 1 if (len(lens) == 2 and k == 0) else int(rng.integers(2))
                parts.append(_COMP[seg[::-1]] if rev else seg)
            read = np.ascontiguousarray(np.concatenate(parts), dtype=np.uint8)
            out.append(dict(family="real", tag="s%d%s" % (len(lens), "d" if k % 2 else "c"), name=b"ch%d_%d_%d" % (len(lens), len(read), k), read=read,
                            expect=None, n_seg=len(lens)))
    return out


# ---- (b) ----
def _segments(ix, rng, opt, lens, revs=None, contigs=None, kws=None):
    """a read of len(lens) segments, each planted at a place of its own at least 11 000 bases from the others (beyond max_chain_gap:
    mem_sort_dedup_patch compares no two of them) -> (read, regions in query order)"""
    parts, regs, taken, at = [], [], [], 0
    for j, ln in enumerate(lens):
        kw = dict(n_mm=0)
        kw.update((kws or {}).get(j, {}))
        while True:
            c = int(rng.integers(ix.n_seqs)) if contigs is None else contigs[j]
            p = int(rng.integers(600, ix.len[c] - 600 - 2 * ln))
            if all(abs(ix.off[c] + p - t) >= 11000 for t in taken):
                break
        taken.append(ix.off[c] + p)
        rev = int(rng.integers(2)) if revs is None else revs[j]
        piece, reg = sec.plant(ix, rng, opt, c, p, ln, rev, **kw)
        reg = sec._full(reg)
        reg["qb"] += at
        reg["qe"] += at
        at += ln
        parts.append(piece)
        regs.append(reg)
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.uint8), regs


def build_cases(ix, opt, seed):
    """The families on the session genome -> list of case dicts (not shuffled).  opt: mem_opt_t contents."""
    rng = np.random.default_rng(seed)
    cases = []
    M = n_xa_max(opt)

    def add(family, tag, read, regs, expect, **kw):
        cases.append(dict(family=family, tag=tag, name=sec._name(rng, len(cases)), read=read, regs=regs, expect=expect, **kw))

    def mixed(regs):
        return [regs[i] for i in rng.permutation(len(regs))]

    def close(reg, k):
        S = reg["score"]
        return swc._spread(ix, rng, reg, [int(rng.integers(int(S * 0.86) + 1, S)) for _ in range(k)])

    for r0 in (0, 1):
        for r1 in (0, 1):
            for same in (True, False):
                c0 = int(rng.integers(ix.n_seqs))
                read, regs = _segments(ix, rng, opt, (75, 75), revs=(r0, r1), contigs=(c0, c0 if same else (c0 + 1) % ix.n_seqs),
                                       kws={0: dict(n_mm=int(rng.integers(0, 3))), 1: dict(n_mm=int(rng.integers(0, 3)))})
                add("two", "%d%d%s" % (r0, r1, "s" if same else "d"), read, mixed(regs), "lines", n_lines=2)
    for rep in range(4):
        read, regs = _segments(ix, rng, opt, (50, 50, 50), kws={1: dict(n_mm=rep % 2)})
        add("three", "t", read, mixed(regs), "lines", n_lines=3)
    for rep in range(4):
        read, regs = _segments(ix, rng, opt, (40, 40, 35, 35))
        add("four", "f", read, mixed(regs), "lines", n_lines=4)
    for rep in range(3):
        read, regs = _segments(ix, rng, opt, (30,) * 5)
        assert all(r["score"] >= opt.T for r in regs)
        add("five", "v", read, mixed(regs), SE_HOST_SUPP)
    for fam, key in (("lead_del", "lead"), ("trail_del", "trail")):
        for g in (1, 2, 9):
            for rev in (0, 1):
                read, regs = _segments(ix, rng, opt, (90, 60), revs=(int(rng.integers(2)), rev), kws={1: {key: g}})
                add(fam, "g%d/%d" % (g, rev), read, mixed(regs), "lines", n_lines=2)
    for rep in range(6):
        read, regs = _segments(ix, rng, opt, (80, 70))
        sub = swc._spread(ix, rng, regs[0], [int(regs[0]["score"] * 0.78)])
        add("cap_mapq", "c", read, mixed(regs + sub), "lines", n_lines=2)
    for fam, under in (("xa_on_0", (0,)), ("xa_on_1", (1,)), ("xa_on_both", (0, 1))):
        for k in range(1, M + 1):
            read, regs = _segments(ix, rng, opt, (80, 70))
            extra = []
            for j in under:
                extra += close(regs[j], k if j == under[0] else 1 + (k % M))
            low = swc._spread(ix, rng, regs[0], [int(regs[0]["score"] * 0.3) + j for j in range(int(rng.integers(0, 5)))], avoid=extra)
            add(fam, "k%d" % k, read, mixed(regs + extra + low), "lines", n_lines=2, has_xa=True,
                n_xa=[k if 0 in under else 0, (k if under == (1,) else 1 + (k % M)) if 1 in under else 0])
    for rep in range(3):
        read, regs = _segments(ix, rng, opt, (80, 70))
        add("xa_over", "o", read, mixed(regs + close(regs[1], M + 1)), "lines", n_lines=2, n_xa=[0, 0])
    for rep in range(4):
        read, regs = _segments(ix, rng, opt, (100,))
        other = sec._elsewhere(ix, rng, regs[0], opt.T - 2, qb=100, qe=150)
        read = np.concatenate([read, rng.integers(0, 4, 50).astype(np.uint8)])
        add("below_T_second", "b", read, mixed(regs + [other]), "plain")
    for rep in range(24):
        read, regs = _segments(ix, rng, opt, (80, 70))
        twin = swc._spread(ix, rng, regs[0], [regs[0]["score"]])
        add("tie", "t", read, [regs[0]] + twin + [regs[1]] if rep % 2 else twin + regs, "lines", n_lines=2, has_xa=True)
    for rep in range(4):
        read, regs = _segments(ix, rng, opt, (200, 50), kws={0: dict(k_indel=30, loss=opt.o_del + 8 * opt.e_del)})
        add("row_over", "r", read, mixed(regs), "lines", n_lines=2)
    return cases


# ---- what the reference's text and list say ----
def eligible(cs, text):
    ln = text.splitlines()
    if len(cs["before"]) > PW_MAXREG or not 2 <= len(ln) <= SE_LINES_CAP or b"\tpa:f:" in text:
        return False
    return all(len(swc.xa_entries(x + b"\n")) <= PW_XA_CAP for x in ln)


def has_xa(text):
    return b"\tXA:Z:" in text


def line_regions(o, after):
    """the places in the list of the regions that become lines (src/bwamem.c:1015-1019 without MEM_F_ALL), in list order"""
    return [j for j, r in enumerate(after) if r["score"] >= o.T and r["secondary"] < 0]


def listed(o, after, z):
    """mem_gen_alt's hits under z in list order, the empty list when there are more than max_XA_hits (src/bwamem_extra.c:98-118)"""
    ratio = float(np.float32(o.XA_drop_ratio))
    hits = [j for j, r in enumerate(after) if r["secondary_all"] == z and int(r["score"]) >= int(after[z]["score"]) * ratio]
    return hits if len(hits) <= n_xa_max(o) else []


def parse_line(line):
    """a line of the reference's text -> dict(flag, rname, pos, mapq, cigar, seq, qual, tags {name: value}, sa [(rname, pos, strand, cigar,
    mapq, nm)], xa entries)"""
    f = line.split(b"\t")
    tags = {t[:2]: t[5:] for t in f[11:]}
    sa = []
    for e in tags.get(b"SA", b"").split(b";")[:-1]:
        name, pos, strand, cig, mq, nm = e.rsplit(b",", 5)
        sa.append((name, int(pos), strand, cig, int(mq), int(nm)))
    return dict(flag=int(f[1]), rname=f[2], pos=int(f[3]), mapq=int(f[4]), cigar=f[5], seq=f[9], qual=f[10], tags=tags, sa=sa,
                xa=swc.xa_entries(line + b"\n"), order=[t[:2] for t in f[11:]])


def row_bytes(line, with_qual, rg):
    """the bytes of the line sam_lines_kernel stages in its row: FLAG, POS MAPQ CIGAR * 0 0, a QUAL of '*', the NM / MD / AS / XS / RG
    tags without the MD and RG values, with their tabs"""
    P = parse_line(line)
    f = line.split(b"\t")
    n = 1 + len(f[1]) + 1 + 1 + len(f[3]) + 1 + len(f[4]) + 1 + len(f[5]) + 1 + 6 + (0 if with_qual else 1)
    for t in (b"NM", b"AS", b"XS"):
        if t in P["tags"]:
            n += 6 + len(P["tags"][t])
    n += 6 if b"MD" in P["tags"] else 0
    n += 6 if rg else 0
    return n


def sa_bytes(line):
    """what the other lines' SA tags say of this line behind its contig name: ",pos,strand,CIGAR with S,mapq,NM;" """
    P = parse_line(line)
    return len(b",%d,+,%s,%d,%s;" % (P["pos"], P["cigar"], P["mapq"], P["tags"].get(b"NM", b"0")))


def reference_lines(o, ix, text, after):
    """per line of the reference's text, in order: dict(region, flag without the strand bit, mapq, score, sub, xa: the listed regions)"""
    zs = line_regions(o, after)
    ln = text.splitlines()
    assert len(zs) == len(ln), (len(zs), text)
    out = []
    for z, line in zip(zs, ln):
        P = parse_line(line)
        r = after[z]
        assert (r["rb"] >= ix.l_pac) == bool(P["flag"] & 0x10) and ix.names[int(r["rid"])] == P["rname"], (line, r)
        out.append(dict(region=r, flag=P["flag"] & ~0x10, mapq=P["mapq"], score=int(P["tags"][b"AS"]), sub=int(P["tags"][b"XS"]) if b"XS" in P["tags"] else -1,
                        xa=[after[j] for j in listed(o, after, z)], n_xa=len(P["xa"])))
    return out


def request_of(o, r, read, pad=0):
    w2 = reg2aln_band(o, int(r["qe"] - r["qb"]), int(r["re"] - r["rb"]), int(r["truesc"]), int(r["w"]))
    return (int(r["rb"]), int(r["re"]), int(read), int(r["qb"]), int(r["qe"]), w2, int(r["truesc"]), int(pad))


def census(cases, want):
    c = dict(reads=len(cases), eligible=0, lines1=0, lines2=0, lines3=0, lines4=0, lines_over=0, gt64=0, xa_over_cap=0, with_xa=0)
    for cs, (text, after) in zip(cases, want):
        n = len(text.splitlines())
        c["lines%d" % n if n <= SE_LINES_CAP else "lines_over"] += 1
        c["gt64"] += len(cs["before"]) > PW_MAXREG
        c["xa_over_cap"] += any(len(swc.xa_entries(x + b"\n")) > PW_XA_CAP for x in text.splitlines())
        if eligible(cs, text):
            c["eligible"] += 1
            c["with_xa"] += has_xa(text)
            c["eligible%d" % n] = c.get("eligible%d" % n, 0) + 1
    return c
