"""Cases of the SAM stage test (sam_emit_kernel behind aln_kernel, through mi355x_sam_batch): pairs of reads planted on an index so that
their regions are true alignments, every family built to reach one branch of the kernel (tests/test_sam_cases.py proves from the
reference's own text that it does), shuffled into one launch so that every wave of 64 reads is mixed.

A case is a pair: two reads (nt4 codes), one name, two regions as mem_alnreg_t holds them, the extra flag and the MAPQ mem_sam_pe
would have decided.  The device gets a SamDesc per read and an AlnReq per region (band: tests/ref_band.py), the reference gets the
regions (oracle/pyoracle.py: RefIndex.pair_records).

Everything is laid out in forward coordinates first — a piece of the reference, edited into the aligned part of the read, a window
around it, clips — and turned into the doubled coordinate and the reverse complement for a read on the reverse strand."""
import numpy as np

from oracle import pyoracle as po
from ref_band import reg2aln_band

FAMILIES = ("plain", "contigs", "clip", "lead_del", "trail_del", "lengths", "row", "declined", "unmapped", "not_mine")

OPTION_SETS = {            # name -> (mem_opt_t fields, with qualities, @RG line)
    "default": ({}, True, None),
    "noqual": ({}, False, None),
    "rg7": ({}, True, b"@RG\\tID:grp0007\\tSM:s"),
    "rg255": ({}, True, b"@RG\\tID:" + b"g" * 255 + b"\\tSM:s"),
    "scoring": (dict(a=2, b=3, o_del=4, e_del=2, o_ins=4, e_ins=2), True, None),
}

SAM_ROW = 260              # bytes of a lane's staging row (sam_kernel.hip)
_COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


class Index:
    """what the generator needs of an index: contig table and the bases of the packed reference (an N of the FASTA is whatever base
    the .pac file holds in its place: the regions are alignments against the .pac)"""

    def __init__(self, prefix, bns):
        b = bns.contents
        self.l_pac = int(b.l_pac)
        self.n_seqs = int(b.n_seqs)
        self.off = [int(b.anns[k].offset) for k in range(self.n_seqs)]
        self.len = [int(b.anns[k].len) for k in range(self.n_seqs)]
        self.names = [bytes(b.anns[k].name) for k in range(self.n_seqs)]
        raw = np.fromfile(prefix + ".pac", dtype=np.uint8)[:(self.l_pac + 3) // 4]
        self.bases = np.stack([(raw >> s) & 3 for s in (6, 4, 2, 0)], axis=1).reshape(-1)[:self.l_pac].astype(np.uint8)


def _aligned_part(ix, rng, c, p, n_query, k_indel, n_mm, n_codes=0):
    """n_query bases that align to the contig c from p on with k_indel single-base indels (insertion, deletion, insertion, ...) at
    least 4 bases apart and n_mm substitutions -> (query part, reference bases consumed)"""
    n_ins, n_del = (k_indel + 1) // 2, k_indel // 2
    n_m = n_query - n_ins
    assert n_m >= 4 * (k_indel + 1)
    cuts = np.sort(rng.choice(np.arange(1, n_m - 4 * k_indel), size=k_indel, replace=False)) + 4 * np.arange(k_indel) if k_indel else np.zeros(0, int)
    runs = np.diff(np.concatenate([[0], cuts, [n_m]])).astype(int)
    assert runs.min() >= 1 and runs.sum() == n_m
    g = ix.off[c] + p
    out = []
    for j, run in enumerate(runs):
        seg = ix.bases[g:g + run].copy()
        g += run
        out.append(seg)
        if j < k_indel:
            if j % 2 == 0:     # insertion: a base that differs from both neighbours
                nb = {int(seg[-1]), int(ix.bases[g])}
                out.append(np.array([min(set(range(4)) - nb)], dtype=np.uint8))
            else:              # deletion of one reference base
                g += 1
    q = np.concatenate(out)
    assert len(q) == n_query
    for pos in rng.choice(n_query, size=n_mm, replace=False) if n_mm else []:
        q[pos] = (int(q[pos]) + 1 + int(rng.integers(3))) & 3
    for pos in rng.choice(n_query, size=n_codes, replace=False) if n_codes else []:
        q[pos] = 4
    return q, g - (ix.off[c] + p)


def plant(ix, rng, opt, c, p, length, rev, cl=0, cr=0, lead=0, trail=0, k_indel=0, n_mm=2, n_codes=0, big_del=0, loss=None,
          score=None, sub=0, w_reg=100):
    """One read of `length` bases whose aligned part starts at base p of contig c (forward coordinates): clips of cl / cr bases in
    front of / behind the aligned part as the forward strand sees it, a window that is `lead` / `trail` bases longer than the aligned
    part at its front / back (the global alignment then starts / ends with a deletion), big_del: a deletion of that many bases in the
    middle.  loss: what the region's local score lacks of a perfect match (sets the band, tests/ref_band.py).
    -> (read codes, region dict)"""
    n_q = length - cl - cr
    if big_del:
        h = n_q // 2
        q1, r1 = _aligned_part(ix, rng, c, p, h, 0, n_mm)
        q2, r2 = _aligned_part(ix, rng, c, p + r1 + big_del, n_q - h, 0, 0)
        part, used = np.concatenate([q1, q2]), r1 + big_del + r2
    else:
        part, used = _aligned_part(ix, rng, c, p, n_q, k_indel, n_mm, n_codes)
    fs, fe = ix.off[c] + p - lead, ix.off[c] + p + used + trail
    assert ix.off[c] <= fs and fe <= ix.off[c] + ix.len[c], "window leaves its contig"
    fwd = np.concatenate([rng.integers(0, 4, cl).astype(np.uint8), part, rng.integers(0, 4, cr).astype(np.uint8)])
    if not rev:
        read, rb, re, qb, qe = fwd, fs, fe, cl, cl + n_q
    else:
        read, rb, re, qb, qe = _COMP[fwd[::-1]], 2 * ix.l_pac - fe, 2 * ix.l_pac - fs, cr, cr + n_q
    if loss is None:
        loss = min(n_mm * (opt.a + opt.b), 14)
    truesc = min(n_q, fe - fs) * opt.a - loss
    reg = dict(rb=rb, re=re, qb=qb, qe=qe, rid=c, truesc=truesc, score=truesc if score is None else score, sub=sub, w=w_reg)
    return np.ascontiguousarray(read), reg


_DIGITS = dict(score=(7, 42, 150), sub=(-1, 0, 19, 123), mapq=(0, 7, 37, 60, 255), flag=(0, 2))


def _pair(family, tag, name, ends, rng):
    regs = [e[1] for e in ends]
    return dict(family=family, tag=tag, name=name, reads=[e[0] for e in ends], regs=regs, flags=[int(rng.choice(_DIGITS["flag"]))] * 2,
                mapqs=[int(rng.choice(_DIGITS["mapq"])) for _ in range(2)])


def _name(rng, k, n=None):
    base = b"r%05d" % k
    if n is None:
        return base + b":" + bytes(rng.choice(np.frombuffer(b"ACGT0123456789_/", np.uint8), int(rng.integers(0, 12))))
    return (base * (n // len(base) + 1))[:n]


def build_cases(ix, opt, seed, lengths_family=True):
    """All families on one index -> list of pair dicts (not shuffled).  opt: mem_opt_t contents."""
    rng = np.random.default_rng(seed)
    cases = []
    digits = lambda: dict(score=int(rng.choice(_DIGITS["score"])), sub=int(rng.choice(_DIGITS["sub"])))
    spot = lambda c, room: int(rng.integers(400, ix.len[c] - 400 - room))
    name = lambda n=None: _name(rng, len(cases), n)

    # plain: the four strand combinations, inserts of either sign, and both mates forward at one position
    for rep in range(40):
        for r0 in (0, 1):
            for r1 in (0, 1):
                c = int(rng.integers(ix.n_seqs))
                p0 = spot(c, 700) + 350
                p1 = p0 + int(rng.integers(-350, 351))
                cases.append(_pair("plain", "s%d%d" % (r0, r1), name(), [plant(ix, rng, opt, c, p0, 150, r0, **digits()),
                                                                           plant(ix, rng, opt, c, p1, 150, r1, **digits())], rng))
    for rep in range(40):
        c = int(rng.integers(ix.n_seqs))
        p0 = spot(c, 200)
        cases.append(_pair("plain", "same", name(), [plant(ix, rng, opt, c, p0, 150, 0, **digits()), plant(ix, rng, opt, c, p0, int(rng.choice([100, 150])), 0, **digits())], rng))

    # contigs: mates on different contigs; regions that start at a contig's first base / end at its last
    last = ix.n_seqs - 1
    for rep in range(30):
        for c0, c1 in [(0, last), (last, 0)] + [(c, (c + 1) % ix.n_seqs) for c in range(ix.n_seqs)]:
            r0, r1 = int(rng.integers(2)), int(rng.integers(2))
            cases.append(_pair("contigs", "%d-%d" % (c0, c1), name(), [plant(ix, rng, opt, c0, spot(c0, 200), 150, r0, **digits()),
                                                                       plant(ix, rng, opt, c1, spot(c1, 200), 150, r1, **digits())], rng))
    for rep in range(12):
        for c in range(ix.n_seqs):
            r0, r1 = int(rng.integers(2)), int(rng.integers(2))
            at_end = plant(ix, rng, opt, c, ix.len[c] - 150, 150, r0, n_mm=1, **digits())
            at_start = plant(ix, rng, opt, (c + 1) % ix.n_seqs, 0, 150, r1, n_mm=1, **digits())
            assert (at_end[1]["re"] if not r0 else 2 * ix.l_pac - at_end[1]["rb"]) == ix.off[c] + ix.len[c]
            cases.append(_pair("contigs", "edge", name(), [at_end, at_start] if rep % 2 else [at_start, at_end], rng))

    # clip: qb > 0, qe < l, both, on either strand
    for rep in range(25):
        for cl, cr in ((int(rng.integers(1, 60)), 0), (0, int(rng.integers(1, 60))), (int(rng.integers(1, 40)), int(rng.integers(1, 40)))):
            for r0 in (0, 1):
                c = int(rng.integers(ix.n_seqs))
                p0 = spot(c, 600)
                cases.append(_pair("clip", "%d/%d/%d" % (cl > 0, cr > 0, r0), name(), [plant(ix, rng, opt, c, p0, 150, r0, cl=cl, cr=cr, **digits()),
                                                                                       plant(ix, rng, opt, c, p0 + int(rng.integers(100, 400)), 150, 1 - r0, cl=cr, cr=cl, **digits())], rng))

    # lead_del / trail_del: the window is g bases longer than the aligned part at the front / at the back
    for fam, key in (("lead_del", "lead"), ("trail_del", "trail")):
        for rep in range(25):
            for g in (1, 2, 9):
                for r0 in (0, 1):
                    c = int(rng.integers(ix.n_seqs))
                    p0 = spot(c, 600)
                    a = plant(ix, rng, opt, c, p0, 150, r0, n_mm=int(rng.integers(0, 3)), **{key: g}, **digits())
                    b = plant(ix, rng, opt, c, p0 + int(rng.integers(-200, 300)), 150, int(rng.integers(2)), **digits())
                    cases.append(_pair(fam, "g%d/%d" % (g, r0), name(), [a, b] if rep % 2 else [b, a], rng))

    # lengths: read lengths around the 64-byte copy loops, names of 1 .. 254 bytes, N in reads of either strand
    if lengths_family:
        for rep in range(6):
            for L in (20, 63, 64, 65, 127, 128, 129, 150, 151, 250, 251):
                for r0 in (0, 1):
                    c = int(rng.integers(ix.n_seqs))
                    p0 = spot(c, 900)
                    L1 = int(rng.choice([20, 63, 64, 65, 127, 128, 129, 150, 151, 250, 251]))
                    nl = (1, 63, 64, 65, 200, 254)[(len(cases)) % 6]
                    cases.append(_pair("lengths", "L%d/%d/n%d" % (L, r0, nl), name(nl),
                                       [plant(ix, rng, opt, c, p0, L, r0, n_mm=min(2, L // 20), n_codes=(rep % 3 == 0) * min(3, L // 20), **digits()),
                                        plant(ix, rng, opt, c, p0 + int(rng.integers(0, 300)), L1, int(rng.integers(2)), n_mm=1, n_codes=(rep % 3 == 1) * 2, **digits())], rng))

    # row: k single-base indels per mate of 250 bp; the short fields (FLAG POS MAPQ CIGAR = PNEXT TLEN NM MC AS XS) pass 260 bytes
    # where the two CIGARs hold ~60 operations together
    ladder = [(k, k) for k in range(31)] + [(0, k) for k in range(1, 31)] + [(k, 30) for k in range(30)]
    ladder += [(k0, t - k0) for rep in range(2) for t in range(32, 45) for k0 in range(t - 30, 31)]
    for k0, k1 in ladder:
        c = int(rng.integers(ix.n_seqs))
        p0 = spot(c, 900)
        r0 = int(rng.integers(2))
        loss = opt.o_del + 8 * opt.e_del
        ends = [plant(ix, rng, opt, c, p0, 250, r0, k_indel=k0, n_mm=0, loss=loss, **digits()),
                plant(ix, rng, opt, c, p0 + int(rng.integers(0, 400)), 250, 1 - r0, k_indel=k1, n_mm=0, loss=loss, **digits())]
        cases.append(_pair("row", "k%d/%d" % (k0, k1), name(), ends if rng.integers(2) else ends[::-1], rng))

    # declined: reads as long as the longest of the launch with a 10-base deletion and a region score so low that the band starts at
    # min(opt.w, > 55): a direction matrix of 2 w + 1 columns x 261 rows is beyond the 80 x (251 + 32) cells aln_kernel keeps on chip
    for rep in range(12):
        c = int(rng.integers(ix.n_seqs))
        p0 = spot(c, 900)
        r0 = int(rng.integers(2))
        a = plant(ix, rng, opt, c, p0, 251, r0, big_del=10, loss=120, score=100)
        b = plant(ix, rng, opt, c, p0 + int(rng.integers(0, 400)), 150, 1 - r0, **digits())
        cases.append(_pair("declined", "d%d" % r0, name(), [a, b] if rep % 2 else [b, a], rng))

    # unmapped: pairs without any hit (req = -3)
    for rep in range(60):
        L = int(rng.choice([30, 64, 150, 151]))
        reads = [rng.integers(0, 5 if rep % 4 == 0 else 4, L).astype(np.uint8) for _ in range(2)]
        cases.append(dict(family="unmapped", tag="u", name=name(), reads=reads, regs=None, flags=[0, 0], mapqs=[0, 0]))
    return cases


def not_mine_pair(rng, k):
    return dict(family="not_mine", tag="n", name=b"nm%05d" % k, reads=[rng.integers(0, 4, 150).astype(np.uint8) for _ in range(2)], regs=None,
                flags=[0, 0], mapqs=[0, 0])


def shuffled_launch(cases, seed):
    """the cases in random order, with req = -1 pairs sprinkled in, two whole waves of them (32 pairs from a multiple of 32) and a run of
    64 reads that starts in the middle of a wave (32 pairs from 32 m + 16)"""
    rng = np.random.default_rng(seed)
    order = [cases[i] for i in rng.permutation(len(cases))]
    for k in range(len(order) // 25):
        order.insert(int(rng.integers(len(order))), not_mine_pair(rng, k))
    for at in (64, 256, 32 * 15 + 16):
        assert at + 32 <= len(order)
        order[at:at] = [not_mine_pair(rng, 1000 + at + j) for j in range(32)]
    return order


def small_launch(cases, n_pairs, seed):
    """n_pairs pairs, one of every family as far as they go (the launches of 2, 62, 64 and 66 reads)"""
    rng = np.random.default_rng(seed)
    by_fam = {}
    for cs in cases:
        by_fam.setdefault(cs["family"], []).append(cs)
    fams = [f for f in FAMILIES if f in by_fam]
    out = []
    for j in range(n_pairs):
        pool = by_fam[fams[(seed + j) % len(fams)]]
        out.append(pool[int(rng.integers(len(pool)))])
    if n_pairs > 4:
        out[int(rng.integers(n_pairs))] = not_mine_pair(rng, 7)
    return out


DESC_DT = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("req", "<i4"), ("rid", "<i4"), ("flag", "<i4"), ("mapq", "<i4"),
                    ("score", "<i4"), ("sub", "<i4")])
AREQ_DT = np.dtype([("rb", "<i8"), ("re", "<i8"), ("read", "<i4"), ("qb", "<i4"), ("qe", "<i4"), ("w2", "<i4"), ("truesc", "<i4"), ("pad", "<i4")])


def _qual(n, k):
    return (33 + (np.arange(n) * 7 + k) % 41).astype(np.uint8).tobytes()


def device_side(order, opt, with_qual):
    """the inputs of Engine.sam_records for the pairs in `order`"""
    n = len(order)
    desc = np.zeros(2 * n, dtype=DESC_DT)
    reqs, req_base = [], [0]
    reads, names, quals = [], [], []
    for k, cs in enumerate(order):
        for e in range(2):
            reads.append(cs["reads"][e])
            names.append(cs["name"])
            quals.append(_qual(len(cs["reads"][e]), k + e))
            d = desc[2 * k + e]
            if cs["family"] == "not_mine":
                d["req"] = -1
                d["rid"] = -1
            elif cs["family"] == "unmapped":   # as pair_simple_kernel describes a pair without any hit
                d["req"] = -3
                d["rid"] = -1
                d["flag"] = 0x1 | 0x4 | 0x8 | (0x40 << e)
            else:
                r = cs["regs"][e]
                for f in ("rb", "re", "qb", "qe", "rid", "score", "sub"):
                    d[f] = r[f]
                d["req"] = e
                d["flag"] = (0x40 << e) | cs["flags"][e]
                d["mapq"] = cs["mapqs"][e]
                w2 = reg2aln_band(opt, r["qe"] - r["qb"], r["re"] - r["rb"], r["truesc"], r["w"])
                reqs.append((r["rb"], r["re"], 2 * k + e, r["qb"], r["qe"], w2, r["truesc"], 0))
        req_base.append(len(reqs))
    return dict(reads=reads, quals=quals if with_qual else None, names=names, desc=desc, reqs=np.array(reqs, dtype=AREQ_DT).reshape(-1),
                req_base=np.array(req_base, dtype=np.int32))


def reference_side(ref, ropt, order, with_qual):
    """the reference's text per read of `order` (None for the reads of req = -1 pairs)"""
    mine = [k for k, cs in enumerate(order) if cs["family"] != "not_mine"]
    regs = np.zeros(2 * len(mine), dtype=po.ALNREG_DT)
    reads, names, quals, flags, mapqs = [], [], [], [], []
    for j, k in enumerate(mine):
        cs = order[k]
        for e in range(2):
            reads.append(cs["reads"][e])
            names.append(cs["name"])
            quals.append(_qual(len(cs["reads"][e]), k + e))
            flags.append(cs["flags"][e])
            mapqs.append(cs["mapqs"][e])
            g = regs[2 * j + e]
            if cs["regs"] is None:
                g["rb"] = g["re"] = -1
                continue
            r = cs["regs"][e]
            for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w"):
                g[f] = r[f]
            g["sub"] = g["csub"] = r["sub"]
            g["secondary"] = g["secondary_all"] = -1
    text = ref.pair_records(ropt, reads, quals if with_qual else None, names, regs, flags, mapqs)
    out = [None] * (2 * len(order))
    for j, k in enumerate(mine):
        out[2 * k], out[2 * k + 1] = text[2 * j], text[2 * j + 1]
    return out


def parse(rec, rg=b""):
    """a record of the reference as fields, tags and the length of its short fields: everything the kernel prints into its staging row,
    i.e. the record without QNAME, RNAME, a mate RNAME that is a name, SEQ, a QUAL that is not '*', the MD value, the RG value, the
    newline — and without the tab between SEQ and QUAL, which the kernel writes on its own between the two copies, not through the row"""
    assert rec.endswith(b"\n") and rec.count(b"\n") == 1
    f = rec[:-1].split(b"\t")
    assert len(f) >= 11
    tags = {t[:2]: t[5:] for t in f[11:]}
    assert all(t[2:3] == b":" and t[4:5] == b":" for t in f[11:])
    long_parts = [f[0], f[2] if f[2] != b"*" else b"", f[6] if f[6] not in (b"=", b"*") else b"", f[9], f[10] if f[10] != b"*" else b"",
                  tags.get(b"MD", b""), rg if b"RG" in tags else b""]
    short = len(rec) - 2 - sum(len(x) for x in long_parts)
    return dict(fields=f, flag=int(f[1]), rname=f[2], pos=int(f[3]), cigar=f[5], rnext=f[6], tlen=int(f[8]), tags=tags, short=short)


def cigar_ref_len(cig):
    n, tot = 0, 0
    for ch in cig.decode():
        if ch.isdigit():
            n = n * 10 + int(ch)
        else:
            if ch in "MD":
                tot += n
            n = 0
    return tot


CONTIG_NAMES = ("c", "n" * 64, "m" * 65, "long_contig_name_" + "x" * 103)


def build_named_index(directory):
    """a small second genome whose contig names are 1, 64, 65 and 120 bytes long, indexed by the product -> prefix"""
    from mpibwa_amd import api, simulate
    _, seqs = simulate.make_genome(80_000, 4, seed=23)
    fa = str(directory / "named.fa")
    simulate.write_fasta(fa, list(CONTIG_NAMES), seqs)
    api.build_index(fa, fa)
    return fa


def arena_launch(cases, reps):
    """the pairs of 150-bp reads, under 254-byte names, `reps` times over: with a 255-byte read group their records outgrow the arena
    the pipeline allots (tests/test_sam_cases.py checks that on the reference's text)"""
    rng = np.random.default_rng(reps)
    pick = [cs for cs in cases if cs["regs"] is not None and cs["family"] not in ("row", "declined") and all(len(r) == 150 for r in cs["reads"])]
    out = []
    for rep in range(reps):
        for j in rng.permutation(len(pick)):
            out.append(dict(pick[j], name=_name(rng, len(out), 254)))
    return out
