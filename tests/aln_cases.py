"""Inputs of the stage test of aln_kernel (mpibwa_amd/csrc/aln_kernel.hip): requests of mem_reg2aln's DP loop planted on references the
test builds itself, the reference's per-round results for them (bwa_gen_cigar2 of oracle/_ref/libbwaref.so), and a plain restatement
of which path the kernel takes for a request — unused slot, invalid, answered without DP, moved from the no-DP list to the DP list,
narrow band, handed to the full-size instantiation, declined (and why) — from which the lengths of the three request lists follow.

tests/test_aln_cases.py shows on the CPU, by the reference's outputs alone, that every family reaches its branch;
tests/test_gpu_aln_stage.py compares the kernel with the reference, exactly, and its flags and list counters with the restatement.

Families (the letters of the case list in DESIGN.md §4.5):
  a  the no-DP bound: loss exactly at the bound / the smallest reachable loss above it (N columns lose a + 1), the tie
     G.A^m.C^n | A^m.C^n.T and its neighbour with a fourth mismatch, w2 = 0 under heavy mismatch
  b  the conditions of mem_reg2aln's loop, each deciding alone: insertion + deletion pairs of size g from w2 = 3
  c  band arithmetic: |rlen - lq|, w2 around d + 3 and around (max_gap + d + 1) >> 1, 2w + 1 around lq, lq / rlen of 1..3, 63..65 rows,
     bands of more than 64 columns
  d  capacity edges: n_col * rlen at aln_zcap_small / aln_zcap and one row more, a request that outgrows the narrow band in round 2
  e  output capacities: 96 / 97 CIGAR operations, 768 / 769 MD bytes, deletions and insertions first and last
  f  strand and placement: tandem repeats, rb = 0, re = l_pac, rb = l_pac, re = 2 l_pac, bridging, over-long windows, N in the read
  g  launch shapes and the reuse of a wave (grid stride, LDS slice, result-pool slabs)
Not constructible: a scoring with amax <= 0 (bwa_fill_scmat gives mat[0] = a, and a <= 0 divides nothing sensible in max_gap);
lq > max_len (the region would lie outside its read); the pool-exhaustion branch (the entry sizes the pool for the worst case)."""
import numpy as np

L_PAC = 40003                      # not a multiple of 4: the last byte of pac is partly used
L_PAC_REUSE = 160003
BIG = 1 << 20                      # a truesc that never stops the loop

DEFAULT = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, w=100)
OPTION_SETS = {
    "default": {},
    "a2": dict(a=2), "a3": dict(a=3),
    "b1": dict(b=1), "b9": dict(b=9),
    "del_1_3": dict(o_del=1, e_del=3),       # max_gap from the insertion side
    "ins_1_3": dict(o_ins=1, e_ins=3),       # ... from the deletion side
    "odel12": dict(o_del=12), "oins12": dict(o_ins=12),
    "e2": dict(e_del=2, e_ins=2),
    "w0": dict(w=0), "w1": dict(w=1), "w2": dict(w=2), "w25": dict(w=25), "w1000": dict(w=1000),
    "combined": dict(a=2, b=3, o_del=4, e_del=2, o_ins=4, e_ins=2),
}
WIDE_SETS = ("default", "combined")          # families d, e and g

ALN_MDCAP, ALN_CIGCAP, ALN_SLAB = 768, 96, 1024


class Opt:
    def __init__(self, name, fields=None):
        self.name = name
        f = dict(DEFAULT)
        f.update(OPTION_SETS[name] if fields is None else fields)
        self.fields = f
        for k, v in f.items():
            setattr(self, k, v)
        self.mat = scmat(self.a, self.b)
        self.oe_del, self.oe_ins = self.o_del + self.e_del, self.o_ins + self.e_ins
        self.bound = self.a + self.oe_del + self.oe_ins     # aln_kernel<0>: the largest loss it answers without DP


def scmat(a, b):
    """bwa_fill_scmat (src/bwa.c:79-93)"""
    m = np.full((5, 5), -1, dtype=np.int32)
    for i in range(4):
        for j in range(4):
            m[i, j] = a if i == j else -b
    return m


def apply(opt_ptr, fill_scmat, o):
    """the fields of an option set into a mem_opt_t of either library"""
    c = opt_ptr.contents
    for k, v in o.fields.items():
        setattr(c, k, v)
    fill_scmat(c.a, c.b, c.mat)
    return opt_ptr


# ---------------------------------------------------------------- the kernel's arithmetic, restated
def aln_zcap(max_len):
    z = (80 * (max_len + 32) + 255) & ~255
    return max(z, 12288)


def aln_zcap_small(max_len):
    return (32 * (max_len + 32) + 255) & ~255


def max_gap(o, lq):
    """src/bwa.c:153-156 (C's int cast truncates toward zero, like int())"""
    half = (lq + 1) >> 1
    g = max(int((half * o.a - o.o_ins) / o.e_ins + 1.), int((half * o.a - o.o_del) / o.e_del + 1.))
    return max(g, 1)


def band(o, lq, rlen, w2):
    """(w, n_col) of a round: src/bwa.c:157-160, and the columns aln_kernel keeps per row"""
    d = abs(rlen - lq)
    w = (max_gap(o, lq) + d + 1) >> 1
    w = min(w, w2)
    w = max(w, d + 3)
    return w, (lq if lq < 2 * w + 1 else 2 * w + 1)


def lds_bytes(max_len):
    """(no-DP, narrow, full) dynamic LDS of a workgroup: launch_aln"""
    tcap = max_len + 256
    full = 2 * (max_len + 2 + 64) * 4 + 4 + ((max_len + 3) & ~3) + ((tcap + 3) & ~3) + aln_zcap(max_len) + ALN_MDCAP + ALN_CIGCAP * 4
    return 2 * ((max_len + 3) & ~3) + ALN_MDCAP + 16, full - (aln_zcap(max_len) - aln_zcap_small(max_len)), full


def grid_for(lds, cus, n_req):
    """launch_aln's grid_for (one wave per workgroup)"""
    per_cu = max(1, min(160 * 1024 // max(lds, 1), 32))
    return min(cus * per_cu * 2, n_req)


# ---------------------------------------------------------------- building requests
def rc(a):
    a = np.asarray(a, np.uint8)
    return np.where(a > 3, 4, 3 - a)[::-1].astype(np.uint8)


def pack2bit(ref):
    pac = np.zeros(len(ref) // 4 + 1, dtype=np.uint8)
    for k in range(4):
        part = ref[k::4]
        pac[:len(part)] |= (part << ((3 - k) * 2)).astype(np.uint8)
    return pac


def seq(x):
    return np.asarray(x, dtype=np.uint8)


def cat(*parts):
    return np.concatenate([seq(p) for p in parts]).astype(np.uint8)


def other(rng, base):
    """a base that is not `base`"""
    return np.uint8((int(base) + int(rng.integers(1, 4))) & 3)


def with_mismatches(rng, q, t, pos):
    q = q.copy()
    for p in pos:
        q[p] = other(rng, t[p])
    return q


class Cases:
    """A reference and requests on it.  fam / sub name the family and what the request is there for; rel[i] = delta asks for
    truesc = (the reference's round-1 score) + delta, which fix_truesc() fills in."""

    def __init__(self, seed, l_pac=L_PAC):
        self.rng = np.random.default_rng(seed)
        self.l_pac = l_pac
        self.ref = self.rng.integers(0, 4, size=l_pac).astype(np.uint8)
        self.cursor, self.phase, self.flip = 1000, 0, 0
        self.reads, self.rb, self.re, self.read, self.qb, self.qe, self.w2, self.truesc = [], [], [], [], [], [], [], []
        self.fam, self.sub, self.rel = [], [], []
        self._pac = None

    def __len__(self):
        return len(self.rb)

    def place(self, t, at=None):
        """write the window t into the forward strand, at the next free place with the next of the four alignments"""
        assert self._pac is None
        if at is None:
            at = self.cursor
            at += ((self.phase >> 1) - at) & 3      # (the strand alternates with every request: the alignment moves on with every second)
            self.phase = (self.phase + 1) & 7
            self.cursor = at + len(t) + 1
            assert self.cursor < self.l_pac - 1000, "reference full"
        self.ref[at:at + len(t)] = t
        return at

    def add(self, fam, sub, t, q, w2, truesc=BIG, strand=None, at=None, head=(), tail=(), rel=None):
        """window t and region q as the forward strand sees them; head / tail: clipped bases of the read around the region"""
        t, q = seq(t), seq(q)
        p = self.place(t, at)
        if strand is None:
            strand = self.flip
            self.flip ^= 1
        rd = cat(head, q, tail)
        if strand == 0:
            rb, re, qb = p, p + len(t), len(head)
        else:
            rb, re, qb, rd = 2 * self.l_pac - (p + len(t)), 2 * self.l_pac - p, len(tail), rc(rd)
        return self.raw(fam, sub, rd, rb, re, qb, qb + len(q), w2, truesc, rel)

    def raw(self, fam, sub, rd, rb, re, qb, qe, w2, truesc=BIG, rel=None):
        self.reads.append(seq(rd))
        self.read.append(len(self.reads) - 1)
        for lst, v in ((self.rb, rb), (self.re, re), (self.qb, qb), (self.qe, qe), (self.w2, w2), (self.truesc, truesc), (self.fam, fam),
                       (self.sub, sub), (self.rel, rel)):
            lst.append(v)
        return len(self.rb) - 1

    def unused(self):
        """an unused slot of the request array, as the pipeline leaves them"""
        for lst, v in ((self.rb, 0), (self.re, 0), (self.read, -1), (self.qb, 0), (self.qe, 0), (self.w2, 0), (self.truesc, 0), (self.fam, "g"),
                       (self.sub, "unused"), (self.rel, None)):
            lst.append(v)

    def again(self, i, fam=None, sub=None):
        """request i once more (same read)"""
        for lst in (self.rb, self.re, self.read, self.qb, self.qe, self.w2, self.truesc, self.rel):
            lst.append(lst[i])
        self.fam.append(fam or self.fam[i])
        self.sub.append(sub or self.sub[i])

    @property
    def pac(self):
        if self._pac is None:
            self._pac = pack2bit(self.ref)
            self.dbl = np.concatenate([self.ref, 3 - self.ref[::-1]]).astype(np.uint8)
        return self._pac

    @property
    def max_len(self):
        return max(len(r) for r in self.reads)

    def window(self, i):
        self.pac
        return self.dbl[self.rb[i]:self.re[i]]

    def query(self, i):
        return self.reads[self.read[i]][self.qb[i]:self.qe[i]]

    def order(self, idx):
        """the requests idx, in that order, on the same reads and reference (a launch of its own)"""
        c = Cases.__new__(Cases)
        c.__dict__.update(self.__dict__)
        for k in ("rb", "re", "read", "qb", "qe", "w2", "truesc", "fam", "sub", "rel"):
            src = getattr(self, k)
            setattr(c, k, [src[i] for i in idx])
        return c


def indel_pair(rng, t, x, g, d, g_del=None):
    """t with g bases inserted at x and, d bases later, g_del (default g) bases deleted"""
    g_del = g if g_del is None else g_del
    return cat(t[:x], rng.integers(0, 4, size=g), t[x:x + d], t[x + d + g_del:])


# ---- family a
def reachable_losses(o, lq=24):
    """loss -> (mismatches, N columns), fewest N first"""
    out = {}
    for n in range(lq):
        for k in range(lq - n):
            out.setdefault(k * (o.a + o.b) + n * (o.a + 1), (k, n))
    return out


def family_a(cs, o):
    rng = cs.rng
    reach = reachable_losses(o)
    at = max(x for x in reach if x <= o.bound)
    above = min(x for x in reach if x > o.bound)
    for sub, loss in (("a.at", at), ("a.above", above)):
        k, n = reach[loss]
        for lq in (40, 97, 31, 64, 40, 97, 31, 64):
            t = rng.integers(0, 4, size=lq).astype(np.uint8)
            pos = sorted(int(x) for x in rng.choice(lq, size=k + n, replace=False))
            q = with_mismatches(rng, t, t, pos[:k])
            q[pos[k:]] = 4
            cs.add("a", "%s%s" % (sub, "" if loss == o.bound or sub == "a.above" else ".below"), t, q, 5)
    for m, n in ((20, 15), (7, 30), (33, 4), (12, 12)):
        for strand in (0, 1):
            cs.add("a", "a.tie", cat([2], [0] * m, [1] * n), cat([0] * m, [1] * n, [3]), 5, strand=strand)
            cs.add("a", "a.tie4", cat([2], [0] * m, [1] * n, [2] * 9), cat([0] * m, [1] * n, [2] * 9, [3]), 5, strand=strand)
    for _ in range(8):
        lq = int(rng.integers(40, 120))
        t = rng.integers(0, 4, size=lq).astype(np.uint8)
        q = with_mismatches(rng, t, t, np.nonzero(rng.random(lq) < 0.3)[0])
        cs.add("a", "a.w0", t, q, 0)
    for k in range(8):   # breadth: 0..7 mismatches, some of them N
        t = rng.integers(0, 4, size=76).astype(np.uint8)
        q = with_mismatches(rng, t, t, rng.choice(76, size=k, replace=False))
        if k & 1:
            q[int(rng.integers(76))] = 4
        cs.add("a", "a.k", t, q, 8)


# ---- family b
def family_b(cs, o, n_each=2):
    rng = cs.rng
    wmax4 = o.w << 2

    def one(sub, gs, w2=3, truesc=BIG, rel=None, g_del=None):
        t = rng.integers(0, 4, size=40 + 55 * len(gs)).astype(np.uint8)
        q, x = t, 12
        for g in gs:
            q = indel_pair(rng, q, x, g, 30, g_del)
            x += 55
        cs.add("b", sub, t, q, w2, truesc, rel=rel)
    for _ in range(n_each):
        for g in (4, 5, 6):
            one("b.r2", [g])                       # found in round 2 (w2 = 6)
            one("b.r3pair", [5, g + 4])            # round 2 finds the first pair and changes the score, round 3 (w2 = 12) the second
            one("b.r3alone", [g + 4])              # out of reach in rounds 1 and 2: a third round only if round 2 changed the score
            one("b.never", [g + 9])                # (12, 24]: ++i < 3 ends the loop first
            one("b.ts_stop", [g], rel=o.a)         # truesc = round-1 score + a: stops
            one("b.ts_go", [g], rel=o.a + 1)       # ... + a + 1: goes on
            one("b.d1", [g], g_del=g + 1)          # rlen = lq + 1: straight to the DP list
        for k, start in enumerate((wmax4, wmax4 >> 1, wmax4 >> 2)):   # w << 2 reached in round 1, 2, 3
            if start > 0:
                # a pair per later round, within reach of that round's band only, so that the score changes in the round that reaches
                # w << 2 and `w2 == w << 2` decides alone (small w only: the band stops growing at (max_gap + d + 1) >> 1)
                gs = [start << j for j in range(1, k + 1) if 3 < start << j <= 24] or [5]
                one("b.wmax%d" % (k + 1), gs, w2=start)
                one("b.wmax%d" % (k + 1), [5], w2=start, g_del=4)
        for k in range(8):      # bands from w << 2 upwards: all cut to w << 2, one round
            one("b.wmax1", [4 + k % 3], w2=wmax4 + (0, 1, 7, 50, wmax4, 1000)[k % 6], g_del=(None, 3)[k & 1])


# ---- family c
def gapped(rng, lq, rlen, n_mm=2, pair=0):
    """window of rlen bases and a read of lq: one gap of |rlen - lq| in the middle, n_mm mismatches, an indel pair of size `pair`"""
    t = rng.integers(0, 4, size=rlen).astype(np.uint8)
    d = rlen - lq
    x = min(lq, rlen) // 2
    q = cat(t[:x], t[x + d:]) if d >= 0 else cat(t[:x], rng.integers(0, 4, size=-d), t[x:])
    assert len(q) == lq
    if pair and lq > 40:
        q = indel_pair(rng, q, 5, pair, 12)
    for p in rng.choice(lq, size=min(int(n_mm), lq), replace=False):
        q[p] = (q[p] + 1) & 3
    return t, q


def family_c(cs, o):
    rng = cs.rng
    lq = 100
    for d in (0, 1, 20, 45):
        for rlen in ((lq,) if d == 0 else (lq + d, lq - d)):
            M = (max_gap(o, lq) + d + 1) >> 1
            for w2 in sorted({0, d + 2, d + 3, d + 4, M - 1, M, M + 1}):
                if w2 >= 0:
                    t, q = gapped(rng, lq, rlen, pair=2 if d == 0 else 0)
                    cs.add("c", "c.d%d" % d, t, q, w2)
    for d in (1, 5, 12):                   # a path that needs every column of the smallest band: d + 3 bases deleted, 3 inserted 30 bases on
        for _ in range(4):
            t = rng.integers(0, 4, size=110 + d).astype(np.uint8)
            q = cat(t[:40], t[40 + d + 3:73 + d], rng.integers(0, 4, size=3), t[73 + d:])
            cs.add("c", "c.minw", t, q, 0)
    for lq in (2, 3, 8, 9, 10):            # 2w + 1 = 9 crosses lq
        for rlen in (lq + 1, lq - 1):
            t, q = gapped(rng, lq, rlen, n_mm=0)
            cs.add("c", "c.cross", t, q, 4)
    for lq, rlen in ((1, 1), (1, 2), (1, 4), (2, 1), (5, 1), (2, 2), (3, 3), (3, 5), (2, 4), (3, 1)):
        for w2 in (0, 3):
            t, q = gapped(rng, lq, rlen, n_mm=lq == rlen)
            cs.add("c", "c.tiny", t, q, w2)
    for rlen in (63, 64, 65):
        for lq in (rlen - 1, rlen + 1, rlen):
            t, q = gapped(rng, lq, rlen, pair=3)
            cs.add("c", "c.rows", t, q, 10)
    for rlen in (149, 151, 150, 140):      # more than 64 columns: two strips per row (the 150 bp read also sets the batch's max_len)
        for w2 in (33, 40):
            t, q = gapped(rng, 150, rlen, pair=4)
            cs.add("c", "c.wide", t, q, w2, truesc=-BIG)    # one round: the doubled band would not fit the full-size matrix under a = 2


# ---- family d
def cap_shape(o, cap, max_len):
    """(lq, rlen, w2) with n_col * rlen == cap, whose neighbour with one row more has the same n_col: smallest |rlen - lq| first"""
    best = None
    for n_col in range(1, max_len + 1):
        if cap % n_col:
            continue
        rlen = cap // n_col
        if rlen + 1 > max_len + 256:
            continue
        for lq in range(n_col, max_len + 1):
            for w2 in ((n_col - 1) >> 1, 0, 10 ** 4):
                if band(o, lq, rlen, w2)[1] == n_col and band(o, lq, rlen + 1, w2)[1] == n_col:
                    key = (abs(rlen - lq), lq, rlen, w2)
                    best = key if best is None or key < best else best
                    break
    assert best is not None, (cap, max_len)
    return best[1:]


def outgrow_shape(o, max_len):
    """(lq, rlen, w2): round 1 fits the narrow band's matrix, round 2 (2 w2) only the full-size one"""
    lq = max_len - 10
    rlen = lq + 1
    for w2 in range(4, 200):
        n1, n2 = band(o, lq, rlen, w2)[1], band(o, lq, rlen, min(2 * w2, o.w << 2))[1]
        if n1 * rlen <= aln_zcap_small(max_len) < n2 * rlen <= aln_zcap(max_len):
            return lq, rlen, w2
    raise AssertionError(max_len)


def family_d(cs, o, max_len):
    rng = cs.rng
    cs.add("d", "d.longest", *gapped(rng, max_len, max_len + 2), 5)     # sets the batch's max_len
    for name, cap in (("small", aln_zcap_small(max_len)), ("full", aln_zcap(max_len))):
        lq, rlen, w2 = cap_shape(o, cap, max_len)
        for _ in range(2):     # (one round: a doubled band would be beyond the capacity the first round just meets)
            cs.add("d", "d.%s.at" % name, *gapped(rng, lq, rlen, n_mm=1), w2, truesc=-BIG)
            cs.add("d", "d.%s.over" % name, *gapped(rng, lq, rlen + 1, n_mm=1), w2, truesc=-BIG)
    lq, rlen, w2 = outgrow_shape(o, max_len)
    for _ in range(4):
        t, q = gapped(rng, lq, rlen, pair=2 * w2 - 1)      # the pair is within reach of round 2 only
        cs.add("d", "d.outgrow", t, q, w2)


# ---- family e
def alternating(rng, n_indel, first_ins, run=13, mm=0, del_len=1):
    """window and read that differ by n_indel single-base indels, insertions and deletions in turn, `run` bases apart;
    first_ins: the read starts with the first inserted base (an insertion first), else with a run; mm: every mm-th base of a run
    is a mismatch"""
    t, q = [], []

    def add_run():
        r = rng.integers(0, 4, size=run).astype(np.uint8)
        qr = r.copy()
        if mm:
            qr[1:-1:mm] = (qr[1:-1:mm] + 1 + rng.integers(0, 3, size=len(qr[1:-1:mm]))) & 3
        t.append(r); q.append(qr)
    for k in range(n_indel):
        if k or not first_ins:
            add_run()
        if k % 2 == 0:
            q.append(seq([other(rng, (t[-1][-1] if t else 0))]))
        else:
            t.append(cat([other(rng, q[-1][-1])], rng.integers(0, 4, size=del_len - 1)))
    add_run()
    return cat(*t), cat(*q)


def family_e(cs, o):
    rng = cs.rng
    for strand in (0, 1):
        cs.add("e", "e.cig96", *alternating(rng, 48, True), 3, strand=strand)
        cs.add("e", "e.cig97", *alternating(rng, 48, False), 3, strand=strand)
        cs.add("e", "e.cig95", *alternating(rng, 47, False), 3, strand=strand)
        # MD: "10" + 383 x "X0" + ... = 768 bytes; 384 mismatches in a row = 769
        t = rng.integers(0, 4, size=393).astype(np.uint8)
        cs.add("e", "e.md768", t, with_mismatches(rng, t, t, range(10, 393)), 0, strand=strand)
        t = rng.integers(0, 4, size=384).astype(np.uint8)
        cs.add("e", "e.md769", t, with_mismatches(rng, t, t, range(384)), 0, strand=strand)
        t = rng.integers(0, 4, size=393).astype(np.uint8)
        cs.add("e", "e.md.dp", t, with_mismatches(rng, t, t, range(10, 393)), 3, strand=strand)
        for g in (1, 7):
            t = rng.integers(0, 4, size=80 + g).astype(np.uint8)
            cs.add("e", "e.del_first", t, t[g:], g + 5, strand=strand)
            cs.add("e", "e.del_last", t, t[:-g], g + 5, strand=strand)
            cs.add("e", "e.del_both", cat(t, rng.integers(0, 4, size=g)), t[g:], 2 * g + 5, strand=strand)
            t = t[:80]
            ins = seq([other(rng, t[0])] * g)
            cs.add("e", "e.ins_first", t, cat(ins, t), g + 5, strand=strand)
            ins = seq([other(rng, t[-1])] * g)
            cs.add("e", "e.ins_last", t, cat(t, ins), g + 5, strand=strand)
    cs.add("e", "e.longest", *gapped(rng, 700, 702), 5)


# ---- family f
def family_f(cs, o):
    rng = cs.rng
    for u in (1, 2, 3, 4):
        unit = rng.permutation(4)[:u].astype(np.uint8)
        left, right = rng.integers(0, 4, size=25).astype(np.uint8), rng.integers(0, 4, size=25).astype(np.uint8)
        left[-1], right[0] = other(rng, unit[-1]), other(rng, unit[0])
        t = cat(left, np.tile(unit, 12), right)
        for strand in (0, 1):
            cs.add("f", "f.tandem.del", t, cat(left, np.tile(unit, 11), right), 10, strand=strand)
            cs.add("f", "f.tandem.ins", t, cat(left, np.tile(unit, 13), right), 10, strand=strand)
            cs.add("f", "f.tandem.both", t, cat(left[:10], left[10 + u:], np.tile(unit, 13), right), 10, strand=strand)
    L = cs.l_pac
    for strand in (0, 1):                   # forward: rb = 0 and re = l_pac; reverse: re = 2 l_pac and rb = l_pac
        t, q = gapped(rng, 60, 62)
        cs.add("f", "f.edge.first", t, q, 6, strand=strand, at=0)
        t, q = gapped(rng, 60, 59)
        cs.add("f", "f.edge.last", t, q, 6, strand=strand, at=L - 59)
        t = rng.integers(0, 4, size=50).astype(np.uint8)
        cs.add("f", "f.edge.first", t, t, 0, strand=strand, at=62)
    for lo, hi in ((L - 20, L + 30), (L - 1, L + 1), (L - 49, L + 1)):
        cs.raw("f", "f.bridging", rng.integers(0, 4, size=50).astype(np.uint8), lo, hi, 0, 50, 5)
    rd = rng.integers(0, 4, size=50).astype(np.uint8)
    cs.raw("f", "f.empty", rd, 5000, 5050, 10, 10, 5)           # lq = 0
    cs.raw("f", "f.empty", rd, 5000, 5000, 0, 50, 5)            # rb = re
    cs.raw("f", "f.overlong", rd, 3000, 3000 + 150 + 257, 0, 50, 5)   # rlen > max_len + 256 (family c's 150 bp reads are in the batch)
    cs.raw("f", "f.overlong", rd, 3000, 3000 + 150 + 256, 0, 50, 5)   # the longest window taken: its band matrix is beyond aln_zcap
    for strand in (0, 1):
        for sign in (1, -1):
            t, q = gapped(rng, 80, 80 + 3 * sign, n_mm=0)
            x = 40
            q[x - 1] = 4                    # N next to the gap
            q[10] = 4
            q[60] = other(rng, q[60])
            q[61] = 4                       # N next to a mismatch
            cs.add("f", "f.N", t, q, 8, strand=strand)
        cs.add("f", "f.clip", *gapped(rng, 70, 72), 6, strand=strand, head=rng.integers(0, 4, size=9), tail=rng.integers(0, 4, size=4))


# ---- sets
def cases(name):
    """families a, b, c, f under the option set `name`"""
    o = Opt(name)
    cs = Cases(1000 + sorted(OPTION_SETS).index(name))
    family_a(cs, o)
    family_b(cs, o)
    family_c(cs, o)
    family_f(cs, o)
    return o, cs


def cases_d(name, max_len):
    o = Opt(name)
    cs = Cases(2000 + max_len + sorted(OPTION_SETS).index(name))
    family_d(cs, o, max_len)
    return o, cs


def cases_e(name):
    o = Opt(name)
    cs = Cases(3000 + sorted(OPTION_SETS).index(name))
    family_e(cs, o)
    return o, cs


LAUNCH_SIZES = (1, 63, 64, 65, 255, 256, 257)


def cases_g(name):
    """a pool of 257 mixed requests (its first n are the launches of n requests) and the interleaved launch"""
    o = Opt(name)
    cs = Cases(4000 + sorted(OPTION_SETS).index(name))
    rng = cs.rng
    for i in range(257):
        lq = int(rng.integers(30, 120))
        kind = i % 3
        if kind == 0:      # same length within the bound
            t = rng.integers(0, 4, size=lq).astype(np.uint8)
            cs.add("g", "g.same", t, with_mismatches(rng, t, t, rng.choice(lq, size=int(rng.integers(0, 2)), replace=False)), 5)
        elif kind == 1:    # one gap
            cs.add("g", "g.gap", *gapped(rng, lq, lq + int(rng.choice([-3, -1, 1, 2, 8]))), 12)
        else:              # same length beyond the bound: moved to the DP list
            t = rng.integers(0, 4, size=lq).astype(np.uint8)
            cs.add("g", "g.moved", t, indel_pair(rng, t, 8, 2, 10), 5)
    same = [i for i in range(257) if i % 3 == 0]
    dp = [i for i in range(257) if i % 3 == 1]
    U = -1
    # waves of aln_classify_kernel (64 consecutive requests) that hold 64, 0, 63, 1 members of a kind, 64 unused slots in a row, sprinkled ones
    order = same[:64] + dp[:64] + same[:63] + dp[:1] + same[:1] + dp[:63] + [U] * 64
    mixed = [same[k % len(same)] if k % 5 < 2 else dp[k % len(dp)] if k % 5 < 4 else U for k in range(64 * 3 + 17)]
    order += mixed
    return o, cs, order


def with_unused(cs, order):
    c = cs.order([])
    for i in order:
        if i < 0:
            c.unused()
        else:
            for k in ("rb", "re", "read", "qb", "qe", "w2", "truesc", "rel", "fam", "sub"):
                getattr(c, k).append(getattr(cs, k)[i])
    return c


def cases_reuse(name):
    """distinct short requests of every kind, to be repeated (reuse_order) until every wave of every instantiation has had two; a 700 bp
    read makes the grids of the DP instantiations small (their LDS grows with the batch's longest read)"""
    o = Opt(name)
    cs = Cases(5000 + sorted(OPTION_SETS).index(name), L_PAC_REUSE)
    rng = cs.rng
    for i in range(900):      # list 0, answered there
        lq = int(rng.integers(30, 51))
        t = rng.integers(0, 4, size=lq).astype(np.uint8)
        q = with_mismatches(rng, t, t, rng.choice(lq, size=int(rng.integers(0, 3)), replace=False))
        cs.add("g", "g.reuse.same", t, q, int(rng.choice([0, 5, 5, 40])))
    for i in range(60):       # long MD: all mismatches, w2 = 0
        lq = int(rng.integers(30, 51))
        t = rng.integers(0, 4, size=lq).astype(np.uint8)
        cs.add("g", "g.reuse.longmd", t, with_mismatches(rng, t, t, range(lq)), 0)
    for i in range(300):      # DP list: one or two gaps
        lq = int(rng.integers(30, 51))
        cs.add("g", "g.reuse.gap", *gapped(rng, lq, lq + int(rng.choice([-5, -2, -1, 1, 2, 3, 9])), n_mm=int(rng.integers(0, 3))), int(rng.choice([3, 8, 20])))
    for i in range(100):      # moved from list 0
        lq = int(rng.integers(36, 51))
        t = rng.integers(0, 4, size=lq).astype(np.uint8)
        cs.add("g", "g.reuse.moved", t, indel_pair(rng, t, 6, int(rng.integers(1, 4)), 12), 5)
    # records of most of a slab (80 to 86 CIGAR operations and about 450 MD bytes: 780 of ALN_SLAB = 1024 bytes), so that the slab a wave holds is
    # often too small for its next record.  A record of MORE than a slab (`take > ALN_SLAB`) needs 96 operations and over 640 MD bytes in
    # a read whose band matrix still fits: a sweep over indel counts, run lengths and mismatch densities found none under the default scores.
    for k in range(6):
        t, q = alternating(rng, 40, True, run=16, mm=3)
        cs.add("g", "g.reuse.big", t, q, 3)
    cs.add("g", "g.reuse.longest", *gapped(rng, 700, 701), 5)
    return o, cs


def reuse_order(cs, pred, cus, seed=7):
    """request numbers of cs, repeated and shuffled, so that list 0 and the DP list (narrow under which = 0, full size under which = 1)
    are longer than twice the grid launch_aln gives them"""
    lds = lds_bytes(cs.max_len)
    in0 = [i for i in range(len(cs)) if pred[i].lists[0] and not pred[i].moved]
    dp = [i for i in range(len(cs)) if not pred[i].lists[0] or pred[i].moved]
    big = 1 << 30
    n0 = 2 * grid_for(lds[0], cus, big) + 1500
    n_dp = 2 * max(grid_for(lds[1], cus, big), grid_for(lds[2], cus, big)) + 500
    rng = np.random.default_rng(seed)
    order = [in0[k % len(in0)] for k in range(n0)] + [dp[k % len(dp)] for k in range(n_dp)]
    order = [order[k] for k in rng.permutation(len(order))]
    return order


# ---------------------------------------------------------------- the reference's rounds and the prediction
class Rounds:
    """bwa_gen_cigar2 of the reference per request and band, computed once"""

    def __init__(self, ri, ropt, cs):
        self.ri, self.ropt, self.cs = ri, ropt, cs
        self.memo = {}

    def __call__(self, i, w2):
        cs = self.cs
        key = (cs.rb[i], cs.re[i], cs.read[i], cs.qb[i], cs.qe[i], w2)
        if key not in self.memo:
            self.memo[key] = self.ri.gen_cigar2(self.ropt, cs.l_pac, cs.pac, cs.query(i), cs.rb[i], cs.re[i], w2)
        return self.memo[key]

    def loop(self, i):
        """the answer to request i: oracle/pyoracle.py: reg2aln_loop, the loop that tests/test_aln_cases.py pins to the reference's own
        mem_reg2aln — the expected value of every comparison with the kernel"""
        cs = self.cs
        key = (cs.rb[i], cs.re[i], cs.read[i], cs.qb[i], cs.qe[i], cs.w2[i], cs.truesc[i], "loop")
        if key not in self.memo:
            self.memo[key] = self.ri.reg2aln_loop(self.ropt, cs.l_pac, cs.pac, cs.query(i), cs.rb[i], cs.re[i], cs.w2[i], cs.truesc[i])
        return self.memo[key]


def fix_truesc(cs, o, rounds):
    for i in range(len(cs)):
        if cs.rel[i] is not None:
            cs.truesc[i] = rounds(i, min(cs.w2[i], o.w << 2))[0] + cs.rel[i]


class Pred:
    """flags: -1 unused slot, 0 answered, 1 declined.  cls: unused / invalid / nodp / narrow / full / declined.  lists: which of the
    three request lists the request was ever on; moved: from list 0 to the DP list; why: the reason of a decline; rounds: the executed
    rounds of the instantiation that answered, [(w2, n_col, score)]; stop: the four conditions of the loop at its end (score == last_sc,
    w2 == w << 2, i == 3, score >= truesc - a); last: (score, cigar, NM, MD) of the last round of that walk, which decides the class;
    result: the expected answer, (score, cigar, NM, MD) of pyoracle's reg2aln_loop (Rounds.loop) — tests/test_aln_cases.py asserts that
    the two agree for every answered request; need: pool bytes"""

    def __init__(self):
        self.flags, self.cls, self.lists, self.moved, self.why, self.rounds, self.stop, self.result, self.need = 0, "", [0, 0, 0], False, None, [], None, None, 0
        self.last = None


def predict(cs, o, rounds, which):
    max_len = cs.max_len
    tcap = max_len + 256
    caps = {1: aln_zcap_small(max_len), 2: aln_zcap(max_len)}
    wmax4 = o.w << 2
    dp_kind = 2 if which else 1
    out, counts = [], [0, 0, 0]

    def run_dp(i, kind, p):
        lq, rlen = cs.qe[i] - cs.qb[i], cs.re[i] - cs.rb[i]
        w2, last, it = cs.w2[i], -(1 << 30), 0
        p.rounds = []
        while True:
            w2 = min(w2, wmax4)
            n_col = band(o, lq, rlen, w2)[1]
            if n_col * rlen > caps[kind]:
                return "zcap"
            res = rounds(i, w2)
            p.rounds.append((w2, n_col, res[0]))
            if len(res[1]) > ALN_CIGCAP:
                return "cigar"
            p.last = res
            p.stop = (res[0] == last, w2 == wmax4, it + 1 >= 3, not res[0] < cs.truesc[i] - o.a)
            # (`w2 == wmax4` is an early exit, not a decision: without it the next round runs with the same w2, gives the same score and
            # ends on `res[0] == last` — no test of outputs can tell a kernel without it apart, which is why that mutation fails nothing)
            if res[0] == last or w2 == wmax4:
                return None
            last = res[0]
            w2 <<= 1
            it += 1
            if not (it < 3 and res[0] < cs.truesc[i] - o.a):
                return None

    for i in range(len(cs)):
        p = Pred()
        out.append(p)
        if cs.read[i] < 0:
            p.flags, p.cls = -1, "unused"
            continue
        lq, rlen = cs.qe[i] - cs.qb[i], cs.re[i] - cs.rb[i]
        bridging = cs.rb[i] < cs.l_pac < cs.re[i]
        if lq <= 0 or rlen <= 0 or bridging or lq > max_len or rlen > tcap:
            p.flags, p.cls, p.why = 1, "invalid", "bridging" if bridging else "empty" if lq <= 0 or rlen <= 0 else "overlong"
            p.lists[dp_kind] = 1       # not of the same length as far as aln_classify_kernel is concerned
            continue
        if lq == rlen:
            p.lists[0] = 1
            w2 = min(cs.w2[i], wmax4)
            score = int(o.mat[cs.window(i), cs.query(i)].sum())
            if w2 == 0 or lq * o.a - score <= o.bound:
                p.cls = "nodp"
                p.rounds = [(w2, 0, score)]
            else:
                p.moved = True
        if p.cls != "nodp":
            kind = dp_kind
            p.lists[kind] = 1
            why = run_dp(i, kind, p)
            if why is not None and kind == 1:
                kind = 2
                p.lists[2] = 1
                why = run_dp(i, kind, p)
            if why is not None:
                p.flags, p.cls, p.why = 1, "declined", why
                continue
            p.cls = "narrow" if kind == 1 else "full"
        p.result = rounds.loop(i)      # (a no-DP answer included: the reference runs its DP for it when w2 > 0)
        if len(p.result[3]) > ALN_MDCAP:
            p.flags, p.cls, p.why = 1, "declined", "md"
            continue
        p.need = 4 * len(p.result[1]) + ((len(p.result[3]) + 3) & ~3)
    for p in out:
        for k in range(3):
            counts[k] += p.lists[k]
    return out, counts


# ---------------------------------------------------------------- mem_reg2aln itself (the pin of reg2aln_loop)
PIN_SETS = {"default": {}, "w2": dict(w=2), "combined": OPTION_SETS["combined"], "w6": dict(w=6)}


def pin_regions(o, contig, n=40, seed=77):
    """regions of family b planted on a contig that starts the index (rid 0, offset 0), as mem_reg2aln takes them:
    [(what, read, rb, re as forward-strand coordinates, qb, qe, truesc, w, reverse, rel)].
    "pair": insertion + deletion pairs of 3..12 bases, truesc chosen so that the inferred band starts between 0 and about 30, clipped
    reads, both strands, leading deletions.  With w <= 8 also, all with the region's w = 3 and a truesc low enough that the inferred band
    is beyond opt.w, so that the loop starts at 3 (src/bwamem.c:1112) and w << 2 does not end it before its third round:
    "ts_stop" / "ts_go": one pair of 5 (out of reach of band 3, found with 6) and rel = a / a + 1: the caller sets truesc = the round-1 score
    + rel, on either side of `score < truesc - a`;
    "round4": pairs of 5, 9 and 16 — the third within reach of a fourth round only (w2 = 24), which `++i < 3` never runs"""
    rng = np.random.default_rng(seed)
    out = []

    def window(L):
        while True:
            p = int(rng.integers(100, len(contig) - 400))
            t = np.asarray(contig[p:p + L], dtype=np.uint8)
            if not (t > 3).any():
                return p, t
    while len(out) < n:
        p, t = window(int(rng.integers(80, 140)))
        L = len(t)
        k = len(out)
        g = int(rng.integers(3, 13))
        q = indel_pair(rng, t, 10, g, 30, g + (k % 3) - 1 if k % 4 == 3 else None)
        if k % 5 == 4:
            q = t[1:] if k % 2 else cat(t, [other(rng, t[-1])])[1:]          # a leading deletion (squeezed), with an insertion last
        head = rng.integers(0, 4, size=int(rng.integers(0, 8)) * (k % 2)).astype(np.uint8)
        tail = rng.integers(0, 4, size=int(rng.integers(0, 8)) * (k % 3 == 0)).astype(np.uint8)
        truesc = len(q) * o.a - int(rng.choice([0, 3, 7, 9, 12, 20, 33]))
        out.append(("pair", cat(head, q, tail), p, p + L, len(head), len(head) + len(q), truesc, int(rng.choice([2, 5, 100])), k % 2 == 1, None))
    if 6 <= o.w <= 8:
        for k in range(24):
            what = ("ts_stop", "ts_go", "round4")[k % 3]
            gs = [5, 9, 16] if what == "round4" else [5]
            p, t = window(40 + 55 * len(gs))
            q, x = t, 12
            for g in gs:
                q = indel_pair(rng, q, x, g, 30)
                x += 55
            rel = {"ts_stop": o.a, "ts_go": o.a + 1, "round4": None}[what]
            out.append((what, q, p, p + len(t), 0, len(q), len(q) * o.a - 20 * o.a - o.o_del - o.o_ins, 3, k % 2 == 1, rel))
    return out
