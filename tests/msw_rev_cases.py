"""Mate-rescue requests for the second pass as msw_rev2_kernel runs it (msw_kernel.hip: the reverse passes two per quad, the two of one
class, the classes made by a stable sort of one byte per request), on top of tests/msw_cases.py: its generator, its expected results,
its comparison.  Shared by tests/test_msw_rev_cases.py (CPU: by the reference's ksw_align2 alone every family reaches what it is for)
and tests/test_gpu_msw_rev.py (the kernels against it, against the run with MPIBWA_MSW_REV2=0, and the work items the device ran
against plan()).

plan() is the device's rule restated: a byte-flavour request that reaches min_seed_len * a unsaturated has the class
1 + 3 (qe // 16) + (score >= 80 a ? 2 : score >= 40 a ? 1 : 0); consecutive members of a class in request order are a pair, an odd
last one rides alone.  It is a function of the results, so the expected results predict it.

Families (built per option set: the byte flavour ends at qlen * a = 250 and a hit starts at min_seed_len * a):
  borders  for reads of 76, 150 and 248 bp (as far as the byte flavour reaches; else its longest read) exact stretches that end on
           qe = 16 s - 1 and on qe = 16 (s - 1) for every segment length s of the reverse pass, s = 1 with qe = 0, 1 and 15 included,
           in three score classes, every one twice (once in a random window, once over two disjoint alphabets, where nothing
           extends the stretch by chance), in reads of their own and both orientations.  What no hit can reach (a stretch
           of qe + 1 < min_seed_len bases) is listed in cs.unreachable and asserted to be exactly that.
  unequal  partners of one class of which one is done long before the other (reads over {A, C} in windows over {G, T}: the scores
           are exact): a stretch that just reaches the score class against the whole read; the same with the short one at the very start of its window (te + 1 rows and not one more); reads that are a
           unit twice over (rows past the stop that reach the maximum again).  cs.partners lists who must share a quad.
           Not constructible, and asserted so: te = 0 (one row scores at most max(mat) < min_seed_len * a) — and, for the record, rows
           past the stop that would RAISE a half's maximum: every cell of the reverse pass is a local alignment inside the forward
           pass's rectangle, so none exceeds the forward score.
  quirks   gaps in the reverse direction: insertion runs laid across every offset around a segment end, deletions next to it, reads
           with N inside the prefix 0..qe and right behind qe
  ceiling  (b >= 8) stretches that score just below 255 - shift next to plain ones and to exact reads at the ceiling: a request whose
           forward pass saturates has no class, and no reverse pass can saturate below it (see above), so a quad never mixes the two
  sizes    classes of exactly 1, 2, 3, 31, 32 and 33 members (reads over {A, C} in windows over {G, T}: score and qe are exact),
           interleaved so that the sort has something to do: alone-riders, a wave of 16 pairs, one pair more
  single   a call with one request
  mixed    msw_regs_cases' three read lengths in one call: register and general forward launches feed one sort"""
import zlib

import numpy as np

import msw_cases as mc
import msw_regs_cases as rc

N_CLASSES = 48
ALL_SETS = tuple(mc.OPTION_SETS)
FAMILY_SETS = dict(borders=ALL_SETS, unequal=ALL_SETS, quirks=("default", "a2b3"), ceiling=("sat", "b9"), sizes=("default",), single=("default",),
                   mixed=("default",))
SIZES = {(2, 0): 1, (3, 0): 2, (4, 1): 3, (5, 1): 31, (6, 2): 32, (8, 2): 33}   # (qe // 16, score class) -> members


def all_cases():
    return [(f, n) for f, names in FAMILY_SETS.items() for n in names]


def rev_class(score, qe, a):
    """msw_rev_class (msw_kernel.hip)"""
    return 1 + (qe >> 4) * 3 + (2 if score >= 80 * a else 1 if score >= 40 * a else 0)


def plan(want):
    """what the second pass runs on the expected results -> dict(cls: per request, 0 = none; members: {class: requests in order};
    pairs: [(A, B)]; alone: [A]; counts: [pairs, alone-riders, items of a register launch, items of the general launch])"""
    cs, res = want.cs, want.res
    minsc = cs.o["min_seed_len"] * cs.o["a"]
    cls = np.zeros(len(cs), dtype=np.int32)
    for i in range(len(cs)):
        if want.byte[i] and not want.sat[i] and res[i][0] >= minsc:
            cls[i] = rev_class(int(res[i][0]), int(res[i][2]), cs.o["a"])
    members = {int(c): [int(i) for i in np.nonzero(cls == c)[0]] for c in sorted(set(cls.tolist()) - {0}, reverse=True)}
    pairs = [(m[k], m[k + 1]) for m in members.values() for k in range(0, len(m) - 1, 2)]
    alone = [m[-1] for m in members.values() if len(m) & 1]
    return dict(cls=cls, members=members, pairs=pairs, alone=alone, counts=[len(pairs), len(alone), 0, len(pairs) + len(alone)])


class _Gen(mc._Gen):
    def __init__(self, name, family):
        super().__init__(name)
        self.rng = np.random.default_rng(zlib.crc32(("rev/%s/%s" % (family, name)).encode()))
        self.fwd = self.rng.integers(0, 4, size=mc.L_PAC).astype(np.uint8)
        cs = self.cs
        cs.unreachable, cs.partners, cs.tag = [], [], {}
        self.n_req = 0

    def finish(self):
        self.cs.fwd = self.fwd
        return self.cs

    def lengths(self):
        """the reads of 76, 150 and 248 bp the byte flavour takes under this set; its longest read where it does not take 248"""
        out = [L for L in (76, 150, 248) if L * self.o["a"] < 250]
        return out if 248 in out else out + [self.Lb]

    def stretch(self, q, rev, s0, qe, p=None, tl=None, tag=None, two=False):
        """one request in a read of its own: the bases s0..qe of the oriented query q, exactly, at row p of a window of tl rows (two:
        over {G, T}), between two bases that do not extend it -> the request's index"""
        cs, rng = self.cs, self.rng
        ql, L = len(q), qe - s0 + 1
        qn = np.minimum(q, 3)
        tl = ql + int(rng.integers(20, 120)) if tl is None else tl
        win = (2 + self.rand(tl, 2)).astype(np.uint8) if two else self.rand(tl)
        p = int(rng.integers(1, tl - L)) if p is None else p
        assert 0 <= s0 <= qe < ql and 0 <= p and p + L <= tl
        win[p:p + L] = qn[s0:qe + 1]
        if not two:
            if s0 > 0 and p > 0:
                win[p - 1] = (qn[s0 - 1] + 1) & 3
            if qe + 1 < ql and p + L < tl:
                win[p + L] = (qn[qe + 1] + 2) & 3
        cs.reads.append(q if not rev else mc.rc(q))
        rb, re = self.put(win)
        i = len(cs)
        cs.rb.append(rb); cs.re.append(re); cs.rd.append(len(cs.reads) - 1); cs.rev.append(int(rev)); cs.kind.append("stretch"); cs.unit.append(0)
        if tag is not None:
            cs.tag[i] = tag
        return i

    def borders(self):
        msl = self.o["min_seed_len"]
        n = 0
        for L in self.lengths():
            for s in range(1, (L + 15) // 16 + 1):
                for qe in ([0, 1, 15] if s == 1 else [16 * (s - 1), min(16 * s - 1, L - 1)]):
                    qe = min(qe, L - 1)
                    if qe + 1 < msl:
                        self.cs.unreachable.append(("borders", L, s, qe))
                        continue
                    for Lh in sorted({min(max(msl, x), qe + 1) for x in (msl, 45, 85)}):
                        for twice in range(2):
                            n += 1
                            # (the second copy over {A, C} in a window over {G, T}: no chance extension moves its qe)
                            self.stretch(self.read(L, "two" if twice else "random"), n & 1, qe - Lh + 1, qe, tag=("border", L, s, qe), two=bool(twice))
        return self.finish()

    def unequal(self):
        cs, o = self.cs, self.o
        msl = o["min_seed_len"]
        cs.unreachable.append(("unequal", "te = 0"))
        n = 0
        top = (255 - max(o["b"], 1) - 1) // o["a"]          # the longest read whose exact hit stays below 255 - shift
        for L in sorted({min(76, self.Lb, top), min(self.Lu, top)}):
            edge = max(msl, 80 if L >= 80 else 40 if L >= 40 else 0)   # the fewest bases of the score class of the whole read
            assert edge + 1 < L
            for short_at_start in (False, True):
                for short_first in (True, False):
                    n += 1
                    tl = L + 100
                    ends = [(L - 1 - edge, 0 if short_at_start else int(self.rng.integers(1, 20))), (0, tl - L - 2)]
                    pair = []
                    for k, (s0, p) in enumerate(ends if short_first else ends[::-1]):
                        pair.append(self.stretch(self.read(L, "two"), (n + k) & 1, s0, L - 1, p=p, tl=tl, tag=("unequal", L, s0, p), two=True))
                    cs.partners.append(tuple(pair))
        for it, L in enumerate((self.Lu, self.Lu)):
            if L >= 2 * msl + 3:
                self.run(self.read(L, "tandem"), it & 1, ["unit"] * 2)
        return self.finish()

    def quirks(self):
        cs, rng, L = self.cs, self.rng, self.Lu
        s = (L + 15) // 16
        for it in range(3 * s):           # an insertion run (bases of the read the window lacks) starting at every offset around a segment end
            g = 2 + it % 5
            c = 4 * s + it - s
            q = self.read(L, "N" if it % 4 == 3 else "random")
            win = self.rand(L + 40)
            self.plant(win, int(rng.integers(0, 40)), np.concatenate([q[:c], q[c + g:]]))
            self.raw(q, it & 1, win, ("ins", c, g))
        for it in range(3 * s):           # a deletion (bases of the window the read lacks) at every offset around a segment end
            g = 1 + it % 4
            c = 7 * s + it - s
            q = self.read(L)
            win = self.rand(L + 60)
            self.plant(win, int(rng.integers(0, 40)), np.concatenate([q[:c], self.rand(g), q[c:]]))
            self.raw(q, it & 1, win, ("del", c, g))
        for it in range(12):              # N inside the prefix 0..qe, and right behind qe
            q = self.read(L)
            qe = int(rng.integers(60, L - 2))
            if it & 1:
                q[qe + 1] = 4
            else:
                q[qe - int(rng.integers(3, 30))] = 4
            self.stretch(q, (it >> 1) & 1, qe - 50, qe, tag=("N", it & 1))
        return self.finish()

    def raw(self, q, rev, win, tag):
        cs = self.cs
        cs.reads.append(q if not rev else mc.rc(q))
        rb, re = self.put(win)
        cs.tag[len(cs)] = tag
        cs.rb.append(rb); cs.re.append(re); cs.rd.append(len(cs.reads) - 1); cs.rev.append(int(rev)); cs.kind.append(tag[0]); cs.unit.append(0)

    def ceiling(self):
        cs, o = self.cs, self.o
        a, Lb = o["a"], self.Lb
        top = (255 - max(o["b"], 1) - 1) // a          # the most matching bases that stay below 255 - shift
        cs.unreachable.append(("ceiling", "a saturating and a plain partner in one quad"))
        assert top < Lb, (top, Lb)
        for it in range(8):
            self.stretch(self.read(Lb), it & 1, Lb - 1 - top + 1, Lb - 1, tag=("top",))           # just below the ceiling
            self.stretch(self.read(Lb), ~it & 1, Lb - 1 - (top - it) + 1, Lb - 1, tag=("plain",))   # its neighbour in the list
            self.run(self.read(Lb), it & 1, ["clean", "miss"])                                       # at the ceiling: no class
        return self.finish()

    def sizes(self):
        todo = []
        for (sq, sb), n in SIZES.items():
            Lh = (25, 45, 85)[sb]
            assert Lh <= 16 * sq + 8
            todo += [(16 * sq + 7, Lh)] * n
        for k in self.rng.permutation(len(todo)):
            qe, Lh = todo[k]
            self.stretch(self.read(150, "two"), int(k) & 1, qe - Lh + 1, qe, two=True, tag=("size", qe >> 4, Lh))
        return self.finish()

    def single(self):
        self.stretch(self.read(150), 1, 0, 149)
        return self.finish()


_CACHE = {}


def cases(family, name):
    """the requests of a family under an option set, once per process; nobody changes them"""
    if family == "mixed":
        return rc.cases("mixed", name)
    if (family, name) not in _CACHE:
        _CACHE[family, name] = getattr(_Gen(name, family), family)()
    return _CACHE[family, name]
