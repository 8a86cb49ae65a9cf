"""Mate-rescue requests for the register form of msw2_kernel (msw_kernel.hip: one instantiation per segment length, launch_msw sorts
the work items by it), on top of tests/msw_cases.py: its generator, its expected results and its comparison.  Shared by
tests/test_msw_regs_cases.py (CPU: the families contain what they claim, by the host's and the reference's ksw_align2) and
tests/test_gpu_msw_regs.py (the kernels against both, and against the run with MPIBWA_MSW_REGS=0).

Families (a few hundred requests each, built per option set because the byte flavour ends at qlen * a = 250):
  boundary  for every instantiated segment length SLEN the read lengths 16 SLEN - 15, one in between and 16 SLEN (as far as the byte
            flavour reaches): padding positions take part in the row maxima at both extremes; lengths without an instantiation
  quads     runs of 1, 2, 3 and 50 windows for one mate (full quads, a lone (k, -1) item, an odd tail); in a pair windows of 1 row,
            shorter than the read, MAX_EXTRA longer; an empty window next to a real one
  mixed     three read lengths interleaved run by run, two with an instantiation and one without: the sort by length, several
            launches sharing the tail lists, the general kernel behind them
  scores    exact mates, chance-only windows, (b >= 6) a score at the 8-bit ceiling, long gaps, tandem and low-complexity reads, and
            insertion runs that cross the end of a segment, where F_seg and F_full part"""
import zlib

import numpy as np

import msw_cases as mc

REGS_SLEN = (5, 7, 8, 10, 13, 16)         # msw_regs_slen (msw_kernel.hip)
OPTION_SETS = ("default", "a2b3", "b9")   # the defaults; a, the mismatch (shift 3) and all four gap costs moved; shift 9 (the ceiling in reach)
FAMILIES = ("boundary", "quads", "mixed", "scores")


def slen_of(qlen):
    return (qlen + 15) // 16


def launch_of(qlen, a):
    """where launch_msw sends a request of a read of qlen bases: 'word' (msw_kernel), the segment length of a register instantiation,
    or 0 (the general form of msw2_kernel)"""
    if qlen * a >= 250:
        return "word"
    return slen_of(qlen) if slen_of(qlen) in REGS_SLEN else 0


def launch_plan(cs):
    """launch_msw's plan from the lengths alone -> {launch_of: [work items]} in list order, and the order of the register launches
    (falling count, ties in the order of REGS_SLEN)"""
    items, word = mc.work_list(cs)
    plan = {}
    for it in items:
        plan.setdefault(launch_of(len(cs.reads[cs.rd[it[0]]]), cs.o["a"]), []).append(it)
    if word:
        plan["word"] = word
    order = sorted((s for s in plan if s not in (0, "word")), key=lambda s: (-len(plan[s]), REGS_SLEN.index(s)))
    return plan, order


def boundary_lengths(name):
    """{SLEN: lengths} of the instantiations the byte flavour reaches under the option set"""
    Lb = (250 + mc.options(name)["a"] - 1) // mc.options(name)["a"] - 1
    out = {}
    for s in REGS_SLEN:
        lens = sorted({L for L in (16 * s - 15, 16 * s - 7, min(16 * s, Lb)) if 16 * s - 15 <= L <= Lb})
        if lens:
            out[s] = lens
    return out


def other_lengths(name):
    """byte-flavour lengths whose segment length has no instantiation"""
    Lb = (250 + mc.options(name)["a"] - 1) // mc.options(name)["a"] - 1
    return [L for L in (33, 90, 96, 176, 161, 224) if L <= Lb and slen_of(L) not in REGS_SLEN]


class _Gen(mc._Gen):
    def __init__(self, name, family):
        super().__init__(name)
        self.rng = np.random.default_rng(zlib.crc32(("regs/%s/%s" % (family, name)).encode()))
        self.fwd = self.rng.integers(0, 4, size=mc.L_PAC).astype(np.uint8)
        self.cs.border = {}               # request -> (first inserted query position, length of the run, segment length)

    HITS = ["clean", "mut", "tail", "miss", "ins:3", "del:5", "second:b1", "second:a1", "miss", "mut", "ins:9", "del:2", "second:x", "clean"]

    def take(self, n):
        at = getattr(self, "_at", 0)
        self._at = at + n
        return [self.HITS[(at + i) % len(self.HITS)] for i in range(n)]

    def finish(self):
        self.cs.fwd = self.fwd
        return self.cs

    def boundary(self):
        rng = self.rng
        for s, lens in boundary_lengths(self.cs.name).items():
            for L in lens:
                for it in range(3):
                    self.run(self.read(L, "N" if it == 1 else "random"), int(rng.integers(0, 2)), self.take((4, 3, 2)[it]))
                # the read's last base decides the maximum: an exact hit ends on position L - 1, next to the padding
                self.run(self.read(L), 1, ["clean", "clean"])
        for L in other_lengths(self.cs.name):
            for it in range(2):
                self.run(self.read(L), it, self.take(3 + it))
        return self.finish()

    def quads(self):
        rng, Lu = self.rng, self.Lu
        for n in (1, 2, 3, 50, 1, 3, 2, 50):
            self.run(self.read(Lu), int(rng.integers(0, 2)), self.take(n))
        L2 = boundary_lengths(self.cs.name)[7][0]
        for n in (1, 3, 50, 2):
            self.run(self.read(L2), int(rng.integers(0, 2)), self.take(n))
        # in a pair: windows of 1 row, shorter than the read, MAX_EXTRA longer — on either side
        for tls in ([1, Lu + mc.MAX_EXTRA], [Lu + mc.MAX_EXTRA, 1], [Lu - 20, Lu + mc.MAX_EXTRA], [Lu + mc.MAX_EXTRA, Lu // 3], [1, 1], [Lu + 40, Lu + mc.MAX_EXTRA]):
            kinds = ["fill" if t < Lu else "mut" for t in tls]
            self.run(self.read(Lu), int(rng.integers(0, 2)), kinds, tls=tls)
        # an empty window next to a real one: neither pairs up
        for kinds, tls in ((["empty", "clean"], [0, Lu + 80]), (["mut", "empty"], [Lu + 80, 0]), (["clean", "empty", "tail"], [Lu + 60, 0, Lu + 90])):
            self.run(self.read(Lu), int(rng.integers(0, 2)), kinds, tls=tls)
        return self.finish()

    def mixed_lengths(self):
        b = boundary_lengths(self.cs.name)
        return b[max(b)][-1], b[7][1], other_lengths(self.cs.name)[0]

    def mixed(self):
        rng = self.rng
        lens = self.mixed_lengths()
        for it in range(120):
            L = lens[it % 3]
            self.run(self.read(L), int(rng.integers(0, 2)), self.take(1 + (it // 3) % 3))
        return self.finish()

    def border_ins(self, L, rev):
        """a read whose window lacks g of its bases, the run laid across the end of a segment"""
        rng, cs = self.rng, self.cs
        q = self.read(L)
        s = slen_of(L)
        g = int(rng.integers(3, 9))
        B = int(rng.integers(3, (L - g - 9) // s + 1)) * s     # position B - 1 ends a segment
        c = B - 1 - int(rng.integers(0, g - 1))                # the run covers B - 1 and B
        assert 8 <= c <= B - 1 and c + g - 1 >= B and c + g + 8 <= L
        win = self.rand(L + 60)
        self.plant(win, int(rng.integers(0, 60 + g)), np.concatenate([q[:c], q[c + g:]]))
        cs.reads.append(q if not rev else mc.rc(q))
        rb, re = self.put(win)
        cs.border[len(cs)] = (c, g, s)
        cs.rb.append(rb); cs.re.append(re); cs.rd.append(len(cs.reads) - 1); cs.rev.append(int(rev)); cs.kind.append("border"); cs.unit.append(0)

    def scores(self):
        rng, Lu, Lb = self.rng, self.Lu, self.Lb
        for it in range(12):
            self.run(self.read(Lu), it & 1, ["clean", "clean", "miss", "miss"])
        # the longest byte-flavour read, exact: qlen * a, which is the ceiling 255 - shift where b >= 6
        for it in range(4):
            self.run(self.read(Lb), it & 1, ["clean", "miss", "clean"])
        gaps = ["ins:%d" % g for g in (12, 16, 20, 24)] + ["del:%d" % g for g in (12, 16, 20, 24)]
        for it in range(8):
            self.run(self.read(Lu), it & 1, [gaps[it], gaps[(it + 3) % 8]])
        for it, L in enumerate((Lu, Lb, Lu - 1, Lu)):
            self.run(self.read(L, "tandem"), it & 1, ["unit"] * 3)
        for it in range(3):
            self.run(self.read(Lu, "lowcx"), it & 1, ["lowcx", "lowcx", "miss"])
        for it in range(40):
            self.border_ins((Lu, Lb, boundary_lengths(self.cs.name)[7][0])[it % 3], it & 1)
        return self.finish()


_CACHE = {}


def cases(family, name):
    """the requests of a family under an option set, once per process; nobody changes them"""
    if (family, name) not in _CACHE:
        _CACHE[family, name] = getattr(_Gen(name, family), family)()
    return _CACHE[family, name]


def all_cases():
    return [(f, n) for f in FAMILIES for n in OPTION_SETS]
