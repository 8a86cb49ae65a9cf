"""Mate-rescue requests on which the scoring options decide the outcome: the cases, the option sets and the comparison shared by
tests/test_msw_cases.py (CPU: the library's host ksw_align2 equals the reference's under every set, and the reference's own results
show that the inputs reach what they are there for) and tests/test_gpu_msw_options.py (msw2_kernel, msw_tail_kernel and msw_kernel
against both).

A case set is built per option set, because what a case is depends on the options: the byte / word flavour changes at
qlen * a = 250, a hit counts from min_seed_len * a, the second-best window is te +- ceil(score / a).  The reference sequence is the
generator's own, l_pac = 240003 (no multiple of 4: the last byte of pac is partly filled), and every window has a stretch of it to
itself, written as the kernel will read it (windows beyond l_pac are the reverse complement of the forward strand)."""
import ctypes as C
import zlib

import numpy as np

KSW_XBYTE, KSW_XSTOP, KSW_XSUBO, KSW_XSTART = 0x10000, 0x20000, 0x40000, 0x80000
FIELDS = ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "min_seed_len")

OPTION_SETS = {
    "default": (1, 4, 6, 1, 6, 1, 19),
    "O0": (1, 4, 0, 1, 0, 1, 19),
    "Oins0": (1, 4, 6, 1, 0, 1, 19),
    "Odel0": (1, 4, 0, 1, 6, 1, 19),
    "asym": (1, 4, 4, 2, 10, 1, 19),
    "O1": (1, 4, 1, 1, 1, 1, 19),
    "Ebig": (1, 4, 2, 5, 2, 5, 19),
    "oi1e3": (1, 4, 6, 1, 1, 3, 19),
    "a2b3": (2, 3, 5, 3, 7, 2, 19),
    "a3": (3, 2, 5, 3, 5, 3, 15),
    "a5": (5, 4, 6, 1, 6, 1, 10),
    "b1": (1, 1, 1, 1, 1, 1, 19),
    "b9": (1, 9, 6, 1, 6, 1, 19),
    "k30": (1, 4, 6, 1, 6, 1, 30),
    "sat": (2, 8, 6, 1, 6, 1, 19),
}
# The sets under which mate rescue does not run on the device (mbw::msw_on_device, device.hip): with o_ins = 0 the reference's lazy-F
# loop stops after the first position of every segment and the kernels' closed form carries further (tests/msw_model.py).
GATED = tuple(n for n, v in OPTION_SETS.items() if v[4] == 0)

L_PAC = 240003
MAX_EXTRA = 300           # a window is at most this much longer than its read
TAIL_BUCKETS = 9


def options(name):
    return dict(zip(FIELDS, OPTION_SETS[name]))


def fill_scmat(a, b):
    """bwa_fill_scmat (src/bwa.c): a on the diagonal, -b off it, -1 against N -> 25 int8"""
    m = np.full(25, -1, dtype=np.int8)
    for i in range(4):
        for j in range(4):
            m[i * 5 + j] = a if i == j else -b
    return m


def set_opt(opt_p, name):
    """the option set on a mem_opt_t, its matrix refilled as the command line does after -A / -B"""
    o = opt_p.contents
    for k, v in options(name).items():
        setattr(o, k, v)
    m = fill_scmat(o.a, o.b)
    for i in range(25):
        o.mat[i] = int(m[i])
    return opt_p


def rc(q):
    return np.where(q[::-1] < 4, 3 - q[::-1], 4).astype(np.uint8)


def tail_bucket(score, qe, a):
    """msw_tail_bucket (msw_kernel.hip)"""
    sb = 2 if score >= 80 * a else 1 if score >= 40 * a else 0
    qb = 2 if qe >= 96 else 1 if qe >= 48 else 0
    return sb * 3 + qb


def reachable_buckets(a, min_seed_len, max_byte_len):
    """The classes a byte-flavour hit can fall into at all: score >= min_seed_len * a (else it has no second pass), score <= (qe + 1) * a
    and qe < max_byte_len (the longest read with qlen * a < 250)."""
    out = set()
    for sb in range(3):
        for qb in range(3):
            qmin, qmax = (0, 48, 96)[qb], min((47, 95, 1 << 30)[qb], max_byte_len - 1)
            smin, smax = max(min_seed_len * a, (0, 40 * a, 80 * a)[sb]), (40 * a - 1, 80 * a - 1, 1 << 30)[sb]
            if qmin <= qmax and smin <= min(smax, (qmax + 1) * a):
                out.add(sb * 3 + qb)
    return out


class Cases:
    """requests in launch order: rb, re, rd (read), rev per request; reads (nt4 codes as the batch holds them); kind: what a request
    is there for; unit: the repeat unit of a tandem read's request, else 0"""

    def __init__(self, name):
        self.name, self.o = name, options(name)
        self.reads, self.rb, self.re, self.rd, self.rev, self.kind, self.unit = [], [], [], [], [], [], []
        self.fwd = None

    def __len__(self):
        return len(self.rb)

    @property
    def mat(self):
        return fill_scmat(self.o["a"], self.o["b"])

    @property
    def dref(self):
        return np.concatenate([self.fwd, 3 - self.fwd[::-1]]).astype(np.uint8)

    @property
    def pac(self):
        n = len(self.fwd)
        f = np.concatenate([self.fwd, np.zeros(-n % 4, dtype=np.uint8)])
        p = np.zeros(n // 4 + 1, dtype=np.uint8)
        for k in range(4):
            v = (f[k::4] << ((3 - k) * 2)).astype(np.uint8)
            p[:len(v)] |= v
        return p

    def query(self, i):
        s = self.reads[self.rd[i]]
        return np.ascontiguousarray(s if not self.rev[i] else rc(s))

    def is_byte(self, i):
        return len(self.reads[self.rd[i]]) * self.o["a"] < 250

    def matesw_args(self):
        """what follows opt in Engine.matesw"""
        return L_PAC, self.pac, self.reads, self.rb, self.re, self.rd, self.rev


# ---- the work list of launch_msw (msw_kernel.hip) ----
def work_list(cs):
    """-> (items of msw2_kernel [(k, partner or -1)], requests of msw_kernel)"""
    items, word, k, n = [], [], 0, len(cs)
    while k < n:
        if not cs.is_byte(k):
            word.append(k)
            k += 1
        elif k + 1 < n and cs.rd[k] == cs.rd[k + 1] and cs.rev[k] == cs.rev[k + 1] and cs.re[k] > cs.rb[k] and cs.re[k + 1] > cs.rb[k + 1]:
            items.append((k, k + 1))
            k += 2
        else:
            items.append((k, -1))
            k += 1
    return items, word


def wave_census(cs):
    """waves of 16 items of msw2_kernel -> (with one segment length throughout: the UNI copy of the forward pass, with several: the
    other copy, items of two requests, of one)"""
    items, word = work_list(cs)
    uni = mixed = 0
    for w in range(0, len(items), 16):
        sl = {(len(cs.reads[cs.rd[k]]) + 15) // 16 for k, _ in items[w:w + 16]}
        if len(sl) == 1:
            uni += 1
        else:
            mixed += 1
    return dict(uniform=uni, mixed=mixed, pairs=sum(1 for _, b in items if b >= 0), alone=sum(1 for _, b in items if b < 0), word=len(word))


# ---- the generator ----
class _Gen:
    def __init__(self, name):
        self.cs = Cases(name)
        self.o = self.cs.o
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.fwd = self.rng.integers(0, 4, size=L_PAC).astype(np.uint8)
        self.cursor = 2000                    # [0, 2000) and the last 2000 bases belong to the boundary windows
        a = self.o["a"]
        self.Lw = (250 + a - 1) // a          # the shortest read of the word flavour
        self.Lb = self.Lw - 1                 # the longest of the byte flavour
        self.Lu = min(150, self.Lb)

    def rand(self, n, alphabet=4):
        return self.rng.integers(0, alphabet, size=n).astype(np.uint8)

    def put(self, win, b=None):
        """a window's content, in the doubled coordinate, into the forward strand -> (rb, re)"""
        tl = len(win)
        if b is None:
            c = self.cursor
            self.cursor += tl + 1
            assert self.cursor < L_PAC - 2000, "reference too short for the cases"
            b = c if self.rng.random() < 0.5 else 2 * L_PAC - (c + tl)
        if b >= L_PAC:
            c = 2 * L_PAC - (b + tl)
            self.fwd[c:c + tl] = 3 - win[::-1]
        else:
            assert b + tl <= L_PAC
            self.fwd[b:b + tl] = win
        return b, b + tl

    @staticmethod
    def plant(win, p, seq):
        """seq at p, clipped to the window"""
        lo, hi = max(p, 0), min(p + len(seq), len(win))
        if hi > lo:
            win[lo:hi] = np.minimum(seq[lo - p:hi - p], 3)

    def mutate(self, q, rate):
        q = q.copy()
        m = self.rng.random(len(q)) < rate
        q[m] = self.rand(int(m.sum()))
        return q

    def window(self, kind, q, tl=None):
        """the content of one window for the oriented query q -> (array, unit)"""
        rng, o = self.rng, self.o
        ql, a, msl = len(q), o["a"], o["min_seed_len"]
        qn = np.minimum(q, 3)
        if tl is None:
            tl = ql + int(rng.integers(20, MAX_EXTRA + 1))
        win = self.rand(tl)
        room = max(tl - ql, 0)
        p = int(rng.integers(0, room + 1))
        name, arg = (kind + ":").split(":")[:2]
        if name == "miss":
            pass
        elif name == "void":      # nothing of a read over {A, C} matches
            win = (2 + self.rand(tl, 2)).astype(np.uint8)
        elif name == "clean":
            self.plant(win, p, qn)
        elif name == "mut":
            self.plant(win, p, self.mutate(qn, 0.04))
        elif name in ("ins", "del"):
            g = int(arg)
            PP = 16 if ql * a < 250 else 8
            slen = (ql + PP - 1) // PP
            c = int(rng.integers(1, PP)) * slen + int(rng.integers(-2, 3))
            g = max(1, min(g, ql - 12))
            c = max(6, min(c, ql - g - 6))
            seq = np.concatenate([qn[:c], qn[c + g:]]) if name == "ins" else np.concatenate([qn[:c], self.rand(g), qn[c:]])
            self.plant(win, min(p, max(tl - len(seq), 0)), seq)
        elif name == "tail":
            cut = int(rng.integers(ql // 2, max(ql // 2 + 1, ql - 5)))
            self.plant(win, p, np.concatenate([qn[:cut], self.rand(ql - cut)]))
        elif name == "second":
            # the whole read at p (score ql * a, te = p + ql - 1, d = ceil(score / a) = ql) and its last m bases ending dx rows outside
            # (dx = 1) or on the edge of (dx = 0) te -+ d; "behind": right behind the hit
            m = min(ql - 1, max(msl + 9, 28))
            side, dx = arg[0], int(arg[1]) if len(arg) > 1 else 0
            if side == "a" and 2 * ql + dx + 2 > tl:
                side = "b"
            if side == "b":
                p = int(rng.integers(min(m + dx + 1, room), room + 1))
                self.plant(win, p - dx - m, qn[-m:])
            elif side == "a":
                p = int(rng.integers(0, tl - 2 * ql - dx - 1))
                self.plant(win, p + 2 * ql + dx - m, qn[-m:])
            else:
                p = int(rng.integers(0, max(room - 30, 0) + 1))
                self.plant(win, p + ql, self.mutate(qn[-30:], 0.03))
            self.plant(win, p, qn)
        elif name in ("thresh", "part"):
            # an exact stretch of L bases of the read ending at query position qe, between two bases that do not extend it.
            # thresh: the read is over {A, C} and the window's background over {G, T}: the stretch scores L * a and nothing else scores
            L, qe = (int(x) for x in arg.split(","))
            if name == "thresh":
                win = (2 + self.rand(tl, 2)).astype(np.uint8)
            s = qe - L + 1
            assert 0 <= s and qe < ql and L + 2 <= tl, (kind, ql, tl)
            p = int(rng.integers(1, tl - L))
            self.plant(win, p, qn[s:qe + 1])
            if name == "part":
                if s > 0:
                    win[p - 1] = (qn[s - 1] + 1) & 3
                if qe + 1 < ql:
                    win[p + L] = (qn[qe + 1] + 2) & 3
        elif name == "unit":
            # one unit of a read that is its unit twice over, the read over {A, C} and the window's background over {G, T}: both copies
            # score U * a in the row the unit ends in, query positions U - 1 and 2 U - 1 tie for its maximum, nothing else scores
            U = ql // 2
            win = (2 + self.rand(tl, 2)).astype(np.uint8)
            p = int(rng.integers(1, tl - U))
            self.plant(win, p, qn[:U])
            return win, U
        elif name == "lowcx":
            n = int(rng.integers(ql // 2, ql + 1))
            self.plant(win, int(rng.integers(0, max(tl - n, 0) + 1)), self.mutate(qn[:n], 0.02))
        elif name == "fill":      # a window shorter than the read: all of it is read
            s = int(rng.integers(0, ql - tl + 1)) if ql >= tl else 0
            self.plant(win, 0, qn[s:s + tl])
        else:
            raise ValueError(kind)
        return win, 0

    def read(self, ql, flavour="random"):
        rng = self.rng
        if flavour == "two":          # over {A, C}
            q = self.rand(ql, 2)
        elif flavour == "tandem":
            u = self.rand(ql // 2, 2)
            q = np.concatenate([u, u, self.rand(ql - 2 * (ql // 2), 2)])
        elif flavour == "lowcx":
            q = np.tile(self.rand(3), ql // 3 + 1)[:ql]
            while len(set(q[:3].tolist())) < 2:
                q = np.tile(self.rand(3), ql // 3 + 1)[:ql]
        else:
            q = self.rand(ql)
            if flavour == "N":
                q[rng.choice(ql, min(2, ql), replace=False)] = 4
        return q

    def run(self, q, rev, kinds, tls=None, at=None):
        """requests next to each other for one read in one orientation; q is the query as the kernel sees it"""
        cs = self.cs
        cs.reads.append(q if not rev else rc(q))
        for n, kind in enumerate(kinds):
            if kind == "empty":
                b = int(self.rng.integers(0, 2 * L_PAC))
                rb, re, unit = b, b, 0
            else:
                win, unit = self.window(kind, q, None if tls is None else tls[n])
                rb, re = self.put(win, None if at is None else at[n](len(win)))
            cs.rb.append(rb); cs.re.append(re); cs.rd.append(len(cs.reads) - 1); cs.rev.append(int(rev)); cs.kind.append(kind); cs.unit.append(unit)

    def build(self):
        rng, o = self.rng, self.o
        a, msl, Lb, Lw, Lu = o["a"], o["min_seed_len"], self.Lb, self.Lw, self.Lu
        gaps = list(range(1, 25))
        hit_kinds = ["clean", "mut", "tail", "second:b1", "second:b0", "second:a0", "second:a1", "second:x", "clean", "miss", "tail", "mut"]
        hit_kinds += ["ins:%d" % g for g in gaps] + ["del:%d" % g for g in gaps] + ["miss"] * 14 + ["second:b1", "second:a1", "tail"] * 4
        hit_kinds = [hit_kinds[i] for i in rng.permutation(len(hit_kinds))]
        at = [0]

        def take(n):
            out = [hit_kinds[(at[0] + i) % len(hit_kinds)] for i in range(n)]
            at[0] += n
            return out
        # 1. a stretch of the work list with one segment length: 66 items of reads of Lu bases, runs of 2 to 6 requests
        n_items = 0
        while n_items < 66:
            n = int(rng.integers(2, 7))
            self.run(self.read(Lu, "N" if n_items % 9 == 4 else "random"), int(rng.integers(0, 2)), take(n))
            n_items += (n + 1) // 2
        # 2. every other length, a run of one length next to a run of another; word-flavour reads in between
        byte_lens = [L for L in (Lb, 16, max(Lb * 2 // 3, 6), 5, max(Lb // 2, 6), Lb, 33 if Lb > 33 else 9) if L * a < 250]
        word_lens = [Lw, 250, 125, 84, 50, 249, 124, 83, 49, Lw, 301]
        word_lens = [L for L in word_lens if L * a >= 250]
        for it in range(56):
            L = byte_lens[it % len(byte_lens)]
            n = 1 if it % 4 == 3 else int(rng.integers(2, 7))          # one run in four is a lone request
            self.run(self.read(L, "N" if it % 5 == 2 else "random"), it & 1, take(n))
            if it % 2 == 0:
                Lx = word_lens[(it // 2) % len(word_lens)]
                self.run(self.read(Lx, "N" if it % 6 == 0 else "random"), (it >> 1) & 1, take(int(rng.integers(1, 5))), )
        self.run(self.read(600), 1, ["clean", "ins:7", "miss"], tls=[800, 900, 700])
        # 3. pairs of windows of which one is four times the other, the hit in the first, the second, both.  The read is over {A, C} and a
        # "void" window over {G, T}: a miss under every set (a random window reaches min_seed_len * a by chance where that is small)
        for long_first in (0, 1):
            for ha, hb in (("tail", "void"), ("void", "tail"), ("tail", "mut")):   # (tail: a hit below the byte flavour's ceiling under every set)
                tl_long = Lu + MAX_EXTRA
                tl_short = tl_long // 4 - 1
                tls = [tl_long, tl_short] if long_first else [tl_short, tl_long]
                kinds = [h if t >= Lu or h == "void" else "fill" for h, t in zip((ha, hb), tls)]
                self.run(self.read(Lu, "two"), long_first, kinds, tls=tls)
        # 4. boundary windows: shorter than the read, 19 bases, empty, and the four ends of the doubled coordinate
        self.run(self.read(Lu), 0, ["fill", "miss", "fill", "empty", "fill"], tls=[Lu - 1, Lu // 2, 19, 0, max(Lu - 30, 8)])
        self.run(self.read(Lb), 1, ["empty"])
        self.run(self.read(Lw), 0, ["fill", "empty", "fill"], tls=[Lw - 7, 0, 19])
        q1, q2 = self.read(Lu), self.read(Lu)
        tl = Lu + 120
        w1, w2 = self.rand(tl), self.rand(tl)
        w1[:Lu], w2[tl - Lu:] = q1, q2
        self.cs.reads += [q1, q2]
        r1, r2 = len(self.cs.reads) - 2, len(self.cs.reads) - 1
        for win, b, rd, rev in ((w1, 0, r1, 0), (w2, L_PAC - tl, r2, 0), (None, L_PAC, r2, 1), (None, 2 * L_PAC - tl + 30, r1, 1)):
            if win is not None:
                self.put(win, b)
            e = min(b + tl, L_PAC if b < L_PAC else 2 * L_PAC)
            cs = self.cs
            cs.rb.append(b); cs.re.append(e); cs.rd.append(rd); cs.rev.append(rev); cs.kind.append("edge"); cs.unit.append(0)
        # 5. hits that score min_seed_len * a and one less, nothing else in the window scoring
        for it, L in enumerate((Lu, Lb, Lw, Lu)):
            if L < msl + 2:
                continue
            ks = []
            for n in range(4):
                Lh = msl - (n & 1)
                ks.append("thresh:%d,%d" % (Lh, int(rng.integers(Lh - 1, L))))
            self.run(self.read(L, "two"), it & 1, ks)
        # 6. partial hits of graded length: three for every class of msw_tail_bucket that a byte-flavour hit can reach
        for b in sorted(reachable_buckets(a, msl, Lb)):
            sb, qb = divmod(b, 3)
            ks = []
            for n in range(3):
                # L matching bases score L * a (a chance extension can only add to it: stay clear of the class's upper end)
                qmin, qmax = (0, 48, 96)[qb], min((47, 95, 1 << 30)[qb], Lb - 1)
                lmin, lmax = max(msl, (0, 40, 80)[sb]), min((39, 79, 1 << 30)[sb], qmax + 1)
                lo = min(lmin + 1, lmax)
                L = int(rng.integers(lo, max(lo, lmax - 4) + 1))
                qe = int(rng.integers(max(qmin, L - 1), qmax + 1))
                ks.append("part:%d,%d" % (L, qe))
            self.run(self.read(Lb), b & 1, ks)
        # 7. reads that are a unit twice over, one unit in the window; reads of a 3-base repeat
        for it, L in enumerate((Lu, Lb, Lw, Lu - 1 if Lu > 2 * msl + 3 else Lu, Lw + 11, Lu)):
            self.run(self.read(L, "tandem"), it & 1, ["unit"] * 3)
        for it, L in enumerate((Lu, Lw)):
            self.run(self.read(L, "lowcx"), it & 1, ["lowcx", "lowcx", "miss"])
        self.cs.fwd = self.fwd
        return self.cs


_CACHE = {}


def cases(name):
    """the case set of an option set, once per process; nobody changes it"""
    if name not in _CACHE:
        _CACHE[name] = _Gen(name).build()
    return _CACHE[name]


# ---- expected results ----
class kswr_t(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("score", "te", "qe", "score2", "te2", "tb", "qb")]


def xtra_of(cs, i, byte=None):
    byte = cs.is_byte(i) if byte is None else byte
    return KSW_XSUBO | KSW_XSTART | (KSW_XBYTE if byte else 0) | (cs.o["min_seed_len"] * cs.o["a"])


def host_results(lib, cs, portable=1, full_width=False):
    """mi355x_host_ksw_align2 as mem_matesw calls ksw_align2 (full_width: without KSW_XBYTE) -> (n, 7) int32"""
    o, mat, dref = cs.o, cs.mat, cs.dref
    out = np.zeros((len(cs), 7), dtype=np.int32)
    for i in range(len(cs)):
        q, win = cs.query(i), np.ascontiguousarray(dref[cs.rb[i]:cs.re[i]])
        lib.mi355x_host_ksw_align2(len(q), q.ctypes.data, len(win), win.ctypes.data, mat.ctypes.data, o["o_del"], o["e_del"], o["o_ins"], o["e_ins"],
                                   xtra_of(cs, i, False if full_width else None), portable, out[i].ctypes.data)
    return out


def reference_results(rl, cs):
    """the reference's ksw_align2 -> (n, 7) int32"""
    rl.ksw_align2.restype = kswr_t
    rl.ksw_align2.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
    o, mat, dref = cs.o, cs.mat, cs.dref
    out = np.zeros((len(cs), 7), dtype=np.int32)
    for i in range(len(cs)):
        q, win = cs.query(i).copy(), np.ascontiguousarray(dref[cs.rb[i]:cs.re[i]]).copy()
        w = rl.ksw_align2(len(q), q.ctypes.data, len(win), win.ctypes.data, 5, mat.ctypes.data, o["o_del"], o["e_del"], o["o_ins"], o["e_ins"],
                          xtra_of(cs, i), None)
        out[i] = (w.score, w.te, w.qe, w.score2, w.te2, w.tb, w.qb)
    return out


class Want:
    """what a request must answer: res (n, 7) as ksw_align2 gives it, sat: the byte flavour's score reaches the 8-bit ceiling
    (the full-width score is >= 255 - shift), where the device hands the request back"""

    def __init__(self, cs, res, full):
        self.cs, self.res = cs, np.asarray(res)
        shift = max(-int(cs.mat.min()), 0)
        byte = np.array([cs.is_byte(i) for i in range(len(cs))])
        self.byte = byte
        self.sat = byte & (np.asarray(full)[:, 0] >= 255 - shift)


def want_from_host(lib, cs, res=None):
    return Want(cs, host_results(lib, cs) if res is None else res, host_results(lib, cs, full_width=True))


def coverage(want):
    """counters of what the expected results themselves reach"""
    cs, res = want.cs, want.res
    minsc = cs.o["min_seed_len"] * cs.o["a"]
    st = dict(n=len(cs), hit=0, miss=0, sat=int(want.sat.sum()), second=0, qe_short=0, tie=0, byte=int(want.byte.sum()), word=int((~want.byte).sum()),
              thresh_eq=0, thresh_lo=0, buckets=[0] * TAIL_BUCKETS)
    # pairs of msw2_kernel of which one window is four times the other: (the long one first, hit in A, hit in B)
    tl = lambda k: cs.re[k] - cs.rb[k]
    st["fourfold"] = sorted({(tl(x) > tl(y), bool(res[x][0] >= minsc), bool(res[y][0] >= minsc)) for x, y in work_list(cs)[0]
                             if y >= 0 and not want.sat[x] and not want.sat[y] and max(tl(x), tl(y)) >= 4 * min(tl(x), tl(y))})
    for i in range(len(cs)):
        if want.sat[i]:
            continue
        r = res[i]
        if cs.kind[i].startswith("thresh"):
            st["thresh_eq"] += r[0] == minsc
            st["thresh_lo"] += r[0] == minsc - cs.o["a"]
        if r[0] < minsc:
            st["miss"] += 1
            continue
        st["hit"] += 1
        st["second"] += r[3] > 0
        st["qe_short"] += r[2] < len(cs.reads[cs.rd[i]]) - 1
        st["tie"] += cs.unit[i] > 0 and r[2] < cs.unit[i]
        if want.byte[i]:
            st["buckets"][tail_bucket(int(r[0]), int(r[2]), cs.o["a"])] += 1
    return st


def compare(got, want):
    """got: Engine.matesw's (n, 8).  flags == 1 exactly where the byte flavour saturates (nothing else is compared there), else
    flags == 0 and: below min_seed_len * a the caller drops the result, so only the score and tb = qb = -1 count; from there on all
    seven fields.  -> coverage(want)"""
    cs, res = want.cs, want.res
    minsc = cs.o["min_seed_len"] * cs.o["a"]
    assert len(got) == len(cs)
    for i in range(len(cs)):
        g, w = got[i], res[i]
        what = (cs.name, i, cs.kind[i], len(cs.reads[cs.rd[i]]), cs.re[i] - cs.rb[i], cs.rev[i], list(g), list(w))
        if want.sat[i]:
            assert g[7] == 1, what
            continue
        assert g[7] == 0, what
        if w[0] < minsc:
            assert g[0] == w[0] and g[5] == -1 and g[6] == -1, what
        else:
            assert (g[:7] == w).all(), what
    return coverage(want)


def check_coverage(name, cs, st):
    """the floors every option set's cases must reach, on the expected results"""
    o = cs.o
    a, Lb = o["a"], (250 + o["a"] - 1) // o["a"] - 1
    n = st["n"]
    assert 400 <= n <= 600, (name, n)
    assert st["hit"] >= 0.4 * n, (name, st)
    assert st["second"] >= 20 and st["qe_short"] >= 20 and st["tie"] >= 5, (name, st)
    assert st["byte"] >= 30 and st["word"] >= 30, (name, st)
    assert st["thresh_eq"] >= 4 and st["thresh_lo"] >= 4, (name, st)
    if name == "sat":
        assert st["sat"] >= 5, (name, st)
    wc = wave_census(cs)
    assert wc["uniform"] >= 3 and wc["mixed"] >= 3 and wc["pairs"] >= 60 and wc["alone"] >= 10 and wc["word"] >= 30, (name, wc)
    # at least six classes of msw_tail_bucket with two or more hits, the shortest (0, 0), the longest (2, 2) and low score / long qe
    # (0, 2) among them — as far as a byte-flavour hit can reach them under this a (reachable_buckets: all nine for a <= 2, five
    # for a = 3, four for a = 5)
    can = reachable_buckets(a, o["min_seed_len"], Lb)
    have = {b for b in range(TAIL_BUCKETS) if st["buckets"][b] >= 2}
    assert len(have) >= min(6, len(can)) and ({0, 8, 2} & can) <= have, (name, st["buckets"], sorted(can))
    # lengths on both sides of qlen * a = 250, the shortest reads and the long one
    lens = {len(r) for r in cs.reads}
    assert {Lb, Lb + 1, 5, 16, 600} <= lens, (name, sorted(lens))
    tls = [cs.re[i] - cs.rb[i] for i in range(len(cs))]
    assert 0 in tls and 19 in tls and all(t <= len(cs.reads[cs.rd[i]]) + MAX_EXTRA for i, t in enumerate(tls))
    assert any(0 < t < len(cs.reads[cs.rd[i]]) for i, t in enumerate(tls))
    assert 0 in cs.rb and L_PAC in cs.re and L_PAC in cs.rb and 2 * L_PAC in cs.re
    # fourfold pairs, the long window first and second: a hit in A only, in B only, in both — by the expected results
    assert {(lf, x, y) for lf in (False, True) for x, y in ((True, False), (False, True), (True, True))} <= set(st["fourfold"]), (name, st["fourfold"])
    # runs of 2 to 6 requests for one mate; N in the read in both orientations; gaps of 1 to 24 bases, insertions and deletions; second
    # hits on both sides of te +- d, on its edge and one row outside, and right behind the hit; the other kinds
    runs = [1]
    for i in range(1, len(cs)):
        if cs.rd[i] == cs.rd[i - 1]:
            runs[-1] += 1
        else:
            runs.append(1)
    assert max(runs) <= 6 and {1, 2, 3, 4, 5, 6} <= set(runs), (name, sorted(set(runs)))
    assert {cs.rev[i] for i in range(len(cs)) if (cs.reads[cs.rd[i]] == 4).any()} == {0, 1}, name
    kinds = set(cs.kind)
    assert {"%s:%d" % (k, g) for k in ("ins", "del") for g in range(1, 25)} <= kinds, name
    assert {"clean", "mut", "miss", "void", "second:b0", "second:b1", "second:a0", "second:a1", "second:x", "tail", "unit", "lowcx", "edge", "empty",
            "fill"} <= kinds, (name, sorted(kinds))
    return wc
