"""Degenerate genomes for both index builders (csrc/index.cpp, csrc/index_gpu.hip) and for the device tables and kernels that read an
index (csrc/fm_kernels.hip): tests/test_index_cases.py (CPU), tests/test_gpu_index_cases.py, tests/test_gpu_fm_degenerate.py.  CPU
only, seeded; the known answer is tests/index_model.py.

What the GPU builder branches on, and so what the families are placed around: N = 2 l_pac against the 29-mer of round 0 (KMER) and its
doublings 58 and 116, against the 16-symbol words, 32-row SA samples and 128-symbol occ blocks of the files; the number of suffixes
that are still tied after round 0 (none; nearly all) and the depth of their ties (the number of doubling rounds); suffixes tied with a
partner on the other strand; where `primary` falls; bases the text does not have."""
import numpy as np

import index_model as im

KMER = 29
LENGTHS = list(range(1, 20)) + list(range(28, 34)) + [57, 58, 59, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1023, 1024, 1025]
PERIODS = (28, 29, 30, 57, 58, 59, 116, 117)
LENGTH_SEED = 1000                           # `len<l_pac>` draws its bases with seed LENGTH_SEED + l_pac, but for
# two of the indexes that are uploaded, whose seeds were found by search (3000, 3001, ...) and are pinned: l_pac = 16 with primary = 32 =
# N (the last row, and a sampled one), l_pac = 64 with primary = 127 (the last row of a block of 32 of the device's occ table: the one
# place where occ_before_row is asked for the rows up to `primary` itself)
LENGTH_SEEDS = {16: 3020, 64: 3020}
PRIMARY_SEEDS = ((50, 2022), (300, 2081))    # (l_pac, seed) of `len<l_pac>-p`: `primary` on a multiple of 32 / of 128
GROUPS = ("lengths_a", "lengths_b", "homopolymers", "periods", "selfrc", "words", "ordinary")


class Case:
    def __init__(self, name, group, codes, contigs=None):
        self.name, self.group = name, group
        self.codes = np.ascontiguousarray(codes, np.uint8)
        self.contigs = [len(self.codes)] if contigs is None else list(contigs)
        assert sum(self.contigs) == len(self.codes) and min(self.contigs) >= 1 and self.codes.max() <= 3

    @property
    def l_pac(self):
        return len(self.codes)

    def seqs(self):
        cut = np.cumsum([0] + self.contigs)
        return [self.codes[a:b] for a, b in zip(cut[:-1], cut[1:])]

    def names(self):
        return ["chrS%d" % (i + 1) for i in range(len(self.contigs))]      # the names bigindex.write_meta_files gives

    def __repr__(self):
        return "Case(%s)" % self.name


def rc(a):
    return (3 - np.asarray(a, np.uint8))[::-1].astype(np.uint8)


def _rand(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def fibonacci_word(a, b, n):
    x, y = [a], [a, b]
    while len(y) < n:
        x, y = y, y + x
    return np.array(y[:n], np.uint8)


def length_case(l_pac):
    rng = np.random.default_rng(LENGTH_SEEDS.get(l_pac, LENGTH_SEED + l_pac))
    return Case("len%d" % l_pac, "lengths_a" if l_pac <= 19 else "lengths_b", _rand(rng, l_pac))


def _three_contigs(case, name):
    """the same bases cut into three contigs, the middle one a single base"""
    n = case.l_pac
    a = n // 3
    return Case(name, case.group, case.codes, [a, 1, n - a - 1])


_cache = []


def all_cases():
    if _cache:
        return _cache
    out = [length_case(l) for l in LENGTHS]
    # none of the lengths above happens to put `primary` on a multiple of 32: seeds found by search (2000, 2001, ...) and pinned.
    # One occ block with primary = 96, and five blocks with primary = 256 (tests/test_index_cases.py asserts both)
    for l_pac, seed in PRIMARY_SEEDS:
        out.append(Case("len%d-p" % l_pac, "lengths_b", _rand(np.random.default_rng(seed), l_pac)))
    for b in range(4):
        out.append(Case("homo" + "ACGT"[b], "homopolymers", np.full(4099, b, np.uint8)))
    for tag, (a, b) in (("AC", (0, 1)), ("AT", (0, 3)), ("CG", (1, 2))):
        out.append(Case("di" + tag, "homopolymers", np.array([a, b] * 2050, np.uint8)))
    out.append(Case("diAT+A", "homopolymers", np.array([0, 3] * 2050 + [0], np.uint8)))
    rng = np.random.default_rng(29)
    for p in PERIODS:
        out.append(Case("period%d" % p, "periods", np.resize(_rand(rng, p), 6000)))
    rng = np.random.default_rng(30)
    u = _rand(rng, 3000)
    out.append(Case("selfrc", "selfrc", np.concatenate([u, rc(u)])))
    out.append(Case("selfrc+C", "selfrc", np.concatenate([u, [1], rc(u)])))
    out.append(Case("doubled", "selfrc", np.concatenate([u, u])))
    v = u.copy()
    v[1500] = (v[1500] + 1) & 3
    out.append(Case("doubled-1", "selfrc", np.concatenate([u, v])))
    out.append(Case("fibAC", "words", fibonacci_word(0, 1, 6765)))
    out.append(Case("fibGT", "words", fibonacci_word(2, 3, 6765)))
    rng = np.random.default_rng(31)
    out.append(Case("runs", "words", np.concatenate([np.full(int(rng.integers(1, 200)), int(rng.integers(0, 4)), np.uint8) for _ in range(80)])))
    unit = _rand(rng, 200)
    copies = []
    for k in range(30):
        c = unit.copy()
        if k % 10 == 9:
            c[-1] = (c[-1] + 1 + k // 10) & 3
        copies.append(c)
    out.append(Case("tandem", "words", np.concatenate(copies)))
    out.append(Case("ordinary", "ordinary", _rand(np.random.default_rng(32), 200_000)))
    by = {c.name: c for c in out}
    out.append(_three_contigs(by["len65"], "len65/3"))
    out.append(_three_contigs(by["period29"], "period29/3"))
    out.append(_three_contigs(by["selfrc"], "selfrc/3"))
    assert len({c.name for c in out}) == len(out)
    _cache.extend(out)
    return _cache


def by_name(name):
    return {c.name: c for c in all_cases()}[name]


def group(name):
    return [c for c in all_cases() if c.group == name]


# the genomes that also run with the round-0 buckets forced to 2, 3 and 4 leading symbols (MPIBWA_IDX_KB)
def kb_cases_short():
    return [c for c in all_cases() if c.l_pac <= 33 and len(c.contigs) == 1]


def kb_cases_long():
    return [by_name(n) for n in ("homoA", "diAT", "diCG", "period29", "selfrc", "ordinary")]


# the indexes that are uploaded to the device (tests/test_gpu_fm_degenerate.py)
FM_CASES = ("len1", "len7", "len15", "len16", "len64", "homoA", "diAT", "period29", "selfrc", "fibGT")


def tied_after_round0(text):
    """the number of suffixes that share [their first 29 symbols | how many of those exist] with another suffix: what the GPU builder
    hands to its doubling rounds"""
    T = np.asarray(text, np.uint64)
    N = len(T)
    pad = np.concatenate([T, np.zeros(KMER, np.uint64)])
    key = np.zeros(N, np.uint64)
    for k in range(KMER):
        key = key << np.uint64(2) | pad[k:k + N]
    key = key << np.uint64(6) | np.minimum(N - np.arange(N), KMER).astype(np.uint64)
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    return int((cnt[inv] > 1).sum())


def reach(case):
    """what a family is meant to reach, from the model alone"""
    _, _, _, info = im.index_files(case.codes, with_info=True)
    T = im.text_of(case.codes)
    N, primary = info["N"], info["primary"]
    return dict(name=case.name, N=N, rounds=info["rounds"], m=tied_after_round0(T), primary=primary, p32=primary % 32, p128=primary % 128,
                n128=N % 128, first_block=N > 128 and primary < 128, last_block=N > 128 and (primary >> 7) == (N >> 7),
                absent=[b for b in range(4) if info["L2"][b + 1] == info["L2"][b]])


# ---------------------------------------------------------------------------------------------------------------------------------
# reads for the uploaded indexes
# ---------------------------------------------------------------------------------------------------------------------------------
READ_LENS = (1, 18, 19, 20, 31, 150, 161, 257)


def fm_reads(case):
    """-> [(tag, read)]: the substrings of the text (both strands, as the index holds it) of READ_LENS bases at positions 0, 1,
    l_pac - len and around the strand boundary, each also with one substitution in the middle; for a text shorter than a read, reads
    that are the text repeated beyond its end"""
    T = im.text_of(case.codes)
    N, l_pac = len(T), case.l_pac
    out, seen = [], set()

    def add(tag, r):
        r = np.ascontiguousarray(r, np.uint8)
        if r.tobytes() not in seen:
            seen.add(r.tobytes())
            out.append((tag, r))
    for L in READ_LENS:
        for s in sorted({0, 1, l_pac - L, l_pac - L + 1, l_pac - L // 2, l_pac - 1, l_pac}):
            if s < 0 or s + L > N:
                continue
            r = T[s:s + L]
            add("%d@%d" % (L, s), r)
            m = r.copy()
            m[L // 2] = (m[L // 2] + 1 + (s & 1)) & 3
            add("%d@%d*" % (L, s), m)
        if L > N:
            add("%d>N" % L, np.resize(T, L))
    if N < 300:
        add("300>N", np.resize(T, 300))
    return out


def absent_base_reads(case, base=1):
    """reads of the text with `base` put in: at the start, in the middle, at the end, everywhere"""
    T = im.text_of(case.codes)
    out = []
    for L in (19, 31, 150, 257):
        r = T[:L].copy()
        for at, tag in (([0], "first"), ([L // 2], "mid"), ([L - 1], "last"), ([0, L - 1], "ends"), (list(range(L)), "all")):
            m = r.copy()
            m[at] = base
            out.append(("%d/%s" % (L, tag), m))
    return out
