"""ks_introsort as mpibwa_amd/csrc/sortutil.h states it (ks_introsort_at: the one statement the host and the kernels share), in Python, over an ORDER array: o holds element numbers, less(x, y) compares
two of them.  It reports what no compiled restatement can be asked: the ranges handed to the comb sort, the swaps the comb sort made
and the deepest frame stack.  `comb=False` is the variant whose fallback is an insertion sort of the range in hand — what a restatement
that forgot the comb sort would do.  Used to build and to count cases (tests/chain_cases.py, tests/dedup_cases.py,
tests/test_introsort_model.py); the expected results of every test still come from the reference's own functions."""
import functools

SHRINK = 1.2473309501039786540366528676643


class Stats:
    def __init__(self):
        self.comb_ranges = []     # (first index, length) of every range the depth budget ran out on
        self.comb_swaps = 0
        self.max_frames = 0

    @property
    def widest(self):
        return max((n for _, n in self.comb_ranges), default=0)


def _insertion(o, s, t, less):   # [s, t)
    for i in range(s + 1, t):
        j = i
        while j > s and less(o[j], o[j - 1]):
            o[j], o[j - 1] = o[j - 1], o[j]
            j -= 1


def _comb(o, a, n, less, st):
    gap = n
    while True:
        if gap > 2:
            gap = int(gap / SHRINK)
            if gap == 9 or gap == 10:
                gap = 11
        swapped = False
        for i in range(a, a + n - gap):
            j = i + gap
            if less(o[j], o[i]):
                o[i], o[j] = o[j], o[i]
                swapped = True
                st.comb_swaps += 1
        if not (swapped or gap > 2):
            break
    if gap != 1:
        _insertion(o, a, a + n, less)


def introsort(o, less, comb=True):
    """sorts the list o in place -> Stats"""
    st = Stats()
    n = len(o)
    if n < 1:
        return st
    if n == 2:
        if less(o[1], o[0]):
            o[0], o[1] = o[1], o[0]
        return st
    d = 2
    while (1 << d) < n:
        d += 1
    stack = []
    s, t = 0, n - 1
    d <<= 1
    while True:
        if s < t:
            d -= 1
            if d == 0:
                st.comb_ranges.append((s, t - s + 1))
                if comb:
                    _comb(o, s, t - s + 1, less, st)
                else:
                    _insertion(o, s, t + 1, less)
                t = s
                continue
            i, j = s, t
            k = i + ((j - i) >> 1) + 1
            if less(o[k], o[i]):
                if less(o[k], o[j]):
                    k = j
            else:
                k = i if less(o[j], o[i]) else j
            pivot = o[k]
            if k != t:
                o[k], o[t] = o[t], o[k]
            while True:
                i += 1
                while less(o[i], pivot):
                    i += 1
                j -= 1
                while i <= j and less(pivot, o[j]):
                    j -= 1
                if j <= i:
                    break
                o[i], o[j] = o[j], o[i]
            o[i], o[t] = o[t], o[i]
            if i - s > t - i:
                if i - s > 16:
                    stack.append((s, i - 1, d))
                s = i + 1 if t - i > 16 else t
            else:
                if t - i > 16:
                    stack.append((i + 1, t, d))
                t = i - 1 if i - s > 16 else s
            st.max_frames = max(st.max_frames, len(stack))
        else:
            if not stack:
                _insertion(o, 0, n, less)
                return st
            s, t, d = stack.pop()


def sort_keys(keys, less=None, comb=True):
    """order of range(len(keys)) under less(key, key) (default <) -> (order, Stats)"""
    lt = (lambda x, y: keys[x] < keys[y]) if less is None else (lambda x, y: less(keys[x], keys[y]))
    o = list(range(len(keys)))
    return o, introsort(o, lt, comb)


def budget(n):
    """2 * ceil(log2 n) as ks_introsort computes it (n >= 3)"""
    d = 2
    while (1 << d) < n:
        d += 1
    return 2 * d


@functools.lru_cache(maxsize=None)
def first_ordered_size_that_combs(limit=64):
    """the smallest n at which an input already in order runs out of depth"""
    for n in range(3, limit):
        if sort_keys(list(range(n)))[1].comb_ranges:
            return n
    return None
