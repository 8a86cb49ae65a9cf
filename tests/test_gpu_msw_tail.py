"""Mate rescue's second pass (the b[] scan behind score2 / te2 and the reverse pass behind tb / qb, msw_tail_kernel) against the
reference's ksw_align2 and the host restatement, on request sets shaped like the bench's: runs of 20-50 windows for one mate of which
5-20 % hold it, so that the waves of the forward kernel mix hits and misses and the second-pass lists mix runs."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

KSW_XBYTE, KSW_XSTOP, KSW_XSUBO, KSW_XSTART = 0x10000, 0x20000, 0x40000, 0x80000


@pytest.fixture(scope="module")
def engine(genome):
    from mpibwa_amd import api
    return api.Engine(genome["prefix"], device=0)


def _rc(q):
    return np.where(q[::-1] < 4, 3 - q[::-1], 4).astype(np.uint8)


def _mutate(rng, q, rate):
    q = q.copy()
    m = rng.random(len(q)) < rate
    q[m] = rng.integers(0, 4, size=int(m.sum()))
    return q


def _cases(rng, l_pac, ref, n_mates, read_lens):
    """Runs of windows for one mate in one orientation; some windows hold the mate (whole or with a random tail: qe at the end or
    not), some of those a second, weaker copy before or after the first (score2 on either side of te +- d), or right behind it (rows
    after the peak: the run rule's last entry)."""
    dref = np.concatenate([ref, 3 - ref[::-1]]).astype(np.uint8)
    reads, rb, re, rd, rev = [], [], [], [], []
    for _ in range(n_mates):
        ql = int(rng.choice(read_lens))
        q = rng.integers(0, 4, size=ql).astype(np.uint8)
        is_rev = int(rng.integers(0, 2))
        mi = len(reads)
        reads.append(q if not is_rev else _rc(q))
        hit_rate = float(rng.uniform(0.05, 0.2))
        for w in range(int(rng.integers(20, 51))):
            tl = int(rng.choice([int(rng.integers(ql + 100, ql + 700)), int(rng.integers(max(ql // 2, 19), ql + 60))]))
            strand = int(rng.integers(0, 2))
            b = int(rng.integers(0, l_pac - tl)) + strand * l_pac
            if rng.random() < hit_rate and tl >= ql:
                # plant the mate into the doubled reference itself: the window then holds it as the kernel reads it
                win = dref[b:b + tl].copy()
                src = _mutate(rng, q, float(rng.choice([0.0, 0.02, 0.06])))
                if rng.random() < 0.3:   # a random tail: the best cell ends before the last base (qe < qlen - 1)
                    cut = int(rng.integers(ql // 2, ql - 5))
                    src[cut:] = rng.integers(0, 4, size=ql - cut)
                p = int(rng.integers(0, tl - ql + 1))
                win[p:p + ql] = src
                kind = rng.random()
                if kind < 0.5 and tl >= ql + 40:   # a weaker partial copy elsewhere in the window (before or after the hit)
                    part = _mutate(rng, q[:int(rng.integers(25, max(26, ql // 2)))], 0.05)
                    p2 = int(rng.integers(0, tl - len(part) + 1))
                    if p2 + len(part) <= p or p2 >= p + ql:
                        win[p2:p2 + len(part)] = part
                elif kind < 0.7 and p + ql + 30 <= tl:   # a copy of the read's last bases right behind the hit: rows past the peak
                    tail = _mutate(rng, q[-30:], 0.03)
                    win[p + ql:p + ql + 30] = tail
                dref[b:b + tl] = win
            rb.append(b); re.append(b + tl); rd.append(mi); rev.append(is_rev)
        if rng.random() < 0.2:   # a lone request of another mate between two runs
            ql2 = int(rng.choice(read_lens))
            q2 = rng.integers(0, 4, size=ql2).astype(np.uint8)
            reads.append(q2)
            tl = int(rng.integers(ql2, ql2 + 500))
            b = int(rng.integers(0, l_pac - tl))
            dref[b:b + ql2] = q2
            rb.append(b); re.append(b + tl); rd.append(len(reads) - 1); rev.append(0)
    return dref, reads, rb, re, rd, rev


def _pac_of(dref, l_pac):
    ref = dref[:l_pac]
    pac = np.zeros(l_pac // 4 + 1, dtype=np.uint8)
    for k in range(4):
        pac[:l_pac // 4] |= (ref[k::4] << ((3 - k) * 2)).astype(np.uint8)
    return pac


def _run(engine, opt_p, mat, seed, read_lens, n_mates, check_ref=True):
    from mpibwa_amd import api
    lib = api.load_library()
    rng = np.random.default_rng(seed)
    l_pac = 120000
    ref = rng.integers(0, 4, size=l_pac).astype(np.uint8)
    dref, reads, rb, re, rd, rev = _cases(rng, l_pac, ref, n_mates, read_lens)
    # the planted windows live in either half of the doubled coordinate: make the forward half their source of truth
    fwd = dref[:l_pac].copy()
    back = 3 - dref[l_pac:][::-1]
    planted_back = back != ref
    fwd[planted_back] = back[planted_back]
    dref = np.concatenate([fwd, 3 - fwd[::-1]]).astype(np.uint8)
    pac = _pac_of(dref, l_pac)
    got, _ = engine.matesw(opt_p, l_pac, pac, reads, rb, re, rd, rev)
    opt = opt_p.contents
    use_ref = check_ref and po.ref_available()
    if use_ref:
        class kswr_t(C.Structure):
            _fields_ = [(n, C.c_int) for n in ("score", "te", "qe", "score2", "te2", "tb", "qb")]
        rl = po.ref_lib()
        rl.ksw_align2.restype = kswr_t
        rl.ksw_align2.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
    minsc = opt.min_seed_len * opt.a
    shift = -int(min(mat.min(), 0)) if mat.min() < 0 else 0
    stats = dict(hit=0, second=0, miss=0, sat=0, qe_short=0)
    for i in range(len(rb)):
        tl = re[i] - rb[i]
        win = np.ascontiguousarray(dref[rb[i]:re[i]])
        s = reads[rd[i]]
        q = np.ascontiguousarray(s if not rev[i] else _rc(s))
        byte = len(q) * opt.a < 250
        xtra = KSW_XSUBO | KSW_XSTART | (KSW_XBYTE if byte else 0) | minsc
        g = got[i]
        if byte:   # the 8-bit ceiling: the device flags the request for the host instead of answering
            full = np.zeros(7, dtype=np.int32)
            lib.mi355x_host_ksw_align2(len(q), q.ctypes.data, tl, win.ctypes.data, mat.ctypes.data, opt.o_del, opt.e_del, opt.o_ins, opt.e_ins,
                                       KSW_XSUBO | KSW_XSTART | minsc, 1, full.ctypes.data)
            if full[0] >= 255 - shift:
                assert g[7] == 1, (i, g, full)
                stats["sat"] += 1
                continue
        want = np.zeros(7, dtype=np.int32)
        lib.mi355x_host_ksw_align2(len(q), q.ctypes.data, tl, win.ctypes.data, mat.ctypes.data, opt.o_del, opt.e_del, opt.o_ins, opt.e_ins,
                                   xtra, 1, want.ctypes.data)
        if use_ref:
            qq, tt = q.copy(), win.copy()
            w = rl.ksw_align2(len(q), qq.ctypes.data, tl, tt.ctypes.data, 5, mat.ctypes.data, opt.o_del, opt.e_del, opt.o_ins, opt.e_ins, xtra, None)
            assert (want == np.array([w.score, w.te, w.qe, w.score2, w.te2, w.tb, w.qb])).all(), (i, want)
        assert g[7] == 0, (i, g, want)
        # the existing stage test's rule: below min_seed_len * a the caller drops the result, so only the score and tb = qb = -1
        if want[0] < minsc:
            assert g[0] == want[0] and g[5] == -1 and g[6] == -1, (i, g, want)
            stats["miss"] += 1
        else:
            assert (g[:7] == want).all(), (i, len(q), tl, rev[i], g, want)
            stats["hit"] += 1
            stats["second"] += want[3] > 0
            stats["qe_short"] += want[2] < len(q) - 1
    return stats, len(rb)


def test_msw_tail_bench_shaped_runs(engine):
    """Default scoring: 150 / 151 / 100 bp mates (the packed kernel) and 251 bp ones (the word flavour) in runs of 20-50 windows."""
    opt_p = engine.opt()
    mat = np.frombuffer(bytes(opt_p.contents.mat), dtype=np.int8).copy()
    st, n = _run(engine, opt_p, mat, 7, [150, 150, 151, 100, 251], 120)
    assert n > 3000
    assert 0.04 * n < st["hit"] < 0.4 * n, st
    assert st["second"] > 20 and st["qe_short"] > 20, st


def test_msw_tail_saturating_scores(engine):
    """Match 2, mismatch -8: a 124 bp mate in the byte flavour can reach the 8-bit ceiling (255 - 8), which the device must flag;
    the hits below it still go through the second pass."""
    opt_p = engine.opt(a=2, b=8)
    opt = opt_p.contents
    for t in range(5):
        for k in range(5):
            opt.mat[t * 5 + k] = -1 if t == 4 or k == 4 else (2 if t == k else -8)
    mat = np.frombuffer(bytes(opt.mat), dtype=np.int8).copy()
    st, n = _run(engine, opt_p, mat, 11, [124, 120, 110], 60, check_ref=False)
    assert st["sat"] > 5 and st["hit"] > 50, st
