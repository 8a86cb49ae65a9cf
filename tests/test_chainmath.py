"""CPU: mpibwa_amd/csrc/chainmath.h itself — the one statement of mem_chain's arithmetic that the host chaining and both chaining kernels
share — as a stand-alone program (tests/chainmath_main.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer.

Every function is compared with a Python restatement of the reference's lines: exact integers for bns_depos / bns_pos2rid / bns_intv2rid
(src/bntseq.c:349-376), test_and_merge (src/bwamem.c:190-211), mem_chain_weight (:213-237) and the max_chain_extend cut (:372-379),
numpy.float32 arithmetic in the reference's expression shape for the two compares of mem_chain_flt (:355, :358), and the window model
of mem_chain2aln that the c2a stage test has (tests/window_model.py, :642-661).  The cases sit on both sides of every threshold; where a
group of cases is there for a verdict, the test asserts on the model's answers that both sides are present."""
import itertools
import os
import subprocess
from bisect import bisect_right
from types import SimpleNamespace

import numpy as np
import pytest

import window_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LQ = 151
NEW, CONTAINED, APPEND = 0, 1, 2


# ---- the reference's lines ----
def depos(l_pac, pos):   # src/bntseq.h:83-86
    return (l_pac << 1) - 1 - pos if pos >= l_pac else pos


def pos2rid(offs, l_pac, pos_f):   # src/bntseq.c:349-363
    if pos_f >= l_pac:
        return -1
    left, mid, right = 0, 0, len(offs)
    while left < right:
        mid = (left + right) >> 1
        if pos_f >= offs[mid]:
            if mid == len(offs) - 1:
                break
            if pos_f < offs[mid + 1]:
                break
            left = mid + 1
        else:
            right = mid
    return mid


def intv2rid(offs, l_pac, rb, re):   # src/bntseq.c:365-376
    if rb < l_pac and re > l_pac:
        return -2
    rid_b = pos2rid(offs, l_pac, depos(l_pac, rb))
    rid_e = pos2rid(offs, l_pac, depos(l_pac, re - 1)) if rb < re else rid_b
    return rid_b if rid_b == rid_e else -1


def merge_verdict(l_pac, w, max_chain_gap, first_r, first_q, last_r, last_q, last_len, rb, qb, ln):   # src/bwamem.c:190-211, past the rid test
    qend, rend = last_q + last_len, last_r + last_len
    if qb >= first_q and qb + ln <= qend and rb >= first_r and rb + ln <= rend:
        return CONTAINED
    if (last_r < l_pac or first_r < l_pac) and rb >= l_pac:
        return NEW
    x, y = qb - last_q, rb - last_r
    if y >= 0 and x - y <= w and y - x <= w and x - last_len < max_chain_gap and y - last_len < max_chain_gap:
        return APPEND
    return NEW


def cover(spans):   # one loop of mem_chain_weight, src/bwamem.c:217-222 / :225-230
    end = w = 0
    for beg, ln in spans:
        if beg >= end:
            w += ln
        elif beg + ln > end:
            w += beg + ln - end
        end = max(end, beg + ln)
    return w


def weight(seeds):   # [(rbeg, qbeg, len)]
    wq, wr = cover([(q, ln) for _, q, ln in seeds]), cover([(r, ln) for r, _, ln in seeds])
    w = min(wq, wr)
    return wq, wr, w if w < 1 << 30 else (1 << 30) - 1


def f32(v):
    return np.float32(v)


def bits(v):
    return int(np.float32(v).view(np.uint32))


def large_overlap(mask_level, max_chain_gap, bj, ej, alt_j, bi, ei, alt_i):   # src/bwamem.c:351-355
    b_max, e_min = max(bj, bi), min(ej, ei)
    if not (e_min > b_max and (not alt_j or alt_i)):
        return 0
    min_l = min(ei - bi, ej - bj)
    return int(bool(f32(e_min - b_max) >= f32(min_l) * f32(mask_level)) and min_l < max_chain_gap)


def drops(drop_ratio, min_seed_len, wj, wi):   # :358
    return int(bool(f32(wi) < f32(wj) * f32(drop_ratio)) and wj - wi >= min_seed_len << 1)


def cut_extend(kept, max_chain_extend):   # :372-379
    kept = list(kept)
    i = k = 0
    while i < len(kept):
        if kept[i] == 0 or kept[i] == 3:
            i += 1
            continue
        k += 1
        if k >= max_chain_extend:
            break
        i += 1
    for j in range(i, len(kept)):
        if kept[j] < 3:
            kept[j] = 0
    return kept


# ---- the cases ----
def contig_table(l_pac, n):
    """where n contigs of unequal lengths start"""
    if n == 1:
        return [0]
    if n == 2:
        return [0, l_pac // 3]
    return [l_pac * k // n + (k * 7) % 5 for k in range(n)]


L_PACS = (1000, (1 << 31) - 3, (1 << 31) + 5, (1 << 32) - 7, (1 << 32) + 11)


def contig_cases():
    out = []
    for l_pac in L_PACS:
        for n in (1, 2, 25):
            offs = contig_table(l_pac, n)
            ends = offs[1:] + [l_pac]
            assert offs == sorted(set(offs)) and offs[0] == 0
            out.append(("C " + " ".join(map(str, offs)), "%d" % n))
            for k in range(n):
                # first and last base of every contig on both strands
                for pos in (offs[k], ends[k] - 1, 2 * l_pac - 1 - offs[k], 2 * l_pac - ends[k]):
                    f = depos(l_pac, pos)
                    assert pos2rid(offs, l_pac, f) == k == bisect_right(offs, f) - 1
                    out.append(("R %d %d" % (l_pac, pos), "%d %d" % (f, k)))
                # intervals: the whole contig, its first and last base, nothing at all (rb == re) at either end, on both strands
                span = ((offs[k], ends[k]), (2 * l_pac - ends[k], 2 * l_pac - offs[k]))
                for b, e in span:
                    for rb, re in ((b, e), (b, b + 1), (e - 1, e), (b, b), (e - 1, e - 1)):
                        assert intv2rid(offs, l_pac, rb, re) == k
                        out.append(("I %d %d %d" % (l_pac, rb, re), "%d" % k))
                # ... and across the contig's right edge on either strand: the next contig, or the other strand
                for e in (ends[k], 2 * l_pac - offs[k]):
                    if e == 2 * l_pac:
                        continue
                    want = intv2rid(offs, l_pac, e - 1, e + 1)
                    assert want == (-2 if e == l_pac else -1)
                    out.append(("I %d %d %d" % (l_pac, e - 1, e + 1), "%d" % want))
            out.append(("I %d %d %d" % (l_pac, l_pac - 19, l_pac + 1), "-2"))
            out.append(("I %d %d %d" % (l_pac, 0, 2 * l_pac), "-2"))
            out.append(("I %d %d %d" % (l_pac, l_pac, l_pac), "%d" % (n - 1)))   # rb == re at the boundary: the rid_b form
            for off, ln in ((offs[-1], l_pac - offs[-1]), (0, ends[0])):
                for rev in (0, 1):
                    out.append(("S %d %d %d %d" % (l_pac, off, ln, rev), "%d %d" % wm.strand_span(l_pac, off, ln, rev)))
    return out


def merge_cases():
    out = []

    def case(group, sides, l_pac, w, gap, first, last, seed):
        want = merge_verdict(l_pac, w, gap, first[0], first[1], last[0], last[1], last[2], seed[0], seed[1], seed[2])
        sides.setdefault(group, set()).add(want)
        out.append(("M %d %d %d %d %d %d %d %d %d %d %d" % (l_pac, w, gap, first[0], first[1], last[0], last[1], last[2], seed[0], seed[1], seed[2]), "%d" % want))
        return want

    sides = {}
    for l_pac, base in ((10 ** 6, 5000), ((1 << 32) + 11, 2 * ((1 << 32) + 11) - 9000), ((1 << 31) - 3, (1 << 31) - 3 - 7000)):
        first, last = (base, 10), (base + 60, 70, 30)    # the chain: query [10, 100), reference [base, base + 90)
        # contained on all four bounds, and one base outside each
        assert case("contained", sides, l_pac, 100, 10000, first, last, (base, 10, 90)) == CONTAINED
        for seed in ((base, 9, 90), (base, 11, 90), (base - 1, 10, 90), (base + 1, 10, 90)):
            assert case("contained", sides, l_pac, 100, 10000, first, last, seed) != CONTAINED
        # y - x and x - y at w and w + 1
        for x, y in ((100, 200), (99, 200), (150, 50), (150, 49)):
            case("band", sides, l_pac, 100, 10000, first, last, (base + 60 + y, 70 + x, 25))
        for x, y in ((2, 4), (1, 4), (9, 7), (9, 6)):
            case("band2", sides, l_pac, 2, 10000, first, last, (base + 60 + y, 70 + x, 40))
        for x, y in ((5, 5), (5, 6), (6, 5)):
            case("band0", sides, l_pac, 0, 10000, first, last, (base + 60 + y, 70 + x, 40))
        # y at -1 and 0 (the seed is longer than the chain's last one: not contained)
        for y in (-1, 0):
            case("y", sides, l_pac, 100, 10000, first, last, (base + 60 + y, 70, 40))
        # x - last_len and y - last_len at max_chain_gap - 1 and max_chain_gap
        for x, y in ((79, 79), (80, 79), (79, 80), (80, 80)):
            case("gap", sides, l_pac, 100, 50, first, last, (base + 60 + y, 70 + x, 25))
    # a reverse-strand seed against a chain whose first or last seed is forward, and against one that is reverse altogether
    l_pac = 5100
    for first_r, last_r in ((5000, 5060), (5000, 5110), (5105, 5110)):
        case("strand", sides, l_pac, 100, 10000, (first_r, 10), (last_r, 70, 30), (last_r + 60, 130, 25))
    case("strand", sides, 10 ** 6, 100, 10000, (5000, 10), (5060, 70, 30), (5120, 130, 25))
    assert sides["contained"] == {CONTAINED, NEW} and all(sides[g] == {NEW, APPEND} for g in sides if g != "contained"), sides
    return out


def weight_cases():
    big = 1 << 29
    sets = [
        [(1000, 0, 20), (1030, 30, 20)],                       # disjoint
        [(1000, 0, 30), (1020, 20, 30)],                       # overlapping on both
        [(1000, 0, 50), (1010, 10, 20)],                       # nested
        [(1000, 0, 30), (1100, 20, 30), (1110, 100, 19)],      # overlapping on the query only
        [(1000, 0, 30), (1000, 20, 30), (1005, 100, 40)],      # a later seed left of the reach so far on the reference
        [(7, 0, 19)],
        [(0, 0, big), (big, big, big - 1)],                    # 2^30 - 1: the cap's value, reached exactly
        [(0, 0, big), (big, big, big)],                        # 2^30: capped
        [(0, 0, big), (big, big, big), (2 * big, 2 * big, big)],
        [((1 << 33) + 5, 0, 30), ((1 << 33) + 25, 20, 30)],
    ]
    sets += [[(q, r, ln) for r, q, ln in s] for s in sets[:6]]   # the same with the query and the reference swapped
    out = []
    for s in sets:
        out.append(("W " + " ".join("%d %d %d" % t for t in s), "%d %d %d" % weight(s)))
    got = [weight(s) for s in sets]
    assert got[3][0] != got[3][1] and got[3][:2] == got[13][1::-1] and got[6][2] == got[7][2] == got[8][2] == (1 << 30) - 1 and got[6][0] == (1 << 30) - 1 < got[7][0]
    return out


def filter_cases():
    out = []
    sides = {}

    def ovl(group, *a):
        want = large_overlap(*a)
        sides.setdefault(group, set()).add(want)
        out.append(("O %d %d %d %d %d %d %d %d" % ((bits(a[0]),) + a[1:]), "%d" % want))

    def drp(group, *a):
        want = drops(*a)
        sides.setdefault(group, set()).add(want)
        out.append(("D %d %d %d %d" % ((bits(a[0]),) + a[1:]), "%d" % want))

    # chain j = [0, min_l) on the query, chain i begins `min_l - overlap` into it and is longer: the overlap at mask_level * min_l and a
    # step to either side (under 0.5 the product is exact; under 0.3f it lies a rounding off 3 / 30 / 45 — the model's float32 decides)
    for mask, min_l in ((0.5, 100), (0.5, 38), (0.5, 7), (0.3, 100), (0.3, 10), (0.3, 150)):
        at = int(min_l * mask)
        for o in (at - 1, at, at + 1):
            ovl(("mask", mask, min_l), mask, 10000, 0, min_l, 0, min_l - o, min_l - o + 200, 0)
            ovl(("mask", mask, min_l), mask, 10000, 500 - o, 700, 0, 500 - min_l, 500, 0)     # the shorter chain is i, on the left
    for o in (0, 1):                                 # e_min > b_max: chains that touch, chains that share one base
        ovl("touch", 0.0, 10000, 0, 50, 0, 50 - o, 120, 0)
    for alt_j, alt_i in itertools.product((0, 1), repeat=2):   # `!ALT(j) || ALT(i)`
        ovl("alt", 0.5, 10000, 0, 100, alt_j, 20, 140, alt_i)
    for gap in (100, 101):                           # min_l < max_chain_gap
        ovl("gap", 0.5, gap, 0, 100, 0, 20, 140, 0)
    for ratio, wj in ((0.5, 100), (0.5, 77), (0.8, 100), (0.8, 65535), (0.8, 45)):
        at = int(wj * ratio)
        for wi in (at - 1, at, at + 1):
            drp(("ratio", ratio, wj), ratio, 1, wj, wi)
    for msl in (19, 10, 30):                         # w_j - w_i at 2 * min_seed_len - 1 and 2 * min_seed_len, w_i below drop_ratio * w_j = 990
        for d in (2 * msl - 1, 2 * msl):
            drp(("seedlen", msl), 0.99, msl, 1000, 1000 - d)
    for ratio in (0.5, 0.8):                         # ... and under the ratios above: w_j = 70, w_i = 33 and 32, below either product
        for d in (37, 38):
            drp(("seedlen", ratio), ratio, 19, 70, 70 - d)
    assert all(v == {0, 1} for v in sides.values()), sides
    return out


def cut_cases():
    arrays = [list(t) for n in (1, 2, 3, 4) for t in itertools.product((0, 1, 2, 3), repeat=n)]
    rng = np.random.default_rng(7)
    arrays += [[int(v) for v in rng.integers(0, 4, n)] for n in (9, 17, 64, 200)]
    out = []
    n_cut = 0
    for a in arrays:
        for mce in sorted({1, 2, len(a)}):
            want = cut_extend(a, mce)
            n_cut += want != a
            out.append(("X %d " % mce + " ".join(map(str, a)), " ".join(map(str, want))))
    assert n_cut > 100
    return out


OPTS = (SimpleNamespace(a=1, o_del=6, e_del=1, o_ins=6, e_ins=1, w=100),     # the defaults
        SimpleNamespace(a=2, o_del=8, e_del=2, o_ins=7, e_ins=3, w=20))


def window_cases():
    out = []
    kinds = set()
    for l_pac, opt in itertools.product(((1 << 31) + 5, (1 << 32) - 7, 40000), OPTS):
        n = 25
        offs = contig_table(l_pac, n)
        contigs = [(o, e - o) for o, e in zip(offs, offs[1:] + [l_pac])]
        gaps = [wm.cal_max_gap(opt, q) for q in range(LQ + 1)]
        out.append(("C " + " ".join(map(str, offs)), "%d" % n))
        out.append(("T " + " ".join(map(str, gaps)), "%d" % len(gaps)))
        far = gaps[100]      # how far beyond the read the seeds below reach
        assert far >= 30
        k = 11
        lo_k, hi_k = offs[k], offs[k + 1]
        starts = {
            "lo<0": 3, "hi>2l": 2 * l_pac - LQ - 3,
            "boundary_fwd": l_pac - LQ - 7, "boundary_rev": l_pac + 7,
            "first_fwd": lo_k + 5, "last_fwd": hi_k - LQ - 5, "last_rev": 2 * l_pac - hi_k + 5, "first_rev": 2 * l_pac - lo_k - LQ - 5,
            "inside_fwd": lo_k + 700, "inside_rev": 2 * l_pac - hi_k + 700,
        }
        for kind, at in starts.items():
            seeds = [(at + 10, 10, 40), (at + 100, 100, 40), (at + 62, 60, 25)]
            rid = pos2rid(offs, l_pac, depos(l_pac, at + 10))
            (lo, hi), (fb, fe), (r0, r1) = wm.chain_window(l_pac, contigs, lambda q: gaps[q], LQ, rid, seeds)
            out.append(("H %d %d %d " % (l_pac, LQ, rid) + " ".join("%d %d %d" % s for s in seeds), "%d %d %d %d" % (fb, fe, r0, r1)))
            for s in seeds:
                out.append(("E %d %d %d %d" % ((LQ,) + s), "%d %d" % wm.seed_reach(s[0], s[1], s[2], LQ, lambda q: gaps[q])))
            out.append(("N %d %d %d %d %d %d" % (l_pac, lo, hi, seeds[0][0], fb, fe), "%d %d" % (r0, r1)))
            # the case is what its name says
            if kind == "lo<0":
                assert lo < 0 and r0 == 0
            elif kind == "hi>2l":
                assert hi > 2 * l_pac and r1 == 2 * l_pac
            elif kind.startswith("boundary"):
                assert lo < l_pac < hi and (r1 == l_pac if kind.endswith("fwd") else r0 == l_pac)
            elif kind.startswith("inside"):
                assert (r0, r1) == (lo, hi)
            else:
                assert (r0 == fb and lo < fb) if kind in ("first_fwd", "last_rev") else (r1 == fe and hi > fe), kind
            kinds.add(kind)
        # chain_window alone: a window across l_pac with the first seed on either strand, at the strand boundary itself
        for first_r in (l_pac - 1, l_pac):
            fb, fe = (0, l_pac) if first_r < l_pac else (l_pac, 2 * l_pac)
            out.append(("N %d %d %d %d %d %d" % (l_pac, l_pac - 50, l_pac + 50, first_r, fb, fe), "%d %d" % wm.clamp(l_pac, l_pac - 50, l_pac + 50, first_r, fb, fe)))
            # ... and windows that begin or end at l_pac: not across it, whatever the first seed's strand (contig bounds left wide open)
            for lo, hi in ((l_pac, l_pac + 50), (l_pac - 50, l_pac)):
                assert wm.clamp(l_pac, lo, hi, first_r, 0, 2 * l_pac) == (lo, hi)
                out.append(("N %d %d %d %d %d %d" % (l_pac, lo, hi, first_r, 0, 2 * l_pac), "%d %d" % (lo, hi)))
    assert len(kinds) == 10
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chainmath") / "chainmath_main")
    # (the sanitizers' runtimes are linked into the program: it starts in whatever environment the suite runs in, unchanged)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g0", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "mpibwa_amd", "csrc"), os.path.join(ROOT, "tests", "chainmath_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("cases", [contig_cases, merge_cases, weight_cases, filter_cases, cut_cases, window_cases], ids=lambda f: f.__name__)
def test_the_header_under_the_sanitizers_against_the_reference_lines(program, cases):
    cs = cases()
    run = subprocess.run([program], input="".join(c + "\n" for c, _ in cs).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    lines = run.stdout.decode().splitlines()
    assert len(lines) == len(cs)
    for (given, want), got in zip(cs, lines):
        assert got == want, given
