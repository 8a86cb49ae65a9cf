"""Host logic (no GPU): the cases of tests/aln_cases.py reach the branches of aln_kernel they are there for, shown by the reference's own
bwa_gen_cigar2 (oracle/_ref/libbwaref.so) and the plain restatement of the kernel's dispatch — before any kernel is involved; and
oracle/pyoracle.py: reg2aln_loop, the loop every comparison of aln_kernel goes through, equals the reference's own mem_reg2aln."""
import collections

import numpy as np
import pytest

import aln_cases as ac
from oracle import pyoracle as po

DECLINES_ALLOWED = ("f.bridging", "f.empty", "f.overlong")


@pytest.fixture(scope="module")
def ref(built):
    if not po.ref_available():
        pytest.skip("the reference library is not built")
    ri = po.RefIndex.__new__(po.RefIndex)
    ri.lib = po.ref_lib()
    return ri


def setup(ri, o, cs):
    ropt = ac.apply(ri.lib.mem_opt_init(), ri.lib.bwa_fill_scmat, o)
    rounds = ac.Rounds(ri, ropt, cs)
    ac.fix_truesc(cs, o, rounds)
    return rounds


_memo = {}


def family_set(ri, name):
    if name not in _memo:
        o, cs = ac.cases(name)
        rounds = setup(ri, o, cs)
        _memo[name] = (o, cs, rounds, ac.predict(cs, o, rounds, 0))
    return _memo[name]


def same_result(x, y):
    return x[0] == y[0] and len(x[1]) == len(y[1]) and (np.asarray(x[1]) == np.asarray(y[1])).all() and x[2] == y[2] and x[3] == y[3]


def agree(pred):
    """the expected answers are pyoracle's reg2aln_loop's (Rounds.loop), which test_reg2aln_loop_is_the_reference_mem_reg2aln pins to
    mem_reg2aln; the walk that predicts the class (aln_cases.predict: run_dp) must end on the same round for every answered request"""
    for p in pred:
        if p.flags == 0 and p.cls != "nodp":
            assert same_result(p.result, p.last), (p.cls, p.rounds)


def subs(cs, pred, sub):
    return [(i, pred[i]) for i in range(len(cs)) if cs.sub[i] == sub]


def test_generated_cases_hold_what_they_promise():
    """what needs no alignment: l_pac, the packed reference, window bounds, all four alignments of a window on both strands"""
    assert ac.L_PAC % 4 != 0 and ac.L_PAC_REUSE % 4 != 0
    o, cs = ac.cases("default")
    pac, L = cs.pac, cs.l_pac
    assert len(pac) == L // 4 + 1
    for p in (0, 1, 2, 3, 4, L - 1, L - 2, 12345):
        assert (pac[p >> 2] >> ((~p & 3) << 1)) & 3 == cs.ref[p]
    for fam in "abcf":
        seen = {(cs.rb[i] & 3, cs.rb[i] >= L) for i in range(len(cs)) if cs.fam[i] == fam}
        assert len(seen) == 8, (fam, seen)
    ends = {(cs.rb[i], cs.re[i]) for i in range(len(cs))}
    assert any(rb == 0 for rb, re in ends) and any(re == L for rb, re in ends) and any(rb == L for rb, re in ends) and any(re == 2 * L for rb, re in ends)
    # a scoring matrix of bwa_fill_scmat has amax = a > 0: the kernel's `amax <= 0` branch is not constructible
    assert all(ac.Opt(n).mat.max() == ac.Opt(n).a > 0 for n in ac.OPTION_SETS)


@pytest.mark.parametrize("name", list(ac.OPTION_SETS))
def test_families_a_b_c_f_reach_their_branches(ref, name):
    o, cs, rounds, (pred, counts) = family_set(ref, name)
    wmax4 = o.w << 2
    # only the bridging, empty and over-long requests are declined
    for i, p in enumerate(pred):
        assert (p.flags == 1) == (cs.sub[i] in DECLINES_ALLOWED), (name, i, cs.sub[i], p.cls, p.why)
        if cs.sub[i] in ("f.bridging", "f.empty"):
            assert rounds(i, 5)[1] is None        # the reference rejects it too
    agree(pred)
    by = collections.Counter((cs.fam[i], p.cls, p.moved) for i, p in enumerate(pred))
    assert by[("a", "nodp", False)] and by[("c", "nodp", False)] and by[("c", "narrow", False)] and by[("c", "full", False)] and by[("f", "narrow", False)]
    if o.w:
        assert by[("a", "narrow", True)] and by[("b", "narrow", True)] and by[("b", "narrow", False)], by
    # ---- a: the bound
    loss = lambda i: (cs.qe[i] - cs.qb[i]) * o.a - int(o.mat[cs.window(i), cs.query(i)].sum())
    at = subs(cs, pred, "a.at") or subs(cs, pred, "a.at.below")
    assert len(at) == 8 and len(subs(cs, pred, "a.above")) == 8
    for i, p in at:
        assert p.cls == "nodp" and (loss(i) == o.bound if cs.sub[i] == "a.at" else loss(i) < o.bound)
        assert len(p.result[1]) == 1 and p.result[0] == (cs.qe[i] - cs.qb[i]) * o.a - loss(i)      # the reference's DP says lqM
    if name == "default":
        assert subs(cs, pred, "a.at") and o.bound == 15
    for i, p in subs(cs, pred, "a.above"):
        assert loss(i) > o.bound and (p.moved if o.w else p.cls == "nodp")
        assert all(l <= o.bound or l >= loss(i) for l in ac.reachable_losses(o))                    # the smallest reachable loss above
    for i, p in at + subs(cs, pred, "a.above"):     # N columns (a + 1 each) exactly where mismatches alone cannot make the loss
        assert int((cs.query(i) == 4).sum()) == ac.reachable_losses(o)[loss(i)][1] and (loss(i) % (o.a + o.b) != 0) == (4 in cs.query(i))
    for i, p in subs(cs, pred, "a.tie"):
        lq = cs.qe[i] - cs.qb[i]
        assert loss(i) == 3 * (o.a + o.b)
        if name == "default":      # 3 mismatches = 1D .. 1I = lq - 15, and the diagonal wins the tie
            assert lq * o.a - loss(i) == (lq - 1) * o.a - o.oe_del - o.oe_ins == p.result[0] and p.cls == "nodp"
            assert list(p.result[1]) == [lq << 4] and p.result[2] == 3
    for i, p in subs(cs, pred, "a.tie4"):
        lq = cs.qe[i] - cs.qb[i]
        assert loss(i) == 4 * (o.a + o.b)
        if name == "default":      # ... with a fourth mismatch the gapped path is better by a + b
            assert p.moved and p.result[0] == (lq - 1) * o.a - o.oe_del - o.oe_ins and [c & 0xf for c in p.result[1]] == [2, 0, 1]
    for i, p in subs(cs, pred, "a.w0"):
        assert p.cls == "nodp" and loss(i) > 2 * o.bound and len(p.result[1]) == 1
    # ---- b: the loop's conditions, each deciding alone (score == last_sc, w2 == w << 2, i == 3, score >= truesc - a)
    alone = collections.Counter((p.stop, len(p.rounds)) for i, p in enumerate(pred) if cs.fam[i] == "b" and p.stop and sum(p.stop) == 1)
    if o.w:
        assert alone[((False, True, False, False), 1)] and alone[((False, False, False, True), 1)], alone       # w << 2 and truesc in round 1
        assert all(len(p.rounds) == 1 for i, p in subs(cs, pred, "b.ts_stop")) and all(len(p.rounds) >= 2 for i, p in subs(cs, pred, "b.ts_go"))
    if o.w >= 3:
        assert alone[((True, False, False, False), 2)] and alone[((False, False, True, False), 3)], alone       # same score in round 2, ++i < 3
        r2 = [p.rounds[1][2] > p.rounds[0][2] for i, p in subs(cs, pred, "b.r2")]
        assert sum(r2) * 2 >= len(r2) > 0, (name, r2)                                    # found in round 2
        r3 = [len(p.rounds) == 3 and p.rounds[2][2] > p.rounds[1][2] > p.rounds[0][2] for i, p in subs(cs, pred, "b.r3pair")]
        assert sum(r3) * 2 >= len(r3) > 0, (name, r3)                                    # round 2 changes the score, round 3 again
        assert all(len(p.rounds) == 3 and p.stop[2] for i, p in subs(cs, pred, "b.never") if not p.stop[0])
    if o.w == 0:
        assert all(p.cls == "nodp" or cs.re[i] - cs.rb[i] != cs.qe[i] - cs.qb[i] for i, p in enumerate(pred) if p.flags == 0)
    # ---- c: which term of the band decides, and the shapes
    terms = collections.Counter()
    for i, p in enumerate(pred):
        if cs.fam[i] == "c" and p.cls != "nodp":
            lq, rlen = cs.qe[i] - cs.qb[i], cs.re[i] - cs.rb[i]
            d, w2 = abs(rlen - lq), p.rounds[0][0]
            w = ac.band(o, lq, rlen, w2)[0]
            M = (ac.max_gap(o, lq) + d + 1) >> 1
            terms[(d, "min_w" if w == d + 3 and min(M, w2) < d + 3 else "w2" if w == w2 < M else "max_gap" if w == M < w2 else "=")] += 1
            terms["n_col=lq" if p.rounds[0][1] == lq else "n_col=2w+1"] += 1
            terms["rows%d" % rlen] += 1
            terms["strips%d" % ((p.rounds[0][1] + 63) // 64)] += 1
    for d in (0, 1, 20, 45):      # w2 on either side of d + 3 and of (max_gap + d + 1) >> 1, whichever of the three terms then decides
        M = (ac.max_gap(o, 100) + d + 1) >> 1
        assert {d + 2, d + 3, d + 4, M - 1, M, M + 1} <= {cs.w2[i] for i, p in subs(cs, pred, "c.d%d" % d)} | {-1}
        assert terms[(d, "min_w")] or (d == 0 and o.w == 0), (name, d, terms)
    assert o.w < 25 or (any(terms[(d, "w2")] for d in (0, 1, 20, 45)) and any(terms[(d, "max_gap")] for d in (0, 1, 20, 45))), (name, terms)
    minw = [(cs.re[i] - cs.rb[i]) - (cs.qe[i] - cs.qb[i]) + 3 in [c >> 4 for c in p.result[1] if c & 0xf == 2] and 3 in [c >> 4 for c in p.result[1] if c & 0xf == 1]
            for i, p in subs(cs, pred, "c.minw")]
    assert len(minw) == 12 and sum(minw) >= 6, (name, minw)       # the reference's path leaves the diagonal by d + 3 = the band
    assert terms["n_col=lq"] and terms["n_col=2w+1"] and terms["rows1"] and terms["rows63"] and terms["rows64"] and terms["rows65"], terms
    assert terms["strips2"] or o.w < 25 or ac.max_gap(o, 150) < 64, terms
    # ---- f
    for sub in ("f.tandem.del", "f.tandem.ins", "f.tandem.both", "f.N", "f.clip", "f.edge.first", "f.edge.last"):
        got = subs(cs, pred, sub)
        assert got and all(p.flags == 0 for i, p in got) and {cs.rb[i] >= cs.l_pac for i, p in got} == {False, True}, sub
    assert all(p.result[2] > 0 for i, p in subs(cs, pred, "f.tandem.del") + subs(cs, pred, "f.N"))
    assert all(4 in cs.query(i) for i, p in subs(cs, pred, "f.N"))
    # the three lists: every live request is on the first or starts on the second, and what is moved or handed on is counted again
    assert counts[0] + counts[1] - sum(p.moved for p in pred) == len(cs) and counts[2] == sum(p.lists[2] for p in pred)


def test_the_loop_conditions_decide_alone_in_every_round(ref):
    """over all option sets: `w2 == w << 2` alone in rounds 1 and 2, and in round 3 with a changed score (there `++i < 3` ends the loop as
    well: nothing tells the two apart); `score == last_sc` alone in round 2, `++i < 3` alone, truesc alone in rounds 1 and 2"""
    alone = collections.Counter()
    for name in ac.OPTION_SETS:
        o, cs, rounds, (pred, counts) = family_set(ref, name)
        alone.update((p.stop, len(p.rounds)) for i, p in enumerate(pred) if cs.fam[i] == "b" and p.stop and (sum(p.stop) == 1 or len(p.rounds) == 3))
    assert alone[((False, True, False, False), 1)] and alone[((False, True, False, False), 2)] and alone[((False, True, True, False), 3)], alone
    assert alone[((True, False, False, False), 2)] and alone[((False, False, True, False), 3)] and alone[((False, False, False, True), 2)], alone


@pytest.mark.parametrize("name", [n for n in ac.OPTION_SETS if n != "default"])
def test_every_option_set_changes_the_answer_of_20_requests(ref, name):
    """the set's requests under the set and under the default options: the reference's answer or the predicted class differs for at least
    20 of them.  w = 25 and w = 1000 cannot do that for a read the kernel takes: they only move `w2 == w << 2`, and a band stops growing
    at (max_gap + d + 1) >> 1, below 100 for reads of up to 150 bp — for these two sets the executed rounds (the w2 of every round the
    loop runs) are what differs, and that is what is counted."""
    o, cs, rounds, (pred, counts) = family_set(ref, name)
    d = ac.Opt("default")
    drounds = ac.Rounds(ref, ac.apply(ref.lib.mem_opt_init(), ref.lib.bwa_fill_scmat, d), cs)
    dpred, dcounts = ac.predict(cs, d, drounds, 0)
    n = 0
    for p, q in zip(pred, dpred):
        same = (p.cls, p.moved, p.flags) == (q.cls, q.moved, q.flags)
        if same and p.flags == 0:
            same = p.result[0] == q.result[0] and p.result[2] == q.result[2] and p.result[3] == q.result[3] and list(p.result[1]) == list(q.result[1])
            if name in ("w25", "w1000"):
                assert same
                same = [r[0] for r in p.rounds] == [r[0] for r in q.rounds]
        n += not same
    assert n >= 20, (name, n)


@pytest.mark.parametrize("name", ac.WIDE_SETS)
def test_families_d_e_g_reach_their_branches(ref, name):
    # ---- d: the capacities of a batch whose longest read is 150, 250, 700 bp
    for max_len in (150, 250, 700):
        o, cs = ac.cases_d(name, max_len)
        rounds = setup(ref, o, cs)
        pred, counts = ac.predict(cs, o, rounds, 0)
        assert cs.max_len == max_len
        agree(pred)
        cells = lambda i, k=0: pred[i].rounds[k][1] * (cs.re[i] - cs.rb[i])
        for i, p in subs(cs, pred, "d.small.at"):
            assert p.cls == "narrow" and cells(i) == ac.aln_zcap_small(max_len) and p.lists == [0, 1, 0]
        for i, p in subs(cs, pred, "d.small.over"):
            assert p.cls == "full" and cells(i) == ac.aln_zcap_small(max_len) + p.rounds[0][1] and p.lists == [0, 1, 1]
        for i, p in subs(cs, pred, "d.full.at"):
            assert p.cls == "full" and cells(i) == ac.aln_zcap(max_len)
        for i, p in subs(cs, pred, "d.full.over"):
            assert (p.cls, p.why, p.lists) == ("declined", "zcap", [0, 1, 1])
            assert ac.band(o, cs.qe[i] - cs.qb[i], cs.re[i] - cs.rb[i], cs.w2[i])[1] * (cs.re[i] - cs.rb[i] - 1) == ac.aln_zcap(max_len)
        out = subs(cs, pred, "d.outgrow")
        assert len(out) == 4
        for i, p in out:      # fits the narrow matrix in round 1, not in round 2: restarted, and the answer is the reference's last round
            assert p.cls == "full" and p.lists == [0, 1, 1] and len(p.rounds) >= 2
            assert cells(i, 0) <= ac.aln_zcap_small(max_len) < cells(i, 1) <= ac.aln_zcap(max_len)
            assert same_result(p.result, p.last) and same_result(p.last, rounds(i, p.rounds[-1][0]))
        assert sum(p.flags for p in pred) == len(subs(cs, pred, "d.full.over")) == 2
    # ---- e
    o, cs = ac.cases_e(name)
    rounds = setup(ref, o, cs)
    pred, counts = ac.predict(cs, o, rounds, 0)
    agree(pred)
    ops = lambda i: [c & 0xf for c in rounds(i, min(cs.w2[i], o.w << 2))[1]]
    for sub, n_ops in (("e.cig95", 95), ("e.cig96", 96), ("e.cig97", 97)):
        got = subs(cs, pred, sub)
        assert len(got) == 2 and all(len(ops(i)) == n_ops for i, p in got), (sub, [len(ops(i)) for i, p in got])
        assert all((p.flags, p.why) == ((1, "cigar") if n_ops > 96 else (0, None)) for i, p in got)
    assert all(ops(i)[0] == 1 for i, p in subs(cs, pred, "e.cig96"))
    for sub, n_md in (("e.md768", 768), ("e.md769", 769)):
        got = subs(cs, pred, sub)
        assert len(got) == 2 and all(len(rounds(i, 0)[3]) == n_md and p.lists == [1, 0, 0] for i, p in got)
        assert all((p.flags, p.why) == ((1, "md") if n_md > 768 else (0, None)) for i, p in got)
    for sub, first, last in (("e.del_first", 2, 0), ("e.del_last", 0, 2), ("e.ins_first", 1, 0), ("e.ins_last", 0, 1)):
        got = subs(cs, pred, sub)
        hit = [i for i, p in got if p.flags == 0 and (p.result[1][0] & 0xf, p.result[1][-1] & 0xf) == (first, last)]
        assert len(got) == 4 and len(hit) >= 3, (sub, [list(p.result[1]) for i, p in got])
        for i in hit:
            p = pred[i]
            if 2 in (first, last):     # MD skips a deletion at either end and NM does not count it
                assert b"^" not in p.result[3] and p.result[2] == 0
            else:
                assert p.result[2] == (p.result[1][0 if first else -1] >> 4)
    assert {p.why for p in pred if p.flags} <= {"cigar", "md"} and {cs.sub[i] for i, p in enumerate(pred) if p.flags} <= {"e.cig97", "e.md769", "e.md.dp"}
    # ---- g
    o, cs, order = ac.cases_g(name)
    rounds = setup(ref, o, cs)
    pred, counts = ac.predict(cs, o, rounds, 0)
    assert all(p.flags == 0 for p in pred) and len(cs) == max(ac.LAUNCH_SIZES)
    agree(pred)
    assert collections.Counter(p.cls for p in pred)["nodp"] > 60 and sum(p.moved for p in pred) > 60 and counts[2] > 5
    mixed = ac.with_unused(cs, order)
    kinds = [-1 if mixed.read[i] < 0 else int(mixed.re[i] - mixed.rb[i] == mixed.qe[i] - mixed.qb[i]) for i in range(len(mixed))]
    waves = [collections.Counter(kinds[k:k + 64]) for k in range(0, len(kinds), 64)]
    for kind in (0, 1):
        assert {0, 1, 63, 64} <= {w[kind] for w in waves}, waves
    assert any(w[-1] == 64 for w in waves) and sum(0 < w[-1] < 64 for w in waves) >= 3
    o, cs = ac.cases_reuse(name)
    rounds = setup(ref, o, cs)
    for which in (0, 1):
        pred, counts = ac.predict(cs, o, rounds, which)
        assert all(p.flags == 0 for p in pred) and cs.max_len == 700 and len(subs(cs, pred, "g.reuse.big")) == 6
        agree(pred)
        order = ac.reuse_order(cs, pred, 256)
        lds = ac.lds_bytes(700)
        n = [sum(pred[i].lists[k] for i in order) for k in range(3)]
        assert lds[2] > 64 * 1024 and n[0] > 2 * ac.grid_for(lds[0], 256, len(order)) and n[2 if which else 1] > 2 * ac.grid_for(lds[2 if which else 1], 256, len(order))
        assert len(order) < 45000 and len({i for i in order}) == len(cs)
        need = [pred[i].need for i in order]
        assert min(need) <= 12 and max(need) > 700 and sum(x > 60 for x in need) > 1000


@pytest.mark.parametrize("name", list(ac.PIN_SETS))
def test_reg2aln_loop_is_the_reference_mem_reg2aln(genome, built, name):
    """oracle/pyoracle.py: reg2aln_loop around bwa_gen_cigar2, started with the band mem_reg2aln infers (tests/ref_band.py), gives the
    CIGAR, NM and MD of the reference's own mem_reg2aln on the session index, once its squeezed deletion and its clips are undone.
    Under w = 6 the regions also sit on either side of `score < truesc - a` and behind `++i < 3`, and the reference's rounds show that
    another reading of either condition would give another answer: with `<=` a "ts_stop" region gets its round-2 answer, with
    `++i < 4` a "round4" region its round-4 answer (both checked once by editing reg2aln_loop: the test fails)."""
    if not po.ref_available():
        pytest.skip("the reference library is not built")
    import ref_band
    ri = po.RefIndex(genome["prefix"])
    o = ac.Opt(name, ac.PIN_SETS[name])
    opt = ac.apply(ri.lib.mem_opt_init(), ri.lib.bwa_fill_scmat, o)
    L = int(ri.bns.contents.l_pac)
    pac = np.ctypeslib.as_array(ri.pac, shape=(L // 4 + 1,))
    n_rounds, seen = collections.Counter(), collections.Counter()
    for what, read, fb, fe, qb, qe, truesc, reg_w, rev, rel in ac.pin_regions(o, genome["seqs"][0]):
        if rev:
            read, fb, fe, qb, qe = ac.rc(read), 2 * L - fe, 2 * L - fb, len(read) - qe, len(read) - qb
        band = lambda t: ref_band.reg2aln_band(o, qe - qb, fe - fb, t, reg_w)
        rnd = lambda w: ri.gen_cigar2(opt, L, pac, read[qb:qe], fb, fe, w)
        if rel is not None:            # truesc = the round-1 score + rel, and the band inferred from it is the one that score was made with
            w2 = band(truesc)
            truesc = rnd(w2)[0] + rel
            assert band(truesc) == w2 == 3
        w2 = band(truesc)
        reg = np.zeros(1, dtype=po.ALNREG_DT)
        reg["rb"], reg["re"], reg["qb"], reg["qe"], reg["rid"], reg["truesc"], reg["score"], reg["w"], reg["secondary"] = fb, fe, qb, qe, 0, truesc, truesc, reg_w, -1
        cig, nm, md, pos, is_rev = ri.reg2aln(opt, read, reg)
        assert bool(is_rev) == rev
        sc, want, want_nm, want_md = ri.reg2aln_loop(opt, L, pac, read[qb:qe], fb, fe, w2, truesc)
        want = list(want)
        if want[0] & 0xf == 2:         # src/bwamem.c:1127-1136
            want = want[1:]
        elif want[-1] & 0xf == 2:
            want = want[:-1]
        assert [c for c in cig if c & 0xf != 3] == want and (nm, md) == (want_nm, want_md), (name, what, rev, w2, list(cig), want, md, want_md)
        assert sum(c >> 4 for c in cig if c & 0xf == 3) == len(read) - (qe - qb)
        n_rounds[w2] += 1
        # what the reference's rounds say about the regions that sit on a condition
        if what in ("ts_stop", "ts_go"):
            r1, r2 = rnd(3), rnd(6)
            assert r2[0] > r1[0] and r1[2:] != r2[2:]                  # stopping after round 1 and going on give different answers
            assert ((nm, md) == r1[2:]) == (what == "ts_stop")         # mem_reg2aln stops at truesc = round-1 score + a and goes on at + a + 1
            seen[what] += 1
        elif what == "round4":
            r = [rnd(w) for w in (3, 6, 12, 24)]
            if r[0][0] < r[1][0] < r[2][0] < r[3][0] and r[2][0] < truesc - o.a:   # every round changes the score: only `++i < 3` ends the loop
                assert (nm, md) == r[2][2:] != r[3][2:]
                seen[what] += 1
    assert len(n_rounds) >= 6 and n_rounds[0] and len(n_rounds) - bool(n_rounds[0]) >= 5 or name == "w6", n_rounds     # inferred bands: none, and five others
    if name == "w6":
        assert seen["ts_stop"] == 8 and seen["ts_go"] == 8 and seen["round4"] >= 4, seen
