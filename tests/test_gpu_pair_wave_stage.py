"""pair_wave_kernel (mpibwa_amd/csrc/pair_wave_kernel.hip) at stage level, through Engine.pairs_wave (the pipeline's own sequence: the
host's rescue listing, the mate-rescue kernel, pair_wave_kernel) and Engine.sam_records, against the reference's own mem_sam_pe on the
regions of its own mem_align1_core (tests/pair_wave_cases.py).

Every pair the kernel takes must be one the reference reports with one line per read and no XA / SA, and both records must equal the
reference's text byte for byte; descriptor and request must say what the reference's line and tests/ref_band.py say; no pair that is
the host's by construction (XA text, supplementary lines, a list past 64, a call with -a / -5 / -P) may be taken; and of the pairs that are
ELIGIBLE by the reference alone the kernel takes at least half (the share and the status histogram are printed).  Launches of 1, 63, 64
and 65 pairs; lists of 9-64 synthetic regions without rescue through the injector of tests/test_pair_stage.py.
Without oracle/_ref/libbwaref.so the tests fail: there is nothing to compare with."""
import numpy as np
import pytest

from mpibwa_amd import abi
from oracle import pyoracle as po

import pair_wave_cases as pw
from ref_band import reg2aln_band
from test_host_pair import CASES

pytestmark = pytest.mark.gpu

OTHER_SCORES = dict(a=1, b=3, o_del=5, e_del=2, o_ins=5, e_ins=2, pen_unpaired=12, T=25)
PATH_OFF = ("MEM_F_ALL", "MEM_F_PRIMARY5", "MEM_F_NOPAIRING")
OPTION_SETS = [dict(c) for c in CASES] + [OTHER_SCORES]


@pytest.fixture(scope="module")
def stage(tmp_path_factory, built):
    from mpibwa_amd import api
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing: the stage test needs the reference"
    api.load_library().mi355x_finalize()
    g = pw.build_index(tmp_path_factory.mktemp("pair_wave_stage"))
    g["engine"] = api.Engine(g["prefix"], device=0)
    g["ref"] = po.RefIndex(g["prefix"])
    return g


def _opts(stage, kw):
    kw = dict(kw)
    flag = abi.MEM_F_PE
    for f in kw.pop("flag_add", "").split("|"):
        if f:
            flag |= getattr(abi, f)
    opt, ropt = stage["engine"].opt(flag=flag, **kw), stage["ref"].opt(flag=flag, **kw)
    if "a" in kw:
        stage["ref"].lib.bwa_fill_scmat(kw["a"], kw["b"], ropt.contents.mat)
        stage["engine"].lib.bwa_fill_scmat(kw["a"], kw["b"], opt.contents.mat)
    return opt, ropt, flag


def _device_regs(pairs):
    from mpibwa_amd import api
    out = []
    for P in pairs:
        for e in range(2):
            a = np.zeros(len(P.before[e]), dtype=api.Engine.REG_DT)
            for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep"):
                a[f] = P.before[e][f]
            out.append(a)
    return out


def _records(eng, opt, pairs, taken, desc, req):
    """the records of the taken pairs through aln_kernel + sam_emit_kernel -> {pair: [record, record]}"""
    reads, quals, names = [], [], []
    d = np.zeros(2 * len(taken), dtype=eng.DESC_DT)
    q = np.zeros(2 * len(taken), dtype=eng.AREQ_DT)
    for j, k in enumerate(taken):
        for e in range(2):
            reads.append(pairs[k].reads[e]); quals.append(pw.quality(len(pairs[k].reads[e]), k)); names.append(pairs[k].name)
            d[2 * j + e] = desc[2 * k + e]
            q[2 * j + e] = req[2 * k + e]
            q[2 * j + e]["read"] = 2 * j + e
    res = eng.sam_records(opt, reads, quals, names, d, q, 2 * np.arange(len(taken) + 1))
    out = {}
    for j, k in enumerate(taken):
        # (a pair whose CIGAR the kernel declines comes back without records: the pipeline hands it to the host; rare, counted by the caller)
        if res["out_len"][2 * j] < 0 or res["out_len"][2 * j + 1] < 0:
            assert res["out_len"][2 * j] == -1 and res["out_len"][2 * j + 1] == -1, (k, res["out_len"][2 * j:2 * j + 2])
            continue
        out[k] = [res["arena"][int(res["out_off"][2 * j + e]):int(res["out_off"][2 * j + e]) + int(res["out_len"][2 * j + e])].tobytes() for e in range(2)]
    return out


def _check(stage, kw, reads, tag):
    """-> (eligible, taken among them, taken)"""
    eng = stage["engine"]
    opt, ropt, flag = _opts(stage, kw)
    pairs, pes = pw.reference_side(stage["ref"], ropt, reads)
    status, desc, req, n_align = eng.pairs_wave(opt, pes, [r for P in pairs for r in P.reads], _device_regs(pairs))
    hist = np.bincount(status, minlength=16)
    taken = [k for k in range(len(pairs)) if status[k] == 1]
    eligible = [k for k, P in enumerate(pairs) if P.eligible]
    if any(flag & getattr(abi, f) for f in PATH_OFF):
        print(tag, "path off: taken", len(taken))
        assert not taken, (tag, len(taken))
        return 0, 0, 0
    rec = _records(eng, opt, pairs, taken, desc, req) if taken else {}
    print(tag, "records handed back by the CIGAR / SAM kernels:", len(taken) - len(rec))
    assert len(rec) * 50 >= len(taken) * 49, (tag, len(taken), len(rec))   # (at most 2 %: the job's own declines, not decisions)
    o = opt.contents
    for k in taken:
        P = pairs[k]
        assert P.plain, (tag, k, "the kernel took a pair the reference reports with XA / SA / extra lines", P.text)
        assert max(P.n_before) <= 64 and max(len(P.after[0]), len(P.after[1])) <= 64, (tag, k, P.n_before)
        for e in range(2):
            if k in rec:
                assert rec[k][e] == P.text[e], (tag, k, e, P.n_before, P.n_rescue, rec[k][e], P.text[e])
            # descriptor and request against the reference's line and its region after the call
            f = P.text[e].split(b"\t")
            d, q = desc[2 * k + e], req[2 * k + e]
            A = P.after[e]
            m = A[(A["rb"] == d["rb"]) & (A["re"] == d["re"]) & (A["qb"] == d["qb"]) & (A["qe"] == d["qe"])]
            assert len(m) == 1, (tag, k, e, "the chosen hit is not one of the reference's", d)
            m = m[0]
            tags = {x[:5]: x[5:] for x in f[11:]}
            assert int(d["flag"]) == int(f[1]) & ~0x30 and int(d["mapq"]) == int(f[4]), (tag, k, e, d, f[:5])
            assert int(d["score"]) == int(tags[b"AS:i:"]) == int(m["score"]) and int(d["sub"]) == int(tags[b"XS:i:"]) == max(int(m["sub"]), int(m["csub"]))
            assert d["req"] == e and (int(q["rb"]), int(q["re"]), int(q["qb"]), int(q["qe"]), int(q["truesc"])) == (int(m["rb"]), int(m["re"]), int(m["qb"]), int(m["qe"]), int(m["truesc"]))
            assert int(q["w2"]) == reg2aln_band(o, int(m["qe"] - m["qb"]), int(m["re"] - m["rb"]), int(m["truesc"]), int(m["w"])), (tag, k, e)
    got = sum(1 for k in eligible if status[k] == 1)
    print(tag, "pairs", len(pairs), "alignments", n_align, "eligible", len(eligible), "taken of them", got, "share %.3f" % (got / max(1, len(eligible))),
          "taken", len(taken), "status histogram", {c: int(v) for c, v in enumerate(hist) if v})
    return len(eligible), got, len(taken)


@pytest.mark.parametrize("case", range(len(OPTION_SETS)))
def test_pair_wave_stage_matches_mem_sam_pe(stage, case):
    from mpibwa_amd import simulate
    from test_sampost import _pairs_of_every_kind
    kw = OPTION_SETS[case]
    damaged = pw.make_reads(stage["seqs"], stage["copies"], True)
    clean = pw.make_reads(stage["seqs"], stage["copies"], False)
    every = _pairs_of_every_kind(stage, n=360, seed=40 + case)
    reads = damaged + every + (clean if case == 0 else [])
    n_el, n_got, n_taken = _check(stage, kw, simulate.reads_to_ascii(reads), "case %d %s" % (case, kw))
    flags = kw.get("flag_add", "")
    if any(f in flags for f in PATH_OFF):
        return
    if "MEM_F_NO_RESCUE" in flags:   # (no rescue: what is left are the long lists)
        assert n_got * 2 >= n_el, (n_el, n_got)
        return
    assert n_el >= 300, n_el
    assert n_got * 2 >= n_el, ("the kernel takes less than half of the eligible pairs", n_el, n_got)


def test_pair_wave_stage_small_launches(stage):
    """launches of 1, 63, 64 and 65 pairs give what the big launch gives for the same pairs (same ids: the first pairs of the list)"""
    from mpibwa_amd import simulate
    eng = stage["engine"]
    opt, ropt, _ = _opts(stage, {})
    reads = simulate.reads_to_ascii(pw.make_reads(stage["seqs"], stage["copies"], True)[1::2][:200])   # (the damaged mates)
    pairs, pes = pw.reference_side(stage["ref"], ropt, reads)
    regs = _device_regs(pairs)
    flat = [r for P in pairs for r in P.reads]
    status, desc, req, _ = eng.pairs_wave(opt, pes, flat, regs)
    assert (status[:65] == 1).sum() >= 10, np.bincount(status[:65])
    for n in (1, 63, 64, 65):
        s, d, q, _ = eng.pairs_wave(opt, pes, flat[:2 * n], regs[:2 * n])
        assert (s == status[:n]).all(), (n, s, status[:n])
        for k in np.flatnonzero(s == 1):
            assert d[2 * k:2 * k + 2].tobytes() == desc[2 * k:2 * k + 2].tobytes() and q[2 * k:2 * k + 2].tobytes() == req[2 * k:2 * k + 2].tobytes(), (n, k)


def _synthetic_lists(offs, l_pac, which_pes, pen_unpaired):
    """300 pairs of 9-64 full-length hits on end 0, most with a mate hit at a proper distance in the library's orientation -> [[end 0, end 1]]"""
    from test_pair_stage import PES_SETS
    low, high = PES_SETS[which_pes][0][1 + which_pes][:2]
    rng = np.random.default_rng(70 + which_pes)
    lists = []
    for k in range(300):
        n0 = int(rng.integers(9, 65))
        ends = [[], []]
        for j in range(n0):   # hit j of end 0 and, for most, a mate hit at a proper distance in the library's orientation
            c = int(rng.integers(0, len(offs) - 1))
            pos = int(rng.integers(offs[c] + 1500, offs[c + 1] - 1500))
            d = int(rng.integers(low + 10, high - 10))
            fp = pos + d - 149 if which_pes == 0 else pos - d - 149   # where the reverse-strand mate starts on the forward strand
            fwd_rb, rev_rb = pos, 2 * l_pac - (fp + 150)
            r0, r1 = (fwd_rb, rev_rb) if rng.random() < 0.5 else (rev_rb, fwd_rb)
            # (full-length hits: every later hit is secondary to the first; scores under 0.8 x 150 get no XA entry, and every fourth
            # pair has many above it: more than max_XA_hits qualifying hits and the reference writes no XA string at all)
            hi = 151 if k % 4 == 0 else 118
            sc = int(rng.integers(60, hi)) if j else 150
            sc1 = int(rng.integers(60, hi)) if j else 150
            ends[0].append((r0, r0 + 150, 0, 150, c, sc))
            if j == 0 or sc >= 150 - pen_unpaired or rng.random() < 0.8:   # (a candidate of mem_sam_pe's rescue loop always has its mate)
                ends[1].append((r1, r1 + 150, 0, 150, c, sc1))
        arr = []
        for e in range(2):
            a = np.zeros(len(ends[e]), dtype=po.ALNREG_DT)
            for i, (rb, re, qb, qe, rid, sc) in enumerate(ends[e]):
                a[i]["rb"], a[i]["re"], a[i]["qb"], a[i]["qe"], a[i]["rid"], a[i]["score"], a[i]["truesc"] = rb, re, qb, qe, rid, sc, sc
                a[i]["w"], a[i]["seedcov"], a[i]["seedlen0"], a[i]["secondary"] = 100, sc // 2, 19, -1
            arr.append(a)
        lists.append(arr)
    return lists, rng


@pytest.mark.parametrize("which_pes", [0, 1])
def test_pair_wave_stage_on_long_synthetic_lists(stage, which_pes):
    """9-64 regions per end that need no rescue (every candidate hit, one within pen_unpaired of the best, has a mate hit at a proper
    distance), through the reference's mem_sam_pe compiled with recorders (oracle/pair_inject.c): the pairs the kernel takes are pairs
    the reference reports through its paired branch without alignment and without XA, with the same region, flag, MAPQ and sub-optimal
    score.  (The recorder answers every alignment mem_matesw asks for with score 0, which the real mate-rescue kernel does not: a pair
    with rescue cannot be judged here; those are judged on real regions above.)"""
    from test_pair_stage import PES_SETS, _pes
    assert po.pair_inject_available(), "oracle/_ref/libpairinj.so is missing"
    eng, ref = stage["engine"], stage["ref"]
    opt, ropt, _ = _opts(stage, {})
    l_pac = int(eng.bns.contents.l_pac)
    offs = [int(eng.bns.contents.anns[k].offset) for k in range(int(eng.bns.contents.n_seqs))] + [l_pac]
    pes = _pes(PES_SETS[which_pes][0])
    lists, rng = _synthetic_lists(offs, l_pac, which_pes, int(opt.contents.pen_unpaired))
    id0 = 777
    wants = [po.ref_pair(ropt, ref.bns, ref.pac, pes, id0 + k, 150, arr[0], arr[1]) for k, arr in enumerate(lists)]
    assert all(w["n_align"] == 0 for w in wants), [k for k, w in enumerate(wants) if w["n_align"]]   # (the lists are what they are meant to be)
    # the lists as they stand after the reference's mem_sort_dedup_patch (the kernel's input), by the library's host twin of it
    reads = [rng.integers(0, 4, 150).astype(np.uint8) for _ in range(2 * len(lists))]
    regs = []
    import ctypes as C
    for k, arr in enumerate(lists):
        for e in range(2):
            mine = arr[e].copy()
            m = eng.lib.mi355x_host_sort_dedup_patch(opt, eng.bns, C.cast(eng.pac, C.c_void_p), reads[2 * k + e].ctypes.data, mine.ctypes.data, len(mine))
            a = np.zeros(m, dtype=eng.REG_DT)
            for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep"):
                a[f] = mine[:m][f]
            regs.append(a)
    status, desc, req, n_align = eng.pairs_wave(opt, pes, reads, regs, n_processed=2 * id0)
    n_taken = n_plain = 0
    for k, want in enumerate(wants):
        plain = want["paired"] and want["n_align"] == 0 and want["n_xa"] == (0, 0) and want["n_lines"] == 2
        n_plain += plain
        if status[k] != 1:
            continue
        n_taken += 1
        assert plain, (k, "the kernel decided a pair the reference treats otherwise", want)
        for e in range(2):
            d, L = desc[2 * k + e], want["lines"][e]
            got = dict(rb=int(d["rb"]), re=int(d["re"]), qb=int(d["qb"]), qe=int(d["qe"]), score=int(d["score"]), sub=int(d["sub"]), flag=int(d["flag"]), mapq=int(d["mapq"]))
            assert got == {f: L[f] for f in got}, (k, e, got, L)
    print("synthetic long lists: pairs", len(lists), "reference-plain", n_plain, "taken", n_taken, "alignments", n_align, "status", np.bincount(status, minlength=16))
    assert n_plain >= 20 and n_taken * 2 >= n_plain, (n_plain, n_taken)


def test_pair_wave_stage_without_insertion_open_penalty(stage):
    """o_ins = 0: mate rescue is not the kernels' (msw_on_device), the stage entry answers every listed alignment with flags = 1, and a
    pair whose replay needs one is left to the host (PW_HOST_NO_RESULT = 12); what the kernel still decides is the reference's."""
    from mpibwa_amd import simulate
    eng = stage["engine"]
    kw = dict(o_ins=0)
    reads = simulate.reads_to_ascii(pw.make_reads(stage["seqs"], stage["copies"], True)[:400])
    opt, ropt, _ = _opts(stage, kw)
    pairs, pes = pw.reference_side(stage["ref"], ropt, reads)
    status, _, _, n_align = eng.pairs_wave(opt, pes, [r for P in pairs for r in P.reads], _device_regs(pairs))
    assert n_align > 0 and (status == 12).sum() >= 10, (n_align, np.bincount(status, minlength=16))
    _check(stage, kw, reads, "o_ins = 0")
    # the same pairs under the defaults: the kernel reads its rescue results and decides more of them
    opt, ropt, _ = _opts(stage, {})
    pairs, pes = pw.reference_side(stage["ref"], ropt, reads)
    status_d, _, _, _ = eng.pairs_wave(opt, pes, [r for P in pairs for r in P.reads], _device_regs(pairs))
    assert (status_d == 1).sum() > (status == 1).sum(), (np.bincount(status_d, minlength=16), np.bincount(status, minlength=16))
