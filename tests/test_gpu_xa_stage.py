"""The XA listing of pair_wave_kernel and the XA text of sam_emit_kernel at stage level: Engine.pairs_wave_xa (the pipeline's own
sequence with XA on) and Engine.sam_records against the reference's own mem_sam_pe on the regions of its own mem_align1_core
(tests/pair_wave_cases.py, tests/xa_cases.py), against its mem_sam_pe on synthetic lists (oracle/pair_inject.c) and against its
mem_gen_alt on hand-made descriptors (tests/sam_stage_cases.py).

Every pair the kernel decides with PW_DECIDED_XA is one the reference reports with one line per read, an XA tag on at least one and no
SA / pa; both records equal the reference's bytes; the XA requests of an end are as many as the tag has entries, each a region of the
reference's list after the call with the band of tests/ref_band.py.  Status 1 still means "both records plain".  Under -a, -5, -P and
with max_XA_hits beyond the kernel's cap nothing is taken with a tag.  Of the XA-only pairs by the reference the kernel takes at least
half, and at most 5 % of the taken pairs come back without records (up to 12 requests a pair where a plain one has 2, whose cap is 2 %).
Without oracle/_ref/libbwaref.so the tests fail: there is nothing to compare with."""
import ctypes as C

import numpy as np
import pytest

from mpibwa_amd import abi
from oracle import pyoracle as po

import pair_wave_cases as pw
import sam_stage_cases as sc
import xa_cases as xc
from ref_band import reg2aln_band
from test_host_pair import CASES

pytestmark = pytest.mark.gpu

XA = 16   # PW_DECIDED_XA
OTHER_SCORES = dict(a=1, b=3, o_del=5, e_del=2, o_ins=5, e_ins=2, pen_unpaired=12, T=25)
PATH_OFF = ("MEM_F_ALL", "MEM_F_PRIMARY5", "MEM_F_NOPAIRING")
OPTION_SETS = [dict(c) for c in CASES] + [OTHER_SCORES, dict(max_XA_hits=3), dict(XA_drop_ratio=0.5), dict(max_XA_hits=9)]


@pytest.fixture(scope="module")
def stage(tmp_path_factory, built):
    from mpibwa_amd import api
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing: the stage test needs the reference"
    api.load_library().mi355x_finalize()
    g = pw.build_index(tmp_path_factory.mktemp("xa_stage"))
    g["engine"] = api.Engine(g["prefix"], device=0)
    g["ref"] = po.RefIndex(g["prefix"])
    assert g["engine"].PW_DECIDED_XA == XA and g["engine"].lib.mi355x_pair_wave_xa_cap() == 8
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


def _records(eng, opt, pairs, taken, desc, req, xa_req):
    """the records of the taken pairs through aln_kernel + sam_emit_kernel, the requests laid out [read 0's, its XA entries', read 1's,
    its XA entries'] -> {pair: [record, record]}"""
    reads, quals, names, q, base, n_q = [], [], [], [], [0], 0
    d = np.zeros(2 * len(taken), dtype=eng.DESC_DT)
    for j, k in enumerate(taken):
        for e in range(2):
            reads.append(pairs[k].reads[e]); quals.append(pw.quality(len(pairs[k].reads[e]), k)); names.append(pairs[k].name)
            d[2 * j + e] = desc[2 * k + e]
            mine = np.concatenate([req[2 * k + e:2 * k + e + 1], xa_req[2 * k + e]])
            assert int(d[2 * j + e]["req"]) == n_q - base[-1] and (mine["read"] == 2 * k + e).all(), (k, e, d[2 * j + e], mine)
            mine["read"] = 2 * j + e
            q.append(mine)
            n_q += len(mine)
        base.append(n_q)
    res = eng.sam_records(opt, reads, quals, names, d, np.concatenate(q), np.array(base, dtype=np.int32))
    assert (res["guard"] == eng.SAM_GUARD_BYTE).all()
    out = {}
    for j, k in enumerate(taken):
        if res["out_len"][2 * j] < 0 or res["out_len"][2 * j + 1] < 0:   # (a declined CIGAR: the pipeline hands the pair to the host)
            assert res["out_len"][2 * j] == -1 and res["out_len"][2 * j + 1] == -1, (k, res["out_len"][2 * j:2 * j + 2])
            continue
        out[k] = [res["arena"][int(res["out_off"][2 * j + e]):int(res["out_off"][2 * j + e]) + int(res["out_len"][2 * j + e])].tobytes() for e in range(2)]
    return out


def _check(stage, kw, reads, tag):
    """-> (XA-only pairs by the reference, taken among them, taken with a tag)"""
    eng = stage["engine"]
    opt, ropt, flag = _opts(stage, kw)
    pairs, pes = pw.reference_side(stage["ref"], ropt, reads)
    status, desc, req, xa_req, n_align = eng.pairs_wave_xa(opt, pes, [r for P in pairs for r in P.reads], _device_regs(pairs))
    hist = np.bincount(status, minlength=17)
    taken = [k for k in range(len(pairs)) if status[k] == XA]
    plain = [k for k in range(len(pairs)) if status[k] == 1]
    xa_only = [k for k, P in enumerate(pairs) if xc.xa_only(P)]
    if any(flag & getattr(abi, f) for f in PATH_OFF):
        print(tag, "path off: taken", len(taken), len(plain))
        assert not taken and not plain, (tag, len(taken), len(plain))
        return 0, 0, 0
    for k in plain:
        assert pairs[k].plain, (tag, k, "status 1 on a pair the reference reports with XA / SA / extra lines", pairs[k].text)
    o = opt.contents
    if min(o.max_XA_hits, o.max_XA_hits_alt) > eng.lib.mi355x_pair_wave_xa_cap():
        print(tag, "max_XA_hits beyond the cap: taken", len(taken), "status histogram", {c: int(v) for c, v in enumerate(hist) if v})
        assert not taken and hist[11] > 0, (tag, len(taken), hist)
        return 0, 0, 0
    rec = _records(eng, opt, pairs, taken, desc, req, xa_req) if taken else {}
    print(tag, "pairs handed back by the CIGAR / SAM kernels:", len(taken) - len(rec), "of", len(taken))
    assert len(rec) * 20 >= len(taken) * 19, (tag, len(taken), len(rec))   # (at most 5 %)
    for k in taken:
        P = pairs[k]
        assert xc.xa_lines(P), (tag, k, "PW_DECIDED_XA on a pair the reference does not report with one line per read and an XA tag", P.text)
        assert max(P.n_before) <= 64 and max(len(P.after[0]), len(P.after[1])) <= 64, (tag, k, P.n_before)
        for e in range(2):
            if k in rec:
                assert rec[k][e] == P.text[e], (tag, k, e, P.n_before, P.n_rescue, rec[k][e], P.text[e])
            f = P.text[e].split(b"\t")
            d, q = desc[2 * k + e], req[2 * k + e]
            A = P.after[e]
            m = A[(A["rb"] == d["rb"]) & (A["re"] == d["re"]) & (A["qb"] == d["qb"]) & (A["qe"] == d["qe"])]
            assert len(m) == 1, (tag, k, e, "the chosen hit is not one of the reference's", d)
            m = m[0]
            n_entries = xc.xa_tag(P.text[e]).count(b";")
            assert len(xa_req[2 * k + e]) == n_entries and int(d["flag"]) >> 16 == n_entries, (tag, k, e, len(xa_req[2 * k + e]), d, P.text[e])
            assert int(d["flag"]) & 0xffff == int(f[1]) & ~0x30 and int(d["mapq"]) == int(f[4]), (tag, k, e, d, f[:5])
            assert int(d["req"]) == (0 if e == 0 else 1 + len(xa_req[2 * k])), (tag, k, e, d)
            assert (int(q["rb"]), int(q["re"]), int(q["qb"]), int(q["qe"]), int(q["truesc"])) == (int(m["rb"]), int(m["re"]), int(m["qb"]), int(m["qe"]), int(m["truesc"]))
            for x in xa_req[2 * k + e]:
                h = A[(A["rb"] == x["rb"]) & (A["re"] == x["re"]) & (A["qb"] == x["qb"]) & (A["qe"] == x["qe"]) & (A["truesc"] == x["truesc"])]
                assert len(h) >= 1 and int(h[0]["rid"]) == int(x["pad"]), (tag, k, e, "an XA request that is no region of the reference's", x)
                assert int(x["w2"]) == reg2aln_band(o, int(x["qe"] - x["qb"]), int(x["re"] - x["rb"]), int(x["truesc"]), int(h[0]["w"])), (tag, k, e, x)
    got = sum(1 for k in xa_only if status[k] == XA)
    print(tag, "pairs", len(pairs), "alignments", n_align, "XA-only", len(xa_only), "taken of them", got, "share %.3f" % (got / max(1, len(xa_only))),
          "taken", len(taken), "status histogram", {c: int(v) for c, v in enumerate(hist) if v})
    return len(xa_only), got, len(taken)


@pytest.mark.parametrize("case", range(len(OPTION_SETS)))
def test_xa_stage_matches_mem_sam_pe(stage, case):
    from mpibwa_amd import simulate
    from test_sampost import _pairs_of_every_kind
    kw = OPTION_SETS[case]
    damaged = pw.make_reads(stage["seqs"], stage["copies"], True)
    clean = pw.make_reads(stage["seqs"], stage["copies"], False)
    every = _pairs_of_every_kind(stage, n=360, seed=40 + case)
    reads = damaged + every + (clean if case == 0 else [])
    n_xo, n_got, n_taken = _check(stage, kw, simulate.reads_to_ascii(reads), "case %d %s" % (case, kw))
    if any(f in kw.get("flag_add", "") for f in PATH_OFF) or kw.get("max_XA_hits", 0) > 8:
        return
    assert n_xo >= 100, n_xo
    assert n_got * 2 >= n_xo, ("the kernel takes less than half of the XA-only pairs", n_xo, n_got)


def test_xa_stage_small_launches(stage):
    """launches of 1, 63, 64 and 65 pairs give what the big launch gives for the same pairs (same ids: the first pairs of the list)"""
    from mpibwa_amd import simulate
    eng = stage["engine"]
    opt, ropt, _ = _opts(stage, {})
    reads = simulate.reads_to_ascii(pw.make_reads(stage["seqs"], stage["copies"], True)[-200:])   # (the pairs at the planted copies)
    pairs, pes = pw.reference_side(stage["ref"], ropt, reads)
    regs = _device_regs(pairs)
    flat = [r for P in pairs for r in P.reads]
    status, desc, req, xa_req, _ = eng.pairs_wave_xa(opt, pes, flat, regs)
    assert (status[:63] == XA).sum() >= 5, np.bincount(status[:65])
    for n in (1, 63, 64, 65):
        s, d, q, x, _ = eng.pairs_wave_xa(opt, pes, flat[:2 * n], regs[:2 * n])
        assert (s == status[:n]).all(), (n, s, status[:n])
        for k in np.flatnonzero((s == 1) | (s == XA)):
            assert d[2 * k:2 * k + 2].tobytes() == desc[2 * k:2 * k + 2].tobytes() and q[2 * k:2 * k + 2].tobytes() == req[2 * k:2 * k + 2].tobytes(), (n, k)
            for r in (2 * k, 2 * k + 1):
                assert x[r].tobytes() == xa_req[r].tobytes(), (n, k, r)


@pytest.mark.parametrize("k_xa", [0, 1, 5, 6])
def test_xa_stage_on_synthetic_lists(stage, k_xa):
    """Full-length hits, the best with score 150 and a mate at a proper distance, k secondaries at the threshold and four just under
    it, through the reference's mem_sam_pe with recorders (oracle/pair_inject.c): PW_DECIDED_XA with k requests for k = 1 and 5; plain
    status 1 for k = 0 and for k = 6 (more than max_XA_hits: no tag at all).
    The threshold: XA_drop_ratio is a float, and the reference compares score >= 150 * (double)0.8f = 120.0000018 (src/bwamem_extra.c:93),
    so 121 is the smallest score that qualifies and exactly 120 = 0.8 x 150 does not — the reference's own count (want["n_xa"]) says so,
    and a kernel that compared in float or against 0.8 would list the hits of 120.  The k hits are of 121; two of 120 and two of 119
    lie under them."""
    from test_pair_stage import PES_SETS, _pes
    assert po.pair_inject_available(), "oracle/_ref/libpairinj.so is missing"
    eng, ref = stage["engine"], stage["ref"]
    opt, ropt, _ = _opts(stage, {})
    assert abs(opt.contents.XA_drop_ratio - 0.8) < 1e-6 and opt.contents.max_XA_hits == 5
    l_pac = int(eng.bns.contents.l_pac)
    offs = [int(eng.bns.contents.anns[k].offset) for k in range(int(eng.bns.contents.n_seqs))] + [l_pac]
    pes = _pes(PES_SETS[0][0])
    low, high = PES_SETS[0][0][1][:2]
    rng = np.random.default_rng(900 + k_xa)
    n_pairs, id0 = 12, 4242
    lists = []
    for p in range(n_pairs):
        def spot():
            c = int(rng.integers(0, len(offs) - 1))
            return c, int(rng.integers(offs[c] + 1500, offs[c + 1] - 1500))
        c, pos = spot()
        d = int(rng.integers(low + 10, high - 10))
        fp = pos + d - 149
        fwd_rb, rev_rb = pos, 2 * l_pac - (fp + 150)
        r0, r1 = (fwd_rb, rev_rb) if p % 2 == 0 else (rev_rb, fwd_rb)
        end0 = [(r0, c, 150)]
        for sc_ in [121] * k_xa + [120] * 2 + [119] * 2:
            c2, p2 = spot()
            end0.append((p2 if rng.random() < 0.5 else 2 * l_pac - (p2 + 150), c2, sc_))
        arr = []
        for hits in (end0, [(r1, c, 150)]):
            a = np.zeros(len(hits), dtype=po.ALNREG_DT)
            for i, (rb, rid, s) in enumerate(hits):
                a[i]["rb"], a[i]["re"], a[i]["qb"], a[i]["qe"], a[i]["rid"], a[i]["score"], a[i]["truesc"] = rb, rb + 150, 0, 150, rid, s, s
                a[i]["w"], a[i]["seedcov"], a[i]["seedlen0"], a[i]["secondary"] = 100, s // 2, 19, -1
            arr.append(a)
        lists.append(arr)
    wants = [po.ref_pair(ropt, ref.bns, ref.pac, pes, id0 + p, 150, arr[0], arr[1]) for p, arr in enumerate(lists)]
    reads = [rng.integers(0, 4, 150).astype(np.uint8) for _ in range(2 * n_pairs)]
    regs = []
    for p, arr in enumerate(lists):
        for e in range(2):
            mine = arr[e].copy()
            m = eng.lib.mi355x_host_sort_dedup_patch(opt, eng.bns, C.cast(eng.pac, C.c_void_p), reads[2 * p + e].ctypes.data, mine.ctypes.data, len(mine))
            assert m == len(arr[e])
            a = np.zeros(m, dtype=eng.REG_DT)
            for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep"):
                a[f] = mine[:m][f]
            regs.append(a)
    status, desc, req, xa_req, n_align = eng.pairs_wave_xa(opt, pes, reads, regs, n_processed=2 * id0)
    want_n = k_xa if 1 <= k_xa <= 5 else 0
    print("synthetic lists, k =", k_xa, "status", status, "n_xa", [w["n_xa"] for w in wants])
    for p, want in enumerate(wants):
        # (the recorder's n_xa: the hits of an end whose XA string is not empty)
        assert want["paired"] and want["n_align"] == 0 and want["n_lines"] == 2 and want["n_xa"] == (1 if want_n else 0, 0), (p, want)
        assert status[p] == (XA if want_n else 1), (p, status[p], want)
        assert (len(xa_req[2 * p]), len(xa_req[2 * p + 1])) == (want_n, 0), (p, xa_req[2 * p], want)
        assert int(desc[2 * p]["flag"]) >> 16 == want_n and int(desc[2 * p + 1]["flag"]) >> 16 == 0 and int(desc[2 * p + 1]["req"]) == 1 + want_n
        for x in xa_req[2 * p]:
            assert int(x["truesc"]) == 121 and int(x["read"]) == 2 * p and int(x["w2"]) == reg2aln_band(opt.contents, 150, 150, 121, 100), (p, x)
        for e in range(2):
            d, L = desc[2 * p + e], want["lines"][e]
            got = dict(rb=int(d["rb"]), re=int(d["re"]), qb=int(d["qb"]), qe=int(d["qe"]), score=int(d["score"]), sub=int(d["sub"]), flag=int(d["flag"]) & 0xffff,
                       mapq=int(d["mapq"]))
            assert got == {f: L[f] for f in got}, (p, e, got, L)


# ---- hand-made XA descriptors through Engine.sam_records against the reference's mem_gen_alt ----
class _alnreg_v(C.Structure):   # mem_alnreg_v (src/bwamem.h:79)
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.c_void_p)]


def _variant(ix, opt, reg, rev, length, dl=0, dr=0, lead=0, trail=0, loss=10):
    """another region of the same read at the same place: dl / dr more bases clipped in front / behind as the forward strand sees the
    read, a window `lead` / `trail` bases longer at its front / back (the alignment then starts / ends with a deletion)"""
    if not rev:
        fs, fe, cl, cr = reg["rb"], reg["re"], reg["qb"], length - reg["qe"]
    else:
        fs, fe, cr, cl = 2 * ix.l_pac - reg["re"], 2 * ix.l_pac - reg["rb"], reg["qb"], length - reg["qe"]
    cl, cr, fs, fe = cl + dl, cr + dr, fs + dl - lead, fe - dr + trail
    n_q = length - cl - cr
    if not rev:
        rb, re, qb, qe = fs, fe, cl, cl + n_q
    else:
        rb, re, qb, qe = 2 * ix.l_pac - fe, 2 * ix.l_pac - fs, cr, cr + n_q
    truesc = min(n_q, fe - fs) * opt.a - loss
    return dict(rb=rb, re=re, qb=qb, qe=qe, rid=reg["rid"], truesc=truesc, score=truesc, sub=0, w=100)


def _elsewhere(ix, opt, reg, c, p):
    """a region of the same query span on contig c from p on, forward strand, band 0: the read does not come from there"""
    n_q = reg["qe"] - reg["qb"]
    return dict(rb=ix.off[c] + p, re=ix.off[c] + p + n_q, qb=reg["qb"], qe=reg["qe"], rid=c, truesc=n_q * opt.a - 4, score=n_q * opt.a - 4, sub=0, w=100)


def _gen_alt(ref, ropt, read, primary, hits):
    """the reference's XA string of `primary` with `hits` under it (mem_gen_alt, src/bwamem_extra.c:98-140)"""
    lib = ref.lib
    lib.mem_gen_alt.restype = C.POINTER(C.c_void_p)
    lib.mem_gen_alt.argtypes = [C.POINTER(abi.mem_opt_t), C.POINTER(abi.bntseq_t), C.POINTER(C.c_uint8), C.POINTER(_alnreg_v), C.c_int, C.c_void_p]
    a = np.zeros(1 + len(hits), dtype=po.ALNREG_DT)
    for i, r in enumerate([primary] + hits):
        for f in ("rb", "re", "qb", "qe", "rid", "truesc", "w"):
            a[i][f] = r[f]
        a[i]["score"] = 100
        a[i]["secondary"] = a[i]["secondary_all"] = -1 if i == 0 else 0
    v = _alnreg_v(len(a), len(a), a.ctypes.data)
    sq = np.ascontiguousarray(read, dtype=np.uint8)
    out = lib.mem_gen_alt(ropt, ref.bns, ref.pac, C.byref(v), len(sq), sq.ctypes.data)
    assert out and out[0]
    s = C.string_at(out[0])
    for i in range(len(a)):
        if out[i]:
            po.libc.free(C.c_void_p(out[i]))
    po.libc.free(C.cast(out, C.c_void_p))
    return s


def test_xa_text_on_hand_made_descriptors(tmp_path_factory, built):
    from mpibwa_amd import api
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    prefix = sc.build_named_index(tmp_path_factory.mktemp("xa_named"))
    eng, ref = api.Engine(prefix, upload=False), po.RefIndex(prefix)
    opt, ropt = eng.opt(), ref.opt()
    o = opt.contents
    ix = sc.Index(prefix, ref.bns)
    longest = max(range(ix.n_seqs), key=lambda c: len(ix.names[c]))
    assert len(ix.names[longest]) == 120
    rng = np.random.default_rng(77)

    def end(rev, length=150, n_mm=2, **kw):
        c = int(rng.integers(ix.n_seqs))
        read, reg = sc.plant(ix, rng, o, c, int(rng.integers(600, ix.len[c] - 1200)), length, rev, n_mm=n_mm, **kw)
        return dict(read=read, reg=reg, rev=rev, len=length, xa=[])

    cases = {}
    # an XA hit on the reverse strand / with a leading deletion / a trailing deletion / clips on both sides, on either strand
    for rev in (0, 1):
        a, b = end(rev), end(1 - rev)
        a["xa"] = [_variant(ix, o, a["reg"], rev, 150)]
        cases["strand%d" % rev] = [a, b]
        a, b = end(rev), end(1 - rev)
        a["xa"] = [_variant(ix, o, a["reg"], rev, 150, lead=g) for g in (1, 9)]
        cases["lead_del%d" % rev] = [a, b]
        a, b = end(rev), end(1 - rev)
        b["xa"] = [_variant(ix, o, b["reg"], 1 - rev, 150, trail=g) for g in (2, 9)]
        cases["trail_del%d" % rev] = [a, b]
        a, b = end(rev), end(1 - rev)
        a["xa"] = [_variant(ix, o, a["reg"], rev, 150, dl=7, dr=31), _variant(ix, o, a["reg"], rev, 150, dl=12), _variant(ix, o, a["reg"], rev, 150, dr=5)]
        cases["clips%d" % rev] = [a, b]
    # another contig, under the longest contig name (the read does not come from there: NM of three digits)
    a, b = end(0), end(1)
    a["xa"] = [_elsewhere(ix, o, a["reg"], longest, 5000), _elsewhere(ix, o, a["reg"], (longest + 1) % ix.n_seqs, 7000)]
    cases["other_contig"] = [a, b]
    # NM of two digits
    a, b = end(0, n_mm=14, loss=14), end(1)
    a["xa"] = [_variant(ix, o, a["reg"], 0, 150, loss=14)]
    cases["nm2"] = [a, b]
    # five entries on both reads; the longest tags: five entries under the longest contig name
    a, b = end(0), end(1)
    a["xa"] = [_variant(ix, o, a["reg"], 0, 150, dl=j, lead=j % 3) for j in range(5)]
    b["xa"] = [_elsewhere(ix, o, b["reg"], longest, 3000 + 211 * j) for j in range(5)]
    cases["five_both"] = [a, b]
    # only read 1 has a tag
    a, b = end(1), end(0)
    b["xa"] = [_variant(ix, o, b["reg"], 0, 150, dr=3)]
    cases["read1_only"] = [a, b]
    # an XA request whose CIGAR the device declines (the `declined` family of tests/sam_stage_cases.py): both records come back
    c = int(rng.integers(ix.n_seqs))
    p0 = int(rng.integers(600, ix.len[c] - 1500))
    read, full = sc.plant(ix, rng, o, c, p0, 251, 0, big_del=10, loss=120, score=100)
    half = dict(full, re=full["rb"] + 125, qe=125, truesc=125 * o.a - 10, score=100)
    a, b = dict(read=read, reg=half, rev=0, len=251, xa=[full]), end(1)
    cases["declined"] = [a, b]
    # plain pairs around them, so that waves mix lines with and without tags
    for j in range(40):
        cases["plain%d" % j] = [end(j & 1), end(1 - (j & 1))]

    names = list(cases)
    order = [names[i] for i in rng.permutation(len(names))]
    reads, quals, qn, reqs, base = [], [], [], [], [0]
    desc = np.zeros(2 * len(order), dtype=eng.DESC_DT)
    plain_regs = np.zeros(2 * len(order), dtype=po.ALNREG_DT)
    for k, nm in enumerate(order):
        for e, E in enumerate(cases[nm]):
            r = E["reg"]
            reads.append(E["read"]); quals.append(pw.quality(E["len"], k)); qn.append(("q%03d_%s" % (k, nm)).encode())
            d = desc[2 * k + e]
            for f in ("rb", "re", "qb", "qe", "rid", "score", "sub"):
                d[f] = r[f]
            d["req"] = len(reqs) - base[-1]
            d["flag"] = (0x40 << e) | 0x3 | (len(E["xa"]) << 16)
            d["mapq"] = (0, 7, 60)[k % 3]
            for j, x in enumerate([r] + E["xa"]):
                w2 = reg2aln_band(o, x["qe"] - x["qb"], x["re"] - x["rb"], x["truesc"], x["w"])
                reqs.append((x["rb"], x["re"], 2 * k + e, x["qb"], x["qe"], w2, x["truesc"], x["rid"] if j else 0))
            g = plain_regs[2 * k + e]
            for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w"):
                g[f] = r[f]
            g["sub"] = g["csub"] = r["sub"]
            g["secondary"] = g["secondary_all"] = -1
        base.append(len(reqs))
    text = ref.pair_records(ropt, reads, quals, qn, plain_regs, [0x3] * len(reads), [(0, 7, 60)[(i // 2) % 3] for i in range(len(reads))])
    res = eng.sam_records(opt, reads, quals, qn, desc, np.array(reqs, dtype=eng.AREQ_DT), np.array(base, dtype=np.int32))
    assert (res["guard"] == eng.SAM_GUARD_BYTE).all(), "bytes behind the arena were written"
    longest_tag = 0
    for k, nm in enumerate(order):
        l0, l1 = int(res["out_len"][2 * k]), int(res["out_len"][2 * k + 1])
        if nm == "declined":
            assert int(res["hdr"]["flags"][base[k] + 1]) != 0 and int(res["hdr"]["flags"][base[k]]) == 0, (nm, res["hdr"][base[k]:base[k + 1]])
            assert (l0, l1) == (-1, -1), (nm, l0, l1)
            continue
        assert l0 > 0 and l1 > 0, (nm, l0, l1, res["hdr"][base[k]:base[k + 1]])
        for e, E in enumerate(cases[nm]):
            want = text[2 * k + e]
            if E["xa"]:   # mem_aln2sam puts the tag behind RG / SA / pa, in front of the newline (src/bwamem.c:940)
                tag = _gen_alt(ref, ropt, E["read"], E["reg"], E["xa"])
                assert tag.count(b";") == len(E["xa"])
                longest_tag = max(longest_tag, len(tag))
                want = want[:-1] + b"\tXA:Z:" + tag + b"\n"
            at = int(res["out_off"][2 * k + e])
            got = res["arena"][at:at + int(res["out_len"][2 * k + e])].tobytes()
            assert got == want, (nm, e, got, want)
    # what the cases were built for, by the reference's text
    tag_of = lambda nm, e: _gen_alt(ref, ropt, cases[nm][e]["read"], cases[nm][e]["reg"], cases[nm][e]["xa"])
    assert b",-" in tag_of("strand1", 0) and b",+" in tag_of("strand0", 0)
    for rev in (0, 1):
        lead, trail, clips = tag_of("lead_del%d" % rev, 0), tag_of("trail_del%d" % rev, 1), tag_of("clips%d" % rev, 0)
        # the window of the second entry is nine bases longer at the front / at the back: the deletion there is squeezed out, and a
        # leading one moves the position to where the primary line has it
        k = order.index("lead_del%d" % rev)
        assert abs(int(lead.split(b";")[1].split(b",")[1])) == int(text[2 * k].split(b"\t")[3]), (lead, text[2 * k])
        assert b"D" not in lead.split(b";")[1].split(b",")[2] and b"D" not in trail.split(b";")[1].split(b",")[2], (lead, trail)
        assert clips.split(b";")[0].split(b",")[2].count(b"S") == 2 and b"H" not in clips, clips
    assert ix.names[longest] in tag_of("other_contig", 0) and len(tag_of("nm2", 0).split(b";")[0].split(b",")[3]) == 2
    assert longest_tag > 5 * 120
    print("hand-made XA descriptors: pairs", len(order), "longest tag", longest_tag)
