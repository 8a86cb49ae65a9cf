"""Stage test of pair_wave_kernel's no_pairing tail (mpibwa_amd/csrc/pair_wave_kernel.hip, status 17) through
mi355x_pair_wave_lines_batch, and of the paired instantiation of sam_lines_kernel (mpibwa_amd/csrc/sam_lines_kernel.hip) behind aln_kernel
through mi355x_sam_pe_lines_batch, against the reference's OWN mem_align1_core, mem_pestat, mem_sort_dedup_patch and mem_sam_pe
(oracle/_ref/libbwaref.so) on the cases of tests/pair_lines_cases.py — tests/test_pair_lines_cases.py shows on the CPU that the sets hold
the pairs the path is for and that every hand-built family reaches its branch.  Without the reference's library the tests fail.

Per option set (pair_lines_cases.OPTION_SETS: default, -Y, -M, -q, no qualities, a read group, XA_drop_ratio 0.5, max_XA_hits 9, a=2 b=5,
MEM_F_NO_RESCUE) and under n_processed = 4 000 and 2^32 + 5, sets (a) + (b) as one chunk and set (c) under that chunk's statistics:
  * every pair decided with 17 is ELIGIBLE by the reference alone, and a pair decided with 1 / 16 has one line per read, both mapped
    (the paired branch may leave 0x2 off when the unpaired alignments are preferred: such a pair is ELIGIBLE and rightly gets 1);
  * decision: the line counts, and per line the region, the flag without the writer's bits, MAPQ, AS, XS, the XA count in bits 16-19,
    the request's place counted from the pair's first, the request (band: tests/ref_band.py) and the XA requests in list order say what
    the reference's text and lists say;
  * text: the writer runs twice — on the kernel's descriptors and on descriptors built from the reference's lists and text, so that a
    wrong decision cannot hide a wrong writer — and both strings of every pair equal the reference's byte for byte, the records back to
    back in [0, cursor), guard bytes intact; a pair comes back (both out_len = -1) exactly when the reference's text says why (a line's
    short fields beyond LINES_ROW, what the SA tags say of a line beyond SA_STAGE, an XA entry beyond XA_STAGE) or aln_kernel declined
    one of its requests by its header;
  * at least half of the ELIGIBLE pairs get 17 (the rule of tests/test_gpu_pair_wave_stage.py: what the kernel leaves with 12 or 14 is
    not the reference's to predict; the status histogram is printed); under the default set at most 2 % of the decided pairs come back
    from the CIGAR / SAM job; every family of (c) gives its expected code;
  * through the existing entries, without the side arrays, no pair gets 17: a pair the tail decides has 8 / 9 / 10 (0 when it has no
    region at all), every other status is the same, and a pair decided with 1 or 16 has the same descriptor and request bytes.
No pair is taken with 17 under -a / -5 / -P.  Launches of 1, 63, 64 and 65 pairs give what the big launch gives."""
import numpy as np
import pytest

import pair_lines_cases as plc
import se_wave_cases as swc
import supp_cases as spc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

N_PROCESSED = 4000
N_PROCESSED_BIG = (1 << 32) + 5


@pytest.fixture(scope="module")
def stage(tmp_path_factory, built):
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing: the stage test needs the reference"
    import pair_wave_cases as pw
    from mpibwa_amd import api, simulate
    lib = api.load_library()
    lib.mi355x_finalize()
    assert lib.mi355x_se_lines_cap() == plc.SE_LINES_CAP and lib.mi355x_pair_wave_xa_cap() == plc.PW_XA_CAP and api.Engine.PW_DECIDED_LINES == plc.PW_DECIDED_LINES
    assert lib.mi355x_sam_lines_row() == spc.LINES_ROW and lib.mi355x_sam_lines_sa_stage() == spc.SA_STAGE
    g = pw.build_index(tmp_path_factory.mktemp("pair_lines_stage"))
    g["lib"] = lib
    g["eng"] = api.Engine(g["prefix"], device=0)
    g["ref"] = po.RefIndex(g["prefix"])
    g["ix"] = spc.Index(g["prefix"], g["ref"].bns)
    b, _ = plc.set_b(g)
    g["reads"] = simulate.reads_to_ascii(plc.set_a(g) + b)
    return g


class Side:
    """both libraries under one option set; the read group is taken back on the way out.  chunk(): sets (a) + (b); families(): set (c)"""

    def __init__(self, stage, name):
        self.st, self.name = stage, name
        self.lib, self.eng, self.ref, self.ix = stage["lib"], stage["eng"], stage["ref"], stage["ix"]
        self.kw = plc.option_fields(name)
        _, self.with_qual, self.rg = plc.OPTION_SETS.get(name, ({}, True, None))

    def __enter__(self):
        self.opt, self.ropt = self.eng.opt(**self.kw), self.ref.opt(**self.kw)
        if "a" in self.kw:
            for lib, o in ((self.lib, self.opt), (self.ref.lib, self.ropt)):
                lib.bwa_fill_scmat(o.contents.a, o.contents.b, o.contents.mat)
        self.rgid = self.ref.set_rg(self.rg)
        assert po.set_rg(self.lib, self.rg) == self.rgid
        self.o = self.ropt.contents
        self.listing = spc.n_xa_max(self.o) <= plc.PW_XA_CAP
        reads = self.st["reads"]
        self.names = [r[0] for r in reads]
        self.codes, self.lists, self.pes = plc.phase1(self.ref, self.ropt, reads)
        return self

    def __exit__(self, *exc):
        self.ref.set_rg(None)
        po.set_rg(self.lib, None)

    def chunk(self, n_processed, first=None):
        n = len(self.names) if first is None else first
        return plc.reference_pairs(self.ref, self.ropt, self.names[:n], self.codes[:2 * n], self.lists[:2 * n], self.pes, n_processed, self.with_qual)

    def families(self, n_processed):
        cases = plc.build_cases(self.ix, self.o, self.pes)
        codes, lists = plc.lists_of_cases(self.ref, self.ropt, cases)
        return cases, plc.reference_pairs(self.ref, self.ropt, [cs["name"] for cs in cases], codes, lists, self.pes, n_processed, self.with_qual)

    def decide(self, pairs, n_processed, **kw):
        return self.eng.pairs_wave_lines(self.opt, self.pes, [r for P in pairs for r in P.reads], plc.device_regs(pairs, self.eng.REG_DT), n_processed=n_processed, **kw)


def _req_tuple(q):
    return tuple(int(q[f]) for f in ("rb", "re", "read", "qb", "qe", "w2", "truesc", "pad"))


def check_decisions(side, pairs, status, n_lines, lines, tag):
    """-> the pairs decided with 17"""
    o = side.o
    taken = []
    for k, P in enumerate(pairs):
        st = int(status[k])
        if st in (plc.PW_DECIDED, plc.PW_DECIDED_XA):
            # (the paired branch: one line per read; it may leave 0x2 off, :319-323, so "eligible" does not say "the tail's")
            assert all(len(x) == 1 for x in P.lines) and not any(plc.unmapped(P)), (tag, k, st, P.text)
        if st != plc.PW_DECIDED_LINES:
            assert n_lines[2 * k] == 0 and n_lines[2 * k + 1] == 0 and lines[2 * k] == [] and lines[2 * k + 1] == [], (tag, k, st)
            continue
        assert plc.eligible(P), (tag, k, "the kernel decided a pair that is not eligible", P.n_before, P.text)
        assert side.listing or not plc.has_xa(P), (tag, k, "a tag without the listing", P.text)
        taken.append(k)
        assert [int(n_lines[2 * k]), int(n_lines[2 * k + 1])] == plc.n_lines(P), (tag, k, n_lines[2 * k:2 * k + 2], P.text)
        at = 0
        for e in range(2):
            ref_lines = plc.reference_lines(o, side.ix, P, e)
            assert len(lines[2 * k + e]) == len(ref_lines), (tag, k, e, len(lines[2 * k + e]), P.text)
            for j, ((d, q, xr), R) in enumerate(zip(lines[2 * k + e], ref_lines)):
                r = R["region"]
                assert all(int(d[f]) == int(r[f]) for f in ("rb", "re", "qb", "qe", "rid")), (tag, k, e, j, d, r)
                assert (int(d["flag"]) & 0xffff, int(d["flag"]) >> 16, int(d["mapq"]), int(d["score"]), int(d["sub"]), int(d["req"])) == \
                       (R["flag"], R["n_xa"], R["mapq"], R["score"], R["sub"], at), (tag, k, e, j, d, R, P.text)
                assert _req_tuple(q) == spc.request_of(o, r, 2 * k + e), (tag, k, e, j, q, r)
                assert len(xr) == len(R["xa"]) == R["n_xa"], (tag, k, e, j, len(xr), R["n_xa"])
                for x, h in zip(xr, R["xa"]):
                    assert _req_tuple(x) == spc.request_of(o, h, 2 * k + e, pad=int(h["rid"])), (tag, k, e, j, x, h)
                at += 1 + len(xr)
    return taken


def reference_descriptors(side, pairs, eng):
    """per eligible pair (without a tag when the listing is off): per read the lines [(desc, req, xa_req)] as the reference's lists and text give them"""
    o = side.o
    out = {}
    for k, P in enumerate(pairs):
        if not plc.eligible(P) or (plc.has_xa(P) and not side.listing):
            continue
        at, mine = 0, [[], []]
        for e in range(2):
            for R in plc.reference_lines(o, side.ix, P, e):
                r = R["region"]
                d = np.zeros((), dtype=eng.DESC_DT)
                for f in ("rb", "re", "qb", "qe", "rid"):
                    d[f] = r[f]
                d["req"], d["flag"], d["mapq"], d["score"], d["sub"] = at, R["flag"] | R["n_xa"] << 16, R["mapq"], R["score"], R["sub"]
                q = np.array([spc.request_of(o, r, 2 * k + e)], dtype=eng.AREQ_DT)[0]
                xr = np.array([spc.request_of(o, h, 2 * k + e, pad=int(h["rid"])) for h in R["xa"]], dtype=eng.AREQ_DT)
                mine[e].append((d, q, xr))
                at += 1 + len(xr)
        out[k] = mine
    return out


def row_bytes(line, with_qual, rg):
    """the bytes of a line the paired instantiation of sam_lines_kernel stages in its row: everything but QNAME, the contig names, SEQ,
    QUAL, the values of MD and RG, and the SA and XA tags"""
    f = line.split(b"\t")
    tags = {t[:2]: t[5:] for t in f[11:]}
    n = 1 + len(f[1]) + 1
    if f[2] == b"*":
        n += len(b"*\t0\t0\t*\t*\t0\t0\t")
    else:
        n += 1 + len(f[3]) + 1 + len(f[4]) + 1 + len(f[5]) + 1 + (1 if f[6] == b"=" else 0) + 1 + len(f[7]) + 1 + len(f[8]) + 1
    n += 0 if with_qual else 1
    for t in (b"NM", b"MC", b"AS", b"XS"):
        if t in tags:
            n += 6 + len(tags[t])
    n += (6 if b"MD" in tags else 0) + (6 if rg else 0)
    return n


def check_records(side, pairs, by_pair, tag):
    """the pairs of by_pair {pair: [lines of read 0, lines of read 1]} through aln_kernel + sam_lines_kernel<true> -> per pair 'dev' or 'back'"""
    if not by_pair:
        return {}
    eng = side.eng
    taken = sorted(by_pair)
    cap = plc.SE_LINES_CAP
    reads, names, quals, q, base = [], [], [], [np.zeros(0, dtype=eng.AREQ_DT)], [0]
    d = np.zeros((2 * len(taken), cap), dtype=eng.DESC_DT)
    d["req"] = -1
    n_lines = np.zeros(2 * len(taken), dtype=np.uint8)
    for j, k in enumerate(taken):
        P = pairs[k]
        n_req = 0
        for e in range(2):
            reads.append(P.reads[e]); names.append(P.name); quals.append(plc.pw.quality(len(P.reads[e]), k))
            n_lines[2 * j + e] = len(by_pair[k][e])
            for l, (dl, ql, xr) in enumerate(by_pair[k][e]):
                d[2 * j + e, l] = dl
                mine = np.concatenate([np.array([ql], dtype=eng.AREQ_DT), np.asarray(xr, dtype=eng.AREQ_DT)])
                assert (mine["read"] == 2 * k + e).all(), (tag, k, e, mine)
                mine["read"] = 2 * j + e
                q.append(mine)
                n_req += len(mine)
        base.append(base[-1] + n_req)
    res = eng.sam_records_pe_lines(side.opt, reads, quals if side.with_qual else None, names, n_lines, d, np.concatenate(q), np.array(base, dtype=np.int32))
    assert (res["guard"] == eng.SAM_GUARD_BYTE).all(), (tag, "bytes behind the arena were written")
    state, spans = {}, []
    for j, k in enumerate(taken):
        P = pairs[k]
        ln = [int(res["out_len"][2 * j + e]) for e in range(2)]
        assert min(ln) >= -1 and (ln[0] < 0) == (ln[1] < 0), (tag, k, ln)
        why = set()
        for e in range(2):
            for line in P.lines[e]:
                if row_bytes(line, side.with_qual, side.rgid) > spc.LINES_ROW:
                    why.add("row")
                if len(P.lines[e]) > 1 and spc.sa_bytes(line) > spc.SA_STAGE:
                    why.add("sa")
                if any(swc.xa_entry_bytes(x) > spc.XA_STAGE for x in swc.xa_entries(line + b"\n")):
                    why.add("xa_stage")
        if (res["hdr"]["flags"][base[j]:base[j + 1]] != 0).any():
            why.add("declined")
        state[k] = "dev" if ln[0] >= 0 else "back"
        assert (ln[0] < 0) == bool(why), (tag, k, ln, why, P.text)
        if ln[0] < 0:
            continue
        for e in range(2):
            at = int(res["out_off"][2 * j + e])
            assert at + ln[e] <= res["cursor"] <= res["arena_bytes"], (tag, k, e, at, ln[e], res["cursor"])
            got = res["arena"][at:at + ln[e]].tobytes()
            assert got == P.text[e], (tag, k, e, got, P.text[e])
            spans.append((at, ln[e]))
    spans.sort()
    for (a, la), (b, _) in zip(spans, spans[1:]):
        assert a + la <= b, (tag, "records overlap", a, la, b)
    assert sum(la for _, la in spans) == res["cursor"], (tag, "the records do not lie back to back in [0, cursor)", res["cursor"])
    assert (res["arena"][res["cursor"]:] == eng.SAM_GUARD_BYTE).all(), (tag, "bytes outside the records were written")
    return state


def run_group(side, pairs, n_processed, tag):
    status, desc, req, xa_req, n_lines, lines, n_align = side.decide(pairs, n_processed, xa=side.listing)
    taken = check_decisions(side, pairs, status, n_lines, lines, tag)
    # the existing entries, without the side arrays
    s0, d0, q0, x0, nl0, l0, _ = side.decide(pairs, n_processed, xa=side.listing, lines=False)
    assert not (s0 == plc.PW_DECIDED_LINES).any() and not nl0.any(), (tag, np.bincount(s0))
    for k, P in enumerate(pairs):
        if status[k] == plc.PW_DECIDED_LINES:
            assert s0[k] in ((0,) if max(P.n_before) == 0 else (plc.PW_HOST_NO_PAIR, plc.PW_HOST_SCORE, plc.PW_HOST_SUPP)), (tag, k, s0[k], P.n_before)
            continue
        # (the tail has exits of its own: more than four lines 10, a tag without room 11, a line beyond the tables 6, a tie met while marking 14)
        assert s0[k] == status[k] or (s0[k] in (plc.PW_HOST_NO_PAIR, plc.PW_HOST_SCORE, plc.PW_HOST_SUPP) and
                                      status[k] in (plc.PW_HOST_SUPP, plc.PW_HOST_XA, plc.PW_HOST_LENGTH, plc.PW_HOST_TIE)), (tag, k, s0[k], status[k])
        if status[k] in (plc.PW_DECIDED, plc.PW_DECIDED_XA):
            assert d0[2 * k:2 * k + 2].tobytes() == desc[2 * k:2 * k + 2].tobytes() and q0[2 * k:2 * k + 2].tobytes() == req[2 * k:2 * k + 2].tobytes(), (tag, k)
            assert all(x0[2 * k + e].tobytes() == xa_req[2 * k + e].tobytes() for e in range(2)), (tag, k)
    state = check_records(side, pairs, {k: [lines[2 * k], lines[2 * k + 1]] for k in taken}, tag + "/kernel")
    ref_state = check_records(side, pairs, reference_descriptors(side, pairs, side.eng), tag + "/reference")
    for k in taken:
        assert state[k] == ref_state[k], (tag, k, state[k], ref_state[k])
    return status, taken, state, n_align


@pytest.mark.parametrize("name", list(plc.OPTION_SETS))
def test_pair_lines_stage_matches_mem_sam_pe(stage, name):
    with Side(stage, name) as side:
        for npr in (N_PROCESSED, N_PROCESSED_BIG):
            pairs = side.chunk(npr)
            status, taken, state, n_align = run_group(side, pairs, npr, "%s/%d" % (name, npr))
            elig = [k for k, P in enumerate(pairs) if plc.eligible(P) and (side.listing or not plc.has_xa(P))]
            got = sum(status[k] == plc.PW_DECIDED_LINES for k in elig)
            back = sum(s == "back" for s in state.values())
            hist = {int(c): int((status == c).sum()) for c in np.unique(status)}
            print(name, npr, "pairs", len(pairs), "alignments", n_align, "eligible", len(elig), "decided with 17:", got, "share %.3f" % (got / max(1, len(elig))),
                  "status of the eligible", {int(c): int(sum(status[k] == c for k in elig)) for c in np.unique(status[elig])}, "status histogram", hist,
                  "handed back by the CIGAR / SAM job %d of %d, share %.4f" % (back, len(taken), back / max(1, len(taken))))
            if name == "default":   # (the floors of tests/test_pair_lines_cases.py: 250 of (a) and 240 of (b))
                assert len(elig) >= 490, len(elig)
            assert 2 * got >= len(elig), ("the kernel decides less than half of the eligible pairs", len(elig), got, hist)
            if name == "default":
                assert 50 * back <= len(taken), (back, len(taken))
            # set (c)
            cases, fam = side.families(npr)
            status, taken, state, _ = run_group(side, fam, npr, "%s/%d/families" % (name, npr))
            print(name, npr, "families", {int(c): int((status == c).sum()) for c in np.unique(status)}, "written", sum(s == "dev" for s in state.values()))
            for k, cs in enumerate(cases):
                # (a tag on a line — a rescued hit next to a planted one can be listed — while the listing is off: 11)
                want = plc.PW_HOST_XA if cs["expect"] == plc.PW_DECIDED_LINES and plc.has_xa(fam[k]) and not side.listing else cs["expect"]
                assert status[k] == want, (name, npr, cs["family"], cs["tag"], int(status[k]), fam[k].n_before, fam[k].n_rescue, fam[k].text)
                if want == plc.PW_DECIDED_LINES:
                    assert state[k] == "dev", (name, cs["family"], cs["tag"])


@pytest.mark.parametrize("name", list(plc.PATH_OFF))
def test_path_off_sets_take_no_pair(stage, name):
    with Side(stage, name) as side:
        pairs = side.chunk(N_PROCESSED, first=360)
        status, desc, req, xa_req, n_lines, lines, _ = side.decide(pairs, N_PROCESSED)
        print(name, "status", np.bincount(status))
        assert not (status == plc.PW_DECIDED_LINES).any() and not n_lines.any() and all(l == [] for l in lines)


def test_launch_sizes(stage):
    with Side(stage, "default") as side:
        pairs = side.chunk(N_PROCESSED, first=360)
        pairs = [P for P in pairs if plc.leaves_the_paired_branch(P)][:65] + pairs[:10]   # (every launch takes the first pairs of this list: the same ids)
        status, desc, req, xa_req, n_lines, lines, _ = side.decide(pairs, N_PROCESSED)
        assert (status[:65] == plc.PW_DECIDED_LINES).sum() >= 20, np.bincount(status[:65])
        for n in (1, 63, 64, 65):
            s, d, q, x, nl, ln, _ = side.decide(pairs[:n], N_PROCESSED)
            assert (s == status[:n]).all() and (nl == n_lines[:2 * n]).all(), (n, s, status[:n])
            for r in range(2 * n):
                assert len(ln[r]) == len(lines[r]), (n, r)
                for a, b in zip(ln[r], lines[r]):
                    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes(), (n, r)
        # the XA listing off: a pair with a tag on a line gets 11, the others are decided as before
        s, d, q, x, nl, ln, _ = side.decide(pairs, N_PROCESSED, xa=False)
        n_tag = 0
        for k in range(len(pairs)):
            if status[k] == plc.PW_DECIDED_LINES:
                with_tag = any(len(l[2]) for e in range(2) for l in lines[2 * k + e])
                n_tag += with_tag
                assert s[k] == (plc.PW_HOST_XA if with_tag else plc.PW_DECIDED_LINES), (k, s[k])
        print("launch sizes: pairs", len(pairs), "status", np.bincount(status), "with a tag on a line", n_tag)
