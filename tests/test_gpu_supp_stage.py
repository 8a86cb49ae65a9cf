"""Stage test of the multi-line branch of se_wave_kernel (mpibwa_amd/csrc/se_wave_kernel.hip, status 17) through
mi355x_se_wave_lines_batch, and of sam_lines_kernel (mpibwa_amd/csrc/sam_lines_kernel.hip) behind aln_kernel through
mi355x_sam_se_lines_batch, against the reference's OWN mem_align1_core / mem_sort_dedup_patch, mem_mark_primary_se (id = n_processed +
read number) and mem_reg2sam (oracle/_ref/libbwaref.so), on the cases of tests/supp_cases.py — tests/test_supp_cases.py shows on the CPU
that every family reaches its branch and that the chimeras hold enough reads of 2, 3 and 4 lines.

Per option set (supp_cases.OPTION_SETS) and under n_processed = 4 000 and 2^32 + 5:
  * decision: EVERY read that is eligible by the reference alone (at most 64 regions, 2 .. 4 lines, no pa:f, no tag past 8 entries) is
    decided with 17 — 11 when a line carries a tag and the listing is off — and no other read is; line count, and per line the
    descriptor (region, flag without the strand bit, MAPQ after the cap, AS, XS, XA count in bits 16-19, the request's place), the
    request (band: tests/ref_band.py) and the XA requests in list order say what the reference's lines say; five gets 10,
    below_T_second 1; reads not decided with 17 have no lines; with the side arrays null the statuses are Engine.singles_wave's.
  * text: sam_lines_kernel runs twice — on the kernel's own descriptors and on descriptors built from the reference's lists and text
    (so that a wrong decision cannot hide a wrong writer) — and every record is byte-identical to the reference's mem_reg2sam string,
    the records back to back in [0, cursor), guard bytes intact.  A read comes back (out_len = -1) exactly when the reference's text
    says why (a line's short fields beyond LINES_ROW, what the SA tags say of a line beyond SA_STAGE, an XA entry beyond XA_STAGE) or
    aln_kernel declined one of its requests by its header; row_over comes back; of the eligible realistic reads under the default
    options at most 10 % come back (the count is printed).
Measured on the MI355X: under the default options the families' 87 reads end in 80 x 17, 4 x 1 and 3 x 10, 76 records are written and 4
(row_over) handed back; all 275 eligible realistic reads (79 / 111 / 85 of 2 / 3 / 4 lines) are decided with 17 and none comes back
(share 0.000) under either n_processed; under max_XA_hits = 9 the 51 family reads and 34 realistic reads with a tag on a line get 11;
under a=2 b=5, 14 family reads come back, each with a reason this test checks."""
import numpy as np
import pytest

import se_wave_cases as swc
import supp_cases as spc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

N_PROCESSED = 4000
N_PROCESSED_BIG = (1 << 32) + 5


@pytest.fixture(scope="module")
def stage(genome, tmp_path_factory):
    # the reference's library travels with the tree: without it this test fails, it does not skip
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    import pair_wave_cases as pw
    from mpibwa_amd import api
    lib = api.load_library()
    assert lib.mi355x_se_lines_cap() == spc.SE_LINES_CAP and lib.mi355x_sam_lines_row() == spc.LINES_ROW and lib.mi355x_sam_lines_sa_stage() == spc.SA_STAGE
    assert lib.mi355x_pair_wave_xa_cap() == spc.PW_XA_CAP and api.Engine.SE_DECIDED_LINES == spc.SE_DECIDED_LINES
    g = pw.build_index(tmp_path_factory.mktemp("supp_stage"))
    out = {"lib": lib, "real_cases": spc.realistic_cases(g)}
    for key, prefix in (("session", genome["prefix"]), ("real", g["prefix"])):
        out[key] = {"prefix": prefix, "eng": api.Engine(prefix, upload=False), "ref": po.RefIndex(prefix)}
    return out


class Side:
    """both libraries on one index under one option set; the read group is taken back on the way out"""

    def __init__(self, stage, which, name):
        self.lib = stage["lib"]
        self.prefix, self.eng, self.ref = stage[which]["prefix"], stage[which]["eng"], stage[which]["ref"]
        self.kw, self.with_qual, self.rg = spc.OPTION_SETS[name]

    def __enter__(self):
        self.opt, self.ropt = self.eng.opt(**self.kw), self.ref.opt(**self.kw)
        if self.kw:
            for lib, o in ((self.lib, self.opt), (self.ref.lib, self.ropt)):
                lib.bwa_fill_scmat(o.contents.a, o.contents.b, o.contents.mat)
        self.rgid = self.ref.set_rg(self.rg)
        assert po.set_rg(self.lib, self.rg) == self.rgid
        self.ix = spc.Index(self.prefix, self.ref.bns)
        self.listing = spc.n_xa_max(self.ropt.contents) <= spc.PW_XA_CAP
        return self

    def __exit__(self, *exc):
        self.ref.set_rg(None)
        po.set_rg(self.lib, None)

    def want(self, order, read_no, n_processed):
        return spc.reference_side(self.ref, self.ropt, order, self.with_qual, n_processed, read_no)

    def decide(self, order, read_no, n_processed, **kw):
        return self.eng.singles_wave_lines(self.opt, read_no, spc.device_lists(order, self.eng.REG_DT), max_len=spc.MAX_LEN, n_processed=n_processed, **kw)


def _req_tuple(q):
    return tuple(int(q[f]) for f in ("rb", "re", "read", "qb", "qe", "w2", "truesc", "pad"))


def check_decisions(side, order, want, read_no, status, lines, tag):
    """-> the work items decided with 17"""
    o = side.ropt.contents
    taken = []
    for t, cs in enumerate(order):
        text, after = want[t]
        st = int(status[t])
        elig = spc.eligible(cs, text)
        if elig:   # the kernel has no reason to decline one
            assert st == (spc.SE_DECIDED_LINES if side.listing or not spc.has_xa(text) else spc.SE_HOST_XA), (tag, t, cs["family"], cs["tag"], st, text)
        else:
            assert st != spc.SE_DECIDED_LINES, (tag, t, cs["family"], cs["tag"], text)
        if cs["expect"] == "lines":
            assert elig or not side.listing, (tag, t, cs["family"], cs["tag"], text)
            if not elig:   # (a tag of nine entries under max_XA_hits = 9)
                assert st == spc.SE_HOST_XA, (tag, t, st)
        elif cs["expect"] == "plain":
            assert st == spc.SE_DECIDED, (tag, t, cs["family"], st)
        elif cs["expect"] is not None:
            assert st == cs["expect"], (tag, t, cs["family"], st)
        if st != spc.SE_DECIDED_LINES:
            assert lines[t] == [], (tag, t, st, lines[t])
            continue
        taken.append(t)
        ref_lines = spc.reference_lines(o, side.ix, text, after)
        assert len(lines[t]) == len(ref_lines), (tag, t, len(lines[t]), text)
        at = 0
        for j, ((d, q, xr), R) in enumerate(zip(lines[t], ref_lines)):
            r = R["region"]
            assert all(int(d[f]) == int(r[f]) for f in ("rb", "re", "qb", "qe", "rid")), (tag, t, j, d, r)
            assert (int(d["flag"]) & 0xffff, int(d["flag"]) >> 16, int(d["mapq"]), int(d["score"]), int(d["sub"]), int(d["req"])) == \
                   (R["flag"], R["n_xa"], R["mapq"], R["score"], R["sub"], at), (tag, t, j, cs["family"], d, R, text)
            assert _req_tuple(q) == spc.request_of(o, r, read_no[t]), (tag, t, j, q, r)
            assert len(xr) == len(R["xa"]) == R["n_xa"], (tag, t, j, len(xr), R["n_xa"])
            for x, h in zip(xr, R["xa"]):
                assert _req_tuple(x) == spc.request_of(o, h, read_no[t], pad=int(h["rid"])), (tag, t, j, x, h)
            at += 1 + len(xr)
    return taken


def reference_descriptors(side, order, want, read_no, eng):
    """per eligible read: the lines [(desc, req, xa_req)] as the reference's lists and text give them"""
    o = side.ropt.contents
    out = {}
    for t, cs in enumerate(order):
        text, after = want[t]
        if not spc.eligible(cs, text):
            continue
        mine, at = [], 0
        for R in spc.reference_lines(o, side.ix, text, after):
            r = R["region"]
            d = np.zeros((), dtype=eng.DESC_DT)
            for f in ("rb", "re", "qb", "qe", "rid"):
                d[f] = r[f]
            d["req"], d["flag"], d["mapq"], d["score"], d["sub"] = at, R["flag"] | R["n_xa"] << 16, R["mapq"], R["score"], R["sub"]
            q = np.array([spc.request_of(o, r, read_no[t])], dtype=eng.AREQ_DT)[0]
            xr = np.array([spc.request_of(o, h, read_no[t], pad=int(h["rid"])) for h in R["xa"]], dtype=eng.AREQ_DT)
            mine.append((d, q, xr))
            at += 1 + len(xr)
        out[t] = mine
    return out


def check_records(side, order, want, read_no, by_read, tag):
    """the reads of by_read {work item: lines} through aln_kernel + sam_lines_kernel -> per read 'dev' or 'back'"""
    if not by_read:
        return {}
    eng = side.eng
    taken = sorted(by_read)
    cap = spc.SE_LINES_CAP
    reads, names, quals, q, base = [], [], [], [], [0]
    d = np.zeros((len(taken), cap), dtype=eng.DESC_DT)
    d["req"] = -1
    n_lines = np.zeros(len(taken), dtype=np.uint8)
    for j, t in enumerate(taken):
        cs = order[t]
        reads.append(cs["read"]); names.append(cs["name"]); quals.append(spc.quality(len(cs["read"]), t))
        n_lines[j] = len(by_read[t])
        for l, (dl, ql, xr) in enumerate(by_read[t]):
            d[j, l] = dl
            mine = np.concatenate([np.array([ql], dtype=eng.AREQ_DT), np.asarray(xr, dtype=eng.AREQ_DT)])
            assert (mine["read"] == read_no[t]).all(), (tag, t, mine)
            mine["read"] = j
            q.append(mine)
        base.append(base[-1] + sum(1 + len(xr) for _, _, xr in by_read[t]))
    res = eng.sam_records_se_lines(side.opt, reads, quals if side.with_qual else None, names, n_lines, d, np.concatenate(q), np.array(base, dtype=np.int32))
    assert (res["guard"] == eng.SAM_GUARD_BYTE).all(), (tag, "bytes behind the arena were written")
    state, spans = {}, []
    for j, t in enumerate(taken):
        text = want[t][0]
        ln = int(res["out_len"][j])
        assert ln >= -1, (tag, t, ln)
        why = set()
        for line in text.splitlines():
            if spc.row_bytes(line, side.with_qual, side.rgid) > spc.LINES_ROW:
                why.add("row")
            if spc.sa_bytes(line) > spc.SA_STAGE:
                why.add("sa")
            if any(swc.xa_entry_bytes(e) > spc.XA_STAGE for e in swc.xa_entries(line + b"\n")):
                why.add("xa_stage")
        if (res["hdr"]["flags"][base[j]:base[j + 1]] != 0).any():
            why.add("declined")
        state[t] = "dev" if ln >= 0 else "back"
        assert (ln < 0) == bool(why), (tag, t, order[t]["family"], order[t]["tag"], ln, why, text)
        if ln < 0:
            continue
        at = int(res["out_off"][j])
        assert at + ln <= res["cursor"] <= res["arena_bytes"], (tag, t, at, ln, res["cursor"])
        got = res["arena"][at:at + ln].tobytes()
        assert got == text, (tag, t, order[t]["family"], order[t]["tag"], got, text)
        spans.append((at, ln))
    spans.sort()
    for (a, la), (b, _) in zip(spans, spans[1:]):
        assert a + la <= b, (tag, "records overlap", a, la, b)
    assert sum(la for _, la in spans) == res["cursor"], (tag, "the records do not lie back to back in [0, cursor)", res["cursor"])
    assert (res["arena"][res["cursor"]:] == eng.SAM_GUARD_BYTE).all(), (tag, "bytes outside the records were written")
    return state


def run_group(side, cases, tag, n_processed=N_PROCESSED, seed=11, text=True):
    order = spc.shuffled(cases, seed)
    read_no = spc.read_numbers(len(order), seed + 1)
    want = side.want(order, read_no, n_processed)
    status, desc, req, xa_req, lines = side.decide(order, read_no, n_processed)
    taken = check_decisions(side, order, want, read_no, status, lines, tag)
    # without the side arrays: Engine.singles_wave's statuses, 10 for every read of several lines
    s0 = side.eng.singles_wave(side.opt, read_no, spc.device_lists(order, side.eng.REG_DT), max_len=spc.MAX_LEN, n_processed=n_processed)[0]
    s1 = side.decide(order, read_no, n_processed, lines=False)[0]
    assert (s0 == s1).all() and not (s0 == spc.SE_DECIDED_LINES).any(), (tag, s0, s1)
    for t, cs in enumerate(order):
        if status[t] == spc.SE_DECIDED_LINES or (status[t] == spc.SE_HOST_XA and want[t][0].count(b"\n") > 1):   # (11: a tag without the listing)
            assert s0[t] == spc.SE_HOST_SUPP, (tag, t, s0[t])
        else:
            assert s0[t] == status[t], (tag, t, s0[t], status[t])
    state = ref_state = {}
    if text:
        state = check_records(side, order, want, read_no, {t: lines[t] for t in taken}, tag + "/kernel")
        ref_state = check_records(side, order, want, read_no, reference_descriptors(side, order, want, read_no, side.eng), tag + "/reference")
        for t in taken:
            assert state[t] == ref_state[t], (tag, t, state[t], ref_state[t])
    return order, want, status, lines, state, ref_state


@pytest.mark.parametrize("name", list(spc.OPTION_SETS))
def test_supp_stage_matches_the_reference(stage, name):
    with Side(stage, "session", name) as side:
        cases = spc.build_cases(side.ix, side.ropt.contents, 3)
        for npr in (N_PROCESSED, N_PROCESSED_BIG):
            order, want, status, lines, state, _ = run_group(side, cases, "%s/families/%d" % (name, npr), n_processed=npr)
            hist = {int(c): int((status == c).sum()) for c in np.unique(status)}
            print(name, npr, "families: reads", len(order), "status", hist, "written", sum(s == "dev" for s in state.values()),
                  "handed back", sum(s == "back" for s in state.values()))
            assert hist.get(spc.SE_DECIDED_LINES, 0) >= 40 and hist.get(spc.SE_HOST_SUPP, 0) == 3 and hist.get(spc.SE_DECIDED, 0) == 4, (name, hist)
            for t, cs in enumerate(order):
                if cs["family"] == "row_over":
                    assert status[t] == spc.SE_DECIDED_LINES and state[t] == "back", (name, t, status[t], state.get(t))
                if cs["family"] in ("two", "three", "four", "lead_del", "trail_del", "xa_over"):
                    assert state[t] == "dev", (name, t, cs["family"])
    with Side(stage, "real", name) as side:
        for npr in (N_PROCESSED, N_PROCESSED_BIG) if name == "default" else (N_PROCESSED,):
            order, want, status, lines, state, ref_state = run_group(side, stage["real_cases"], "%s/real/%d" % (name, npr), n_processed=npr)
            c = spc.census(order, want)
            elig = [t for t, cs in enumerate(order) if spc.eligible(cs, want[t][0])]
            back = sum(ref_state[t] == "back" for t in elig)
            hist = {int(c_): int((status == c_).sum()) for c_ in np.unique(status)}
            print(name, npr, "realistic reads", c, "status", hist, "eligible reads handed back %d of %d, share %.3f" % (back, len(elig), back / max(1, len(elig))))
            if name == "default":
                assert all(c.get("eligible%d" % k, 0) >= 30 for k in (2, 3, 4)), c
                assert 10 * back <= len(elig), (back, len(elig))


def test_launch_sizes(stage):
    with Side(stage, "session", "default") as side:
        cases = spc.build_cases(side.ix, side.ropt.contents, 3)
        order = spc.shuffled(cases, 11)
        read_no = spc.read_numbers(len(order), 12)
        side.want(order, read_no, N_PROCESSED)   # (the lists the device is handed are the reference's, after its mem_sort_dedup_patch)
        status, desc, req, xa_req, lines = side.decide(order, read_no, N_PROCESSED)
        assert (status == spc.SE_DECIDED_LINES).sum() >= 40
        for n in (1, 2, 63, 65):
            s, d, q, x, ln = side.decide(order[:n], read_no[:n], N_PROCESSED)
            assert (s == status[:n]).all(), (n, s, status[:n])
            for t in range(n):
                assert len(ln[t]) == len(lines[t]), (n, t)
                for a, b in zip(ln[t], lines[t]):
                    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes(), (n, t)
        # the lines' XA listing off: reads with a tag on a line get 11, the others are decided as before
        s, d, q, x, ln = side.decide(order, read_no, N_PROCESSED, xa=False)
        for t in range(len(order)):
            if status[t] == spc.SE_DECIDED_LINES:
                with_tag = any(len(l[2]) for l in lines[t])
                assert s[t] == (spc.SE_HOST_XA if with_tag else spc.SE_DECIDED_LINES), (t, s[t])
                if not with_tag:
                    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(ln[t], lines[t])), t


def test_tie_family_follows_the_hash(stage):
    """two hits of equal score on the span of line 0: hash_64(id + place in the list) says which is the line and which its XA entry —
    under an id above 2^32 too"""
    with Side(stage, "session", "default") as side:
        cases = [cs for cs in spc.build_cases(side.ix, side.ropt.contents, 3) if cs["family"] == "tie"]
        first = []
        for npr in (N_PROCESSED, N_PROCESSED_BIG):
            order, want, status, lines, _, _ = run_group(side, cases, "tie/%d" % npr, n_processed=npr, text=False)
            assert (status == spc.SE_DECIDED_LINES).all() and all(len(ln) == 2 and len(ln[0][2]) == 1 for ln in lines)
            first.append([int(ln[0][0]["rb"]) for ln in lines])
        flips = sum(a != b for a, b in zip(*first))
        print("tie: line 0 changes with n_processed in", flips, "of", len(cases))
        assert flips >= 4, flips
