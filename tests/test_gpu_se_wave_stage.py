"""Stage test of se_wave_kernel (mpibwa_amd/csrc/se_wave_kernel.hip): the decisions through mi355x_se_wave_batch (the pipeline's own
launch function), then the text through mi355x_sam_se_batch (aln_kernel and the single-end instantiation of sam_emit_kernel) with the
kernel's own request bases, against the reference's OWN mem_align1_core / mem_sort_dedup_patch, mem_mark_primary_se (id = n_processed +
read number) and mem_reg2sam (oracle/_ref/libbwaref.so), on the cases of tests/se_wave_cases.py — tests/test_se_wave_cases.py shows on
the CPU that every family reaches its branch and that the realistic reads hold what the kernel is for.

Per option set (se_stage_cases.OPTION_SETS, max_XA_hits = 8: the cap of the side array, max_XA_hits = 9: no listing):
  * every read taken (status 1 or 16) is eligible by the reference alone; descriptor (region, flag without the strand bit, MAPQ, AS, XS)
    and request (band: tests/ref_band.py) say what the reference's line says; xa_cnt, bits 16-19 of the flag and the XA requests, in
    order, name exactly the hits of the reference's tag (the hits under the line's hit within XA_drop_ratio in the reference's own list,
    their contig and strand as the tag spells them) with mem_reg2aln's band;
  * completeness: every eligible realistic read and every family built to be the device's is taken (without the listing: the XA ones
    get 11), every family built to be the host's is left with its code; desc.req = req.read = -1 for every read not taken;
  * text: byte-identical to the reference's record, back to back in [0, cursor), guard bytes intact; a read is handed back exactly when
    the reference's text says why — short fields beyond the 260-byte row, an XA entry beyond XA_STAGE — or aln_kernel declined one of its
    requests by its header; at least half of the eligible XA reads of (a) come back written (the share is printed).
Launches of 1, 2, 63, 64, 65 and all work items and a run with xa_req = NULL give what the big launch gives; the tie family follows
the hash under n_processed = 4000 and under a value above 2^32, with read numbers that are not 0 .. n-1."""
import numpy as np
import pytest

import se_stage_cases as sec
import se_wave_cases as swc
from oracle import pyoracle as po
from ref_band import reg2aln_band

pytestmark = pytest.mark.gpu

N_PROCESSED = 4000
N_PROCESSED_BIG = (1 << 32) + 5
MAX_LEN = 150


@pytest.fixture(scope="module")
def stage(genome, genome_alt, tmp_path_factory):
    # the reference's library travels with the tree: without it this test fails, it does not skip
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    import pair_wave_cases as pw
    from mpibwa_amd import api
    lib = api.load_library()
    assert hasattr(lib, "mi355x_se_wave_batch") and lib.mi355x_pair_wave_maxreg() == swc.PW_MAXREG and lib.mi355x_pair_wave_xa_cap() == swc.PW_XA_CAP
    g = pw.build_index(tmp_path_factory.mktemp("se_wave_stage"))
    out = {"lib": lib, "real_cases": swc.realistic_cases(g)}
    for key, prefix in (("session", genome["prefix"]), ("alt", genome_alt["prefix"]), ("real", g["prefix"])):
        out[key] = {"prefix": prefix, "eng": api.Engine(prefix, upload=False), "ref": po.RefIndex(prefix)}
    return out


class Side:
    """both libraries on one index under one option set; the read group is taken back on the way out"""

    def __init__(self, stage, which, name):
        self.lib = stage["lib"]
        self.prefix, self.eng, self.ref = stage[which]["prefix"], stage[which]["eng"], stage[which]["ref"]
        self.kw, self.with_qual, self.rg = swc.OPTION_SETS[name]

    def __enter__(self):
        self.opt, self.ropt = self.eng.opt(**self.kw), self.ref.opt(**self.kw)
        if self.kw:
            for lib, o in ((self.lib, self.opt), (self.ref.lib, self.ropt)):
                lib.bwa_fill_scmat(o.contents.a, o.contents.b, o.contents.mat)
        self.rgid = self.ref.set_rg(self.rg)
        assert po.set_rg(self.lib, self.rg) == self.rgid
        self.ix = swc.Index(self.prefix, self.ref.bns)
        self.listing = swc.n_xa_max(self.ropt.contents) <= swc.PW_XA_CAP
        return self

    def __exit__(self, *exc):
        self.ref.set_rg(None)
        po.set_rg(self.lib, None)

    def want(self, order, read_no, n_processed=N_PROCESSED):
        return swc.reference_side(self.ref, self.ropt, order, self.with_qual, n_processed, read_no)

    def decide(self, order, read_no, n_processed=N_PROCESSED, xa=True):
        return self.eng.singles_wave(self.opt, read_no, swc.device_lists(order, self.eng.REG_DT), max_len=MAX_LEN, n_processed=n_processed, xa=xa)


def check_decisions(side, order, want, read_no, status, desc, req, xa_req, tag):
    """every taken read is eligible and described as the reference's line and tag say -> (taken work items, those with an XA position
    that mem_reg2aln moved off the hit's first base: the request holds the region, the text test covers the position)"""
    o = side.ropt.contents
    ix = side.ix
    ratio = float(np.float32(o.XA_drop_ratio))
    taken, moved = [], set()
    for t, cs in enumerate(order):
        text, after = want[t]
        st = int(status[t])
        if st not in (swc.SE_DECIDED, swc.SE_DECIDED_XA):
            assert desc[t]["req"] == -1 and req[t]["read"] == -1 and len(xa_req[t]) == 0, (tag, t, st)
            continue
        taken.append(t)
        assert swc.eligible(cs, text), (tag, t, cs["family"], cs["tag"], len(cs["before"]), text)
        entries = swc.xa_entries(text)
        assert (st == swc.SE_DECIDED_XA) == bool(entries), (tag, t, cs["family"], st, text)
        region, flag, mapq, score, sub = sec.the_line(o, text, after)
        d, q = desc[t], req[t]
        assert (int(d["flag"]) & 0xffff, int(d["flag"]) >> 16, int(d["mapq"]), int(d["score"]), int(d["sub"])) == (flag, len(entries), mapq, score, sub), \
            (tag, t, cs["family"], d, text)
        assert len(xa_req[t]) == len(entries), (tag, t, len(xa_req[t]), entries)
        if region is None:
            assert d["req"] == -3 and d["rid"] == -1 and q["read"] == -1 and not entries, (tag, t, d, q)
            continue
        assert d["req"] == 0 and all(int(d[f]) == int(region[f]) for f in ("rb", "re", "qb", "qe", "rid")), (tag, t, d, region)
        w2 = reg2aln_band(o, int(region["qe"] - region["qb"]), int(region["re"] - region["rb"]), int(region["truesc"]), int(region["w"]))
        assert (int(q["rb"]), int(q["re"]), int(q["read"]), int(q["qb"]), int(q["qe"]), int(q["w2"]), int(q["truesc"]), int(q["pad"])) == \
               (int(region["rb"]), int(region["re"]), int(read_no[t]), int(region["qb"]), int(region["qe"]), w2, int(region["truesc"]), 0), (tag, t, q, region, w2)
        # the hits of the tag: those under the line's hit within the ratio, in the order of the reference's own list
        z = [j for j, r in enumerate(after) if r["secondary"] < 0 and r["score"] >= o.T]
        assert len(z) == 1
        listed = [r for r in after if r["secondary_all"] == z[0] and int(r["score"]) >= int(after[z[0]]["score"]) * ratio]
        if entries:
            assert len(listed) == len(entries), (tag, t, len(listed), entries)
        for x, h, e in zip(xa_req[t], listed, entries):
            assert (int(x["rb"]), int(x["re"]), int(x["qb"]), int(x["qe"]), int(x["truesc"]), int(x["pad"]), int(x["read"])) == \
                   (int(h["rb"]), int(h["re"]), int(h["qb"]), int(h["qe"]), int(h["truesc"]), int(h["rid"]), int(read_no[t])), (tag, t, x, h)
            assert int(x["w2"]) == reg2aln_band(o, int(h["qe"] - h["qb"]), int(h["re"] - h["rb"]), int(h["truesc"]), int(h["w"])), (tag, t, x)
            rev = int(h["rb"]) >= ix.l_pac
            assert e[0] == ix.names[int(h["rid"])] and (e[1] == b"-") == rev, (tag, t, e, h)
            first = (2 * ix.l_pac - int(h["re"]) if rev else int(h["rb"])) - ix.off[int(h["rid"])] + 1
            if e[2] != first:   # (mem_reg2aln moved the position: an alignment that starts with a deletion)
                moved.add(t)
    return taken, moved


def check_records(side, order, want, read_no, taken, desc, req, xa_req, tag):
    """the taken reads through aln_kernel + sam_emit_kernel with the kernel's own request bases -> per taken read 'dev' or 'back'"""
    if not taken:
        return {}
    eng = side.eng
    reads, names, quals, q, base = [], [], [], [], [0]
    d = np.zeros(len(taken), dtype=eng.DESC_DT)
    for j, t in enumerate(taken):
        cs = order[t]
        reads.append(cs["read"]); names.append(cs["name"]); quals.append(swc.quality(len(cs["read"]), t))
        d[j] = desc[t]
        if desc[t]["req"] >= 0:   # [the line's request, its XA entries']; the unmapped record has none
            mine = np.concatenate([req[t:t + 1], xa_req[t]])
            assert (mine["read"] == read_no[t]).all() and int(desc[t]["req"]) == 0, (tag, t, mine)
            mine["read"] = j
            q.append(mine)
        base.append(base[-1] + (1 + len(xa_req[t]) if desc[t]["req"] >= 0 else 0))
    qs = np.concatenate(q) if q else np.zeros(0, dtype=eng.AREQ_DT)
    res = eng.sam_records_se(side.opt, reads, quals if side.with_qual else None, names, d, qs, np.array(base, dtype=np.int32))
    assert (res["guard"] == eng.SAM_GUARD_BYTE).all(), (tag, "bytes behind the arena were written")
    state, spans = {}, []
    for j, t in enumerate(taken):
        text = want[t][0]
        ln = int(res["out_len"][j])
        assert ln >= -1, (tag, t, ln)
        why = set()
        if desc[t]["req"] >= 0:
            if sec.parse(swc.without_xa(text), side.rgid)["short"] > swc.SAM_ROW:
                why.add("row")
            if any(swc.xa_entry_bytes(e) > swc.XA_STAGE for e in swc.xa_entries(text)):
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


def run_group(side, cases, tag, n_processed=N_PROCESSED, seed=11):
    order = swc.shuffled(cases, seed)
    read_no = swc.read_numbers(len(order), seed + 1)
    assert not (read_no == np.arange(len(order))).any()
    want = side.want(order, read_no, n_processed)
    status, desc, req, xa_req = side.decide(order, read_no, n_processed)
    taken, moved = check_decisions(side, order, want, read_no, status, desc, req, xa_req, tag)
    # completeness: what the reference alone says the kernel can take, it takes; what a family is built for, it gets
    for t, cs in enumerate(order):
        text = want[t][0]
        st = int(status[t])
        if cs["expect"] is None:
            if swc.eligible(cs, text):
                is_xa = bool(swc.xa_entries(text))
                assert st == (swc.SE_DECIDED if not is_xa else swc.SE_DECIDED_XA if side.listing else swc.SE_HOST_XA), (tag, t, st, len(cs["before"]), text)
        elif cs["expect"] == "plain":
            assert st == swc.SE_DECIDED, (tag, t, cs["family"], cs["tag"], st)
        elif cs["expect"] == "xa":
            assert st == (swc.SE_DECIDED_XA if side.listing else swc.SE_HOST_XA), (tag, t, cs["family"], cs["tag"], st)
            assert not side.listing or len(xa_req[t]) == cs["n_xa"], (tag, t, cs["family"], len(xa_req[t]))
        else:
            assert st == cs["expect"], (tag, t, cs["family"], cs["tag"], st)
    state = check_records(side, order, want, read_no, taken, desc, req, xa_req, tag)
    return order, read_no, want, status, desc, req, xa_req, state


@pytest.mark.parametrize("name", list(swc.OPTION_SETS))
def test_se_wave_stage_matches_the_reference(stage, name):
    with Side(stage, "session", name) as side:
        cases = swc.build_cases(side.ix, side.ropt.contents, 3)
        order, _, want, status, _, _, _, state = run_group(side, cases, name + "/families")
        hist = {int(c): int((status == c).sum()) for c in np.unique(status)}
        print(name, "families: reads", len(order), "status", hist, "written", sum(s == "dev" for s in state.values()), "handed back", sum(s == "back" for s in state.values()))
        for code in (swc.SE_DECIDED, swc.SE_HOST_LENGTH, swc.SE_HOST_SUPP, swc.SE_HOST_FULL, swc.SE_DECIDED_XA if side.listing else swc.SE_HOST_XA):
            assert hist.get(code, 0) > 0, (name, code, hist)
    with Side(stage, "alt", name) as side:
        is_alt = [int(side.ref.bns.contents.anns[c].is_alt) for c in range(side.ix.n_seqs)]
        order, _, _, status, _, _, _, _ = run_group(side, swc.build_alt_cases(side.ix, is_alt, side.ropt.contents, 6), name + "/alt")
        assert (status == swc.SE_HOST_ALT).all()
    with Side(stage, "real", name) as side:
        order, _, want, status, _, _, _, state = run_group(side, stage["real_cases"], name + "/real")
        c = swc.census(order, want)
        xa = [t for t, cs in enumerate(order) if swc.eligible(cs, want[t][0]) and swc.xa_entries(want[t][0])]
        xa_dev = sum(state.get(t) == "dev" for t in xa)
        hist = {int(c_): int((status == c_).sum()) for c_ in np.unique(status)}
        print(name, "realistic reads", c, "status", hist, "written", sum(s == "dev" for s in state.values()), "handed back", sum(s == "back" for s in state.values()),
              "eligible XA reads written %d of %d, share %.3f" % (xa_dev, len(xa), xa_dev / max(1, len(xa))))
        assert c["plain_gt8"] >= 50 and c["xa"] >= 50, c
        if side.listing:
            assert 2 * xa_dev >= len(xa), (name, xa_dev, len(xa))


def test_launch_sizes_and_no_listing(stage):
    with Side(stage, "session", "default") as side:
        cases = swc.build_cases(side.ix, side.ropt.contents, 3)
        order = swc.shuffled(cases, 11)
        read_no = swc.read_numbers(len(order), 12)
        side.want(order, read_no)   # (the lists the device is handed are the reference's, after its mem_sort_dedup_patch)
        status, desc, req, xa_req = side.decide(order, read_no)
        assert (status[:63] == swc.SE_DECIDED_XA).sum() >= 3 and (status[:63] == swc.SE_DECIDED).sum() >= 3, np.bincount(status[:65])
        for n in (1, 2, 63, 64, 65, len(order)):
            s, d, q, x = side.decide(order[:n], read_no[:n])
            assert (s == status[:n]).all(), (n, s, status[:n])
            for t in range(n):
                assert d[t].tobytes() == desc[t].tobytes() and q[t].tobytes() == req[t].tobytes() and x[t].tobytes() == xa_req[t].tobytes(), (n, t)
        # without the side array: the XA reads are left with 11, every other read as before
        s, d, q, x = side.decide(order, read_no, xa=False)
        for t in range(len(order)):
            if status[t] == swc.SE_DECIDED_XA:
                assert s[t] == swc.SE_HOST_XA and d[t]["req"] == -1 and q[t]["read"] == -1, (t, s[t])
            else:
                assert s[t] == status[t] and d[t].tobytes() == desc[t].tobytes() and q[t].tobytes() == req[t].tobytes(), (t, s[t], status[t])
            assert len(x[t]) == 0


def test_tie_family_follows_the_hash(stage):
    """two hits of equal score on one span: hash_64(id + place in the list) says which is the line and which the XA entry, so the hash,
    id0 = n_processed and the read number are all observable — under an id above 2^32 too"""
    with Side(stage, "session", "default") as side:
        cases = [cs for cs in swc.build_cases(side.ix, side.ropt.contents, 3) if cs["family"] == "tie"]
        lines = []
        for npr in (N_PROCESSED, N_PROCESSED_BIG):
            order, _, want, status, desc, _, xa_req, _ = run_group(side, cases, "tie/%d" % npr, n_processed=npr)
            assert (status == swc.SE_DECIDED_XA).all() and all(len(x) == 1 for x in xa_req)
            lines.append([int(d["rb"]) for d in desc])
        flips = sum(a != b for a, b in zip(*lines))
        print("tie: the line changes with n_processed in", flips, "of", len(cases))
        assert flips >= 8, flips
