"""Stage test of the single-end decisions and records on the device: se_simple_kernel through mi355x_se_batch, then aln_kernel and the
single-end instantiation of sam_emit_kernel through mi355x_sam_se_batch (the pipeline's own launch sequence), against the reference's
OWN mem_sort_dedup_patch, mem_mark_primary_se and mem_reg2sam (oracle/_ref/libbwaref.so, called the way the single-end branch of
worker2 calls them), on the cases of tests/se_stage_cases.py — tests/test_se_cases.py shows on the CPU that every family reaches its
branch.

Per option set (default, no qualities, a 7-byte and a 255-byte read group, other scores):
  * every read the kernel takes (status 1) is one the reference reports with exactly one line and neither XA nor SA; its descriptor
    (region, flag, MAPQ, score, sub) and its request (the band from tests/ref_band.py) say what the reference's line says;
  * in the families built to be plain no read is left to the host, in the families built to be the host's no read is taken, and the
    other status codes name the test the family was built for;
  * the text of the taken reads is the reference's record byte for byte; the records lie back to back in [0, cursor), nothing else is
    written, the guard keeps its pattern; a read is handed back (-1, alone) exactly when the short fields of its record, measured on
    the reference's text, are longer than the 260-byte staging row or aln_kernel declined its CIGAR: 260 is written, 261 goes back;
  * the same launch with an arena of half and of a tenth of the need, with three workgroups, and launches of 1, 63, 64 and 65 reads.
On a random set (the ends of pair_cases.adversarial_pairs, each as a single-end read) a read taken must be reference-plain, and the
kernel must take at least half of the reads that are reference-plain and have at most mi355x_pair_maxreg() regions — the project's
"most of" floor, with the reference alone deciding the denominator; the share is printed."""
import numpy as np
import pytest

import se_stage_cases as sec
from oracle import pyoracle as po
from ref_band import reg2aln_band

pytestmark = pytest.mark.gpu

N_PROCESSED = 4000


@pytest.fixture(scope="module")
def stage(genome):
    # the reference's library travels with the tree: without it this test fails, it does not skip
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    from mpibwa_amd import api
    lib = api.load_library()
    assert hasattr(lib, "mi355x_se_batch") and hasattr(lib, "mi355x_sam_se_batch")
    return {"lib": lib, "prefix": genome["prefix"], "eng": api.Engine(genome["prefix"], upload=False), "ref": po.RefIndex(genome["prefix"])}


class Side:
    """both libraries under one option set; the read group is taken back on the way out"""

    def __init__(self, stage, name):
        self.prefix, self.eng, self.ref, self.lib = stage["prefix"], stage["eng"], stage["ref"], stage["lib"]
        self.kw, self.with_qual, self.rg = sec.OPTION_SETS[name]

    def __enter__(self):
        self.opt, self.ropt = self.eng.opt(**self.kw), self.ref.opt(**self.kw)
        if self.kw:
            for lib, o in ((self.lib, self.opt), (self.ref.lib, self.ropt)):
                lib.bwa_fill_scmat(o.contents.a, o.contents.b, o.contents.mat)
        self.rgid = self.ref.set_rg(self.rg)
        assert po.set_rg(self.lib, self.rg) == self.rgid
        self.ix = sec.Index(self.prefix, self.ref.bns)
        self.maxreg = int(self.lib.mi355x_pair_maxreg())
        return self

    def __exit__(self, *exc):
        self.ref.set_rg(None)
        po.set_rg(self.lib, None)

    def decide(self, order, max_len):
        regs, n_regs = sec.device_regions(order, self.eng.REG_DT, self.maxreg)
        return self.eng.singles(self.opt, regs, n_regs, max_len=max_len, n_processed=N_PROCESSED)

    def want(self, order):
        return sec.reference_side(self.ref, self.ropt, order, self.with_qual, n_processed=N_PROCESSED)

    def records(self, order, desc, req, **kw):
        return self.eng.sam_records_se(self.opt, **sec.read_inputs(order, self.with_qual), desc=desc, reqs=req,
                                       req_base=np.arange(len(order) + 1, dtype=np.int32), **kw)


def check_decisions(side, order, want, status, desc, req, tag):
    """every taken read is reference-plain and described as the reference's line says -> indices of the taken reads"""
    o = side.ropt.contents
    taken = []
    for i, cs in enumerate(order):
        text, after = want[i]
        if status[i] != 1:
            assert desc[i]["req"] == -1 and req[i]["read"] == -1, (tag, i, int(status[i]))
            continue
        taken.append(i)
        assert sec.is_plain(text), (tag, i, cs["family"], cs["tag"], text)
        assert len(cs["regs"]) <= side.maxreg
        region, flag, mapq, score, sub = sec.the_line(o, text, after)
        d, q = desc[i], req[i]
        assert (int(d["flag"]), int(d["mapq"]), int(d["score"]), int(d["sub"])) == (flag, mapq, score, sub), (tag, i, cs["family"], d, text)
        if region is None:
            assert d["req"] == -3 and d["rid"] == -1 and q["read"] == -1, (tag, i, d, q)
            continue
        assert d["req"] == 0 and all(int(d[f]) == int(region[f]) for f in ("rb", "re", "qb", "qe", "rid")), (tag, i, d, region)
        w2 = reg2aln_band(o, int(region["qe"] - region["qb"]), int(region["re"] - region["rb"]), int(region["truesc"]), int(region["w"]))
        assert (int(q["rb"]), int(q["re"]), int(q["read"]), int(q["qb"]), int(q["qe"]), int(q["w2"]), int(q["truesc"])) == \
               (int(region["rb"]), int(region["re"]), i, int(region["qb"]), int(region["qe"]), w2, int(region["truesc"])), (tag, i, q, region, w2)
    return taken


def check_records(side, order, want, status, res, tag, whole_arena=True):
    """-> per read: 'dev' (record returned and equal), 'back' (handed back), 'none' (not the device's)"""
    out_len, out_off, arena = res["out_len"], res["out_off"], res["arena"]
    assert (res["guard"] == side.eng.SAM_GUARD_BYTE).all(), (tag, "bytes behind the arena were written")
    state, spans = [], []
    for i, cs in enumerate(order):
        ln = int(out_len[i])
        if status[i] != 1:
            assert ln == -2, (tag, i, ln)
            state.append("none")
            continue
        assert ln >= -1, (tag, i, cs["family"], ln)
        if ln < 0:
            state.append("back")
            continue
        state.append("dev")
        at = int(out_off[i])
        assert at + ln <= min(res["cursor"], res["arena_bytes"]), (tag, i, at, ln, res["cursor"], res["arena_bytes"])
        got = arena[at:at + ln].tobytes()
        assert got == want[i][0], (tag, i, cs["family"], cs["tag"], got, want[i][0])
        spans.append((at, ln))
    spans.sort()
    covered = np.zeros(len(arena), dtype=bool)
    for (a, la), (b, _) in zip(spans, spans[1:]):
        assert a + la <= b, (tag, "records overlap", a, la, b)
    for a, la in spans:
        covered[a:a + la] = True
    assert (arena[~covered] == side.eng.SAM_GUARD_BYTE).all(), (tag, "bytes outside the records were written")
    if whole_arena:   # nothing turned away: the records lie back to back from 0 to the cursor
        assert res["cursor"] <= res["arena_bytes"] and sum(la for _, la in spans) == res["cursor"], (tag, res["cursor"], res["arena_bytes"])
    return state


def check_exact(side, order, want, status, desc, res, tag):
    """a launch whose arena holds everything: handed back exactly where there is a reason (row overflow by the reference's text, or
    aln_kernel's header says it declined)"""
    state = check_records(side, order, want, status, res, tag)
    for i, cs in enumerate(order):
        if state[i] == "none":
            continue
        why = set()
        if desc[i]["req"] >= 0:
            if sec.parse(want[i][0], side.rgid)["short"] > sec.SAM_ROW:
                why.add("row")
            if int(res["hdr"]["flags"][i]) != 0:
                why.add("declined")
        assert (state[i] == "back") == bool(why), (tag, i, cs["family"], cs["tag"], state[i], why, int(res["out_len"][i]))
    return state


HOST_CODE = dict(xa=11, tie=11, supp=10, maxreg=3)


@pytest.mark.parametrize("name", list(sec.OPTION_SETS))
def test_se_stage_matches_mem_reg2sam(stage, name):
    with Side(stage, name) as side:
        cases = sec.build_cases(side.ix, side.opt.contents, 1)
        order = sec.shuffled(cases, 2)
        want = side.want(order)
        status, desc, req = side.decide(order, sec.MAX_LEN)
        taken = set(check_decisions(side, order, want, status, desc, req, name))
        # the cap on what the kernel may leave out, and on what it may take
        for i, cs in enumerate(order):
            if cs["expect"] == "plain":
                assert i in taken, (name, i, cs["family"], cs["tag"], int(status[i]))
            else:
                assert i not in taken and int(status[i]) == HOST_CODE[cs["family"]], (name, i, cs["family"], cs["tag"], int(status[i]))
        res = side.records(order, desc, req)
        state = check_exact(side, order, want, status, desc, res, name)
        # the boundary of the staging row, on both sides: 260 is the device's, 261 goes back
        shorts = [sec.parse(want[i][0], side.rgid)["short"] if cs["family"] == "row" else 0 for i, cs in enumerate(order)]
        # (among the reads whose CIGAR aln_kernel computed: a declined one goes back whatever its length)
        done = [int(res["hdr"]["flags"][i]) == 0 for i in range(len(order))]
        at260 = [i for i, s in enumerate(shorts) if s == sec.SAM_ROW and done[i]]
        at261 = [i for i, s in enumerate(shorts) if s == sec.SAM_ROW + 1 and done[i]]
        assert at260 and at261 and all(state[i] == "dev" for i in at260) and all(state[i] == "back" for i in at261), (name, at260, at261)
        n_dev, n_back = sum(s == "dev" for s in state), sum(s == "back" for s in state)
        print(name, "reads", len(order), "taken", len(taken), "written", n_dev, "handed back", n_back, "of them declined by aln_kernel",
              sum(s == "back" and not d for s, d in zip(state, done)), "at 260 / 261 bytes", len(at260), len(at261))
        assert n_dev >= 1170 and n_back >= 50 and all(order[i]["family"] == "row" for i, s in enumerate(state) if s == "back")

        used = res["cursor"]
        # an arena that is too small: whole waves are handed back, nothing is written outside it or into the room of those waves
        for frac in (0.5, 0.1):
            tag = "%s/arena x %.1f" % (name, frac)
            small = side.records(order, desc, req, arena_bytes=int(used * frac))
            st2 = check_records(side, order, want, status, small, tag, whole_arena=False)
            assert small["cursor"] > small["arena_bytes"], tag
            waves = [set(st2[w:w + 64]) - {"none"} for w in range(0, len(order), 64)]
            assert any(w == {"back"} for w in waves) and any("dev" in w for w in waves), tag
            for i, s in enumerate(st2):      # what the full launch handed back stays handed back
                assert not (state[i] == "back" and s == "dev"), (tag, i)
        # three workgroups: every wave walks a third of the batches, its staging rows reused from one batch to the next
        strided = side.records(order, desc, req, grid_blocks=3)
        assert len(order) > 3 * 64 * 4
        assert check_exact(side, order, want, status, desc, strided, name + "/3 blocks") == state
        # launches of 1, 63, 64 and 65 reads
        for n in (1, 63, 64, 65):
            few = sec.small_launch(cases, n, n)
            w4 = side.want(few)
            s4, d4, r4 = side.decide(few, sec.MAX_LEN)
            tk = check_decisions(side, few, w4, s4, d4, r4, "%s/%d reads" % (name, n))
            assert set(tk) == {i for i, cs in enumerate(few) if cs["expect"] == "plain"}
            check_exact(side, few, w4, s4, d4, side.records(few, d4, r4), "%s/%d reads" % (name, n))


@pytest.mark.parametrize("name", list(sec.OPTION_SETS))
def test_se_stage_on_random_region_lists(stage, name):
    with Side(stage, name) as side:
        order = sec.random_cases(side.ix, 1500, 77)
        want = side.want(order)
        status, desc, req = side.decide(order, 150)
        taken = check_decisions(side, order, want, status, desc, req, name + "/random")
        could = [i for i, cs in enumerate(order) if sec.is_plain(want[i][0]) and len(cs["regs"]) <= side.maxreg]
        codes = {int(c): int((status == c).sum()) for c in np.unique(status)}
        print(name, "random reads", len(order), "reference-plain with <= %d regions" % side.maxreg, len(could), "taken", len(taken),
              "share %.3f" % (len(taken) / max(1, len(could))), "status codes", codes)
        assert set(taken) <= set(could)
        assert len(could) >= 500 and len(taken) >= len(could) / 2, (len(taken), len(could), codes)
        res = side.records(order, desc, req)
        check_exact(side, order, want, status, desc, res, name + "/random")
