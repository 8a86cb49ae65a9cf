"""Stage test of the SAM text on the device: aln_kernel and sam_emit_kernel through mi355x_sam_batch (the pipeline's own launch
sequence for the pairs decided on the device) against the reference's OWN mem_reg2aln and mem_aln2sam (oracle/_ref/libbwaref.so, called
the way mem_sam_pe's paired branch calls them), on the cases of tests/sam_stage_cases.py — tests/test_sam_cases.py shows on the CPU that
every family reaches its branch.

Per option set (default, no qualities, a 7-byte and a 255-byte read group, other scores): every record the device returns equals the
reference's text byte for byte; the records lie back to back in [0, cursor); out_len is -2 exactly for the descriptors that are not the
device's; a pair is handed back (-1, both reads) exactly when the test can say why without the kernel — the short fields of one of
its records, measured on the reference's text, are longer than the 260-byte staging row, or aln_kernel declined one of its CIGARs
(AlnHdr.flags) — so the row boundary is asserted on both sides (260 returned, 261 handed back) and no other record may come back.
Then the same launch with an arena of half and of a tenth of what the records need (every read byte-identical or -1, nothing written
past the arena: 4 096 guard bytes behind it keep their pattern, nor into the room of a wave that was turned away), with three
workgroups (the grid-stride loop and the reuse of the staging rows), and launches of 2, 62, 64 and 66 reads.

Not reached by any input, and therefore not tested: n_p == 0 (CIGAR '*' for a mapped record — aln_kernel never returns an empty
CIGAR for a region that is not declined) and positions beyond 2^32 (Sink::num's 64-bit branch: tests/test_gpu_bigindex.py)."""
import numpy as np
import pytest

import sam_stage_cases as sc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stage(genome, tmp_path_factory):
    # the reference's library travels with the tree: without it this test fails, it does not skip
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    from mpibwa_amd import api
    lib = api.load_library()
    named = sc.build_named_index(tmp_path_factory.mktemp("named"))
    # (the entry needs the host side of an index only: contig table and .pac; nothing is uploaded)
    return {"lib": lib, "main": (genome["prefix"], api.Engine(genome["prefix"], upload=False), po.RefIndex(genome["prefix"])),
            "named": (named, api.Engine(named, upload=False), po.RefIndex(named))}


class Side:
    """both libraries under one option set; the read group is taken back on the way out"""

    def __init__(self, stage, which, name):
        self.prefix, self.eng, self.ref = stage[which]
        self.lib = stage["lib"]
        self.kw, self.with_qual, self.rg = sc.OPTION_SETS[name]

    def __enter__(self):
        self.opt, self.ropt = self.eng.opt(**self.kw), self.ref.opt(**self.kw)
        if self.kw:
            for lib, o in ((self.lib, self.opt), (self.ref.lib, self.ropt)):
                lib.bwa_fill_scmat(o.contents.a, o.contents.b, o.contents.mat)
        self.rgid = self.ref.set_rg(self.rg)
        assert po.set_rg(self.lib, self.rg) == self.rgid
        self.ix = sc.Index(self.prefix, self.ref.bns)
        return self

    def __exit__(self, *exc):
        self.ref.set_rg(None)
        po.set_rg(self.lib, None)

    def run(self, order, **kw):
        dev = sc.device_side(order, self.opt.contents, self.with_qual)
        return dev, self.eng.sam_records(self.opt, **dev, **kw)

    def want(self, order):
        return sc.reference_side(self.ref, self.ropt, order, self.with_qual)


def check(side, order, text, dev, res, tag, whole_arena=True):
    """-> per pair: 'dev' (both records returned and equal), 'back' (handed back), 'none' (not the device's)"""
    out_len, out_off, arena = res["out_len"], res["out_off"], res["arena"]
    assert (res["guard"] == side.eng.SAM_GUARD_BYTE).all(), (tag, "bytes behind the arena were written", np.nonzero(res["guard"] != side.eng.SAM_GUARD_BYTE)[0][:8])
    state, spans = [], []
    for k, cs in enumerate(order):
        l0, l1 = int(out_len[2 * k]), int(out_len[2 * k + 1])
        if cs["family"] == "not_mine":
            assert (l0, l1) == (-2, -2), (tag, k, l0, l1)
            state.append("none")
            continue
        assert l0 != -2 and l1 != -2 and (l0 < 0) == (l1 < 0) and min(l0, l1) >= -1, (tag, k, cs["family"], cs["tag"], l0, l1)
        if l0 < 0:
            state.append("back")
            continue
        state.append("dev")
        for e, ln in ((0, l0), (1, l1)):
            at = int(out_off[2 * k + e])
            assert at + ln <= min(res["cursor"], res["arena_bytes"]), (tag, k, e, at, ln, res["cursor"], res["arena_bytes"])
            got, exp = arena[at:at + ln].tobytes(), text[2 * k + e]
            assert got == exp, (tag, k, e, cs["family"], cs["tag"], got, exp)
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


def reasons(side, order, text, dev, res):
    """per pair: why the device may hand it back — 'row' (short fields of a record beyond the staging row, by the reference's text),
    'declined' (aln_kernel's header says so), both, or nothing"""
    out = []
    for k, cs in enumerate(order):
        why = set()
        if cs["family"] not in ("not_mine", "unmapped"):
            if max(sc.parse(text[2 * k + e], side.rgid)["short"] for e in range(2)) > sc.SAM_ROW:
                why.add("row")
            b = int(dev["req_base"][k])
            if any(int(res["hdr"]["flags"][b + e]) != 0 for e in range(2)):
                why.add("declined")
        out.append(why)
    return out


def check_exact(side, order, text, dev, res, tag):
    """a launch whose arena holds everything: handed back exactly where there is a reason"""
    state = check(side, order, text, dev, res, tag)
    why = reasons(side, order, text, dev, res)
    for k, cs in enumerate(order):
        if state[k] == "none":
            continue
        assert (state[k] == "back") == bool(why[k]), (tag, k, cs["family"], cs["tag"], state[k], why[k], [int(x) for x in res["out_len"][2 * k:2 * k + 2]])
        if why[k]:
            assert cs["family"] in ("row", "declined"), (tag, k, cs["family"], cs["tag"], why[k])
    return state, why


@pytest.mark.parametrize("name", list(sc.OPTION_SETS))
def test_sam_stage_matches_mem_aln2sam(stage, name):
    with Side(stage, "main", name) as side:
        cases = sc.build_cases(side.ix, side.opt.contents, 1)
        order = sc.shuffled_launch(cases, 2)
        text = side.want(order)
        dev, res = side.run(order)
        state, why = check_exact(side, order, text, dev, res, name)
        # the boundary of the staging row, on both sides: 260 is the device's, 261 goes back
        shorts = [max(sc.parse(text[2 * k + e], side.rgid)["short"] for e in range(2)) if cs["family"] == "row" else 0 for k, cs in enumerate(order)]
        at260 = [k for k, s in enumerate(shorts) if s == sc.SAM_ROW]
        at261 = [k for k, s in enumerate(shorts) if s == sc.SAM_ROW + 1]
        assert at260 and at261 and all(state[k] == "dev" for k in at260) and all(state[k] == "back" for k in at261), (name, at260, at261)
        assert sum(s == "dev" for s, cs in zip(state, order) if cs["family"] == "row") >= 300
        # declined: a band of min(opt.w, > 55) on 251 x 261 bases is beyond the direction matrix aln_kernel keeps (80 columns x (251 + 32) rows)
        n_decl = [k for k, cs in enumerate(order) if cs["family"] == "declined"]
        assert len(n_decl) >= 12 and all("declined" in why[k] for k in n_decl), (name, [why[k] for k in n_decl])
        assert sum(s == "dev" for s in state) >= 1200 and sum(s == "back" for s in state) >= 30

        used = res["cursor"]
        # an arena that is too small: whole waves are handed back, nothing is written outside it or into the room of those waves
        for frac in (0.5, 0.1):
            tag = "%s/arena x %.1f" % (name, frac)
            dev2, small = side.run(order, arena_bytes=int(used * frac))
            st2 = check(side, order, text, dev2, small, tag, whole_arena=False)
            assert small["cursor"] > small["arena_bytes"], tag
            waves = [set(st2[w:w + 32]) - {"none"} for w in range(0, len(order), 32)]
            assert any(w == {"back"} for w in waves) and any("dev" in w for w in waves), tag
            for k, s in enumerate(st2):      # what the full launch handed back stays handed back
                assert not (state[k] == "back" and s == "dev"), (tag, k)
        # three workgroups: every wave walks a third of the batches, its staging rows reused from one batch to the next
        dev3, strided = side.run(order, grid_blocks=3)
        assert len(order) * 2 > 3 * 64 * 8
        st3, _ = check_exact(side, order, text, dev3, strided, name + "/3 blocks")
        assert st3 == state
        # launches of 2, 62, 64 and 66 reads
        for n_pairs in (1, 31, 32, 33):
            few = sc.small_launch(cases, n_pairs, n_pairs)
            d4, r4 = side.run(few)
            check_exact(side, few, side.want(few), d4, r4, "%s/%d pairs" % (name, n_pairs))


def test_sam_stage_when_the_pipeline_arena_is_too_small(stage):
    """254-byte names and a 255-byte read group on 150-bp reads, with the arena the pipeline allots (arena_bytes = 0): too small by
    construction (tests/test_sam_cases.py shows it on the reference's record lengths) — the waves that do not fit are handed back
    whole, the others are byte-identical, nothing is written outside"""
    with Side(stage, "main", "rg255") as side:
        order = sc.arena_launch(sc.build_cases(side.ix, side.opt.contents, 1), 3)
        text = side.want(order)
        dev, res = side.run(order)
        assert res["arena_bytes"] == 2 * len(order) * (2 * 150 + 320) + (1 << 20) < sum(len(t) for t in text)
        state = check(side, order, text, dev, res, "pipeline arena", whole_arena=False)
        assert res["cursor"] > res["arena_bytes"]
        waves = [set(state[w:w + 32]) for w in range(0, len(order), 32)]
        assert sum(w == {"back"} for w in waves) >= 1 and sum(w == {"dev"} for w in waves) >= 1, waves
        assert all(len(w) == 1 for w in waves), "a wave is returned or handed back as a whole"


def test_sam_stage_contig_names(stage):
    """contig names of 1, 64, 65 and 120 bytes as RNAME and as the mate's RNAME (the 64-byte copy loops)"""
    with Side(stage, "named", "default") as side:
        assert [len(x) for x in side.ix.names] == [1, 64, 65, 120]
        order = sc.shuffled_launch(sc.build_cases(side.ix, side.opt.contents, 5), 6)
        dev, res = side.run(order)
        check_exact(side, order, side.want(order), dev, res, "named")
