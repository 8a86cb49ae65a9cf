"""Designed stage test of pair_simple_kernel (mpibwa_amd/csrc/pair_kernel.hip) through mi355x_pair_stage_batch, against the reference's
OWN mem_sam_pe (oracle/_ref/libpairinj.so: oracle/pair_inject.c) on the cases of tests/pair_stage_cases.py — tests/test_pair_stage_cases.py
shows on the CPU that every case falls where its `expect` says.  tests/test_pair_stage.py stays the random counterpart.

Per option set, and per set of insert-size statistics its cases run under, ONE shuffled launch:
  * status == expect for every case that names a code — no share and no floor: in a designed family every case has its code;
  * a decided pair is one the reference reports through its paired branch without rescue alignment and without XA, and its two
    descriptors and requests say what the reference's lines say: region, contig, flag, MAPQ, score, sub, truesc, and the band of
    tests/ref_band.py; the pair without any hit has its two unmapped records (flags 77 / 141, req -3, rid -1, no request);
  * every other pair is marked as the host's: both requests are the empty one (read -1), both descriptors have req -1;
  * nothing is written behind pair n - 1: status, descriptors and requests come back whole, with room for a workgroup more than the
    grid covers, and keep the pattern they were filled with;
  * launches of the first and of the last 1, 63, 64, 65 and 129 pairs of the list (the `tie` family stands last; the launch's first pair
    number is shifted so that every pair keeps its number) give what the full launch gave.
pair_ok = 0 gives code 2 and the host's marks, the rest of the descriptors untouched, and changes nothing for the other pairs.  The `tie`
family also runs at pair numbers on both sides of 2^23 and 2^31."""
import numpy as np
import pytest

import pair_stage_cases as psc
from oracle import pyoracle as po
from ref_band import reg2aln_band

pytestmark = pytest.mark.gpu

ID0 = 1234
FILL = 0xA5


@pytest.fixture(scope="module")
def stage(genome):
    # the reference's libraries travel with the tree: without them this test fails, it does not skip
    assert po.ref_available() and po.pair_inject_available(), "oracle/_ref/libbwaref.so or libpairinj.so is missing"
    from mpibwa_amd import api
    lib = api.load_library()
    assert hasattr(lib, "mi355x_pair_stage_batch") and hasattr(lib, "mi355x_pair_stage_room")
    ref = po.RefIndex(genome["prefix"])
    return {"lib": lib, "eng": api.Engine(genome["prefix"], upload=False), "ref": ref, "ix": psc.Geometry(ref.bns), "seqs": genome["seqs"], "sets": {}}


class Side:
    """both libraries under one option set, and the set's cases (built once per set, left unchanged)"""

    def __init__(self, stage, name):
        self.name, self.eng, self.ref, self.ix = name, stage["eng"], stage["ref"], stage["ix"]
        kw = psc.OPTION_SETS[name]["kw"]
        self.opt = psc.set_options(stage["lib"], self.eng.opt(**kw), name)
        self.ropt = psc.set_options(self.ref.lib, self.ref.opt(**kw), name)
        self.maxreg = int(stage["lib"].mi355x_pair_maxreg())
        self.max_len = psc.max_len_of(name)
        if name not in stage["sets"]:
            fams = psc.OPTION_SETS[name]["families"] or psc.FAMILIES
            lists = psc.patch_lists(self.ref, self.ropt, stage["seqs"], self.maxreg) if "dedup" in fams else ()
            stage["sets"][name] = psc.by_stats(psc.build_cases(self.ix, self.ropt.contents, name, lists))
        self.launches = stage["sets"][name]

    def decide(self, order, pes, id0, pair_ok=None):
        regs, n_regs = psc.device_regions(order, self.eng.REG_DT, self.maxreg)
        return self.eng.pairs_stage(self.opt, psc._pes(psc.STATS[pes]), regs, n_regs, pair_ok=pair_ok, max_len=self.max_len, n_processed=2 * id0, fill=FILL)

    def want(self, order, id0):
        return psc.reference_side(self.ref, self.ropt, order, id0)


def pattern(a):
    return bool((np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8) == FILL).all())


def check_launch(side, order, want, out, tag, pair_ok=None):
    """everything the module's docstring says of one launch -> the number of decided pairs"""
    status, desc, req = out
    n = len(order)
    o = side.ropt.contents
    room = (n + 63) // 64 * 64 + 64
    assert len(status) == room and len(desc) == 2 * room and len(req) == 2 * room, (tag, n, len(status))
    assert pattern(status[n:]) and pattern(desc[2 * n:]) and pattern(req[2 * n:]), (tag, "written behind the last pair")
    n_decided = 0
    for k, cs in enumerate(order):
        where = (tag, k, cs["family"], cs["tag"], int(status[k]))
        d2, q2, w = desc[2 * k:2 * k + 2], req[2 * k:2 * k + 2], want[k]
        if status[k] != psc.PR_DECIDED:      # the host's pair: the empty request twice, req -1 twice
            for e in range(2):
                assert int(d2[e]["req"]) == -1 and int(q2[e]["read"]) == -1, where
                assert all(int(q2[e][f]) == 0 for f in ("rb", "re", "qb", "qe", "w2", "truesc", "pad")), (where, q2[e])
        if pair_ok is not None and not pair_ok[k]:
            assert status[k] == psc.PR_HOST_NO_HIT, where
            for e in range(2):      # nothing of the descriptor but req is written
                assert all(pattern(d2[e:e + 1][f]) for f in d2.dtype.names if f != "req"), (where, d2[e])
            continue
        if cs["expect"] is not None:
            assert status[k] == cs["expect"], (where, "expected", cs["expect"], {f: v for f, v in w.items() if f != "lines"})
        if status[k] != psc.PR_DECIDED:
            continue
        n_decided += 1
        if len(cs["regs0"]) == 0 and len(cs["regs1"]) == 0:
            assert not w["paired"] and w["n_reg2aln"] == 0, where
            for e in range(2):
                d = d2[e]
                assert (int(d["flag"]), int(d["req"]), int(d["rid"]), int(d["mapq"]), int(d["score"]), int(d["sub"])) == ((77, 141)[e], -3, -1, 0, 0, 0), (where, d)
                assert (int(d["rb"]), int(d["re"]), int(d["qb"]), int(d["qe"])) == (0, 0, 0, 0) and int(q2[e]["read"]) == -1, (where, d, q2[e])
            continue
        assert psc.is_plain(w), (where, "the kernel decided a pair the reference treats otherwise", w)
        assert max(len(cs["regs0"]), len(cs["regs1"])) <= side.maxreg, where
        for e in range(2):
            d, q, L = d2[e], q2[e], w["lines"][e]
            got = {f: int(d[f]) for f in ("rb", "re", "qb", "qe", "score", "sub", "flag", "mapq")}
            assert got == {f: L[f] for f in got}, (where, e, got, L)
            assert int(d["req"]) == e and int(d["rid"]) == side.ix.rid_of(L["rb"], L["re"] - L["rb"]), (where, e, d)
            w2 = reg2aln_band(o, L["qe"] - L["qb"], L["re"] - L["rb"], L["truesc"], L["w"])
            assert (int(q["rb"]), int(q["re"]), int(q["read"]), int(q["qb"]), int(q["qe"]), int(q["w2"]), int(q["truesc"]), int(q["pad"])) == \
                   (L["rb"], L["re"], 2 * k + e, L["qb"], L["qe"], w2, L["truesc"], 0), (where, e, q, L, w2)
    return n_decided


def same_as(full, part, start, n):
    """the launch of pairs [start, start + n) of a list gave what the full launch gave for them (a request names its read by its place
    in the launch)"""
    status, desc, req = full
    s, d, q = part
    if not (s[:n] == status[start:start + n]).all():
        return False
    shifted = req[2 * start:2 * (start + n)].copy()
    shifted["read"] = np.where(shifted["read"] >= 0, shifted["read"] - 2 * start, shifted["read"])
    return d[:2 * n].tobytes() == desc[2 * start:2 * (start + n)].tobytes() and q[:2 * n].tobytes() == shifted.tobytes()


@pytest.mark.parametrize("name", list(psc.OPTION_SETS))
def test_pair_stage_codes_and_fields(stage, name):
    side = Side(stage, name)
    for pes, cases in side.launches.items():
        tag = "%s/%s" % (name, pes)
        order = psc.shuffled(cases, last="tie")
        want = side.want(order, ID0)
        out = side.decide(order, pes, ID0)
        n_decided = check_launch(side, order, want, out, tag)
        codes = {int(c): int((out[0][:len(order)] == c).sum()) for c in np.unique(out[0][:len(order)])}
        print(tag, "pairs", len(order), "decided", n_decided, "status codes", codes)
        if name != "default":
            continue
        # launches of a few pairs: the head of the list, and its tail (where the `tie` family stands) under the numbers it had
        N = len(order)
        for n in (1, 63, 64, 65, 129):
            if n > N:
                continue
            for start in (0, N - n):
                part = side.decide(order[start:start + n], pes, ID0 + start)
                check_launch(side, order[start:start + n], want[start:start + n], part, "%s/%d pairs from %d" % (tag, n, start))
                assert same_as(out, part, start, n), (tag, n, start)


def test_pair_ok_and_what_is_left_untouched(stage):
    side = Side(stage, "default")
    order = psc.shuffled(side.launches["FR"], last="tie")
    want = side.want(order, ID0)
    full = side.decide(order, "FR", ID0)
    rng = np.random.default_rng(psc.SHUFFLE_SEED + 1)
    ok = (rng.random(len(order)) >= 0.2).astype(np.uint8)
    ok[:3] = (0, 1, 0)
    assert 50 < int((ok == 0).sum()) < len(order) // 2
    out = side.decide(order, "FR", ID0, pair_ok=ok)
    check_launch(side, order, want, out, "pair_ok", pair_ok=ok)
    # the pairs the host did pass: as in the launch where it passed them all
    keep = np.flatnonzero(ok)
    assert (out[0][keep] == full[0][keep]).all()
    both = np.stack([2 * keep, 2 * keep + 1], axis=1).reshape(-1)
    assert out[1][both].tobytes() == full[1][both].tobytes() and out[2][both].tobytes() == full[2][both].tobytes()


@pytest.mark.parametrize("id0", [0, (1 << 23) - 40, (1 << 31) - 40])
def test_tie_family_across_pair_numbers(stage, id0):
    """n_processed = 2 id0: the pair numbers of each launch pass 2^23, where the reference's `id << 8` on an int is undefined, and 2^31,
    where its int wraps; the reference is compiled as it is (tests/test_pair_stage_cases.py compares it with the pinned arithmetic)"""
    side = Side(stage, "default")
    for pes, cases in side.launches.items():
        ties = psc.shuffled([cs for cs in cases if cs["family"] == "tie"])
        if not ties:
            continue
        assert len(ties) >= 80
        want = side.want(ties, id0)
        out = side.decide(ties, pes, id0)
        assert check_launch(side, ties, want, out, "tie/%s from %d" % (pes, id0)) == len(ties)
        qb = [w["lines"][1 - cs["anchor"]]["qb"] for cs, w in zip(ties, want)]
        assert min(qb.count(0), qb.count(75)) >= 10, (pes, id0, qb)      # (either hit wins some: the hash decides, not the order)
