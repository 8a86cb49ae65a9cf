"""Stage test of aln_kernel (mpibwa_amd/csrc/aln_kernel.hip: the CIGAR / MD / NM kernel, all three instantiations) through
mi355x_global_batch against the reference's OWN bwa_gen_cigar2 under mem_reg2aln's loop (oracle/_ref/libbwaref.so), on the cases of
tests/aln_cases.py — tests/test_aln_cases.py shows on the CPU that every family reaches its branch.  Without the reference's library
the tests fail.

For every launch, under both dispatch modes (which = 0: no-DP / narrow band / full size; 1: DP requests straight to the full size):
  * flags of every request equal the restatement's prediction (aln_cases.predict): 0 answered, 1 declined, -1 an unused slot — the entry
    fills the headers with -1, so a live request nobody answered would show;
  * an answered request has the reference's score, NM, every CIGAR word and every MD byte: what oracle/pyoracle.py: reg2aln_loop around
    bwa_gen_cigar2 gives (aln_cases.Rounds.loop) — the loop tests/test_aln_cases.py pins to the reference's own mem_reg2aln, and checks
    against the round-by-round walk that predicts the class;
  * the final lengths of the three request lists equal the predicted ones, and the pool bytes handed out cover the sum of the records;
  * which = 1 gives byte-identical headers, CIGARs and MDs to which = 0.
Nothing is tolerated and no count of declines is "small enough": a decline is predicted with its reason or it is a failure.

The reuse launch repeats distinct short requests until the no-DP list and the DP list are longer than twice the grid launch_aln gives
them (grid_for restated in aln_cases, with the device's CU count), so that every wave walks its list at least twice: the grid-stride
loop, the wave's LDS slice taken over by its next request, and the slabs of the result pool (records that overlap corrupt each other).
Under which = 0 that holds for the no-DP and the narrow instantiation, under which = 1 for the full-size one.
Not covered: the pool-exhaustion branch (the entry sizes the pool for the worst case) and a single record larger than a slab."""
import numpy as np
import pytest

import aln_cases as ac
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stage(genome):
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing: the stage test needs the reference"
    from mpibwa_amd import api
    ri = po.RefIndex.__new__(po.RefIndex)
    ri.lib = po.ref_lib()
    return {"eng": api.Engine(genome["prefix"], device=0), "ri": ri}


def device_cus(stage):
    """the CU count launch_aln sizes its grids by (hipDeviceProp_t::multiProcessorCount), as the library itself reads it"""
    n = stage["eng"].lib.mi355x_device_cus()
    assert n > 0
    return n


def both_opts(stage, o):
    eng, ri = stage["eng"], stage["ri"]
    return ac.apply(eng.opt(), eng.lib.bwa_fill_scmat, o), ac.apply(ri.lib.mem_opt_init(), ri.lib.bwa_fill_scmat, o)


def launch(stage, opt, cs, which):
    eng = stage["eng"]
    hdr, cigs, mds, ms = eng.global_align(opt, cs.l_pac, cs.pac, cs.reads, cs.rb, cs.re, cs.read, cs.qb, cs.qe, cs.w2, cs.truesc, which=which,
                                          cigar_cap=128, md_cap=800)
    return hdr, cigs, mds, eng.global_align_counts()


def compare(label, cs, pred, counts, got):
    hdr, cigs, mds, got_counts = got
    bad = []
    for i, p in enumerate(pred):
        what = (label, i, cs.sub[i], p.cls, p.why)
        if hdr[i, 4] != p.flags:
            bad.append(what + ("flags", int(hdr[i, 4]), p.flags))
        elif p.flags == 0:
            sc, cig, nm, md = p.result
            if (hdr[i, 0], hdr[i, 1]) != (sc, nm) or len(cigs[i]) != len(cig) or (cigs[i] != cig).any() or mds[i] != md:
                bad.append(what + (list(hdr[i]), sc, nm, list(cigs[i][:8]), list(cig[:8]), mds[i][:40], md[:40]))
        elif p.flags == -1 and not (hdr[i] == -1).all():
            bad.append(what + ("header of an unused slot", list(hdr[i])))
    assert not bad, (len(bad), bad[:4])
    assert got_counts[:3] == counts, (label, got_counts, counts)
    assert got_counts[3] >= sum(p.need for p in pred), (label, got_counts)


def check(stage, o, cs, label):
    """both dispatch modes against the prediction, and against each other; the prediction of which = 0"""
    opt, ropt = both_opts(stage, o)
    rounds = ac.Rounds(stage["ri"], ropt, cs)
    ac.fix_truesc(cs, o, rounds)
    got, preds = {}, {}
    for which in (0, 1):
        preds[which], counts = ac.predict(cs, o, rounds, which)
        got[which] = launch(stage, opt, cs, which)
        compare((label, which), cs, preds[which], counts, got[which])
    assert (got[0][0] == got[1][0]).all(), label
    assert all((a == b).all() for a, b in zip(got[0][1], got[1][1])) and got[0][2] == got[1][2], label
    return preds[0]


@pytest.mark.parametrize("name", list(ac.OPTION_SETS))
def test_families_a_b_c_f_under_every_option_set(stage, name):
    """the no-DP bound, the loop conditions, the band arithmetic, strand and placement"""
    o, cs = ac.cases(name)
    pred = check(stage, o, cs, name)
    assert all(p.flags == 0 for i, p in enumerate(pred) if cs.sub[i] not in ("f.bridging", "f.empty", "f.overlong"))


@pytest.mark.parametrize("max_len", [150, 250, 700])
@pytest.mark.parametrize("name", ac.WIDE_SETS)
def test_capacity_edges(stage, name, max_len):
    """n_col * rlen at aln_zcap_small / aln_zcap of the batch's longest read and one row more; the restart by the full-size instantiation.
    700 bp: the full-size instantiation's LDS is beyond 64 KB (hipFuncSetAttribute)"""
    o, cs = ac.cases_d(name, max_len)
    assert cs.max_len == max_len and (ac.lds_bytes(max_len)[2] > 64 * 1024) == (max_len == 700)
    pred = check(stage, o, cs, (name, max_len))
    by = {s: {pred[i].cls for i in range(len(cs)) if cs.sub[i] == s} for s in set(cs.sub)}
    assert by["d.small.at"] == {"narrow"} and by["d.small.over"] == {"full"} and by["d.full.at"] == {"full"} and by["d.full.over"] == {"declined"}, by


@pytest.mark.parametrize("name", ac.WIDE_SETS)
def test_output_capacities(stage, name):
    """96 / 97 CIGAR operations, 768 / 769 MD bytes, deletions and insertions at the ends"""
    o, cs = ac.cases_e(name)
    check(stage, o, cs, name)


@pytest.mark.parametrize("name", ac.WIDE_SETS)
def test_launch_shapes(stage, name):
    """launches of 1 .. 257 requests, and one whose classify waves hold 0, 1, 63 and 64 members of a kind between unused slots"""
    o, cs, order = ac.cases_g(name)
    for n in ac.LAUNCH_SIZES:
        check(stage, o, cs.order(range(n)), (name, n))
    mixed = ac.with_unused(cs, order)
    pred = check(stage, o, mixed, (name, "interleaved"))
    assert sum(p.flags == -1 for p in pred) >= 64 + 40


@pytest.mark.parametrize("name", ac.WIDE_SETS)
def test_every_wave_takes_a_second_request(stage, name):
    """the grid-stride loop, the reuse of a wave's LDS slice, the slabs of the result pool"""
    cus = device_cus(stage)
    o, cs = ac.cases_reuse(name)
    opt, ropt = both_opts(stage, o)
    rounds = ac.Rounds(stage["ri"], ropt, cs)
    got = {}
    for which in (0, 1):
        pred, _ = ac.predict(cs, o, rounds, which)
        order = ac.reuse_order(cs, pred, cus)
        big = cs.order(order)
        pbig = [pred[i] for i in order]
        counts = [sum(p.lists[k] for p in pbig) for k in range(3)]
        lds = ac.lds_bytes(cs.max_len)
        grids = [ac.grid_for(lds[k], cus, len(big)) for k in range(3)]
        assert lds[2] > 64 * 1024 and counts[0] > 2 * grids[0], (counts, grids)
        assert counts[2 if which else 1] > 2 * grids[2 if which else 1], (counts, grids)
        needs = sorted({p.need for p in pbig})
        assert needs[0] < 16 and needs[-1] > ac.ALN_SLAB // 2 and sum(p.need for p in pbig) > 40 * ac.ALN_SLAB
        got[which] = launch(stage, opt, big, which)
        compare((name, "reuse", which), big, pbig, counts, got[which])
    assert (got[0][0] == got[1][0]).all()
    assert all((a == b).all() for a, b in zip(got[0][1], got[1][1])) and got[0][2] == got[1][2]
