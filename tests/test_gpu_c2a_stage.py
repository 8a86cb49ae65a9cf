"""Stage test of chain -> alignment regions: c2a_kernel, its chain groups (c2a_groups.hip) and reg_pack_kernel through
mi355x_c2a_batch, against the reference's own mem_chain2aln (oracle/_ref/libbwaref.so) applied chain by chain as mem_align1_core does.

For every option set of tests/c2a_cases.py, natural chains of designed reads (A) and hand-built chains at exact thresholds (B), each in a
launch of its own, go through every variant of the stage: the groups path at thresholds 8 (production), 0 (one wavefront per read) and 1
(every multi-chain read split), early row stops on and off, both slot layouts; then once with early = 2, which must report no extension
whose outputs change.  Every region list must equal the reference's: count, order and every field, frac_rep bit for bit.  The stage
counters must show that the no-DP closed form and the groups path were exercised."""
import ctypes as C

import numpy as np
import pytest

import c2a_cases as cc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

VARIANTS = [(h, e, l) for h in (8, 0, 1) for e in (1, 0) for l in (0, 1)]


@pytest.fixture(scope="module")
def stage(tmp_path_factory, built):
    # the reference's library travels with the tree: without it this test fails, it does not skip
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    from mpibwa_amd import api, simulate
    d = tmp_path_factory.mktemp("c2a_genome")
    names, seqs = simulate.make_genome(240_000, 3, seed=17, repeat_frac=0.35)
    fa = str(d / "r.fa")
    simulate.write_fasta(fa, names, seqs)
    api.build_index(fa, fa)
    lib = api.load_library()
    lib.mi355x_finalize()
    eng = api.Engine(fa, device=0)
    return {"prefix": fa, "seqs": seqs, "eng": eng, "lib": lib}


def _eng_opt(stage, kw):
    eng = stage["eng"]
    opt = eng.opt(**kw)
    if "a" in kw or "b" in kw:
        stage["lib"].bwa_fill_scmat(opt.contents.a, opt.contents.b, opt.contents.mat)
    return opt


def _run(eng, opt, cases, want, tag, **v):
    got, st, units = eng.chain2aln(opt, [r for _, r, _ in cases], [c for _, _, c in cases], **v)
    bad = cc.compare(cases, want, got, "%s %s" % (tag, v))
    assert not bad, "\n".join(bad[:20]) + ("\n... %d more" % (len(bad) - 20) if len(bad) > 20 else "")
    return st, units


@pytest.mark.parametrize("name", list(cc.OPTION_SETS))
def test_c2a_stage_matches_mem_chain2aln(stage, name):
    kw = cc.OPTION_SETS[name]
    ref = cc.Reference(stage["prefix"], kw)
    seqs, eng = stage["seqs"], stage["eng"]
    opt = _eng_opt(stage, kw)
    nat, _ = cc.natural_cases(ref, seqs, np.random.default_rng(5))
    hand = cc.built_cases(ref, seqs, np.random.default_rng(6))
    heavy = any(len(c) > 8 for _, _, c in nat + hand)
    assert heavy
    for label, cases in (("A", nat), ("B", hand)):
        want, _ = cc.reference_side(ref, cases, alone=False)
        tag = "%s/%s" % (name, label)
        for h, e, l in VARIANTS:
            st, units = _run(eng, opt, cases, want, tag, heavy_t=h, early=e, layout=l)
            if h == 8 and e == 1 and any(len(c) > 8 for _, _, c in cases):
                assert units > 1, (tag, units)
            if h == 0:
                assert units == 0, (tag, units)
            if e == 1 and name == "default":
                assert st["n_closed"] > 0, (tag, st)
            if e == 0:
                assert st["n_closed"] == 0, (tag, st)
        st, _ = _run(eng, opt, cases, want, tag, heavy_t=8, early=2, layout=0)
        assert st["n_diff"] == 0 and st["n_ext"] > 0, (tag, st)


def test_c2a_one_mismatch_flanks_go_to_the_dp_when_a_plus_b_is_too_large(stage):
    """with a + b >= min(o) + min(e) (the b9 set) a flank with one mismatch is no longer closed: the family with exactly one mismatch per
    flank gives fewer extensions without DP than under the default scores, and the regions still equal the reference's"""
    seqs, eng = stage["seqs"], stage["eng"]
    closed = {}
    for name in ("default", "b9"):
        kw = cc.OPTION_SETS[name]
        ref = cc.Reference(stage["prefix"], kw)
        nat, _ = cc.natural_cases(ref, seqs, np.random.default_rng(5))
        one = [x for x in nat if x[0] == "one_mm"]
        assert len(one) >= 8
        want, _ = cc.reference_side(ref, one, alone=False)
        st, _ = _run(eng, _eng_opt(stage, kw), one, want, name + "/one_mm", heavy_t=8, early=1, layout=0)
        closed[name] = (st["n_closed"], st["n_ext"])
    assert closed["b9"][0] < closed["default"][0] and closed["default"][0] > 0, closed
