"""The library's host chaining (host_chain.cpp: the reads the chaining kernels decline — more than 4 096 seeds, two chains at one
position, long enough for mem_flt_chained_seeds to act — and every read under MPIBWA_HOST_CHAIN=1) against the reference's own
mem_chain + mem_chain_flt (src/bwamem.c:251-385) on adversarial seed sets, and the contig bounds and reference window it hands to the
extension against the model of mem_chain2aln's lines (tests/window_model.py); no GPU involved (mi355x_chain_batch with which = 1 is
host code of the product)."""
import numpy as np
import pytest

import window_model

from oracle import pyoracle as po


@pytest.mark.skipif(not po.chain_inject_available(), reason="oracle/_ref/libchaininj.so not present")
def test_host_chaining_matches_the_reference_mem_chain(genome):
    from mpibwa_amd import api
    from chain_cases import adversarial_interval_sets, reference_chains
    eng = api.Engine(genome["prefix"], upload=False)
    ref = po.RefIndex(genome["prefix"])
    l_pac = int(eng.bns.contents.l_pac)
    n_seqs = int(eng.bns.contents.n_seqs)
    offs = [int(eng.bns.contents.anns[k].offset) for k in range(n_seqs)] + [l_pac]
    for kw in (dict(), dict(mask_level=0.3, drop_ratio=0.8, max_chain_gap=200), dict(min_chain_weight=40, w=10)):
        rng = np.random.default_rng(5)
        lens, seedsets, want = reference_chains(ref, ref.opt(**kw), adversarial_interval_sets(rng, 1500, l_pac, offs, n_seqs))
        host = eng.chains(eng.opt(**kw), lens, [0] * len(lens), seedsets, 1)
        for h, w, sd in zip(host, want, seedsets):
            assert [(c[0], c[5], c[6]) for c in h] == w, (kw, sd)
        window_model.ChainWindows(eng.bns, eng.opt(**kw)).check(lens, want, host, kw)
        assert sum(len(w) > 9 for w in want) > 5 and sum(len(s) > 64 for s in seedsets) > 20


@pytest.mark.skipif(not po.chain_inject_available(), reason="oracle/_ref/libchaininj.so not present")
def test_host_chain_filter_on_reads_of_high_copy_repeats(genome):
    """Hundreds of equal-weight chains that overlap completely: mem_chain_flt's kept list grows with every chain (the library
    scans it as columns of ints, host_chain.cpp: chain_filter); max_occ raised so that every hit is a seed, as a user's -c does."""
    from mpibwa_amd import api
    from chain_cases import repeat_like_interval_sets, reference_chains
    eng = api.Engine(genome["prefix"], upload=False)
    ref = po.RefIndex(genome["prefix"])
    l_pac = int(eng.bns.contents.l_pac)
    n_seqs = int(eng.bns.contents.n_seqs)
    offs = [int(eng.bns.contents.anns[k].offset) for k in range(n_seqs)] + [l_pac]
    for kw in (dict(max_occ=1000), dict(max_occ=1000, mask_level=0.3, drop_ratio=0.8), dict(max_occ=1000, min_chain_weight=25, max_chain_extend=50)):
        rng = np.random.default_rng(11)
        lens, seedsets, want = reference_chains(ref, ref.opt(**kw), repeat_like_interval_sets(rng, 40, l_pac, offs, n_seqs))
        host = eng.chains(eng.opt(**kw), lens, [0] * len(lens), seedsets, 1)
        for h, w, sd in zip(host, want, seedsets):
            assert [(c[0], c[5], c[6]) for c in h] == w, kw
        window_model.ChainWindows(eng.bns, eng.opt(**kw)).check(lens, want, host, kw)
        assert max(len(sd) for sd in seedsets) > 500 and max(len(w) for w in want) >= 30   # hundreds of chains in, the cap of max_chain_extend out


@pytest.mark.skipif(not po.chain_inject_available(), reason="oracle/_ref/libchaininj.so not present")
def test_host_chain_sort_on_reads_that_reach_the_comb_sort(genome):
    """Chains that arrive at mem_chain_flt's sort in the order that spends ks_introsort's depth budget (chain_cases.sorted_tail_chain_sets;
    tests/test_introsort_model.py shows that they do): the order of equal weights is the comb sort's.  Under the default options every
    chain comes back; under the second set some are dropped and the kept ones must still stand in the reference's order."""
    from mpibwa_amd import api
    import chain_cases as cc
    eng = api.Engine(genome["prefix"], upload=False)
    ref = po.RefIndex(genome["prefix"])
    l_pac = int(eng.bns.contents.l_pac)
    n_seqs = int(eng.bns.contents.n_seqs)
    offs = [int(eng.bns.contents.anns[k].offset) for k in range(n_seqs)] + [l_pac]
    cases = cc.sorted_tail_chain_sets(np.random.default_rng(cc.SORTED_TAIL_SEED), cc.SORTED_TAIL_SIZES, l_pac, offs, n_seqs)
    for kw in (dict(), dict(mask_level=0.3, drop_ratio=0.8)):
        lens, seedsets, want = cc.reference_chains(ref, ref.opt(**kw), cases)
        host = eng.chains(eng.opt(**kw), lens, [0] * len(lens), seedsets, 1)
        n_all = 0
        for h, w, sd in zip(host, want, seedsets):
            assert [(c[0], c[5], c[6]) for c in h] == w, (kw, len(sd), len(w))
            n_all += len(w) == len(sd)
        window_model.ChainWindows(eng.bns, eng.opt(**kw)).check(lens, want, host, kw)
        print(kw, "reads", len(want), "with every chain kept", n_all)
        assert n_all == (len(cases) if not kw else 0), (kw, n_all)
