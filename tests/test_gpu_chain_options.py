"""chain_kernel<16, 4>, <64, 9>, <255, 9> and chain_heavy_kernel<256 / 1024 / 2048 / 4096> under every option they read (ChainParams: w,
max_chain_gap, min_chain_weight, min_seed_len, max_chain_extend, mask_level, drop_ratio), through engine.chains against the reference's
own mem_chain + mem_chain_flt (oracle/chain_inject.c) on the reads of tests/chain_option_cases.py.  tests/test_chain_option_cases.py shows
on the CPU that the option decides the reference's answer on enough reads of every launch class; the floors are asserted here again from
what is actually sent."""
import numpy as np
import pytest

import chain_option_cases as oc
import window_model
from mpibwa_amd import abi, simulate
from oracle import pyoracle as po

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not po.chain_inject_available(), reason="oracle/_ref/libchaininj.so not present")]


@pytest.fixture(scope="module")
def engine(genome):
    from mpibwa_amd import api
    api.load_library().mi355x_finalize()     # (the device index is a process-wide singleton: this module's genome)
    return api.Engine(genome["prefix"], device=0)


@pytest.fixture(scope="module")
def ref(genome):
    return po.RefIndex(genome["prefix"])


def _check(engine, kw, ev, what, l_rep=None):
    """one batch through the device; every read answered, every chain the reference's, in its order.  l_rep given: frac_rep is
    float32(l_rep) / float32(read length) on every chain (the reference's injected intervals have l_rep = 0)"""
    n = len(ev.lens)
    dev = engine.chains(engine.opt(**kw), ev.lens, [0] * n if l_rep is None else l_rep, ev.seedsets, 0)
    n_chains = 0
    for k, (d, w, sd) in enumerate(zip(dev, ev.want, ev.seedsets)):
        assert d is not None, (what, k, ev.klass[k], len(sd), "declined")
        if l_rep is not None:
            fb = int((np.float32(l_rep[k]) / np.float32(ev.lens[k])).view(np.uint32))
            w = [(rid, fb, seeds) for rid, _, seeds in w]
        dd = [(c[0], c[5], c[6]) for c in d]
        assert dd == w, (what, k, ev.klass[k], len(sd), len(dd), len(w), [(a, b) for a, b in zip(dd, w) if a != b][:2])
        n_chains += len(w)
    # ... and its contig bounds and reference window those of mem_chain2aln on the reference's chain, under this option set's gap table
    window_model.ChainWindows(engine.bns, engine.opt(**kw)).check(ev.lens, ev.want, dev, what)
    return n_chains


@pytest.mark.parametrize("name", list(oc.OPTION_SETS))
def test_chain_kernels_match_the_reference_under_the_option(engine, ref, genome, name):
    """(a) No read is declined (no two seeds at one position, at most 4 096 seeds, 151 bases: mem_flt_chained_seeds is a no-op); a read
    the reference leaves without a chain comes back as an empty list."""
    cases, base = oc.evaluated(ref, genome["prefix"], "default")
    _, ev = oc.evaluated(ref, genome["prefix"], name)
    n_class, n_sens = oc.check_floors(name, ev, base)
    print(name, "reads per class", n_class, "on which the option decides", n_sens)
    assert None not in ev.klass and all(n_class[k] >= oc.HEAVY_FLOOR for k in oc.CLASSES), n_class
    for (fam, (lq, ivs)), sd in zip(cases, ev.seedsets):
        assert len({s[0] for s in sd}) == len(sd) <= 4096 and lq == oc.LQ, (fam, "two seeds at one position")
    if "min_chain_weight" in oc.OPTION_SETS[name]:
        empty = [ev.klass[k] for k, w in enumerate(ev.want) if not w]
        assert sum(c in oc.LANE for c in empty) >= 3 and sum(c in oc.HEAVY for c in empty) >= 3, empty
    _check(engine, oc.OPTION_SETS[name], ev, name)


@pytest.mark.parametrize("name", ["default", "combined"])
def test_frac_rep_of_a_nonzero_l_rep(engine, ref, genome, name):
    """(b) l_rep uniform in [1, read length) per read: frac_rep's bits against float32 division, every other field against the reference"""
    _, ev = oc.evaluated(ref, genome["prefix"], name)
    rng = np.random.default_rng(4103)
    l_rep = [int(rng.integers(1, lq)) for lq in ev.lens]
    assert _check(engine, oc.OPTION_SETS[name], ev, name + " with l_rep", l_rep) > 1000


def test_device_steps_aside_where_mem_flt_chained_seeds_acts(engine, ref, genome):
    """(c) min_chain_weight = 5 and 151 bases: 1.1f * 5 = 5.5 <= 0.05f * 151 = 7.55, mem_flt_chained_seeds (src/bwamem.c:600-602) goes on,
    and the device declines every read of every launch class; the host path equals the reference on them.  min_chain_weight = 7:
    7.7 > 7.55, no read is declined."""
    _, ev = oc.evaluated(ref, genome["prefix"], "weight5", kw=dict(min_chain_weight=5))
    n_class = ev.count()
    assert all(n_class[k] >= oc.HEAVY_FLOOR for k in oc.CLASSES) and all(len(sd) > 0 for sd in ev.seedsets), n_class
    n = len(ev.lens)
    dev = engine.chains(engine.opt(min_chain_weight=5), ev.lens, [0] * n, ev.seedsets, 0)
    not_declined = [(k, ev.klass[k]) for k, d in enumerate(dev) if d is not None]
    assert not not_declined, (len(not_declined), not_declined[:5])
    host = engine.chains(engine.opt(min_chain_weight=5), ev.lens, [0] * n, ev.seedsets, 1)
    for k, (h, w) in enumerate(zip(host, ev.want)):
        assert [(c[0], c[5], c[6]) for c in h] == w, ("host path", k, ev.klass[k])
    window_model.ChainWindows(engine.bns, engine.opt(min_chain_weight=5)).check(ev.lens, ev.want, host, "host path")
    _, ev7 = oc.evaluated(ref, genome["prefix"], "weight7", kw=dict(min_chain_weight=7))
    _check(engine, dict(min_chain_weight=7), ev7, "min_chain_weight=7")


def test_windows_cut_at_contig_edges_and_at_the_strand_boundary(engine, ref, genome):
    """(c2) the reads of oc.edge_cases (tests/test_chain_option_cases.py shows that their windows are cut where they are meant to be), in
    chain_kernel<16, 4> and in chain_heavy_kernel<256>"""
    _, ev = oc.evaluated(ref, genome["prefix"], "default", oc.edge_cases)
    assert set(ev.klass) == {"lane16x4", "heavy256"}
    _check(engine, {}, ev, "edges")


@pytest.mark.parametrize("name", oc.ALT_SETS)
def test_alt_contigs_in_the_filter(genome_alt, engine, name):
    """(d) ann_alt with ALT contigs: reads in which a kept primary chain lies under a heavier ALT chain, and the opposite nesting
    (counted from the reference's own w, is_alt and seeds), then device == reference.  (engine.chains takes the contig table from
    the index it is given, not from the resident one.)"""
    from mpibwa_amd import api
    ref_alt = po.RefIndex(genome_alt["prefix"])
    eng_alt = api.Engine(genome_alt["prefix"], upload=False)
    flags = [[int(x.bns.contents.anns[i].is_alt) for i in range(x.bns.contents.n_seqs)] for x in (eng_alt, ref_alt)]
    assert flags[0] == flags[1] and sum(flags[0]) == len(genome_alt["alt"])
    n = oc.alt_coverage(ref_alt, genome_alt["prefix"], name)
    print(name, n)
    oc.check_alt_coverage(name, n)
    cases, ev = oc.evaluated(ref_alt, genome_alt["prefix"], name, oc.alt_cases)
    for (fam, _), sd in zip(cases, ev.seedsets):
        assert len({s[0] for s in sd}) == len(sd), (fam, "two seeds at one position")
    _check(eng_alt, oc.OPTION_SETS[name], ev, "alt " + name)


@pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref/libbwaref.so not present")
@pytest.mark.parametrize("kw", [dict(max_chain_extend=3, min_chain_weight=30, w=20, max_chain_gap=100), dict(min_chain_weight=5)])
def test_whole_call_under_chaining_options(engine, ref, reads_pe, kw):
    """(e) mem_process_seqs on pairs, SAM against the reference's; under min_chain_weight = 5 every read of 150 bases takes the host
    chaining with mem_flt_chained_seeds live"""
    reads = simulate.reads_to_ascii(reads_pe)
    kw = dict(kw, flag=abi.MEM_F_PE)
    want = ref.process(ref.opt(**kw), reads)
    got = engine.process(engine.opt(**kw), reads)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (kw, i, a[:300], b[:300])
