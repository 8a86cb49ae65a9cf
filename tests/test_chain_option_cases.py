"""CPU companion of tests/test_gpu_chain_options.py: the generators of tests/chain_option_cases.py and the reference's own mem_chain +
mem_chain_flt alone, no GPU.  Under every option set the reads must be ones on which the option decides the reference's answer, in every
launch class of the chaining kernels, so that the device test cannot pass without entering the branches the option guards; and the
library's host chaining (host_chain.cpp, mi355x_chain_batch with which = 1: host code of the product) must equal the reference on all of
them, field for field."""
import numpy as np
import pytest

import chain_option_cases as oc
import window_model
from oracle import pyoracle as po

pytestmark = pytest.mark.skipif(not po.chain_inject_available(), reason="oracle/_ref/libchaininj.so not present")


@pytest.fixture(scope="module")
def ref(genome):
    return po.RefIndex(genome["prefix"])


@pytest.fixture(scope="module")
def host(genome):
    from mpibwa_amd import api
    return api.Engine(genome["prefix"], upload=False)


def _table(name, n_class, n_sens):
    return "%-15s " % name + "  ".join("%s %d/%d" % (k, n_sens[k], n_class[k]) for k in oc.CLASSES)


def test_no_read_has_two_seeds_at_one_position(ref, genome):
    cases, _ = oc.evaluated(ref, genome["prefix"], "default")
    for fam, (lq, ivs) in cases:
        pos = [p for _, _, hits in ivs for p in hits]
        assert len(set(pos)) == len(pos), (fam, "two seeds at one position")
        assert len(set((qb, qe) for qb, qe, _ in ivs)) == len(ivs) and all(0 <= qb and qe <= lq and len(h) <= oc.MAX_HITS for qb, qe, h in ivs)
        assert min(pos) >= 0 and max(p + qe - qb for qb, qe, hits in ivs for p in hits) <= 2 * oc.Geometry(ref.bns).l_pac
        assert len(pos) <= 4096


@pytest.mark.parametrize("name", list(oc.OPTION_SETS))
def test_the_option_decides_the_reference_answer_in_every_class(ref, genome, name):
    """sensitive reads / reads per launch class (the table goes to the log), and the branches only some options reach"""
    cases, base = oc.evaluated(ref, genome["prefix"], "default")
    _, ev = oc.evaluated(ref, genome["prefix"], name)
    assert None not in ev.klass
    n_class, n_sens = oc.check_floors(name, ev, base)
    print(_table(name, n_class, n_sens))
    kw = oc.OPTION_SETS[name]
    empty = [k for k, w in enumerate(ev.want) if len(w) == 0 and len(ev.seedsets[k]) > 0]
    if "min_chain_weight" in kw:
        # reads the filter leaves with no chain (the kernels' `n == 0` exits), in a lane's launch and in chain_heavy_kernel
        assert sum(ev.klass[k] in oc.LANE for k in empty) >= 3 and sum(ev.klass[k] in oc.HEAVY for k in empty) >= 3, (name, len(empty))
    if list(kw) == ["max_chain_extend"]:
        # the cut removes chains the pairwise pass had kept: the answer is the default one less some chains, in its order
        cut = dict.fromkeys(oc.CLASSES, 0)
        for k, (a, b) in enumerate(zip(ev.want, base.want)):
            assert [c for c in b if c in a] == a, (name, k)
            cut[ev.klass[k]] += len(a) < len(b)
        print(name, "reads with a chain cut", cut)
        assert all(cut[c] >= 1 for c in oc.CLASSES if oc.floor(name, c)), (name, cut)
    # chain_heavy_kernel's reads keep chains of several seeds (the existing tests of its classes merge no seed)
    multi = dict.fromkeys(oc.HEAVY, 0)
    for k, w in enumerate(ev.want):
        if ev.klass[k] in oc.HEAVY:
            multi[ev.klass[k]] += any(len(c[2]) > 1 for c in w)
    print(name, "heavy reads that keep a chain of several seeds", multi)
    assert all(multi[c] >= 2 for c in oc.HEAVY), (name, multi)


@pytest.mark.parametrize("name", list(oc.OPTION_SETS))
def test_host_chaining_matches_the_reference_under_the_option(ref, host, genome, name):
    _, ev = oc.evaluated(ref, genome["prefix"], name)
    got = host.chains(host.opt(**oc.OPTION_SETS[name]), ev.lens, [0] * len(ev.lens), ev.seedsets, 1)
    for k, (h, w) in enumerate(zip(got, ev.want)):
        hh = [(c[0], c[5], c[6]) for c in h]
        assert hh == w, (name, k, ev.klass[k], len(ev.seedsets[k]), len(hh), len(w), [(a, b) for a, b in zip(hh, w) if a != b][:2])
    window_model.ChainWindows(host.bns, host.opt(**oc.OPTION_SETS[name])).check(ev.lens, ev.want, got, name)


def test_windows_clamp_at_contig_edges_and_at_the_strand_boundary(ref, host, genome):
    """The reads of oc.edge_cases: a chain within 100 bases of a contig's first and last base and of l_pac, on both strands, in a lane's
    launch and in chain_heavy_kernel<256>.  Its window is cut at the contig's edge on either side and on either strand, and at the strand
    boundary from either strand (the other reads lie 500 bases clear of both: none of their windows is cut); the host chaining hands
    out the model's windows for them."""
    cases, ev = oc.evaluated(ref, genome["prefix"], "default", oc.edge_cases)
    win = window_model.ChainWindows(ref.bns, ref.opt())
    cut = {}
    for (fam, _), lq, w, klass in zip(cases, ev.lens, ev.want, ev.klass):
        at_edge = [(rid, seeds) for rid, _, seeds in w if any(win.clamps(lq, rid, seeds))]
        assert len(at_edge) == 1 and len(at_edge[0][1]) == 2 and klass in ("lane16x4", "heavy256"), (fam, klass, len(w))
        rid, seeds = at_edge[0]
        fb, fe, r0, r1 = win.of(lq, rid, seeds)
        contig, strand = win.clamps(lq, rid, seeds)
        rev = seeds[0][0] >= win.l_pac
        assert rev == fam.endswith("rev") and contig and (r0 == fb if fam.startswith("first") != rev else r1 == fe), (fam, fb, fe, r0, r1)
        if fam.startswith("boundary"):
            assert strand and (r0 == win.l_pac if rev else r1 == win.l_pac), (fam, r0, r1)
        cut[fam, klass] = cut.get((fam, klass), 0) + 1
    assert cut == {(f, k): len(oc.EDGE_DIST) for f in oc.EDGE_FAMILIES for k in ("lane16x4", "heavy256")}, cut
    _, base = oc.evaluated(ref, genome["prefix"], "default")
    assert not any(any(win.clamps(lq, rid, seeds)) for lq, w in zip(base.lens, base.want) for rid, _, seeds in w)
    got = host.chains(host.opt(), ev.lens, [0] * len(ev.lens), ev.seedsets, 1)
    assert [[(c[0], c[5], c[6]) for c in h] for h in got] == ev.want
    win.check(ev.lens, ev.want, got, "edges")


def test_alt_reads_nest_both_ways(genome_alt):
    """on the index with ALT contigs: reads in which a kept primary chain lies under a heavier ALT chain (the pairs that
    `!ALT(j) || ALT(i)` takes out of the mask test) and the opposite nesting, in the lanes' launches and in chain_heavy_kernel; the
    host chaining equals the reference on them"""
    from mpibwa_amd import api
    ref = po.RefIndex(genome_alt["prefix"])
    host = api.Engine(genome_alt["prefix"], upload=False)
    for name in oc.ALT_SETS:
        n = oc.alt_coverage(ref, genome_alt["prefix"], name)
        print(name, n)
        oc.check_alt_coverage(name, n)
        cases, ev = oc.evaluated(ref, genome_alt["prefix"], name, oc.alt_cases)
        for (fam, (lq, ivs)), sd in zip(cases, ev.seedsets):
            assert len({s[0] for s in sd}) == len(sd), (fam, "two seeds at one position")
        got = host.chains(host.opt(**oc.OPTION_SETS[name]), ev.lens, [0] * len(ev.lens), ev.seedsets, 1)
        for k, (h, w) in enumerate(zip(got, ev.want)):
            assert [(c[0], c[5], c[6]) for c in h] == w, (name, k, ev.klass[k])
        window_model.ChainWindows(host.bns, host.opt(**oc.OPTION_SETS[name])).check(ev.lens, ev.want, got, "alt " + name)
