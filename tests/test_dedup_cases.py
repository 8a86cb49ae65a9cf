"""CPU: the cases of the stage test of the redundancy pass (tests/dedup_cases.py) are what that file says they are — shown on the
reference's own mem_sort_dedup_patch (oracle/_ref/libbwaref.so), without any kernel.  Every list goes through it twice: with
bns = pac = query = 0, where mem_patch_reg returns at once and nothing can be patched, and with the sequences.  Per option set:
  same_span  the two calls agree on every list; per size, a list without planted twins loses a region (only the redundancy scan can have
             taken it: no two of its regions that the scan leaves both alive are equal in (score, rb, qb) unless the scan compared them)
             and a list with planted twins keeps exactly one of the two (only the removal of adjacent equal elements can have taken
             the other: the scan from one never reaches the other); per size above 16 a list holds regions of one rid with equal `re`
             that differ otherwise, the ties of the first sort
  far        the two calls agree and nothing is removed
  patch      in at least 20 reads the two results differ: the reference merged
  junction, mixed, random   the counts are printed; the stage test holds them to its invariant alone."""
import collections

import numpy as np
import pytest

import dedup_cases as dc
from oracle import pyoracle as po

pytestmark = pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref/libbwaref.so not present")


@pytest.fixture(scope="module")
def ref(genome):
    return po.RefIndex(genome["prefix"])


@pytest.mark.parametrize("name", list(dc.OPTION_SETS))
def test_families_reach_their_branches(ref, genome, name):
    ropt = ref.opt(**dc.OPTION_SETS[name])
    ix = dc.Index(genome["prefix"], ref.bns)
    cases, want = dc.full_set(ref, ropt, ix, genome["seqs"], n_random=400)
    bare = dc.reference_results(ref, ropt, cases, False)
    n = collections.Counter()
    differ = collections.Counter()
    lost_scan, lost_twin, ties = set(), set(), set()
    sizes = set()
    for cs, w, b in zip(cases, want, bare):
        fam, raw = cs["family"], cs["regs"]
        n[fam] += 1
        same = dc.same_lists(w, b)
        differ[fam] += not same
        assert len(w) <= len(raw) and len(b) <= len(raw)
        if fam == "same_span":
            assert same, (name, cs["tag"])
            assert len(set(zip(raw["qb"].tolist(), raw["qe"].tolist()))) == 1
            k = len(raw)
            sizes.add(k)
            if cs["twins"] is None:
                if len(w) < k:
                    lost_scan.add(k)
            else:
                t, sc = cs["twins"]
                assert int(((raw["rb"] == t) & (raw["score"] == sc)).sum()) == 2
                if int(((w["rb"] == t) & (w["score"] == sc)).sum()) == 1:
                    lost_twin.add(k)
            for rid in np.unique(raw["rid"]):
                g = raw[raw["rid"] == rid]
                for e in np.unique(g["re"]):
                    h = g[g["re"] == e]
                    if len(h) > 1 and (len(np.unique(h["rb"])) > 1 or len(np.unique(h["score"])) > 1):
                        ties.add(k)
        elif fam == "far":
            assert same and len(w) == len(raw), (name, cs["tag"], len(w), len(raw))
        elif fam == "patch":
            assert cs["merged"] == (not same)
            assert (cs["expect"] == "patch") == cs["merged"]
    print(name, "lists", dict(n), "results that differ with the sequences", dict(differ))
    assert sizes == set(dc.SAME_SPAN_SIZES)
    assert lost_scan == sizes, (name, sorted(sizes - lost_scan))
    assert lost_twin == sizes, (name, sorted(sizes - lost_twin))
    assert {k for k in sizes if k > 16} <= ties, (name, sorted(sizes - ties))
    assert differ["patch"] >= 20, (name, differ["patch"], n["patch"])
    assert n["junction"] == 60 and n["mixed"] >= 80 and n["random"] == 800 and n["far"] == 4 * len(dc.FAR_SIZES)
