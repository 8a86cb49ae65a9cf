"""CPU: the families built to reach ks_introsort's comb sort do reach it, and nothing else in the suite does.

tests/introsort_model.py restates mpibwa_amd/csrc/sortutil.h in Python and reports what the sort did.  Here it is
  * pinned to the reference's own ks_introsort: on every sorted_tail chain case the order it gives to the chain weights is the order of
    the chains the reference's mem_chain + mem_chain_flt return (all n come back under the default options);
  * asked for the census of the three new families (chain_cases.sorted_tail_chain_sets, dedup_cases sorted_re and sorted_score): every
    case of 26 or more elements hands a range of at least 17 to the comb sort, which swaps, and the variant whose fallback is an
    insertion sort gives another result; the cases of 25 elements do not get there — 25 / 26 is the edge;
  * asked for the census of the families that were there before, which is printed and written into DESIGN.md, not asserted."""
import numpy as np
import pytest

import chain_cases as cc
import dedup_cases as dc
import introsort_model as im
from oracle import pyoracle as po

HEAVIER = lambda x, y: x > y   # noqa: E731  ("less" of mem_chain_flt's descending sort)


def _geometry(ref):
    b = ref.bns.contents
    n_seqs, l_pac = int(b.n_seqs), int(b.l_pac)
    return l_pac, [int(b.anns[k].offset) for k in range(n_seqs)] + [l_pac], n_seqs


def test_ordered_input_runs_out_of_depth_from_26_elements():
    assert im.first_ordered_size_that_combs() == 26
    assert [n for _, n in im.sort_keys(list(range(26)))[1].comb_ranges] == [17]
    assert not dc.can_run_out_of_depth(25) and dc.can_run_out_of_depth(26)
    rng = np.random.default_rng(1)
    for n in (3, 16, 17, 25, 26, 100, 700):   # the model sorts, with either fallback
        keys = [0] + [int(v) for v in rng.integers(1, 9, n)] + list(range(9, 9 + im.budget(n)))
        for comb in (True, False):
            o, _ = im.sort_keys(keys, comb=comb)
            assert sorted(o) == list(range(len(keys))) and [keys[k] for k in o] == sorted(keys)


@pytest.mark.skipif(not po.chain_inject_available(), reason="oracle/_ref/libchaininj.so not present")
def test_model_gives_the_reference_order_and_sorted_tail_reaches_the_comb_sort(genome):
    ref = po.RefIndex(genome["prefix"])
    l_pac, offs, n_seqs = _geometry(ref)
    cases = cc.sorted_tail_chain_sets(np.random.default_rng(cc.SORTED_TAIL_SEED), cc.SORTED_TAIL_SIZES, l_pac, offs, n_seqs)
    lens, seedsets, want = cc.reference_chains(ref, ref.opt(), cases)
    sizes = []
    for cs, sd, w in zip(cases, seedsets, want):
        wt = cc.single_seed_weights(cs)
        n = len(wt)
        sizes.append(n)
        pos = sorted(rb for rb, _, _ in sd)
        assert len(set(pos)) == n and len(w) == n and all(len(c[2]) == 1 for c in w), (n, len(w))
        o, st = im.sort_keys(wt, HEAVIER)
        assert [pos[k] for k in o] == [c[2][0][0] for c in w], (n, "the model's order is not the reference's")
        flat, _ = im.sort_keys(wt, HEAVIER, comb=False)
        print("sorted_tail n", n, "comb ranges", st.comb_ranges, "comb swaps", st.comb_swaps, "frames", st.max_frames)
        if n == 25:
            assert not st.comb_ranges
        else:
            assert st.widest >= 17 and st.comb_swaps >= 1 and flat != o, (n, st.comb_ranges, st.comb_swaps)
    assert sorted(set(sizes)) == sorted(cc.SORTED_TAIL_SIZES)
    assert all(sizes.count(n) == (4 if n <= 255 else 2) for n in cc.SORTED_TAIL_SIZES)


@pytest.mark.skipif(not po.chain_inject_available(), reason="oracle/_ref/libchaininj.so not present")
def test_tied_small_family_reaches_the_one_node_sort_with_ties(genome):
    """chain_cases.tied_small_chain_sets, the family of the sort in chain_read (ks_small_introsort_at over a lane's 3-9 chains): every
    read has the seed and chain counts of the launch it is built for (none is declined for size), the reference returns all of its
    chains with the weights built, in the model's order; per launch at least 8 reads whose sort sees 3 or more chains with a tie, and
    at least one on which a stable sort of the same weights gives another order than ks_introsort."""
    ref = po.RefIndex(genome["prefix"])
    l_pac, offs, n_seqs = _geometry(ref)
    cases, meta = cc.tied_small_chain_sets(np.random.default_rng(cc.TIED_SMALL_SEED), l_pac, offs, n_seqs)
    lens, seedsets, want = cc.reference_chains(ref, ref.opt(), cases)
    tied, unstable = [0, 0, 0], [0, 0, 0]
    for (launch, w), (lq, ivs), sd, exp in zip(meta, cases, seedsets, want):
        (s_lo, s_hi), (c_lo, c_hi) = cc.TIED_SMALL_LAUNCHES[launch]
        assert s_lo <= len(sd) <= s_hi and c_lo <= len(w) <= c_hi and cc.tied_small_launch(len(sd), len(w)) == launch, (launch, len(sd), len(w))
        raw = po.ref_chains(ref.opt(), ref.bns, lq, sorted(ivs, key=lambda t: (t[0] << 32) | t[1]))
        o, st = im.sort_keys(w, HEAVIER)
        assert not st.comb_ranges and st.max_frames == 0
        pos = sorted(min(rb for rb, _, _ in c[5]) for c in raw)
        assert len(raw) == len(exp) == len(w) and sum(len(c[5]) for c in raw) == len(sd), (launch, len(raw), len(w))
        assert [c[1] for c in raw] == [w[k] for k in o] and [pos.index(min(rb for rb, _, _ in c[5])) for c in raw] == o, (launch, w, "the model's order is not the reference's")
        tied[launch] += len(w) >= 3 and len(set(w)) < len(w) and w != sorted(w, reverse=True)
        unstable[launch] += o != sorted(range(len(w)), key=lambda i: -w[i])
    print("tied_small: reads with a tie per launch", tied, "reads where a stable sort differs", unstable)
    assert min(tied) >= 8 and min(unstable) >= 1, (tied, unstable)


@pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref/libbwaref.so not present")
def test_sorted_region_families_reach_the_comb_sort(genome):
    ref = po.RefIndex(genome["prefix"])
    ix = dc.Index(genome["prefix"], ref.bns)
    cases = dc.sorted_cases(ix)
    assert len(cases) == 2 * dc.SORTED_PER_SIZE * len(dc.SORTED_SIZES)
    want = dc.reference_results(ref, ref.opt(), cases, True)
    for cs, w in zip(cases, want):
        regs, n, k = cs["regs"], len(cs["regs"]), cs["family"] == "sorted_score"
        assert cs["tag"] == "n%d" % n and len(set(zip(regs["qb"].tolist(), regs["qe"].tolist()))) == 1
        real = dc.model_pass(regs)
        # the model of the pass is the reference's pass on these lists
        assert dc.kept_rows(regs, real["kept"]) == dc.kept_rows(w, range(len(w))), (cs["family"], cs["tag"])
        st = real["second" if k else "first"]
        print(cs["family"], cs["tag"], "comb ranges", st.comb_ranges, "comb swaps", st.comb_swaps, "kept", len(w))
        if k:
            assert len(real["sorted"]) == n and len(w) == n - len(cs["twins"])       # nothing but one of every twin pair goes
            assert regs["re"].tolist() == sorted(regs["re"].tolist())                # ... and the survivors arrive as built
        if n == 25:
            assert not st.comb_ranges
            continue
        assert st.widest >= 17 and st.comb_swaps >= 1, (cs["family"], cs["tag"], st.comb_ranges, st.comb_swaps)
        mut = dc.model_pass(regs, comb=(k, not k))
        if k:
            assert dc.twin_order(mut["sorted"], cs["twins"]) != dc.twin_order(real["sorted"], cs["twins"])
        # with an insertion sort for the comb sort the pass keeps other regions than the reference does
        assert dc.kept_rows(regs, mut["kept"]) != dc.kept_rows(w, range(len(w))), (cs["family"], cs["tag"])


def _census(name, key_lists, less=None):
    hit = sum(1 for keys in key_lists if im.sort_keys(keys, less)[1].comb_ranges)
    big = sum(1 for keys in key_lists if len(keys) >= 26)
    print("census %-34s lists %5d  of 26 or more %5d  enter the comb sort %d" % (name, len(key_lists), big, hit))
    return hit


def test_census_of_the_earlier_families(genome):
    """printed, not asserted (DESIGN.md quotes the numbers)"""
    from mpibwa_amd import api
    eng = api.Engine(genome["prefix"], upload=False)
    ix = dc.Index(genome["prefix"], eng.bns)
    built = dc.build_cases(ix, 5)
    rnd = dc.random_cases(ix, 1500, 8)
    for name, cases in (("dedup build_cases", built), ("dedup random_cases", rnd)):
        _census(name + ", first sort", [cs["regs"]["re"].tolist() for cs in cases])
        # (the second sort sees the survivors; the whole list in its raw order is the upper bound that can be had without the pass)
        _census(name + ", second sort (raw list)", [list(zip((-cs["regs"]["score"]).tolist(), cs["regs"]["rb"].tolist(), cs["regs"]["qb"].tolist())) for cs in cases])
    # chain weights follow from the seeds only where every chain has one seed; these families merge seeds into chains: not determined
    for name in ("adversarial_interval_sets", "repeat_like_interval_sets"):
        print("census %-34s not determined (chains of several seeds: the weights are mem_chain's to compute)" % name)
