"""CPU companion of tests/test_gpu_c2a_stage.py: the case generator of tests/c2a_cases.py and the reference's own mem_chain2aln alone, no
GPU.  Every family must reach the branch it is there for, counted from the reference's outputs, so that the stage test cannot pass
without exercising it."""
import numpy as np
import pytest

import c2a_cases as cc
from oracle import pyoracle as po

pytestmark = pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref/libbwaref.so not built")

# floors per option set, over both launches (A natural chains, B hand-built ones)
FLOORS = dict(
    skipped_seed=50,        # reads with fewer regions than seeds: a seed was skipped as covered
    cross_chain=4,          # reads where the chains run alone give more regions than in sequence (cross-chain skipping) ...
    cross_chain_heavy=2,    # ... also inside a component of a read with more than 8 chains
    left_local=20, left_to_end=20, right_local=20, right_to_end=20,
    clamped=10,             # windows clamped at a contig edge or at the forward/reverse boundary
    regs_gt8=4,             # reads with more than 8 regions (C2A_CAP_R) ...
    seeds_gt64=2,           # ... and more than 64 seeds (C2A_CAP_S)
    win_gt_cap=2,           # windows longer than c2a_win_cap(max_len) of their launch
)
# floors that only some option sets reach: the set, the count, the floor
SET_FLOORS = [("default", "doubled", 4), ("w20", "doubled", 4), ("maxocc20", "frac_rep", 2), ("default", "emptied", 1)]


@pytest.fixture(scope="module")
def genome(tmp_path_factory, built):
    from mpibwa_amd import api, simulate
    d = tmp_path_factory.mktemp("c2a_genome")
    names, seqs = simulate.make_genome(240_000, 3, seed=17, repeat_frac=0.35)
    fa = str(d / "r.fa")
    simulate.write_fasta(fa, names, seqs)
    api.build_index(fa, fa)
    return {"prefix": fa, "seqs": seqs}


def coverage(genome, name):
    ref = cc.Reference(genome["prefix"], cc.OPTION_SETS[name])
    nat, emptied = cc.natural_cases(ref, genome["seqs"], np.random.default_rng(5))
    hand = cc.built_cases(ref, genome["seqs"], np.random.default_rng(6))
    _, ca = cc.reference_side(ref, nat)
    _, cb = cc.reference_side(ref, hand)
    cov = {k: ca[k] + cb[k] for k in ca}
    cov["emptied"] = emptied
    cov["long_lds_over_64k"] = max(len(r) for _, r, _ in nat)
    fams = {}
    for f, _, _ in nat + hand:
        fams[f] = fams.get(f, 0) + 1
    return cov, fams


@pytest.mark.parametrize("name", list(cc.OPTION_SETS))
def test_c2a_case_families_reach_their_branches(genome, name):
    cov, fams = coverage(genome, name)
    print(name, cov, fams)
    low = {k: (cov[k], f) for k, f in FLOORS.items() if cov[k] < f}
    assert not low, (name, low)
    for s, k, f in SET_FLOORS:
        if s == name:
            assert cov[k] >= f, (name, k, cov[k])
    # every family is there; the repeat families keep only reads with more than 8 chains
    for f in ("closed", "one_mm", "ambig", "indel_end", "deletion", "two_piece", "tandem", "repeat", "edge", "n_run", "long", "thr10", "ceil95",
              "band_edge", "many_seeds", "many_regions", "groups_touch", "contig_start", "contig_end", "drift"):
        assert fams.get(f, 0) > 0, (name, f)
    # the longest read takes c2a_kernel's LDS beyond 64 KB (c2a_lds_bytes: about 13 bytes per base)
    assert cov["long_lds_over_64k"] >= 5000


def test_c2a_thresholds_flip_the_reference(genome):
    """the hand-built threshold pairs are on both sides of their threshold: each pair gives different region counts"""
    ref = cc.Reference(genome["prefix"], {})
    hand = cc.built_cases(ref, genome["seqs"], np.random.default_rng(6))
    for fam in ("thr10", "ceil95", "band_edge"):
        n = [len(ref.chain2aln(r, c)) for f, r, c in hand if f == fam]
        flips = sum(a != b for a, b in zip(n[0::2], n[1::2]))
        assert flips >= 2, (fam, n)
