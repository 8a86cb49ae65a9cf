"""Stage test of the seed enumeration between SMEM and SA lookup: seed_prep_kernel (sort of a read's intervals by info, l_rep, number
of seeds) and seed_enum_kernel (BWT row and (qbeg, len) of every seed, a stride through intervals larger than max_occ), through
mi355x_seed_batch — the pipeline's launch sequence without the SA lookup — against the plain restatement of src/bwamem.c:161, 265-283 in
tests/seed_stage_cases.py.  Integers only: every comparison is exact.

The restatement itself is pinned on the CPU against the reference's OWN mem_chain (oracle/chain_inject.c): with hits far apart every
seed mem_chain visits becomes a chain of its own, so the seeds of its chains are the enumeration and frac_rep is (float)l_rep / l_seq
(src/bwamem.c:310)."""
import numpy as np
import pytest

import seed_stage_cases as ss
from oracle import pyoracle as po

CAP = 16


def _compare(eng, reads, cap, max_occ, tag):
    srt, n_seeds, l_rep, per = eng.seeds([np.array(r, dtype=np.uint64).reshape(-1, 4) for r in reads], cap, max_occ)
    n_rep = n_step = 0
    for r, iv in enumerate(reads):
        want_iv, want_lrep, (rows, qb, ln) = ss.expected(iv, cap, max_occ)
        assert [tuple(int(x) for x in t) for t in srt[r]] == want_iv, (tag, r, "sorted intervals")
        assert int(l_rep[r]) == want_lrep, (tag, r, "l_rep", int(l_rep[r]), want_lrep, want_iv)
        assert int(n_seeds[r]) == len(rows), (tag, r, "n_seeds", int(n_seeds[r]), len(rows), want_iv)
        assert (per[r][0] == rows).all() and (per[r][1][:, 0] == qb).all() and (per[r][1][:, 1] == ln).all(), (tag, r, "seeds", want_iv)
        n_rep += want_lrep > 0
        n_step += any(t[2] >= 2 * max_occ for t in want_iv)
    return n_rep, n_step


@pytest.mark.gpu
@pytest.mark.parametrize("max_occ", ss.MAX_OCCS)
def test_seed_kernels_on_crafted_intervals(built, max_occ):
    from mpibwa_amd import api
    eng = api.Engine.__new__(api.Engine)      # (the entry needs no index)
    eng.lib = api.load_library()
    reads = ss.crafted_reads(max_occ, CAP, 40 + max_occ)
    assert any(len(r) > CAP for r in reads) and any(len(r) == CAP for r in reads) and any(len(r) == 0 for r in reads)
    n_rep, n_step = _compare(eng, reads, CAP, max_occ, "max_occ=%d" % max_occ)
    assert n_rep >= 60 and n_step >= 30, (n_rep, n_step)
    # launches of 1, 127, 128 and 129 reads (one thread per read, 128 per workgroup)
    for n in (1, 127, 128, 129):
        _compare(eng, (reads * 2)[:n], CAP, max_occ, "max_occ=%d/%d reads" % (max_occ, n))


@pytest.mark.gpu
@pytest.mark.parametrize("max_occ", [500, 50, 3])
def test_seed_kernels_on_the_intervals_of_real_reads(genome, reads_pe, reads_var, max_occ):
    """the intervals mi355x_smem_batch returns for the session's reads, handed over in reverse order"""
    from mpibwa_amd import api
    api.load_library().mi355x_finalize()
    eng = api.Engine(genome["prefix"], device=0)
    seqs = [np.asarray(s, dtype=np.uint8) for rd in list(reads_pe) + list(reads_var) for s in rd[1:3] if s is not None]
    got, _, _ = eng.smem(eng.opt(), seqs, cap=512)
    assert sum(len(g) for g in got) > 2 * len(seqs)
    n_rep, n_step = _compare(eng, [g[::-1] for g in got], 512, max_occ, "real/max_occ=%d" % max_occ)
    if max_occ == 3:
        assert n_rep >= 20 and n_step >= 20, (n_rep, n_step)


@pytest.mark.gpu
def test_seed_kernels_on_a_repeat_rich_genome(built, tmp_path_factory):
    """a few hundred reads of a genome that is repeats by a third: intervals of hundreds of occurrences under the default max_occ"""
    from mpibwa_amd import api, simulate
    names, seqs = simulate.make_genome(240_000, 3, seed=17, repeat_frac=0.35)
    fa = str(tmp_path_factory.mktemp("seed_rep") / "r.fa")
    simulate.write_fasta(fa, names, seqs)
    api.build_index(fa, fa)
    api.load_library().mi355x_finalize()
    eng = api.Engine(fa, device=0)
    reads = simulate.simulate_reads(seqs, 200, 150, paired=True, seed=3)
    rd = [np.asarray(s, dtype=np.uint8) for pair in reads for s in pair[1:3]]
    got, _, _ = eng.smem(eng.opt(), rd, cap=512)
    for max_occ in (500, 20, 5):
        n_rep, n_step = _compare(eng, [g[::-1] for g in got], 512, max_occ, "repeats/max_occ=%d" % max_occ)
    assert n_rep >= 20 and n_step >= 20, (n_rep, n_step)


@pytest.mark.skipif(not po.chain_inject_available(), reason="oracle/_ref/libchaininj.so not present")
@pytest.mark.parametrize("max_occ", [1, 2, 5])
def test_the_restatement_matches_the_reference_mem_chain(genome, max_occ):
    """CPU: tests/seed_stage_cases.py: expected() against the reference.  Every hit of an interval lies 700 bases after the one before,
    so no two seeds chain (band 100) and the chains of mem_chain, unfiltered, are its seeds; row k of an interval is hit k."""
    ref = po.RefIndex(genome["prefix"])
    ropt = ref.opt(max_occ=max_occ)
    n_checked = n_rep = 0
    for read in ss.crafted_reads(max_occ, CAP, 40 + max_occ):
        read = [t for t in read if t[2] <= 60 and (t[3] & 0xffffffff) - (t[3] >> 32) >= 19][:CAP]
        if not read or len({t[3] for t in read}) < len(read):
            continue
        # rows of the read's intervals: consecutive runs of a table of positions
        at, ivs, table, rows_of = 0, [], [], []
        for x0, x1, size, inf in read:
            hits = [1000 + 700 * (at + j) for j in range(size)]
            ivs.append((inf >> 32, inf & 0xffffffff, hits))
            rows_of.append((at, size, inf))
            table += hits
            at += size
        if 1000 + 700 * at > 100_000:
            continue
        chains = po.ref_chains(ropt, ref.bns, 150, ivs, do_flt=False)
        want_iv, want_lrep, (rows, qb, ln) = ss.expected([(a, 0, size, inf) for a, size, inf in rows_of], CAP, max_occ)
        want = sorted((table[int(r)], int(q), int(l)) for r, q, l in zip(rows, qb, ln))
        got = sorted(s for c in chains for s in c[5])
        assert got == want, (read, got, want)
        for c in chains:
            assert c[4] == int((np.float32(want_lrep) / np.float32(150)).view(np.uint32)), (read, c[4], want_lrep)
        n_checked += 1
        n_rep += want_lrep > 0
    assert n_checked >= 40 and n_rep >= 20, (n_checked, n_rep)
