"""chain_heavy_kernel<256 / 1024 / 2048 / 4096>: the borders between its classes, the batched shifts of its ordered map, its LDS (map,
columns, sort frames) reused by resident waves, and its phase counters, all through engine.chains against the reference's own mem_chain +
mem_chain_flt (oracle/chain_inject.c).

Every read here is n single-seed chains at distinct positions, so a chain's place in the map is its seed's position and the order in
which the seeds are visited decides where every insert lands.  reference_chains sorts the intervals by (qbeg, qend) and takes the hits
of one interval in the order given: a visiting order is cut into consecutive groups of at most 400 (< max_occ) seeds, group g gets the
interval (g, g + its length).  Why no seed merges into another chain (test_and_merge, src/bwamem.c:190-211): the chain at or before a
seed starts `step` or more bases before it on the reference (y >= step) while the two query starts differ by less than the number of
groups (|x| <= 10), so y - x > w = 100 whenever step > 110; and no seed of at most 140 bases that starts 170 or more behind a chain's
only seed ends inside it.  Positions are `step` apart: 400 as in chain_cases.sorted_tail_chain_sets while the read's chains fit on
the test genome's two strands that way (1 788 of them), otherwise the widest step at which they fit (340 for 2 048, 172 for 4 096),
500 bases clear of contig ends and of the strand boundary."""
import os

import numpy as np
import pytest

import window_model
from oracle import pyoracle as po

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not po.chain_inject_available(), reason="oracle/_ref/libchaininj.so not present")]

LQ = 151
MAX_HITS = 400
BORDER_SIZES = (255, 256, 257, 1024, 1025, 2048, 2049, 4096)
SHIFT_SIZES = (63, 64, 65, 255, 256, 257, 511, 513, 1030)


@pytest.fixture(scope="module")
def engine(genome):
    from mpibwa_amd import api
    return api.Engine(genome["prefix"], device=0)


def _contigs(engine):
    l_pac = int(engine.bns.contents.l_pac)
    n_seqs = int(engine.bns.contents.n_seqs)
    offs = [int(engine.bns.contents.anns[k].offset) for k in range(n_seqs)] + [l_pac]
    return l_pac, offs, n_seqs


_SLOTS = {}


def _slots(l_pac, offs, n_seqs, n):
    """-> (step, ascending positions `step` apart on both strands of every contig); step 400 where n fit, the widest that fits otherwise"""
    for step in (400, 340, 172):
        if (l_pac, step) in _SLOTS and len(_SLOTS[l_pac, step]) >= n:
            return step, _SLOTS[l_pac, step]
    spans = []
    for k in range(n_seqs):
        spans.append((offs[k] + 500, offs[k + 1] - 500 - LQ))
        spans.append((2 * l_pac - offs[k + 1] + 500, 2 * l_pac - offs[k] - 500 - LQ))
    spans.sort()
    for step in (400, 340, 172):
        slots = _SLOTS[l_pac, step] = [p for lo, hi in spans for p in range(lo, hi, step)]
        if len(slots) >= n:
            return step, slots
    raise AssertionError((n, len(slots)))


def single_seed_read(rng, l_pac, offs, n_seqs, n, order):
    """One read of n single-seed chains.  order: "up" / "down" / "mixed" — the positions as mem_chain visits them.
    -> ((lq, [(qb, qe, hits)]), positions in visiting order)"""
    step, slots = _slots(l_pac, offs, n_seqs, n)
    pick = np.sort(rng.choice(len(slots), n, replace=False))
    pos = [slots[i] for i in pick]
    if order == "down":
        pos = pos[::-1]
    elif order == "mixed":
        pos = [pos[i] for i in rng.permutation(n)]
    n_groups = max((n + MAX_HITS - 1) // MAX_HITS, min(8, n))
    assert n_groups <= 11 and step - n_groups > 110, (n, step, n_groups)
    lens = rng.choice(np.arange(40, 141), n_groups, replace=False)     # a group's chains weigh the same: ties, kept and dropped chains
    ivs, at = [], 0
    for g in range(n_groups):
        m = n // n_groups + (1 if g < n % n_groups else 0)
        assert 0 < m <= MAX_HITS
        ivs.append((g, g + int(lens[g]), pos[at:at + m]))
        at += m
    return (LQ, ivs), pos


def _reference(engine, genome, cases, visits=None):
    """The checks every generated set passes on the CPU, and what the reference makes of it."""
    import chain_cases as cc
    ref = po.RefIndex(genome["prefix"])
    lens, seedsets, want = cc.reference_chains(ref, ref.opt(), cases)
    for k, (sd, w) in enumerate(zip(seedsets, want)):
        assert len({s[0] for s in sd}) == len(sd), (k, "two seeds at one position")
        assert len(w) > 0, (k, "the reference keeps no chain")
        if visits is not None and visits[k] is not None:
            assert [s[0] for s in sd] == visits[k], (k, "not the intended visiting order")
    return lens, seedsets, want


def _check(engine, lens, seedsets, want, what):
    dev = engine.chains(engine.opt(), lens, [0] * len(lens), seedsets, 0)
    for k, (d, w, sd) in enumerate(zip(dev, want, seedsets)):
        assert d is not None, (what, k, len(sd), "declined")
        dd = [(c[0], c[5], c[6]) for c in d]
        assert dd == w, (what, k, len(sd), len(dd), len(w), [(a, b) for a, b in zip(dd, w) if a != b][:2])
    # ... and its contig bounds and reference window those of mem_chain2aln on the reference's chain
    window_model.ChainWindows(engine.bns, engine.opt()).check(lens, want, dev, what)
    return dev


def test_reads_at_the_borders_of_the_classes(engine, genome):
    """255 | 256, 257 ... 1 024 | 1 025 ... 2 048 | 2 049 ... 4 096 seeds (and as many chains): the last read of a class and the first of
    the next, positions visited in shuffled order.  None is declined; every read's chains are the reference's."""
    l_pac, offs, n_seqs = _contigs(engine)
    rng = np.random.default_rng(3301)
    made = [single_seed_read(rng, l_pac, offs, n_seqs, n, "mixed") for n in BORDER_SIZES]
    lens, seedsets, want = _reference(engine, genome, [c for c, _ in made], [v for _, v in made])
    assert tuple(len(sd) for sd in seedsets) == BORDER_SIZES
    _check(engine, lens, seedsets, want, "borders")


def test_shift_batches(engine, genome):
    """Positions DESCENDING in visiting order: every insert lands at slot 0 and moves the whole map, so the number of entries moved
    crosses every multiple of 64 (a lane's reach) and of 256 (a batch of four) up to the chain count.  Ascending: no shift at all.
    Shuffled: shifts of every length."""
    l_pac, offs, n_seqs = _contigs(engine)
    rng = np.random.default_rng(3302)
    made = [single_seed_read(rng, l_pac, offs, n_seqs, n, "down") for n in SHIFT_SIZES]
    made += [single_seed_read(rng, l_pac, offs, n_seqs, 700, "up"), single_seed_read(rng, l_pac, offs, n_seqs, 700, "mixed")]
    for (_, visit), order in zip(made, ["down"] * len(SHIFT_SIZES) + ["up", "mixed"]):
        d = np.diff(visit)
        assert (d < 0).all() if order == "down" else (d > 0).all() if order == "up" else ((d < 0).any() and (d > 0).any())
    lens, seedsets, want = _reference(engine, genome, [c for c, _ in made], [v for _, v in made])
    assert tuple(len(sd) for sd in seedsets) == SHIFT_SIZES + (700, 700)
    _check(engine, lens, seedsets, want, "shifts")


def test_lds_reuse_by_resident_waves(engine, genome):
    """One batch of 6 000 reads of 10-40 chains, more than chain_heavy_kernel<256> has waves (5 120, all resident): its waves take
    several reads each and reuse map, columns and sort frames; among them the reads of the comb-sort test
    (chain_cases.sorted_tail_chain_sets), whose sorts stack the most frames, in the classes of 256, 1 024 and 2 048 seeds."""
    import chain_cases as cc
    l_pac, offs, n_seqs = _contigs(engine)
    rng = np.random.default_rng(3303)
    cases = [single_seed_read(rng, l_pac, offs, n_seqs, int(rng.integers(10, 41)), ("up", "down", "mixed")[k % 3])[0] for k in range(6000)]
    tails = cc.sorted_tail_chain_sets(np.random.default_rng(cc.SORTED_TAIL_SEED), cc.SORTED_TAIL_SIZES, l_pac, offs, n_seqs)
    every = len(cases) // len(tails)
    for k, t in enumerate(tails):
        cases.insert(k * (every + 1), t)
    lens, seedsets, want = _reference(engine, genome, cases)
    assert len(cases) == 6000 + len(tails) and max(len(sd) for sd in seedsets) == 2000
    _check(engine, lens, seedsets, want, "reuse")


def test_phase_counters_change_nothing(engine, genome):
    """The same small batch with MPIBWA_CHAIN_PROF unset and set to 1 (the phase table goes to stderr): identical chains."""
    l_pac, offs, n_seqs = _contigs(engine)
    rng = np.random.default_rng(3304)
    cases = [single_seed_read(rng, l_pac, offs, n_seqs, n, "mixed")[0] for n in (12, 40, 200, 300, 1100, 2100)]
    lens, seedsets, want = _reference(engine, genome, cases)
    old = os.environ.pop("MPIBWA_CHAIN_PROF", None)
    try:
        off = _check(engine, lens, seedsets, want, "counters off")
        os.environ["MPIBWA_CHAIN_PROF"] = "1"
        on = _check(engine, lens, seedsets, want, "counters on")
    finally:
        os.environ.pop("MPIBWA_CHAIN_PROF", None)
        if old is not None:
            os.environ["MPIBWA_CHAIN_PROF"] = old
    assert on == off
