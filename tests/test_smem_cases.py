"""CPU side of the stage test of the seeding kernels (tests/test_gpu_smem_options.py): the oracle's mem_collect_intv is pinned against the
reference's own under every option set of tests/smem_cases.py, and the cases are shown to bite — on the oracle's output alone, every
option moves the intervals of at least twenty reads, the third pass and re-seeding each emit on at least fifty, and every staircase
read's list outgrows LDS.  Integers only: every comparison is exact."""
import os
import re

import numpy as np
import pytest

import smem_cases as sc
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def repeats(built, tmp_path_factory):
    names, seqs = sc.repeat_genome()
    fa = sc.write_index(tmp_path_factory.mktemp("smem_rep"), "rep", names, seqs)
    r150, rvar, rlong = sc.repeat_reads(seqs)
    return {"prefix": fa, "fm": po.OracleFM(fa), "reads": r150 + rvar + rlong, "batches": sc.class_batches(r150, rvar, rlong)}


@pytest.fixture(scope="module")
def stairs(built, tmp_path_factory):
    names, seqs, reads = sc.staircase_genome()
    fa = sc.write_index(tmp_path_factory.mktemp("smem_stairs"), "stairs", names, seqs)
    return {"prefix": fa, "fm": po.OracleFM(fa), "text": seqs[0], "reads": reads}


def _sorted_rows(a):
    return np.array(sorted(map(tuple, a.tolist())), dtype=np.uint64).reshape(-1, 4)


def _oracle(fm, reads, kw):
    """what the callers of mem_collect_intv see: nothing for a read shorter than a seed (src/bwamem.c:260)"""
    args = sc.oracle_args(kw)
    return [fm.collect_intv(r, *args) if len(r) >= args[0] else np.zeros((0, 4), np.uint64) for r in reads]


def test_the_constants_are_the_kernels_own():
    src = lambda f: open(os.path.join(ROOT, "mpibwa_amd", "csrc", f)).read()
    fmk, p3k, dev = src("fm_kernels.hip"), src("smem_kernels.hip"), src("device.hip")
    for name, v in (("LCAP_S", sc.LCAP_S), ("QSLOT_S", sc.QSLOT_S), ("LCAP", sc.LCAP), ("QSLOT", sc.QSLOT), ("SMEM_FETCH", sc.SMEM_FETCH)):
        assert re.search(r"#define %s (\d+)" % name, fmk).group(1) == str(v), name
    assert re.search(r"#define SMEM2_BLOCK (\d+)", p3k).group(1) == str(sc.P3_BLOCK)
    p3 = dev[dev.index("static void maybe_build_p3()"):]
    assert re.search(r"int k = (\d+);", p3).group(1) == str(sc.P3_K)
    kmt = dev[dev.index("static void maybe_build_kmt()"):]
    assert "while (k < 14 && ((uint64_t)1 << (2 * k)) < g_idx.fm.seq_len) ++k;" in kmt
    assert sc.REPEAT_KMT == 10 and sc.kmt_depth(1 << 20) == 10 and sc.kmt_depth((1 << 20) + 1) == 11 and sc.kmt_depth(1 << 40) == 14
    # the option sets the issue names, each option moved alone, and the corner
    ids = set(sc.OPTION_IDS)
    assert {"default", "corner", "min_seed_len=9", "min_seed_len=10", "min_seed_len=12", "min_seed_len=13", "min_seed_len=25", "split_factor=0.5",
            "split_factor=1", "split_factor=4", "split_width=0", "split_width=1", "split_width=200", "max_mem_intv=0", "max_mem_intv=1",
            "max_mem_intv=2", "max_mem_intv=500"} == ids and len(sc.OPTION_SETS) == len(ids)


def test_staircase_lists_outgrow_lds(stairs):
    """list_entries, a brute-force count on the text: every staircase sweep has at least LCAP + 3 entries; and the oracle, for its part,
    re-seeds every hill read at its middle (an interval that starts inside the read's left half and ends inside its right half)"""
    sc.check_staircases(stairs["text"], stairs["reads"])
    assert sum(t.startswith("stair") for t, _ in stairs["reads"]) == 12 and sum(t.startswith("hill") for t, _ in stairs["reads"]) == 12
    for L in (150, 250, 300):
        assert sum(len(r) == L for _, r in stairs["reads"]) == 8
    for tag, r in stairs["reads"]:
        got = stairs["fm"].collect_intv(r)
        assert any(int(i) >> 32 == 0 and int(i) & 0xffffffff == len(r) for i in got[:, 3]), tag       # the whole read, once
        if tag.startswith("hill") and not tag.endswith("_rc"):
            mid = len(r) >> 1
            inner = [(int(i) >> 32, int(i) & 0xffffffff) for i in got[:, 3] if 0 < int(i) >> 32 < mid < int(i) & 0xffffffff < len(r)]
            # (a_k falling: every step of the hill is a match of its own; a_k random: only those no other step contains)
            assert len(inner) >= (10 if tag.endswith("_0") else 2), (tag, inner)


@pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref/libbwaref.so not built")
@pytest.mark.parametrize("name,kw", sc.OPTION_SETS, ids=sc.OPTION_IDS)
def test_oracle_matches_the_reference_under_every_option_set(genome, repeats, stairs, name, kw):
    n = 0
    for prefix, fm, reads in ((repeats["prefix"], repeats["fm"], repeats["reads"]),
                              (stairs["prefix"], stairs["fm"], [r for _, r in stairs["reads"]]),
                              (genome["prefix"], po.OracleFM(genome["prefix"]), [r for _, r in sc.edge_reads(genome["seqs"])])):
        ref = po.RefIndex(prefix)
        ropt = ref.opt(**kw)
        for k, (r, b) in enumerate(zip(reads, _oracle(fm, reads, kw))):
            a = ref.collect_intv(ropt, r.copy())
            assert a.shape == b.shape, (name, prefix, k, len(r), a.shape, b.shape)
            assert (_sorted_rows(a) == _sorted_rows(b)).all(), (name, prefix, k)
            assert len(b) < 2 or (np.diff(b[:, 3].astype(np.int64)) >= 0).all()
            n += len(b)
    assert n > 1000 or kw.get("min_seed_len", 19) > 19


def _differ(a, b):
    return sum(x.shape != y.shape or not (x == y).all() for x, y in zip(a, b))


def _gain(a, b):
    return sum(len(y) > len(x) for x, y in zip(a, b))


def test_every_option_set_moves_the_intervals(repeats):
    """on the two batches the GPU test runs every option set on, together"""
    small, _, large = repeats["batches"]
    reads = small + large
    base = _oracle(repeats["fm"], reads, {})
    for name, kw in sc.OPTION_SETS[1:]:
        n = _differ(base, _oracle(repeats["fm"], reads, kw))
        print(name, n)
        assert n >= 20, (name, n)


def test_the_third_pass_and_reseeding_emit(repeats):
    fm = repeats["fm"]
    for reads in repeats["batches"]:
        base = _oracle(fm, reads, {})
        n3 = _gain(_oracle(fm, reads, dict(max_mem_intv=0)), base)
        n2 = _gain(_oracle(fm, reads, dict(split_width=0)), base)
        print(len(reads), n3, n2)
        assert n3 >= 50 and n2 >= 50, (n3, n2)


def test_edge_reads_sit_on_the_boundaries(genome):
    reads = dict(sc.edge_reads(genome["seqs"]))
    lens = {len(r) for r in reads.values()}
    assert {7, 8, 9, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 159, 160, 161, 255, 256, 257} <= lens
    for p in (0, 7, 8, sc.P3_K - 1, sc.P3_K, sc.P3_K + 1, 149):
        r = reads["N@%d/150" % p]
        assert r[p] == 4 and (r > 3).sum() == 1
    assert (np.flatnonzero(reads["N@20+8/150"] > 3) == [20, 28]).all() and (np.flatnonzero(reads["N/13/150"] > 3) == np.arange(0, 150, 13)).all()
    assert (reads["allN/150"] == 4).all() and len(set(reads["homo0/150"])) == 1 and len(set(reads["di01/150"])) == 2
