"""The device tables derived from an index at upload (occ32_build_kernel, kmt_build_kernel, p3_build_kernel, sa_expand_kernel) and the
kernels that read them (sa_kernel, sa_dense_kernel, smem_kernel, smem_p3_kernel) on ten degenerate indexes of tests/index_cases.py: one
occ block, no SA sample beside row 0, `primary` in the first and the last row, bases the text lacks, a text that is one period or its
own reverse complement.  The suffix array is compared row by row — every row, not a sample — with the plain model
(tests/index_model.py), the intervals word by word with the oracle's mem_collect_intv (held against the reference's on the same reads
and indexes in tests/test_index_cases.py).  The default tables are under test: no upload option is set but MPIBWA_KMT=0 for the variant
without k-mer tables."""
import numpy as np
import pytest

import index_cases as ic
import index_model as im
import smem_cases as sc
import test_gpu_smem_options as so
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

ROW0 = np.uint64(0xFFFFFFFFFFFFFFFF)      # bwt_sa(0): the stored sa[0] = -1 (src/bwt.c:86-96)


@pytest.fixture(scope="module", autouse=True)
def _leave_no_index_behind():
    yield
    from mpibwa_amd import api
    api.load_library().mi355x_finalize()
    so._dev.update(key=None, eng=None)
    so._want.clear()


@pytest.fixture(scope="module")
def indexes(built, tmp_path_factory):
    """name -> (case, prefix of its index as the CPU builder writes it: equal to the model, tests/test_index_cases.py)"""
    d = tmp_path_factory.mktemp("fm_degenerate")
    out = {}
    for k, name in enumerate(ic.FM_CASES):
        c = ic.by_name(name)
        out[name] = (c, sc.write_index(d, "i%d" % k, c.names(), c.seqs()))
    return out


@pytest.mark.parametrize("name", ic.FM_CASES)
def test_every_row_of_the_suffix_array(indexes, name):
    """sa_kernel's walk on every row 0 .. N (row 0 as bwt_sa has it) and the dense table of sa_expand_kernel on every row 1 .. N against
    the model's suffix array; the walk's bytes are the oracle's LF steps"""
    c, prefix = indexes[name]
    eng = so._engine(prefix)
    sa_full = im.index_files(c.codes)[2].astype(np.uint64)
    N = 2 * c.l_pac
    assert len(sa_full) == N + 1 and int(eng.bwt.contents.seq_len) == N and int(eng.bwt.contents.n_sa) == (N + 32) // 32
    rows = np.arange(N + 1, dtype=np.uint64)
    fm = po.OracleFM(prefix)
    fm.reset_counters()
    for r in rows:
        fm.sa_lookup(int(r))
    got, _, nbytes = eng.sa(rows)
    want = sa_full.copy()
    want[0] = ROW0
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (name, "walk", len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert nbytes == fm.fm.n_sa_steps * 64 + 8 * len(rows), (name, nbytes, int(fm.fm.n_sa_steps))
    res = eng.sa_dense(rows[1:])
    assert res is not None, "dense SA was not expanded at upload"
    bad = np.flatnonzero(res[0] != want[1:])
    assert len(bad) == 0, (name, "dense", len(bad), (bad[:8] + 1).tolist(), res[0][bad[:8]].tolist(), want[1:][bad[:8]].tolist())
    if N >= 32:         # the sampled rows themselves, in an order of their own
        ks = rows[::32][::-1].copy()
        assert (eng.sa(ks)[0][:-1] == want[::32][::-1][:-1]).all()


INSTANCES = [(n, v, o) for n in ic.FM_CASES for v in ("count", "kmt", "nokmt") for o in ("default", "corner")]


@pytest.mark.parametrize("name,variant,opts", INSTANCES, ids=["%s-%s-%s" % t for t in INSTANCES])
def test_intervals_match_the_oracle(indexes, monkeypatch, name, variant, opts):
    """the three kernel variants under the default options and with every option off its default: substrings of the text at its start,
    its end and across the strand boundary, with and without a substitution, and reads longer than the whole text — every word"""
    c, prefix = indexes[name]
    eng, counting = so._variant(monkeypatch, prefix, variant)
    reads = [r for _, r in ic.fm_reads(c)]
    kw = {} if opts == "default" else sc.CORNER
    want = []
    for cls in (0, 1, 2):           # one launch per length class, as launch_smem picks its instantiation
        batch = [r for r in reads if sc.length_class([r]) == cls]
        if batch:
            want += so._compare(eng, prefix, batch, kw, counting, (name, variant, cls))
    assert len(want) == len(reads)
    if 2 * c.l_pac >= sc.oracle_args(kw)[0]:      # (a text shorter than a seed holds none)
        assert sum(len(w) for w in want) >= 1
    if name == "homoA":             # every extension changes the size: the lists of the long reads live in the HBM spill
        assert max(len(r) for r in reads) == 257 and sc.list_entries(c.codes, np.zeros(150, np.uint8), 0) > sc.LCAP


@pytest.mark.parametrize("variant", ["count", "kmt", "nokmt"])
@pytest.mark.parametrize("name", ["homoA", "fibGT"])
def test_reads_with_a_base_the_text_lacks(indexes, monkeypatch, name, variant):
    """C in reads on an index without C (A x 4099: neither strand has it) and on one whose forward strand lacks it (the Fibonacci word
    over G, T).  A sweep that starts on the lacking base begins with an empty interval, walks to the end of the read and reports it
    (size 0); the k-mer tables must hand such a sweep what its steps would give.  Every word of every entry is the oracle's."""
    c, prefix = indexes[name]
    eng, counting = so._variant(monkeypatch, prefix, variant)
    reads = [r for _, r in ic.absent_base_reads(c)]
    n_empty = 0
    for kw in ({}, sc.CORNER):
        for cls in (0, 2):
            batch = [r for r in reads if sc.length_class([r]) == cls]
            want = so._compare(eng, prefix, batch, kw, counting, (name, variant, cls))
            n_empty += sum(int((w[:, 2] == 0).sum()) for w in want)
    if name == "homoA":
        assert n_empty >= 10, n_empty       # the empty interval is reported: the case is what it claims to be
