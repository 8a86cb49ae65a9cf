"""Stage test of the seeding kernels under every option they read and in every instantiation: smem_p3_kernel (csrc/smem_kernels.hip) and
smem_kernel<QLDS, LC, QS, COUNT, KMT> (csrc/fm_kernels.hip) through mi355x_smem_batch against the oracle's mem_collect_intv, read by
read and word by word.  tests/test_smem_cases.py pins the oracle against the reference under the same option sets and shows, on the
CPU, that the cases of tests/smem_cases.py reach what they are meant to reach.

Which kernel runs: the longest read of the batch picks <true, LCAP_S, QSLOT_S>, <true, LCAP, QSLOT> or <false, LCAP, QSLOT>;
MPIBWA_SMEM_COUNT unset picks the counting variant <.., true, false>, MPIBWA_SMEM_COUNT=0 the production variants <.., false, true>
(k-mer tables, built at upload: the default) or <.., false, false> (MPIBWA_KMT=0 at upload)."""
import ctypes as C
import os

import numpy as np
import pytest

import smem_cases as sc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

CAP = 512
_dev = {"key": None, "eng": None}
_fms, _want = {}, {}


def _engine(prefix, kmt=None):
    """the engine of (index, MPIBWA_KMT at upload); the device index is a process-wide singleton, uploaded again when either changes"""
    from mpibwa_amd import api
    if _dev["key"] != (prefix, kmt):
        api.load_library().mi355x_finalize()
        old = os.environ.pop("MPIBWA_KMT", None)
        if kmt is not None:
            os.environ["MPIBWA_KMT"] = kmt
        try:
            _dev.update(key=None, eng=None)
            _dev.update(eng=api.Engine(prefix, device=0), key=(prefix, kmt))
        finally:
            os.environ.pop("MPIBWA_KMT", None)
            if old is not None:
                os.environ["MPIBWA_KMT"] = old
    return _dev["eng"]


@pytest.fixture(scope="module", autouse=True)
def _leave_no_index_behind():
    yield
    from mpibwa_amd import api
    api.load_library().mi355x_finalize()   # (in particular not one uploaded without k-mer tables)
    _dev.update(key=None, eng=None)
    _want.clear()


@pytest.fixture(scope="module")
def repeats(built, tmp_path_factory):
    names, seqs = sc.repeat_genome()
    fa = sc.write_index(tmp_path_factory.mktemp("smem_rep"), "rep", names, seqs)
    r150, rvar, rlong = sc.repeat_reads(seqs)
    return {"prefix": fa, "batches": sc.class_batches(r150, rvar, rlong)}


@pytest.fixture(scope="module")
def stairs(built, tmp_path_factory):
    names, seqs, reads = sc.staircase_genome()
    return {"prefix": sc.write_index(tmp_path_factory.mktemp("smem_stairs"), "stairs", names, seqs), "reads": reads}


def _expected(prefix, reads, kw):
    """-> (the oracle's intervals of every read, the occ blocks the oracle touched for them); a read shorter than a seed never reaches
    mem_collect_intv (src/bwamem.c:260).  Computed once per (index, options, read)."""
    fm = _fms.get(prefix) or _fms.setdefault(prefix, po.OracleFM(prefix))
    args = sc.oracle_args(kw)
    want, blocks = [], 0
    for r in reads:
        key = (prefix, args, r.tobytes())
        if key not in _want:
            if len(r) < args[0]:
                _want[key] = (np.zeros((0, 4), np.uint64), 0)
            else:
                fm.reset_counters()
                _want[key] = (fm.collect_intv(r, *args), int(fm.fm.n_blocks))
        want.append(_want[key][0])
        blocks += _want[key][1]
    return want, blocks


def _compare(eng, prefix, reads, kw, counting, tag, cap=CAP):
    """engine.smem == the oracle: shape and every word of every read; the counting variant's bytes are the oracle's own block count"""
    got, _, nbytes = eng.smem(eng.opt(**kw), reads, cap=cap)
    want, blocks = _expected(prefix, reads, kw)
    assert len(got) == len(reads)
    for k, (r, a, b) in enumerate(zip(reads, got, want)):
        assert a.shape == b.shape, (tag, kw, "read %d of %d bases" % (k, len(r)), a.shape, b.shape, a[:, 2:].tolist(), b[:, 2:].tolist())
        assert (a == b).all(), (tag, kw, "read %d of %d bases" % (k, len(r)), a.tolist(), b.tolist())
    if counting:
        assert nbytes == blocks * 64 + sum(len(r) for r in reads) + 32 * sum(len(b) for b in want), (tag, kw, nbytes, blocks)
    else:
        assert nbytes == 0
    return want


def _variant(monkeypatch, prefix, variant):
    """-> (engine, counting) with the environment of one of the three kernel variants"""
    if variant == "count":
        monkeypatch.delenv("MPIBWA_SMEM_COUNT", raising=False)
    else:
        monkeypatch.setenv("MPIBWA_SMEM_COUNT", "0")
    return _engine(prefix, "0" if variant == "nokmt" else None), variant == "count"


# the variant outermost: the index is uploaded again only where MPIBWA_KMT changes; the last tests of the module use the default again
INSTANCES = [(v, c, o) for v in ("count", "kmt", "nokmt") for c in (0, 1, 2) for o in ("default", "corner")]


@pytest.mark.parametrize("variant,cls,opts", INSTANCES, ids=["%s-class%d-%s" % t for t in INSTANCES])
def test_every_instantiation_matches_the_oracle(repeats, monkeypatch, variant, cls, opts):
    """the nine smem_kernel instantiations: three variants x three batches whose longest read is <= 160, 161-256, > 256 (that one with
    reads on either side of 256: the per-read q_lds), under the default options and with every option off its default at once"""
    eng, counting = _variant(monkeypatch, repeats["prefix"], variant)
    reads = repeats["batches"][cls]
    assert sc.length_class(reads) == cls
    want = _compare(eng, repeats["prefix"], reads, {} if opts == "default" else sc.CORNER, counting, (variant, cls))
    assert sum(len(w) for w in want) > 2 * len(reads)


@pytest.mark.parametrize("which", ["production-class0", "count-class2"])
@pytest.mark.parametrize("name,kw", sc.OPTION_SETS, ids=sc.OPTION_IDS)
def test_every_option_set_matches_the_oracle(repeats, monkeypatch, name, kw, which):
    eng, counting = _variant(monkeypatch, repeats["prefix"], "kmt" if which == "production-class0" else "count")
    _compare(eng, repeats["prefix"], repeats["batches"][0 if which == "production-class0" else 2], kw, counting, which)


@pytest.mark.parametrize("kw", [{}, dict(split_width=200), dict(min_seed_len=10)], ids=["default", "split_width=200", "min_seed_len=10"])
@pytest.mark.parametrize("length", [150, 250, 300])
def test_staircase_reads_match_the_oracle(stairs, monkeypatch, length, kw):
    """interval lists of more than LCAP + 3 entries (tests/smem_cases.py: staircase_genome): the spill to HBM in all three length classes,
    and backward rows of several groups of four whose entries die one by one or share a size; five copies of every read, so that
    several quads spill side by side"""
    reads = [r for _, r in stairs["reads"] if len(r) == length] * 5
    assert len(reads) == 40 and sc.length_class(reads) == (150, 250, 300).index(length)
    for variant in ("kmt", "count"):
        eng, counting = _variant(monkeypatch, stairs["prefix"], variant)
        want = _compare(eng, stairs["prefix"], reads, kw, counting, (variant, length))
        assert all(len(w) >= 1 for w in want)


@pytest.mark.parametrize("kw", [{}, dict(min_seed_len=12), dict(min_seed_len=13)], ids=["default", "min_seed_len=12", "min_seed_len=13"])
def test_edge_reads_match_the_oracle(genome, reads_var, monkeypatch, kw):
    """read lengths around min_seed_len, the jump table's k-mer, the 8-base windows and the LDS slots; ambiguous bases on the same edges;
    homopolymers and short tandem repeats; alone and among ordinary reads, in each length class"""
    edge = [r for _, r in sc.edge_reads(genome["seqs"])]
    var = [np.asarray(r[1], np.uint8) for r in reads_var[:60]]
    for variant in ("kmt", "count"):
        eng, counting = _variant(monkeypatch, genome["prefix"], variant)
        for top in (sc.QSLOT_S, sc.QSLOT, 1 << 30):
            _compare(eng, genome["prefix"], [r for r in edge if len(r) <= top], kw, counting, (variant, top))
        mixed = [r for pair in zip(edge, var * (len(edge) // len(var) + 1)) for r in pair]
        _compare(eng, genome["prefix"], mixed, kw, counting, (variant, "mixed"))


@pytest.mark.parametrize("variant", ["kmt", "count"])
def test_batch_sizes_around_the_fetch_and_the_workgroup(genome, reads_pe, reads_var, monkeypatch, variant):
    """the first n reads of one list, n around SMEM_FETCH (16 reads per refill of a wave), a workgroup of smem_kernel (64 quads) and
    one of smem_p3_kernel (256 lanes): what a read gets does not depend on the batch it came in"""
    eng, counting = _variant(monkeypatch, genome["prefix"], variant)
    pe = [np.asarray(s, np.uint8) for rd in reads_pe[:160] for s in rd[1:3]]
    var = [np.asarray(r[1], np.uint8) for r in reads_var]
    reads = [r for pair in zip(pe, var) for r in pair]
    assert len(reads) == 600
    full = _compare(eng, genome["prefix"], reads, {}, counting, "full batch")
    for n in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257):
        got, _, _ = eng.smem(eng.opt(), reads[:n], cap=CAP)
        assert len(got) == n
        for k in range(n):
            assert got[k].shape == full[k].shape and (got[k] == full[k]).all(), (n, k)


def _smem_raw(eng, opt, seqs, cap):
    """mi355x_smem_batch itself: Engine.smem raises on overflow, the entry point still hands back every read"""
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.concatenate(seqs).astype(np.uint8)
    out = np.zeros((len(seqs), cap, 4), dtype=np.uint64)
    cnt = np.zeros(len(seqs), dtype=np.int32)
    ms, nbytes = C.c_double(0), C.c_uint64(0)
    rc = eng.lib.mi355x_smem_batch(opt, len(seqs), flat.ctypes.data, off.ctypes.data, cap, out.ctypes.data, cnt.ctypes.data,
                                   C.byref(ms), C.byref(nbytes))
    return rc, out, cnt


def _check_overflow(eng, prefix, reads, cap, tag):
    """cap too small for some reads: reported, those reads counted past cap, every other read as the oracle has it"""
    want, _ = _expected(prefix, reads, {})
    rc, out, cnt = _smem_raw(eng, eng.opt(), reads, cap)
    assert rc != 0, tag
    n_over = n_fit = 0
    for k, w in enumerate(want):
        if len(w) > cap:
            assert cnt[k] > cap, (tag, k, cnt[k], len(w))
            n_over += 1
        else:
            assert cnt[k] == len(w) and (out[k, :len(w)] == w).all(), (tag, k, cnt[k], len(w))
            n_fit += 1
    return n_over, n_fit


@pytest.mark.parametrize("variant", ["kmt", "count"])
def test_overflow_is_reported_and_spares_the_other_reads(repeats, monkeypatch, variant):
    eng, counting = _variant(monkeypatch, repeats["prefix"], variant)
    prefix, reads = repeats["prefix"], repeats["batches"][2]
    want, _ = _expected(prefix, reads, {})
    most = max(len(w) for w in want)
    _compare(eng, prefix, reads, {}, counting, "cap == the largest count", cap=most)
    with pytest.raises(RuntimeError):
        eng.smem(eng.opt(), reads, cap=most - 1)
    n_over, n_fit = _check_overflow(eng, prefix, reads, most - 1, "cap == the largest count - 1")
    assert n_over >= 1 and n_fit >= len(reads) - 10
    # a read whose third pass alone overflows (smem_kernel finds nout > cap when it takes the read over); passes 1 and 2 do not look at
    # max_mem_intv and the third pass looks at nothing else, so its count is what max_mem_intv = 0 takes away
    p3 = [len(w) - len(v) for w, v in zip(want, _expected(prefix, reads, dict(max_mem_intv=0))[0])]
    k = int(np.argmax(p3))
    cap = p3[k] - 1
    assert cap >= 8
    n_over, n_fit = _check_overflow(eng, prefix, reads, cap, "cap == a third pass's count - 1")
    assert n_over >= 1 and n_fit >= 50, (cap, n_over, n_fit)
    with pytest.raises(RuntimeError):
        eng.smem(eng.opt(), reads, cap=cap)
