"""End-to-end parity of single-end calls of mem_process_seqs() with se_wave_kernel in the SAM stage (se_simple_kernel -> se_wave_kernel
on the reads it leaves for long lists or an XA tag -> a CIGAR-and-SAM job of their own) against the compiled reference
(oracle/_ref/libbwaref.so), byte for byte: the mates of tests/pair_wave_cases.py's pairs as single-end reads (tests/se_wave_cases.py)
and the repeat-rich recipe of tests/test_gpu_se_e2e.py (1 200 reads), under the default options, XA_drop_ratio = 0.5, max_XA_hits = 8
and without qualities, and with MPIBWA_SUBBATCH_MIN=100 and MPIBWA_SAM_PARTS=2.

The counters, with the reference alone deciding the denominators (its own mem_align1_core lists and mem_reg2sam text per read:
se_wave_cases.eligible / klass): n_se_wave_dev is at least half the eligible plain reads with more than eight regions, n_se_xa_dev at
least half the eligible XA reads, n_se_xa_sam_dev <= n_se_xa_dev.  With MPIBWA_HOST_SE_WAVE=1 the three are 0, n_se_dev and n_sam_dev
are what se_simple_kernel alone gives, and the SAM is the same; with MPIBWA_HOST_XA=1 n_se_xa_dev is 0 and n_se_wave_dev unchanged;
under -a, -5 and with a comment column all three are 0; a paired call afterwards reports n_pair_dev > 0 and the three at 0."""
import ctypes as C

import numpy as np
import pytest

import se_wave_cases as swc
from mpibwa_amd import abi, simulate
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

NEW = ("n_se_wave_dev", "n_se_xa_dev", "n_se_xa_sam_dev")
_CODE = {65: 0, 67: 1, 71: 2, 84: 3}


def _cases_of(reads):
    """[(name, ACGT bytes, None)] -> the case dicts of se_wave_cases.reference_side"""
    return [dict(family="real", tag="e", name=n.encode() if isinstance(n, str) else n,
                 read=np.array([_CODE.get(b, 4) for b in s], dtype=np.uint8), expect=None) for n, s, _ in reads]


def _denominators(ref, kw, reads, n_processed=0):
    """eligible reads by class, from the reference alone (read number = place in the chunk)"""
    cases = _cases_of(reads)
    want = swc.reference_side(ref, ref.opt(**kw), cases, True, n_processed, np.arange(len(cases)))
    return swc.census(cases, want)


def _cmp(eng, ref, reads, kw, **pk):
    want = ref.process(ref.opt(**kw), reads, **pk)
    got = eng.process(eng.opt(**kw), reads, **pk)
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, (kw, pk, len(bad), bad[:5], got[bad[0]][:600], want[bad[0]][:600])
    return want


@pytest.fixture(scope="module")
def wave(tmp_path_factory, built):
    import pair_wave_cases as pw
    from mpibwa_amd import api
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    api.load_library().mi355x_finalize()
    g = pw.build_index(tmp_path_factory.mktemp("se_wave_e2e"))
    reads = [(cs["name"].decode(), bytes(b"ACGTN"[c] for c in cs["read"]), None) for cs in swc.realistic_cases(g)]
    out = {"eng": api.Engine(g["prefix"], device=0), "ref": po.RefIndex(g["prefix"]), "reads": reads,
           "pairs": simulate.reads_to_ascii(pw.make_reads(g["seqs"], g["copies"], False)[:300])}
    yield out
    api.load_library().mi355x_finalize()


def _check_counters(st, c, tag):
    print(tag, "reference: eligible plain > 8 regions", c["plain_gt8"], "eligible XA", c["xa"], "| n_se_dev", st["n_se_dev"], "n_sam_dev", st["n_sam_dev"],
          "n_se_wave_dev", st["n_se_wave_dev"], "n_se_xa_dev", st["n_se_xa_dev"], "n_se_xa_sam_dev", st["n_se_xa_sam_dev"])
    assert st["n_se_wave_dev"] * 2 >= c["plain_gt8"], (tag, st["n_se_wave_dev"], c["plain_gt8"])
    assert st["n_se_xa_dev"] * 2 >= c["xa"], (tag, st["n_se_xa_dev"], c["xa"])
    assert st["n_se_xa_sam_dev"] <= st["n_se_xa_dev"]
    assert st["n_se_wave_dev"] <= st["n_se_dev"] and st["n_sam_dev"] <= st["n_se_dev"] <= c["reads"]


@pytest.mark.parametrize("kw,pk", [(dict(flag=0), {}), (dict(flag=0, XA_drop_ratio=0.5), {}), (dict(flag=0, max_XA_hits=8), {}),
                                   (dict(flag=0), dict(with_qual=False))])
def test_single_end_calls_on_the_pair_wave_mates(wave, kw, pk):
    eng, ref, reads = wave["eng"], wave["ref"], wave["reads"]
    _cmp(eng, ref, reads, kw, n_processed=4000, **pk)
    c = _denominators(ref, kw, reads, 4000)
    assert c["plain_gt8"] >= 50 and c["xa"] >= 50, c
    _check_counters(eng.stats(), c, "%s %s" % (kw, pk))


def test_switches_sub_batches_parts_and_a_paired_call_afterwards(wave, monkeypatch):
    eng, ref, reads = wave["eng"], wave["ref"], wave["reads"]
    kw = dict(flag=0)
    want = _cmp(eng, ref, reads, kw)
    on = eng.stats()
    _check_counters(on, _denominators(ref, kw, reads), "default")
    assert on["n_se_wave_dev"] > 0 and on["n_se_xa_dev"] > 0 and on["n_se_xa_sam_dev"] > 0
    # off: the three counters are 0, the other two are se_simple_kernel's alone, the SAM is the same
    monkeypatch.setenv("MPIBWA_HOST_SE_WAVE", "1")
    assert eng.process(eng.opt(**kw), reads) == want
    off = eng.stats()
    assert all(off[k] == 0 for k in NEW), off
    assert off["n_se_dev"] == on["n_se_dev"] - on["n_se_wave_dev"] and 0 < off["n_sam_dev"] <= off["n_se_dev"]
    assert 0 <= on["n_sam_dev"] - off["n_sam_dev"] <= on["n_se_wave_dev"]
    monkeypatch.delenv("MPIBWA_HOST_SE_WAVE")
    # the XA half alone off: long plain lists are still decided
    monkeypatch.setenv("MPIBWA_HOST_XA", "1")
    assert eng.process(eng.opt(**kw), reads) == want
    st = eng.stats()
    assert st["n_se_xa_dev"] == 0 and st["n_se_xa_sam_dev"] == 0 and st["n_se_wave_dev"] == on["n_se_wave_dev"] and st["n_se_dev"] == on["n_se_dev"], st
    monkeypatch.delenv("MPIBWA_HOST_XA")
    for var, val in (("MPIBWA_SUBBATCH_MIN", "100"), ("MPIBWA_SAM_PARTS", "2")):
        monkeypatch.setenv(var, val)
        assert eng.process(eng.opt(**kw), reads) == want
        st = eng.stats()
        assert all(st[k] == on[k] for k in NEW + ("n_se_dev", "n_sam_dev")), (var, st, on)
        monkeypatch.delenv(var)
    # the calls that are the host's: -a, -5, a comment column
    for kw2, pk in ((dict(flag=abi.MEM_F_ALL), {}), (dict(flag=abi.MEM_F_PRIMARY5), {}), (dict(flag=0), dict(comment="BC:Z:ACGT+TTAG"))):
        _cmp(eng, ref, reads[:1500], kw2, **pk)
        st = eng.stats()
        assert all(st[k] == 0 for k in NEW) and st["n_se_dev"] == 0, (kw2, pk, st)
    _cmp(eng, ref, wave["pairs"], dict(flag=abi.MEM_F_PE))
    st = eng.stats()
    assert st["n_pair_dev"] > 0 and all(st[k] == 0 for k in NEW) and st["n_se_dev"] == 0, st


def test_repeat_rich_single_end(tmp_path_factory, built):
    """the recipe of tests/test_gpu_se_e2e.py: dozens of regions per read, XA tags"""
    from mpibwa_amd import api, bigindex
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    lib = api.load_library()
    lib.mi355x_finalize()
    lib.mi355x_index_build_gpu.restype = C.c_int
    lib.mi355x_index_build_gpu.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_char_p, C.POINTER(C.c_double)]
    pac, lens = bigindex.synth_packed_genome_grch38like(6e6, seed=17, n_contigs=3, repeat_frac=0.5)
    prefix = str(tmp_path_factory.mktemp("rep_se_wave") / "rep.fa")
    bigindex.write_meta_files(prefix, pac, lens)
    secs = C.c_double(0)
    assert lib.mi355x_index_build_gpu(0, pac.ctypes.data, int(lens.sum()), prefix.encode(), C.byref(secs)) == 0
    eng = api.Engine(prefix, device=0)
    idx, ref = bigindex.BigIndex(prefix, pac, lens, eng), po.RefIndex(prefix)
    se = [(n, a, None) for n, a, _ in idx.simulate_pairs(1200, seed=105, read_len=150)]
    for kw, pk in ((dict(flag=0), {}), (dict(flag=0, XA_drop_ratio=0.5), {}), (dict(flag=0, max_XA_hits=8), {}), (dict(flag=0), dict(with_qual=False))):
        _cmp(eng, ref, se, kw, **pk)
        st = eng.stats()
        c = _denominators(ref, kw, se)
        _check_counters(st, c, "repeat-rich %s %s" % (kw, pk))
        assert c["plain_gt8"] + c["xa"] >= 50, c
    lib.mi355x_finalize()
