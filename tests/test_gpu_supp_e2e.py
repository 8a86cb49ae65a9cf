"""End-to-end parity of single-end calls of mem_process_seqs() whose chunk holds reads with supplementary lines (se_simple_kernel ->
se_wave_kernel on the reads it leaves, status 10 among them -> their requests in the CIGAR-and-SAM job of se_wave_kernel's reads ->
sam_lines_kernel behind sam_emit_kernel) against the compiled reference (oracle/_ref/libbwaref.so), byte for byte: the chimeras of
tests/supp_cases.py mixed 1 : 3 with the ordinary reads of tests/se_wave_cases.py, under the default options, -Y, -M and without
qualities; with MPIBWA_SUBBATCH_MIN=100 and MPIBWA_SAM_PARTS=2; with three calls in flight from threads.

The counters, with MPIBWA_HOST_SUPP=0 set explicitly and the reference alone deciding the denominator (supp_cases.eligible on its own
mem_align1_core lists and mem_reg2sam text): n_se_supp_dev is at least half the eligible reads, n_se_supp_sam_dev <= n_se_supp_dev, and
the other n_se_* counters and n_sam_dev are exactly what they are with MPIBWA_HOST_SUPP=1.  With MPIBWA_HOST_SUPP=1, with
MPIBWA_HOST_SE_WAVE=1, under -a, -5, with a comment column and in a paired call afterwards both new counters are 0 and the SAM is the
same.
Measured on the MI355X (1 128 reads, 275 of them eligible under every option set): n_se_supp_dev 275, n_se_supp_sam_dev 275; n_se_dev 806,
n_se_wave_dev 148, n_se_xa_dev 42, n_se_xa_sam_dev 42 and n_sam_dev 806 with the path on and off."""
import threading

import numpy as np
import pytest

import se_wave_cases as swc
import supp_cases as spc
from mpibwa_amd import abi, simulate
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

NEW = ("n_se_supp_dev", "n_se_supp_sam_dev")
OTHERS = ("n_se_dev", "n_se_wave_dev", "n_se_xa_dev", "n_se_xa_sam_dev", "n_sam_dev")


def _cmp(eng, ref, reads, kw, **pk):
    want = ref.process(ref.opt(**kw), reads, **pk)
    got = eng.process(eng.opt(**kw), reads, **pk)
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, (kw, pk, len(bad), bad[:5], got[bad[0]][:900], want[bad[0]][:900])
    return want


@pytest.fixture(scope="module")
def mix(tmp_path_factory, built):
    import pair_wave_cases as pw
    from mpibwa_amd import api
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    api.load_library().mi355x_finalize()
    g = pw.build_index(tmp_path_factory.mktemp("supp_e2e"))
    chim = spc.realistic_cases(g)
    plain = swc.realistic_cases(g)[:3 * len(chim)]
    cases = []
    for k, cs in enumerate(chim):   # one chimera, three ordinary reads
        cases += [cs] + plain[3 * k:3 * k + 3]
    reads = [(cs["name"].decode(), bytes(b"ACGTN"[c] for c in cs["read"]), None) for cs in cases]
    out = {"eng": api.Engine(g["prefix"], device=0), "ref": po.RefIndex(g["prefix"]), "reads": reads, "cases": cases,
           "pairs": simulate.reads_to_ascii(pw.make_reads(g["seqs"], g["copies"], False)[:300])}
    yield out
    api.load_library().mi355x_finalize()


def _eligible(ref, kw, cases, n_processed=0):
    """the eligible reads of several lines, from the reference alone (read number = place in the chunk)"""
    cs = [dict(c) for c in cases]
    want = spc.reference_side(ref, ref.opt(**kw), cs, True, n_processed, np.arange(len(cs)))
    return sum(spc.eligible(c, w[0]) for c, w in zip(cs, want))


@pytest.mark.parametrize("kw,pk", [(dict(flag=0), {}), (dict(flag=abi.MEM_F_SOFTCLIP), {}), (dict(flag=abi.MEM_F_NO_MULTI), {}), (dict(flag=0), dict(with_qual=False))])
def test_single_end_calls_with_chimeric_reads(mix, kw, pk, monkeypatch):
    eng, ref, reads = mix["eng"], mix["ref"], mix["reads"]
    monkeypatch.setenv("MPIBWA_HOST_SUPP", "0")
    want = _cmp(eng, ref, reads, kw, n_processed=4000, **pk)
    on = eng.stats()
    n_el = _eligible(ref, kw, mix["cases"], 4000)
    print(kw, pk, "reads", len(reads), "eligible reads of several lines", n_el, {k: on[k] for k in NEW + OTHERS})
    assert n_el >= 200 and on["n_se_supp_dev"] * 2 >= n_el and on["n_se_supp_sam_dev"] <= on["n_se_supp_dev"], (n_el, on)
    assert on["n_se_supp_sam_dev"] > 0 and on["n_sam_dev"] <= on["n_se_dev"]
    monkeypatch.setenv("MPIBWA_HOST_SUPP", "1")
    assert eng.process(eng.opt(**kw), reads, n_processed=4000, **pk) == want
    off = eng.stats()
    assert all(off[k] == 0 for k in NEW) and all(off[k] == on[k] for k in OTHERS), (on, off)


def test_switches_sub_batches_parts_callers_and_a_paired_call_afterwards(mix, monkeypatch):
    eng, ref, reads = mix["eng"], mix["ref"], mix["reads"]
    kw = dict(flag=0)
    monkeypatch.setenv("MPIBWA_HOST_SUPP", "0")
    want = _cmp(eng, ref, reads, kw)
    on = eng.stats()
    assert on["n_se_supp_dev"] > 0 and on["n_se_supp_sam_dev"] > 0, on
    for var, val in (("MPIBWA_SUBBATCH_MIN", "100"), ("MPIBWA_SAM_PARTS", "2")):
        monkeypatch.setenv(var, val)
        assert eng.process(eng.opt(**kw), reads) == want, var
        st = eng.stats()
        assert all(st[k] == on[k] for k in NEW + OTHERS), (var, st, on)
        monkeypatch.delenv(var)
    # three calls in flight
    out, err = {}, []

    def caller(t):
        try:
            for r in range(2):
                out[(t, r)] = eng.process(eng.opt(**kw), reads)
        except BaseException as e:   # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=caller, args=(t,)) for t in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    assert len(out) == 6 and all(got == want for got in out.values())
    # off: by its own switch and by se_wave_kernel's
    for var in ("MPIBWA_HOST_SUPP", "MPIBWA_HOST_SE_WAVE"):
        monkeypatch.setenv(var, "1")
        assert eng.process(eng.opt(**kw), reads) == want, var
        st = eng.stats()
        assert all(st[k] == 0 for k in NEW), (var, st)
        monkeypatch.setenv("MPIBWA_HOST_SUPP", "0")
        monkeypatch.delenv("MPIBWA_HOST_SE_WAVE", raising=False)
    # the calls that are the host's: -a, -5, a comment column
    for kw2, pk in ((dict(flag=abi.MEM_F_ALL), {}), (dict(flag=abi.MEM_F_PRIMARY5), {}), (dict(flag=0), dict(comment="BC:Z:ACGT+TTAG"))):
        _cmp(eng, ref, reads, kw2, **pk)
        st = eng.stats()
        assert all(st[k] == 0 for k in NEW), (kw2, pk, st)
    _cmp(eng, ref, mix["pairs"], dict(flag=abi.MEM_F_PE))
    st = eng.stats()
    assert st["n_pair_dev"] > 0 and all(st[k] == 0 for k in NEW), st
