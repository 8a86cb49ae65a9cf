"""End-to-end parity of paired calls of mem_process_seqs() whose chunk holds pairs that mem_sam_pe reports end by end (pair_simple_kernel
-> pair_wave_kernel on the pairs it leaves, codes 8 / 9 / 10 and the pairs without a hit among them -> status 17 -> their requests in the
CIGAR-and-SAM job of the wave's XA pairs -> the paired instantiation of sam_lines_kernel behind sam_emit_kernel) against the compiled
reference (oracle/_ref/libbwaref.so), byte for byte: sets (a) and (b) of tests/pair_lines_cases.py mixed 1 : 2 with the ordinary pairs of
tests/pair_wave_cases.py; with the path on and with MPIBWA_HOST_PAIR_LINES=1; with one sub-batch and with two (MPIBWA_SUBBATCH_MIN,
MPIBWA_SAM_PARTS=2); with two calls in flight from threads; under -a / -5 / -P, where the path is off.

The counters, the reference alone deciding the denominator (pair_lines_cases.eligible on its own lists and text): n_pair_lines_dev is at
least half the eligible pairs, 0 < n_pair_lines_sam_dev <= n_pair_lines_dev, and every other counter of mi355x_stats_t is what it is with
MPIBWA_HOST_PAIR_LINES=1 — n_aln apart, the number of CIGAR requests aln_kernel answered: it is lower with the path on, because the
host's list asks for the two mates' alignments of src/bwamem_pair.c:379-380 next to the lines' own, where the device reads line 0 of the
other end.
Measured on the MI355X: 1 887 pairs, 533 eligible; n_pair_lines_dev 483, n_pair_lines_sam_dev 483; n_pair_dev 986, n_pair_wave_dev 281,
n_pair_xa_dev 123, n_sam_dev 2 780 and n_msw 10 758 with the path on and off; n_aln 9 931 on, 10 739 off."""
import threading

import pytest

import pair_lines_cases as plc
from mpibwa_amd import abi, simulate
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

NEW = ("n_pair_lines_dev", "n_pair_lines_sam_dev")
N_PROCESSED = 4000


def _counters(st):
    return {k: v for k, v in st.items() if k.startswith("n_") and k not in NEW and k != "n_aln"}


@pytest.fixture(scope="module")
def mix(tmp_path_factory, built):
    import pair_wave_cases as pw
    from mpibwa_amd import api
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    api.load_library().mi355x_finalize()
    g = pw.build_index(tmp_path_factory.mktemp("pair_lines_e2e"))
    b, _ = plc.set_b(g)
    special = plc.set_a(g) + b[plc.B_N_PLAIN:]
    plain = pw.make_reads(g["seqs"], g["copies"], False)[:2 * len(special)]
    reads = []
    for k, p in enumerate(special):   # one of the sets' pairs, two ordinary pairs
        reads += [("s%d_%s" % (k, p[0]), p[1], p[2])] + plain[2 * k:2 * k + 2]
    out = {"eng": api.Engine(g["prefix"], device=0), "ref": po.RefIndex(g["prefix"]), "reads": simulate.reads_to_ascii(reads)}
    yield out
    api.load_library().mi355x_finalize()


def _eligible(ref, reads, n_processed):
    ropt = ref.opt(flag=abi.MEM_F_PE)
    codes, lists, pes = plc.phase1(ref, ropt, reads)
    return sum(plc.eligible(P) for P in plc.reference_pairs(ref, ropt, [r[0] for r in reads], codes, lists, pes, n_processed))


def test_paired_calls_with_pairs_reported_end_by_end(mix, monkeypatch):
    eng, ref, reads = mix["eng"], mix["ref"], mix["reads"]
    kw = dict(flag=abi.MEM_F_PE)
    monkeypatch.setenv("MPIBWA_HOST_PAIR_LINES", "0")
    want = ref.process(ref.opt(**kw), reads, n_processed=N_PROCESSED)
    got = eng.process(eng.opt(**kw), reads, n_processed=N_PROCESSED)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert len(got) == len(want) and not bad, (len(bad), bad[:5], got[bad[0]][:900], want[bad[0]][:900])
    on = eng.stats()
    n_el = _eligible(ref, reads, N_PROCESSED)
    print("pairs", len(reads), "eligible", n_el, {k: on[k] for k in NEW}, _counters(on), "n_aln", on["n_aln"])
    assert n_el >= 490 and on["n_pair_lines_dev"] * 2 >= n_el, (n_el, on)
    assert 0 < on["n_pair_lines_sam_dev"] <= on["n_pair_lines_dev"], on
    monkeypatch.setenv("MPIBWA_HOST_PAIR_LINES", "1")
    assert eng.process(eng.opt(**kw), reads, n_processed=N_PROCESSED) == want
    off = eng.stats()
    print("off", _counters(off), "n_aln", off["n_aln"])
    assert all(off[k] == 0 for k in NEW) and _counters(off) == _counters(on), (on, off)
    # one sub-batch and two, one part and two: the same text, the same counters
    monkeypatch.setenv("MPIBWA_HOST_PAIR_LINES", "0")
    for var, val in (("MPIBWA_SUBBATCH_MIN", "100"), ("MPIBWA_SUBBATCH_MIN", "100000000"), ("MPIBWA_SAM_PARTS", "2")):
        monkeypatch.setenv(var, val)
        assert eng.process(eng.opt(**kw), reads, n_processed=N_PROCESSED) == want, (var, val)
        st = eng.stats()
        assert all(st[k] == on[k] for k in NEW) and {k: v for k, v in _counters(st).items() if k != "n_sub"} == {k: v for k, v in _counters(on).items() if k != "n_sub"}, (var, val, st, on)
        monkeypatch.delenv(var)


def test_two_callers_and_the_calls_that_are_the_hosts(mix, monkeypatch):
    eng, ref, reads = mix["eng"], mix["ref"], mix["reads"][:600]
    kw = dict(flag=abi.MEM_F_PE)
    monkeypatch.setenv("MPIBWA_HOST_PAIR_LINES", "0")
    want = ref.process(ref.opt(**kw), reads)
    out, err = {}, []

    def caller(t):
        try:
            for r in range(2):
                out[(t, r)] = eng.process(eng.opt(**kw), reads)
        except BaseException as e:   # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=caller, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    assert len(out) == 4 and all(got == want for got in out.values())
    assert eng.stats()["n_pair_lines_dev"] > 0
    # off with pair_wave_kernel, and in the calls that are the host's: -a, -5, -P
    monkeypatch.setenv("MPIBWA_HOST_RESCUE", "1")
    assert eng.process(eng.opt(**kw), reads) == want
    assert all(eng.stats()[k] == 0 for k in NEW)
    monkeypatch.delenv("MPIBWA_HOST_RESCUE")
    for f in (abi.MEM_F_ALL, abi.MEM_F_PRIMARY5, abi.MEM_F_NOPAIRING):
        kw2 = dict(flag=abi.MEM_F_PE | f)
        assert eng.process(eng.opt(**kw2), reads) == ref.process(ref.opt(**kw2), reads), f
        st = eng.stats()
        assert all(st[k] == 0 for k in NEW), (f, st)
