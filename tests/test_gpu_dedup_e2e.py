"""Whole mem_process_seqs calls with the redundancy pass of mem_sort_dedup_patch on the device (dedup_kernel.hip behind reg_pack and
first_reg in phase 1): paired and single-end calls on the session genome, sub-batched and as one chunk, with three callers in flight, and
once on the repeat-rich genome of tests/test_gpu_repeats.py.  MPIBWA_DEV_DEDUP=1 enables the stage (the tests set it: DESIGN §4.3c says
why it ships switched off).  The SAM text equals the reference's mem_process_seqs byte for byte, with the stage and with
MPIBWA_HOST_DEDUP=1 on top, which restores the host's path.  The counters: with the switch n_dedup_dev is 0 and n_dedup_host is the sum
of both counters of the run without it (the reads with two or more raw regions); without it n_dedup_dev > 0; a call with neither
variable counts as the one with the switch.  The split is printed, without a floor."""
import threading

import pytest

from mpibwa_amd import abi, simulate
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def both(genome):
    from mpibwa_amd import api
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    api.load_library().mi355x_finalize()   # the device index is a process-wide singleton: (re)upload this module's genome
    return api.Engine(genome["prefix"], device=0), po.RefIndex(genome["prefix"])


def _same(got, want, tag):
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, (tag, len(bad), bad[:5], got[bad[0]][:500], want[bad[0]][:500])


def _with_and_without(eng, opt, reads, want, monkeypatch, tag):
    monkeypatch.delenv("MPIBWA_DEV_DEDUP", raising=False)
    _same(eng.process(opt, reads), want, (tag, "no variable"))
    plain = eng.stats()
    monkeypatch.setenv("MPIBWA_DEV_DEDUP", "1")
    _same(eng.process(opt, reads), want, tag)
    on = eng.stats()
    monkeypatch.setenv("MPIBWA_HOST_DEDUP", "1")
    _same(eng.process(opt, reads), want, (tag, "MPIBWA_HOST_DEDUP"))
    off = eng.stats()
    monkeypatch.delenv("MPIBWA_HOST_DEDUP")
    print(tag, "reads", on["n_reads"], "with two or more raw regions", on["n_dedup_dev"] + on["n_dedup_host"], "taken from the device", on["n_dedup_dev"],
          "sorted by the host", on["n_dedup_host"])
    assert on["n_dedup_dev"] > 0, (tag, on["n_dedup_dev"], on["n_dedup_host"])
    assert off["n_dedup_dev"] == 0 and off["n_dedup_host"] == on["n_dedup_dev"] + on["n_dedup_host"], (tag, off["n_dedup_dev"], off["n_dedup_host"], on)
    assert (plain["n_dedup_dev"], plain["n_dedup_host"]) == (0, off["n_dedup_host"]), (tag, plain["n_dedup_dev"], plain["n_dedup_host"])
    return on


@pytest.mark.parametrize("sub", ["2", "1"])
def test_paired_and_single_end_calls(both, reads_pe, reads_var, monkeypatch, sub):
    eng, ref = both
    monkeypatch.setenv("MPIBWA_SUBBATCH_MIN", "100")   # sub-batches and lanes as for big chunks
    monkeypatch.setenv("MPIBWA_SUBBATCH", sub)         # 2: two sub-batches on two lanes; 1: the chunk in one piece
    pe, se = simulate.reads_to_ascii(reads_pe), simulate.reads_to_ascii(reads_var)
    _with_and_without(eng, eng.opt(flag=abi.MEM_F_PE), pe, ref.process(ref.opt(flag=abi.MEM_F_PE), pe), monkeypatch, "paired, MPIBWA_SUBBATCH=" + sub)
    assert eng.stats()["n_sub"] == int(sub)
    _with_and_without(eng, eng.opt(flag=0), se, ref.process(ref.opt(flag=0), se), monkeypatch, "single-end, MPIBWA_SUBBATCH=" + sub)
    kw = dict(flag=abi.MEM_F_PE, mask_level_redun=0.8, w=40, max_chain_gap=300)
    _with_and_without(eng, eng.opt(**kw), pe, ref.process(ref.opt(**kw), pe), monkeypatch, "paired, other options, MPIBWA_SUBBATCH=" + sub)


def test_three_callers_in_flight(both, reads_pe, reads_var, monkeypatch):
    eng, ref = both
    monkeypatch.setenv("MPIBWA_SUBBATCH_MIN", "100")
    monkeypatch.setenv("MPIBWA_DEV_DEDUP", "1")
    pe, se = simulate.reads_to_ascii(reads_pe), simulate.reads_to_ascii(reads_var)
    want = {True: ref.process(ref.opt(flag=abi.MEM_F_PE), pe), False: ref.process(ref.opt(flag=0), se)}
    out, err = {}, []

    def caller(t):
        try:
            for r in range(2):
                paired = (t + r) % 2 == 0
                out[(t, r, paired)] = eng.process(eng.opt(flag=abi.MEM_F_PE if paired else 0), pe if paired else se)
        except BaseException as e:   # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=caller, args=(t,)) for t in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    assert len(out) == 6
    for key, got in out.items():
        _same(got, want[key[2]], key)


def test_repeat_rich_genome(tmp_path_factory, built, monkeypatch):
    """the genome of tests/test_gpu_repeats.py: half of it in families of up to thousands of copies, dozens of regions per read"""
    import ctypes as C
    from mpibwa_amd import api, bigindex
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    lib = api.load_library()
    lib.mi355x_finalize()
    pac, lens = bigindex.synth_packed_genome_grch38like(6e6, seed=17, n_contigs=3, repeat_frac=0.5)
    prefix = str(tmp_path_factory.mktemp("dd_rep") / "rep.fa")
    bigindex.write_meta_files(prefix, pac, lens)
    secs = C.c_double(0)
    assert lib.mi355x_index_build_gpu(0, pac.ctypes.data, int(lens.sum()), prefix.encode(), C.byref(secs)) == 0
    eng = api.Engine(prefix, device=0)
    idx, ref = bigindex.BigIndex(prefix, pac, lens, eng), po.RefIndex(prefix)
    reads = idx.simulate_pairs(1500, seed=141, read_len=150)
    want = ref.process(ref.opt(flag=abi.MEM_F_PE), reads)
    _with_and_without(eng, eng.opt(flag=abi.MEM_F_PE), reads, want, monkeypatch, "repeat-rich")
    lib.mi355x_finalize()
