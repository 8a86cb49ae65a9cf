"""Whole mem_process_seqs calls with the XA listing of pair_wave_kernel in the pipeline (mpibwa_amd/csrc/sam_stage.hip): on the case
genome of tests/pair_wave_cases.py the SAM text equals the reference's mem_process_seqs byte for byte — with the device units' job early
and late, with one and two parts of the SAM stage, with several calls in flight — and equals the same call under MPIBWA_HOST_XA=1,
where n_pair_xa_dev is 0 and the two other counters of pairs decided on the device are what they were.  n_pair_xa_dev is at least half
the number of XA-only pairs by the reference alone (tests/xa_cases.py); -a and MEM_F_NO_RESCUE calls take none.  The repeat-rich
genome of tests/test_gpu_repeats.py is run once, without a floor."""
import threading

import pytest

from mpibwa_amd import abi, simulate
from oracle import pyoracle as po

import pair_wave_cases as pw
import xa_cases as xc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wave(tmp_path_factory, built):
    from mpibwa_amd import api
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    api.load_library().mi355x_finalize()
    g = pw.build_index(tmp_path_factory.mktemp("xa_e2e"))
    g["engine"] = api.Engine(g["prefix"], device=0)
    g["ref"] = po.RefIndex(g["prefix"])
    g["reads"] = simulate.reads_to_ascii(pw.make_reads(g["seqs"], g["copies"], True) + pw.make_reads(g["seqs"], g["copies"], False))
    g["want"] = g["ref"].process(g["ref"].opt(flag=abi.MEM_F_PE), g["reads"])
    pairs, _ = pw.reference_side(g["ref"], g["ref"].opt(flag=abi.MEM_F_PE), g["reads"])
    g["xa_only"] = sum(1 for P in pairs if xc.xa_only(P))
    return g


def _same(got, want, tag):
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, (tag, len(bad), bad[:5], got[bad[0]][:700], want[bad[0]][:700])


def test_whole_calls_match_the_reference_and_the_host_path(wave, monkeypatch):
    eng = wave["engine"]
    opt = eng.opt(flag=abi.MEM_F_PE)
    assert wave["xa_only"] >= 400
    for env in ({}, {"MPIBWA_DEV_JOB_LATE": "1"}, {"MPIBWA_SAM_PARTS": "2"}, {"MPIBWA_SAM_PARTS": "2", "MPIBWA_DEV_JOB_LATE": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _same(eng.process(opt, wave["reads"]), wave["want"], env)
        st = eng.stats()
        print(env, "pairs", len(wave["reads"]), "XA-only", wave["xa_only"], "n_pair_xa_dev", st["n_pair_xa_dev"], "n_pair_wave_dev", st["n_pair_wave_dev"],
              "n_pair_dev", st["n_pair_dev"], "n_sam_dev", st["n_sam_dev"])
        assert st["n_pair_xa_dev"] * 2 >= wave["xa_only"], (env, st["n_pair_xa_dev"], wave["xa_only"])
        monkeypatch.setenv("MPIBWA_HOST_XA", "1")
        _same(eng.process(opt, wave["reads"]), wave["want"], ("MPIBWA_HOST_XA", env))
        off = eng.stats()
        assert off["n_pair_xa_dev"] == 0 and off["n_pair_dev"] == st["n_pair_dev"] and off["n_pair_wave_dev"] == st["n_pair_wave_dev"], (env, off, st)
        # (the records of the XA pairs that did not come back were written on the device)
        assert st["n_sam_dev"] > off["n_sam_dev"] and st["n_sam_dev"] - off["n_sam_dev"] <= 2 * st["n_pair_xa_dev"], (env, st, off)
        monkeypatch.delenv("MPIBWA_HOST_XA")
        for k in env:
            monkeypatch.delenv(k)


def test_several_calls_in_flight(wave):
    eng = wave["engine"]
    opt = eng.opt(flag=abi.MEM_F_PE)
    out, err = {}, []

    def caller(t):
        try:
            for r in range(2):
                out[(t, r)] = eng.process(opt, wave["reads"])
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
        _same(got, wave["want"], key)


@pytest.mark.parametrize("flag", [abi.MEM_F_PE | abi.MEM_F_ALL, abi.MEM_F_PE | abi.MEM_F_NO_RESCUE])
def test_calls_that_take_no_xa_pair(wave, flag):
    eng, ref = wave["engine"], wave["ref"]
    reads = wave["reads"][:1200]
    _same(eng.process(eng.opt(flag=flag), reads), ref.process(ref.opt(flag=flag), reads), flag)
    assert eng.stats()["n_pair_xa_dev"] == 0


def test_repeat_rich_genome(tmp_path_factory, built, monkeypatch):
    """the genome of tests/test_gpu_repeats.py: half of it in families of up to thousands of copies"""
    import ctypes as C
    from mpibwa_amd import api, bigindex
    lib = api.load_library()
    lib.mi355x_finalize()
    pac, lens = bigindex.synth_packed_genome_grch38like(6e6, seed=17, n_contigs=3, repeat_frac=0.5)
    prefix = str(tmp_path_factory.mktemp("xa_rep") / "rep.fa")
    bigindex.write_meta_files(prefix, pac, lens)
    secs = C.c_double(0)
    assert lib.mi355x_index_build_gpu(0, pac.ctypes.data, int(lens.sum()), prefix.encode(), C.byref(secs)) == 0
    eng = api.Engine(prefix, device=0)
    idx, ref = bigindex.BigIndex(prefix, pac, lens, eng), po.RefIndex(prefix)
    reads = idx.simulate_pairs(2000, seed=131, read_len=150)
    want = ref.process(ref.opt(flag=abi.MEM_F_PE), reads)
    _same(eng.process(eng.opt(flag=abi.MEM_F_PE), reads), want, "repeat-rich")
    st = eng.stats()
    print("repeat-rich: pairs", len(reads), "n_pair_xa_dev", st["n_pair_xa_dev"], "n_pair_wave_dev", st["n_pair_wave_dev"], "n_pair_dev", st["n_pair_dev"],
          "n_sam_dev", st["n_sam_dev"])
    monkeypatch.setenv("MPIBWA_HOST_XA", "1")
    _same(eng.process(eng.opt(flag=abi.MEM_F_PE), reads), want, "repeat-rich, XA on the host")
    off = eng.stats()
    print("repeat-rich, MPIBWA_HOST_XA=1: n_pair_wave_dev", off["n_pair_wave_dev"], "n_pair_dev", off["n_pair_dev"], "n_sam_dev", off["n_sam_dev"])
    assert off["n_pair_xa_dev"] == 0 and off["n_pair_dev"] == st["n_pair_dev"] and off["n_pair_wave_dev"] == st["n_pair_wave_dev"]
    lib.mi355x_finalize()
