"""End-to-end parity of single-end calls of mem_process_seqs() with the device path of the stage after the CIGAR kernel
(se_simple_kernel -> aln_kernel -> the single-end instantiation of sam_emit_kernel) against the compiled reference
(oracle/_ref/libbwaref.so), byte for byte: the variable-length reads of the session, a simulated 50-300 bp chunk, the single-end list
of the ALT genome and the repeat-rich generator, under the option variants that keep the call on the device path (plain, -Y, -M, other
thresholds, no qualities, a read group) and the ones that send it to the host (-a, -5, -C, MPIBWA_HOST_SE=1).

The counters: with the default options n_se_dev and n_sam_dev are at least half the number of reads the reference reports with one
line and no XA / SA tag (counted from the reference's own output); they are 0 with MPIBWA_HOST_SE=1, under -a and with a comment
column; a paired call afterwards still reports n_pair_dev > 0 and n_se_dev = 0.

Measured on the MI355X (tools/bench_se.py -> profiles/se_device_path.json; BASELINE config 3's shape: 3 chunks x 300 000 single-end
reads of 50-300 bases against the 3.1 Gbp index, two alternating repeats): device path 2.976 / 2.936 Mreads/s, MPIBWA_HOST_SE=1
2.885 / 2.984 Mreads/s, the same SAM hash; emit_ms 7.7 / 8.0 against 13.4 / 11.6; host CPU-seconds per chunk 0.431 / 0.448 against
0.516 / 0.474; n_se_dev / n_reads = 0.9589, n_sam_dev / n_reads = 0.9588 (the rest: 3.0 % more than eight regions, 1.0 % an XA entry).
On this file's own reads: 1 343 of 1 500 and 272 of 300 reads decided and written on the device."""
import ctypes as C

import pytest

from mpibwa_amd import abi, simulate
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def both(genome):
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    from mpibwa_amd import api
    api.load_library().mi355x_finalize()
    return api.Engine(genome["prefix"], device=0), po.RefIndex(genome["prefix"])


@pytest.fixture(scope="module")
def chunk(genome):
    """trimmed single-end reads, 50-300 bp"""
    return simulate.reads_to_ascii(simulate.simulate_reads(genome["seqs"], 1500, 150, paired=False, seed=41, var_len=(50, 300)))


def _cmp(eng, ref, reads, kw, **pk):
    want = ref.process(ref.opt(**kw), reads, **pk)
    got = eng.process(eng.opt(**kw), reads, **pk)
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, (kw, pk, len(bad), bad[:5], got[bad[0]][:400], want[bad[0]][:400])
    return want


def _plain(want):
    """reads the reference reports with one line and neither XA nor SA"""
    return sum(s.count(b"\n") == 1 and b"\tXA:Z:" not in s and b"\tSA:Z:" not in s for s in want)


VARIANTS = [
    (dict(flag=0), {}, True),
    (dict(flag=abi.MEM_F_SOFTCLIP), {}, True),
    (dict(flag=abi.MEM_F_NO_MULTI), {}, True),
    (dict(flag=abi.MEM_F_ALL), {}, False),
    (dict(flag=abi.MEM_F_PRIMARY5), {}, False),
    (dict(flag=0, T=20, drop_ratio=0.3), {}, True),
    (dict(flag=0, XA_drop_ratio=0.5), {}, True),
    (dict(flag=0), dict(with_qual=False), True),
    (dict(flag=0), dict(comment="BC:Z:ACGT+TTAG"), False),
]


@pytest.mark.parametrize("kw,pk,on_device", VARIANTS)
def test_single_end_variants(both, reads_var, chunk, kw, pk, on_device):
    eng, ref = both
    for reads, n_processed in ((simulate.reads_to_ascii(reads_var), 0), (chunk, 3000)):
        want = _cmp(eng, ref, reads, kw, n_processed=n_processed, **pk)
        st = eng.stats()
        print(kw, pk, "reads", len(reads), "reference-plain", _plain(want), "n_se_dev", st["n_se_dev"], "n_sam_dev", st["n_sam_dev"])
        assert st["n_pair_dev"] == 0
        if not on_device:
            assert st["n_se_dev"] == 0 and st["n_sam_dev"] == 0, (kw, pk, st["n_se_dev"], st["n_sam_dev"])
        elif kw == dict(flag=0) and not pk:
            assert st["n_se_dev"] >= _plain(want) / 2 and st["n_sam_dev"] >= _plain(want) / 2, (st["n_se_dev"], st["n_sam_dev"], _plain(want))
            assert st["n_sam_dev"] <= st["n_se_dev"] <= len(reads)
        else:
            assert st["n_se_dev"] > 0 and st["n_sam_dev"] > 0


def test_read_group(both, chunk):
    eng, ref = both
    try:
        rgid = ref.set_rg(b"@RG\\tID:grp.7\\tSM:y")
        assert po.set_rg(eng.lib, b"@RG\\tID:grp.7\\tSM:y") == rgid
        want = _cmp(eng, ref, chunk, dict(flag=0))
        assert all(b"\tRG:Z:grp.7" in line for s in want for line in s.splitlines())
        assert eng.stats()["n_sam_dev"] >= _plain(want) / 2
    finally:
        ref.set_rg(None)
        po.set_rg(eng.lib, None)


def test_host_switch_sub_batches_and_a_paired_call_afterwards(both, chunk, reads_pe, monkeypatch):
    eng, ref = both
    want = _cmp(eng, ref, chunk, dict(flag=0))
    assert eng.stats()["n_se_dev"] >= _plain(want) / 2 and eng.stats()["n_sam_dev"] >= _plain(want) / 2
    monkeypatch.setenv("MPIBWA_HOST_SE", "1")
    assert eng.process(eng.opt(flag=0), chunk) == want
    assert eng.stats()["n_se_dev"] == 0 and eng.stats()["n_sam_dev"] == 0
    monkeypatch.delenv("MPIBWA_HOST_SE")
    monkeypatch.setenv("MPIBWA_SUBBATCH_MIN", "100")   # two sub-batches: two slices of the chunk-wide region arrays
    assert eng.process(eng.opt(flag=0), chunk) == want
    assert eng.stats()["n_se_dev"] >= _plain(want) / 2
    monkeypatch.delenv("MPIBWA_SUBBATCH_MIN")
    monkeypatch.setenv("MPIBWA_SAM_PARTS", "2")        # the two-part software pipeline of the SAM stage
    assert eng.process(eng.opt(flag=0), chunk) == want
    monkeypatch.delenv("MPIBWA_SAM_PARTS")
    ra = simulate.reads_to_ascii(reads_pe)
    _cmp(eng, ref, ra, dict(flag=abi.MEM_F_PE))
    assert eng.stats()["n_pair_dev"] > 0 and eng.stats()["n_se_dev"] == 0
    # reads without any seed, shorter than a seed, all N: the unmapped record of the device
    odd = [("short", b"ACGTACGTAC", None), ("allN", b"N" * 80, None), ("homo", b"A" * 150, None)] + chunk[:5]
    _cmp(eng, ref, odd, dict(flag=0))
    assert eng.stats()["n_se_dev"] >= 3


def test_alt_genome_single_end(genome_alt):
    from mpibwa_amd import api
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    api.load_library().mi355x_finalize()
    eng, ref = api.Engine(genome_alt["prefix"], device=0), po.RefIndex(genome_alt["prefix"])
    seqs = genome_alt["seqs"]
    n_pri = len(seqs) - len(genome_alt["alt"])
    rd = simulate.simulate_reads(seqs, 500, 150, paired=True, seed=31)
    rd += [("a" + n, a, b) for n, a, b in simulate.simulate_reads(seqs[n_pri:], 900, 150, paired=True, seed=32, frac_random=0.0)]
    rd = simulate.reads_to_ascii(rd)
    se = [(n, a, None) for n, a, _ in rd] + [(n + "m", b, None) for n, a, b in rd[500:900]]
    want = b"".join(_cmp(eng, ref, se, dict(flag=0)))
    assert b"\tpa:f:" in want and eng.stats()["n_se_dev"] > 0   # reads with ALT hits are the host's, the others the device's
    api.load_library().mi355x_finalize()


def test_repeat_rich_single_end(tmp_path_factory, built):
    """test_gpu_repeats.py's generator: dozens of regions per read, XA tags — mostly the host's reads, next to the device's"""
    import numpy as np
    from mpibwa_amd import api, bigindex
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    lib = api.load_library()
    lib.mi355x_finalize()
    lib.mi355x_index_build_gpu.restype = C.c_int
    lib.mi355x_index_build_gpu.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_char_p, C.POINTER(C.c_double)]
    pac, lens = bigindex.synth_packed_genome_grch38like(6e6, seed=17, n_contigs=3, repeat_frac=0.5)
    prefix = str(tmp_path_factory.mktemp("rep_se") / "rep.fa")
    bigindex.write_meta_files(prefix, pac, lens)
    secs = C.c_double(0)
    assert lib.mi355x_index_build_gpu(0, pac.ctypes.data, int(lens.sum()), prefix.encode(), C.byref(secs)) == 0
    eng = api.Engine(prefix, device=0)
    idx, ref = bigindex.BigIndex(prefix, pac, lens, eng), po.RefIndex(prefix)
    se = [(n, a, None) for n, a, _ in idx.simulate_pairs(1200, seed=105, read_len=150)]
    want = _cmp(eng, ref, se, dict(flag=0))
    st = eng.stats()
    print("repeat-rich: reads", len(se), "reference-plain", _plain(want), "n_se_dev", st["n_se_dev"], "n_sam_dev", st["n_sam_dev"])
    assert sum(b"\tXA:Z:" in s for s in want) > 20 and 0 < st["n_se_dev"] <= _plain(want)
    lib.mi355x_finalize()
