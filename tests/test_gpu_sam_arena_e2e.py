"""End-to-end companion of the SAM stage test's small-arena cases: a chunk whose records outgrow the arena the pipeline allots to
sam_emit_kernel (reads x (2 x longest + 320) + 1 MB per part) — 250-byte names and a 255-byte read group on 150-bp pairs, repeated
until they do.  The kernel hands the waves that do not fit back, the host formats those pairs itself: the chunk must still equal the
reference's text byte for byte, and part of it must have come from the device."""
import pytest

from mpibwa_amd import abi, simulate
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


def test_pe_chunk_with_long_names_and_read_group_outgrows_the_device_arena(genome, reads_pe):
    assert po.ref_available(), "oracle/_ref/libbwaref.so is missing"
    from mpibwa_amd import api
    lib = api.load_library()
    lib.mi355x_finalize()
    eng, ref = api.Engine(genome["prefix"], device=0), po.RefIndex(genome["prefix"])
    ascii_reads = simulate.reads_to_ascii(reads_pe)
    reads = [(("q%06d_" % (rep * len(ascii_reads) + k)).ljust(250, "x"), s1, s2) for rep in range(20) for k, (_, s1, s2) in enumerate(ascii_reads)]
    # the same chunk under short names and without a read group: what the device writes when everything fits
    eng.process(eng.opt(flag=abi.MEM_F_PE), [(n[:7], s1, s2) for n, s1, s2 in reads])
    n_fit = eng.stats()["n_sam_dev"]
    rg = b"@RG\\tID:" + b"L" * 255 + b"\\tSM:s"
    try:
        assert ref.set_rg(rg) == po.set_rg(lib, rg) == b"L" * 255
        want = ref.process(ref.opt(flag=abi.MEM_F_PE), reads)
        got = eng.process(eng.opt(flag=abi.MEM_F_PE), reads)
    finally:
        ref.set_rg(None)
        po.set_rg(lib, None)
    st = eng.stats()
    n = len(got)
    assert n == len(want) == 2 * len(reads)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, (len(bad), bad[:5], got[bad[0]][:700], want[bad[0]][:700])
    # the device's records (n_fit of n when everything fits) need more than the arenas of both parts of the chunk together, so whole
    # waves were handed back — and the device still wrote the others
    assert sum(len(s) for s in want) * n_fit // n > int(lib.mi355x_sam_arena_bytes(n, 150)) + (1 << 20) + 64 * 1000
    assert 0 < st["n_sam_dev"] <= n_fit - 64, (st["n_sam_dev"], n_fit)
