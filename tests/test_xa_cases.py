"""CPU: the reads of tests/pair_wave_cases.py are worth running for the XA listing of pair_wave_kernel — seen through the reference alone
(mem_align1_core, mem_pestat, mem_sam_pe of oracle/_ref/libbwaref.so) the clean and the damaged read set each hold a few hundred pairs
whose records differ from plain ones by an XA tag alone (tests/xa_cases.py), many of them with a rescue attempt or more than eight
regions on an end, with tags of one to five entries, the longest of them too long for sam_emit_kernel's 260-byte staging row next to the
short fields.  The floors are the issue's; the counts are printed.  No GPU involved."""
import pytest

from mpibwa_amd import abi
from oracle import pyoracle as po

import pair_wave_cases as pw
import xa_cases as xc

pytestmark = pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref/libbwaref.so not built")


@pytest.fixture(scope="module")
def wave_genome(tmp_path_factory, built):
    return pw.build_index(tmp_path_factory.mktemp("xa_cases"))


@pytest.mark.parametrize("damaged", [False, True], ids=["clean", "damaged"])
def test_the_cases_hold_xa_only_pairs(wave_genome, damaged):
    from mpibwa_amd import simulate
    ref = po.RefIndex(wave_genome["prefix"])
    opt = ref.opt(flag=abi.MEM_F_PE)
    reads = pw.make_reads(wave_genome["seqs"], wave_genome["copies"], damaged)
    pairs, _ = pw.reference_side(ref, opt, simulate.reads_to_ascii(reads))
    c = xc.census(pairs)
    print("damaged" if damaged else "clean", c)
    assert c["xa_only"] >= 200, c
    assert c["with_rescue"] >= 80 and c["over_8_regions"] >= 50, c
    assert all(c["tags_by_entries"].get(k, 0) >= 20 for k in range(1, 6)), c
    assert max(c["tags_by_entries"]) <= 5, c   # (max_XA_hits)
    assert c["longest_tag"] > 128, c           # with the short fields of a record it cannot fit the 260-byte row
