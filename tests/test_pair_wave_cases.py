"""CPU: the cases of tests/pair_wave_cases.py are worth running — seen through the reference alone (mem_align1_core, mem_pestat, mem_sam_pe
of oracle/_ref/libbwaref.so) they hold the pairs pair_wave_kernel is for: several hundred that need mate rescue or carry more than eight
regions on an end and still end as a plain proper pair, dozens of them with 33-64 regions on an end, a hundred and more rescued from an
end without any region, and — as the pairs the kernel must leave alone — a hundred and more with XA text or extra lines.  The floors
are the issue's; the counts are printed.  No GPU involved."""
import pytest

from mpibwa_amd import abi
from oracle import pyoracle as po

import pair_wave_cases as pw

pytestmark = pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref/libbwaref.so not built")


@pytest.fixture(scope="module")
def wave_genome(tmp_path_factory, built):
    return pw.build_index(tmp_path_factory.mktemp("pair_wave"))


def test_the_recipe_is_fixed(wave_genome):
    names, seqs, copies = pw.build_genome()
    assert [len(s) for s in seqs] == [len(s) for s in wave_genome["seqs"]] and len(copies) == sum(f[1] for f in pw.FAMILIES)
    assert all((a == b).all() for a, b in zip(seqs, wave_genome["seqs"]))
    assert len(pw.make_reads(seqs, copies, True)) == pw.N_PLAIN + pw.N_AT_COPIES


def test_the_cases_hold_what_pair_wave_kernel_is_for(wave_genome, genome):
    from mpibwa_amd import simulate
    from test_sampost import _pairs_of_every_kind
    ref = po.RefIndex(wave_genome["prefix"])
    opt = ref.opt(flag=abi.MEM_F_PE)
    total = dict(eligible=0, eligible_33_64=0, eligible_from_no_region=0, xa_or_extra_lines=0)
    for tag, reads in (("clean", pw.make_reads(wave_genome["seqs"], wave_genome["copies"], False)),
                       ("damaged", pw.make_reads(wave_genome["seqs"], wave_genome["copies"], True)),
                       ("every kind", _pairs_of_every_kind(wave_genome, n=360, seed=40))):
        pairs, _ = pw.reference_side(ref, opt, simulate.reads_to_ascii(reads))
        c = pw.census(pairs)
        print(tag, c)
        for k in total:
            total[k] += c[k]
    print("all", total)
    assert total["eligible"] >= 400, total
    assert total["eligible_33_64"] >= 30, total
    assert total["eligible_from_no_region"] >= 100, total
    assert total["xa_or_extra_lines"] >= 100, total
