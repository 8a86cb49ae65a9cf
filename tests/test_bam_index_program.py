"""mpibwa_sort --index and --index-only on the host paths (driver/mpibwa_sort.c): the .bai beside the output is the
model's index of the file that was written, an input that is not in coordinate order or reaches beyond 2^29 gives one line, a non-zero
exit and no .bai, and without the new flags nothing is written beside OUT.bam.  No GPU."""
import os
import subprocess

import pytest

import bam_index_cases as ic
import bam_index_model as mi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mpibwa_amd", "mpibwa_sort")


@pytest.fixture(scope="module")
def files(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("indexprog")
    what, bam, _ = ic.good_cases()[-1]
    (d / "sorted.bam").write_bytes(bam)
    (d / "in.bam").write_bytes(ic.unsorted(bam))
    return d, bam


def run(args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_index_beside_the_sorted_file(files):
    d, _ = files
    r = run(["--index", "-o", d / "out.bam", d / "in.bam"])
    assert r.returncode == 0, r.stderr[-2000:]
    out = (d / "out.bam").read_bytes()
    assert (d / "out.bam.bai").read_bytes() == mi.build(out)
    r = run(["-o", d / "plain.bam", d / "in.bam"])
    assert r.returncode == 0 and (d / "plain.bam").read_bytes() == out and not (d / "plain.bam.bai").exists()
    assert r.stderr.strip() == "[mpibwa_sort] wrote %s: %d bytes" % (d / "plain.bam", len(out))


def test_index_only(files):
    d, bam = files
    r = run(["--index-only", d / "sorted.bam"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert (d / "sorted.bam.bai").read_bytes() == mi.build(bam)
    assert (d / "sorted.bam").read_bytes() == bam


def test_the_refusals_are_one_line_each_and_leave_no_bai(files):
    d, bam = files
    bad = {w: (b, code) for w, b, code, _ in ic.bad_cases()}
    (d / "long.bam").write_bytes(bad["end == 2^29 + 1"][0])
    (d / "text.sam").write_bytes(b"@HD\tVN:1.6\nr\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
    first_unsorted = None
    try:
        mi.build((d / "in.bam").read_bytes())
    except mi.Refused as e:
        first_unsorted = e.offset
    for what, args, word in (("unsorted", ["--index-only", d / "in.bam"], "not in coordinate order: the record at offset %d " % first_unsorted),
                             ("beyond 2^29", ["--index-only", d / "long.bam"], "beyond 2^29, the limit of a BAI index"),
                             ("beyond 2^29, sorting", ["--index", "-o", d / "long_out.bam", d / "long.bam"], "beyond 2^29, the limit of a BAI index"),
                             ("SAM text", ["--index-only", d / "text.sam"], "text.sam is not a BAM file"),
                             ("-o with --index-only", ["--index-only", "-o", d / "x.bam", d / "sorted.bam"], "usage:")):
        r = run(args)
        assert r.returncode != 0, what
        assert word in r.stderr and (what.startswith("-o") or len(r.stderr.strip().splitlines()) == 1), (what, r.stderr)
    assert not any((d / n).exists() for n in ("in.bam.bai", "long.bam.bai", "long_out.bam.bai", "long_out.bam", "text.sam.bai", "x.bam"))
