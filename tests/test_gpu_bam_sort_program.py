"""mpibwa_sort (driver/mpibwa_sort.c) on the example data's --bam file: with --device and without it the output decodes to
tests/bam_sort_model.py's result; an input that is not BAM, an input that is also the output and a file that the device refuses for
memory (MPIBWA_BAM_SORT_MAX_BYTES: the library's cap on the admitted bytes, not a full device) each give one line and a non-zero exit."""
import os
import subprocess

import pytest

import bam_sort_cases as sc
import bam_sort_model as sm
from test_gpu_bam import example  # noqa: F401  (the fixture: the library's SAM text of the example data's first 1 500 pairs)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mpibwa_amd", "mpibwa_sort")


@pytest.fixture(scope="module")
def lib(built):
    from mpibwa_amd import api
    return api.load_library()


@pytest.fixture(scope="module")
def files(lib, example, tmp_path_factory):
    eng, text = example
    d = tmp_path_factory.mktemp("sortprog")
    bam = sc.example_bam(lib, eng.bns, text)
    (d / "in.bam").write_bytes(bam)
    return d, bam


def run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=e)


def test_both_paths_write_the_models_file(files):
    d, bam = files
    header, recs = sm.sort_bam(bam)
    for name, flags in (("dev.bam", ["--device"]), ("host.bam", []), ("host9.bam", ["--level", "9"])):
        r = run(flags + ["-o", d / name, d / "in.bam"])
        assert r.returncode == 0, r.stderr[-2000:]
        g_header, g_recs, payloads = sm.decode_sorted((d / name).read_bytes())
        assert g_header == header and g_recs == recs, name
        sm.check_blocks(header, payloads)
    r = run(["--device", "--level", "5", "-o", d / "dev5.bam", d / "in.bam"])
    assert r.returncode == 0 and "--level has no effect" in r.stderr
    assert (d / "dev5.bam").read_bytes() == (d / "dev.bam").read_bytes()


def test_the_refusals_are_one_line_each(files):
    d, bam = files
    import gzip
    (d / "plain.gz").write_bytes(gzip.compress(b"@HD\tVN:1.6\n"))
    (d / "text.sam").write_bytes(b"@HD\tVN:1.6\nr\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
    for what, args, env, word in (("plain gzip", ["-o", d / "o1.bam", d / "plain.gz"], None, "plain.gz is not a BAM file"),
                                  ("SAM text", ["--device", "-o", d / "o2.bam", d / "text.sam"], None, "text.sam is not a BAM file"),
                                  ("IN is OUT", ["-o", d / "in.bam", d / "in.bam"], None, "both the input and the output"),
                                  ("IN is OUT by another name", ["-o", d / "." / "in.bam", d / "in.bam"], None, "both the input and the output"),
                                  ("memory", ["--device", "-o", d / "o3.bam", d / "in.bam"], {"MPIBWA_BAM_SORT_MAX_BYTES": "1"}, "in.bam does not fit the device")):
        r = run(args, env)
        assert r.returncode != 0, what
        assert len(r.stderr.strip().splitlines()) == 1 and word in r.stderr, (what, r.stderr)
    assert not any((d / n).exists() for n in ("o1.bam", "o2.bam", "o3.bam"))
    assert (d / "in.bam").read_bytes() == bam
    line = run(["--device", "-o", d / "o3.bam", d / "in.bam"], {"MPIBWA_BAM_SORT_MAX_BYTES": "1"}).stderr
    assert "needed" in line and "free" in line
