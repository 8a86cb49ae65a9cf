"""CPU: mpibwa_amd/csrc/pairmath.h itself — the one statement of mem_sam_pe's arithmetic that the host and the pairing, single-end
and redundancy kernels share — as a stand-alone program (tests/pairmath_main.cpp) under AddressSanitizer and
UndefinedBehaviorSanitizer.

The INTEGER functions are compared with exact Python-integer restatements of the reference's lines: hash_64 (src/utils.h:98-109),
mem_infer_dir (src/bwamem_pair.c:23-30), infer_bw and the band of mem_reg2aln (tests/ref_band.py), the key of a hit in mem_pair
(src/bwamem_pair.c:191-196) and the `id << 8` of its hash tie-break (:222) — on the reference's int id that shift is undefined from
id = 2^23 on, and a chunk's pair numbers pass it; the header states it as unsigned arithmetic, whose value the test pins.  The
floating-point functions are only CALLED here (the F case), so that the sanitizers see them: their values stay pinned to the reference's
own mem_sam_pe by the stage tests (test_host_pair.py, test_pair_wave_cases.py, test_se_cases.py, ...), not to a model of ours."""
import os
import subprocess
from types import SimpleNamespace

import pytest

import ref_band

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


def _s64(v):
    """a 64-bit pattern as the signed number the program reads"""
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def hash_64(key):   # src/utils.h:98-109
    key = (key + (~(key << 32) & M64)) & M64
    key ^= key >> 22
    key = (key + (~(key << 13) & M64)) & M64
    key ^= key >> 8
    key = (key + (key << 3)) & M64
    key ^= key >> 15
    key = (key + (~(key << 27) & M64)) & M64
    key ^= key >> 31
    return key


def infer_dir(l_pac, b1, b2):   # src/bwamem_pair.c:23-30
    r1, r2 = b1 >= l_pac, b2 >= l_pac
    p2 = b2 if r1 == r2 else (l_pac << 1) - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), abs(p2 - b1)


def pair_key(l_pac, rb, rid, offset, score, i, r):   # src/bwamem_pair.c:191-196
    x = rb if rb < l_pac else (l_pac << 1) - 1 - rb
    return (rid << 32 | (x - offset)) & M64, score << 32 | i << 2 | (rb >= l_pac) << 1 | r


def id_mix(pair_id):
    """`id << 8` of src/bwamem_pair.c:222 on the 32-bit int the reference holds the pair's number in, as two's-complement arithmetic"""
    v = ((pair_id & 0xffffffff) << 8) & 0xffffffff
    return v - (1 << 32) if v >> 31 else v


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pairmath") / "pairmath_main")
    # (the sanitizers' runtimes are linked into the program: it starts in whatever environment the suite runs in, unchanged)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g0", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "mpibwa_amd", "csrc"), os.path.join(ROOT, "tests", "pairmath_main.cpp"), "-o", exe])
    return exe


def _cases():
    """(input line, expected output line or None where the result is only printed)"""
    out = []
    for key in (0, 1, 2, 0xffffffff, 1 << 32, (1 << 63) - 1, 1 << 63, M64, 0x0123456789abcdef, 6 << 1 | 1, (1 << 23) << 8):
        out.append(("H %d" % _s64(key), "%d" % hash_64(key)))
    # orientation and distance: both hits on either side of l_pac, l_pac near 2^31 and near 2^32 (the doubled coordinate passes 2^32 / 2^33)
    for l_pac in (1000, (1 << 31) - 3, (1 << 31) + 5, (1 << 32) - 7, (1 << 32) + 11):
        pos = (0, 1, 150, l_pac - 151, l_pac - 1, l_pac, l_pac + 1, l_pac + 150, 2 * l_pac - 151, 2 * l_pac - 1)
        for b1 in pos:
            for b2 in pos:
                out.append(("D %d %d %d" % (l_pac, b1, b2), "%d %d" % infer_dir(l_pac, b1, b2)))
        # the key of a hit: the same positions, contig 0 at offset 0 and a later contig, the index and the end in the low bits
        for rb in pos:
            for rid, off in ((0, 0), (24, 700)):
                if rb < off or 2 * l_pac - 1 - rb < off:
                    continue
                for score, i, r in ((150, 0, 0), (19, 63, 1), (0x7fffffff, 5, 1)):
                    out.append(("K %d %d %d %d %d %d %d" % (l_pac, rb, rid, off, score, i, r), "%d %d" % pair_key(l_pac, rb, rid, off, score, i, r)))
    # infer_bw: l1 == l2 on the zero branch (fewer mismatches than two gaps cost) and off it, l1 != l2, and the default and other penalties
    bw = []
    for a, q, r in ((1, 6, 1), (1, 6, 2), (2, 4, 3), (1, 0, 1)):
        for l1, l2 in ((150, 150), (151, 151), (100, 100), (150, 153), (153, 150), (40, 150), (19, 19), (250, 251)):
            for miss in (0, 1, (q + r - a) * 2 - 1, (q + r - a) * 2, (q + r - a) * 2 + 1, 30, 200):
                bw.append((l1, l2, min(l1, l2) * a - miss, a, q, r))
    assert any(l1 == l2 and ref_band.infer_bw(l1, l2, s, a, q, r) == 0 for l1, l2, s, a, q, r in bw)
    assert any(l1 == l2 and ref_band.infer_bw(l1, l2, s, a, q, r) > 0 for l1, l2, s, a, q, r in bw)
    for c in bw:
        out.append(("W %d %d %d %d %d %d" % c, "%d" % ref_band.infer_bw(*c)))
    # the band: regions with w = 0 (a hit from mate rescue), below and above the inferred band, under a narrow and the default -w
    n_zero = 0
    for l1, l2, truesc, a, _, _ in bw[::3]:
        for o_del, e_del, o_ins, e_ins in ((6, 1, 6, 1), (4, 2, 9, 1), (9, 1, 4, 3)):
            for w_opt in (100, 3, 0):
                for w_reg in (0, 2, 100, 400):
                    opt = SimpleNamespace(a=a, o_del=o_del, e_del=e_del, o_ins=o_ins, e_ins=e_ins, w=w_opt)
                    want = ref_band.reg2aln_band(opt, l1, l2, truesc, w_reg)
                    n_zero += w_reg == 0 and want == 0 and max(ref_band.infer_bw(l1, l2, truesc, a, o_del, e_del), ref_band.infer_bw(l1, l2, truesc, a, o_ins, e_ins)) > w_opt
                    out.append(("B %d %d %d %d %d %d %d %d %d %d" % (l1, l2, truesc, a, o_del, e_del, o_ins, e_ins, w_opt, w_reg), "%d" % want))
    assert n_zero > 0   # (a rescued hit whose inferred band passes -w gets band 0)
    for t in ((1, 4, 6, 1, 6, 1), (1, 4, 2, 1, 3, 3), (2, 9, 1, 1, 1, 1), (0, 0, 0, 0, 0, 0)):
        out.append(("T %d %d %d %d %d %d" % t, "%d" % max(t[0] + t[1], t[2] + t[3], t[4] + t[5])))
    # `id << 8`: undefined on an int from 2^23 on; the pair (k, i) in y as mem_pair packs it
    for pair_id in (0, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 1, (1 << 31) - 1, 1 << 31, (1 << 32) + 5, (1 << 40) + (1 << 23)):
        for y in (0, 1 << 32 | 2, 63 << 32 | 127):
            mix = id_mix(pair_id)
            out.append(("M %d %d" % (pair_id, y), "%d %d" % (mix, hash_64(y ^ (mix & M64)) & 0xffffffff)))
    # every floating-point function, pair numbers on both sides of 2^23 again
    for pair_id in ((1 << 23) - 1, 1 << 23, (1 << 31) - 1):
        out.append(("F %d %d 1000 1300 150 140 100 600 30000 5000 1 4" % (pair_id, (1 << 31) + 5), None))
        out.append(("F %d %d 1000 9000 150 140 100 600 30000 5000 1 4" % (pair_id, (1 << 32) - 7), None))
    return out


def test_the_header_under_the_sanitizers_and_its_integer_functions(program):
    cases = _cases()
    run = subprocess.run([program], input="".join(c + "\n" for c, _ in cases).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    lines = run.stdout.decode().splitlines()
    assert len(lines) == len(cases)
    for (given, want), got in zip(cases, lines):
        if want is not None:
            assert got == want, given
            continue
        # F: "n_candidates (x y)* raw q_pe q_se q_se_in_pair redundant patch_w overlap" — the first input has the two hits 300 apart
        # (one candidate pair (0, 1), its hash word the mix's), the second 8000 apart (none)
        f = [int(v) for v in got.split()]
        pair_id, far = int(given.split()[1]), given.split()[4] == "9000"
        assert f[0] == (0 if far else 1) and len(f) == 1 + 2 * f[0] + 7, (given, got)
        if not far:
            assert f[2] == 0 << 32 | 1 and f[1] & 0xffffffff == hash_64(f[2] ^ (id_mix(pair_id) & M64)) & 0xffffffff, (given, got)
        assert all(0 <= q <= 60 for q in f[-6:-3]) and f[-3:] == [0, 2, 1], (given, got)
