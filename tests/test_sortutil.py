"""CPU: mpibwa_amd/csrc/sortutil.h itself — the one statement of ks_introsort that the host and every kernel share — as a stand-alone
program (tests/sortutil_main.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer.

The program sorts an order array over each key list with ks_introsort_at, its frame arrays malloc'ed at the device capacities (16
frames up to 512 elements: dedup_wave_kernel; 32 up to 4096: chain_heavy_kernel), so a frame beyond the stated bound n <= 16 << FRAMES
is a heap overflow the sanitizer reports; with ks_small_introsort_at for n <= 16; and with the host's ks_introsort over a T*.  The
orders are compared with tests/introsort_model.py, which tests/test_introsort_model.py pins to the reference's own ks_introsort.  All
families have equal keys (but the distinct one): the order of equal keys is what the restatement is for.  The comb sort is entered by
the ordered family (from 26 elements on) and by the sorted_tail family, and it swaps in the latter only: a range that arrives in order
gives it nothing to swap, whatever the keys (model: 0 swaps in every ordered list of every size here)."""
import os
import subprocess

import numpy as np
import pytest

import chain_cases as cc
import introsort_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 2, 3, 8, 9, 16, 17, 25, 26, 33, 64, 512, 4096)


def _runs(rng, n, longest=7):
    """n keys in ascending order, 1-longest elements per key"""
    keys, k = [], 0
    while len(keys) < n:
        keys += [k] * int(rng.integers(1, longest + 1))
        k += 1
    return keys[:n]


def _lists():
    rng = np.random.default_rng(1907)
    out = []
    for n in SIZES:
        for rep in range(4 if n < 512 else 2):
            out.append(("ordered", _runs(rng, n, 7 if rep else 1)))   # (the first one with one element per key)
            out.append(("reversed", _runs(rng, n)[::-1]))
            out.append(("few_keys", [int(v) for v in rng.integers(0, int(rng.integers(2, 7)), n)]))
            out.append(("distinct", [int(v) for v in rng.permutation(n)]))
            if n >= 17:   # (the shape needs 1 + 2 * ceil(log2 n) elements; heavier first = ascending in the negated weight)
                out.append(("sorted_tail", [-w for w in cc.sorted_tail_weights(rng, n)]))
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sortutil") / "sortutil_main")
    # (the sanitizers' runtimes are linked into the program: it starts in whatever environment the suite runs in, unchanged)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "mpibwa_amd", "csrc"), os.path.join(ROOT, "tests", "sortutil_main.cpp"), "-o", exe])
    return exe


def test_the_header_sorts_like_the_model_under_the_sanitizers(program):
    lists = _lists()
    text = "".join("%d %s\n" % (len(k), " ".join(map(str, k))) for _, k in lists)
    run = subprocess.run([program], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    lines = iter(run.stdout.decode().splitlines())
    combs = {}
    for fam, keys in lists:
        n = len(keys)
        want, st = im.sort_keys(keys)
        assert [keys[k] for k in want] == sorted(keys)
        # the frames the model needed fit the capacity the program ran with (and the header's bound)
        cap = 16 if n <= 512 else 32
        assert st.max_frames < cap and n <= 16 << cap and (st.max_frames == 0 or n > 16 << (st.max_frames - 1)), (fam, n, st.max_frames)
        tag, *full = next(lines).split()
        assert tag == "F" and [int(v) for v in full] == want, (fam, n, "ks_introsort_at")
        if n <= 16:
            tag, *small = next(lines).split()
            assert tag == "S" and small == full, (fam, n, "ks_small_introsort_at is not ks_introsort_at")
            assert not st.comb_ranges and st.max_frames == 0
        tag, *host = next(lines).split()
        assert tag == "H" and host == full, (fam, n, "ks_introsort")
        c = combs.setdefault((fam, n), [0, 0, 0])
        c[0] += 1; c[1] += bool(st.comb_ranges); c[2] += st.comb_swaps > 0
    assert next(lines, None) is None
    for (fam, n), (lists_n, entered, swapped) in sorted(combs.items()):
        print("%-12s n %5d lists %d enter the comb sort %d and swap there %d" % (fam, n, lists_n, entered, swapped))
        if fam == "ordered":
            # Input in order runs out of depth from 26 elements on with one element per key (test_introsort_model.py) and from 64 on
            # with runs of equal keys (at 26 and 33 the runs stop the scans early enough to save the budget).  The range it hands to the
            # comb sort is in order, so the comb sort has nothing to swap there: its swaps are the sorted_tail family's to show.
            assert entered == (lists_n if n >= 64 else 1 if n >= 26 else 0) and swapped == 0, (n, entered, swapped)
        if fam == "sorted_tail" and n >= 26:
            assert entered == lists_n and swapped == lists_n, (n, entered, swapped)
