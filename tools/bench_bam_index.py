"""The BAI index from the device on tools/bench_bam_sort.py's file -> profiles/bam_index_dev.json (or --out FILE).

  python tools/bench_bam_index.py [--mb 270] [--gb 2] [--rounds 5] [--threads 16] [--out FILE]

(a) mi355x_bam_sort_index_dev against mi355x_bam_sort_dev, taking turns in one process, --rounds times after one warm-up call each: wall
    seconds per call, the plain call's spread, what the fused call adds in ms and as a share of the call, and that both wrote the same
    bytes.
(b) the index kernels' summed device ms (events round the launches, mi355x_bam_index_dev_stage_ms) and the wall ms of the index stages
    and the serialisation inside the fused call, beside the walk, the sort and the gather of the sort itself.
(c) on the sorted file: mi355x_bam_index_dev against mi355x_bam_index on --threads host threads, wall seconds and CPU-seconds of this
    process (all threads) per call; all three indexes are compared byte for byte.
A measurement needs an MI355X; without one the device call ends the process."""
import ctypes as C
import json
import os
import platform
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mpibwa_amd import api  # noqa: E402
from bench_bam_sort import make_file  # noqa: E402

libc = C.CDLL(None)
libc.free.argtypes = [C.c_void_p]


def taken(p, n):
    bai = C.string_at(p.value, n.value)
    libc.free(p)
    return bai


def main():
    args = sys.argv[1:]

    def opt(name, default, kind):
        return kind(args[args.index(name) + 1]) if name in args else default
    mb, gb, rounds, threads = opt("--mb", 270, int), opt("--gb", 2.0, float), opt("--rounds", 5, int), opt("--threads", 16, int)
    os.environ["MPIBWA_SAMPOST_THREADS"] = str(threads)
    lib = api.load_library()
    bam, n_rec, u, n_chunks = make_file(lib, mb, gb)
    cap = lib.mi355x_bam_sort_bound(bam, len(bam))
    assert cap > 0
    out, out2 = C.create_string_buffer(cap), C.create_string_buffer(cap)
    last = {}

    def plain():
        return lib.mi355x_bam_sort_dev(bam, len(bam), out, cap)

    def fused():
        p, n, why = C.c_void_p(), C.c_size_t(0), C.c_int(-1)
        size = lib.mi355x_bam_sort_index_dev(bam, len(bam), out2, cap, C.byref(p), C.byref(n), C.byref(why))
        assert size > 0 and why.value == 0, (size, why.value)
        last["bai"] = taken(p, n)
        return size
    legs = {"sort_device": plain, "sort_index_device": fused}
    sizes = {name: f() for name, f in legs.items()}   # warm-up: buffers, streams, code objects
    assert sizes["sort_device"] == sizes["sort_index_device"] > 0 and out.raw[:sizes["sort_device"]] == out2.raw[:sizes["sort_device"]]
    times = {k: [] for k in legs}
    sort_stages, index_stages = [], []
    for _ in range(rounds):
        for name, f in legs.items():
            t0 = time.perf_counter()
            n = f()
            times[name].append(time.perf_counter() - t0)
            assert n == sizes[name]
            ms = (C.c_double * 8)()
            lib.mi355x_bam_sort_dev_stage_ms(ms)
            if name == "sort_device":
                sort_stages.append(list(ms))
            else:
                ix = (C.c_double * 8)()
                lib.mi355x_bam_index_dev_stage_ms(ix)
                index_stages.append(list(ix))
    med = {k: statistics.median(v) for k, v in times.items()}
    added = med["sort_index_device"] - med["sort_device"]
    res = {"box": platform.node(), "cores": int(lib.mi355x_host_cpus()), "host_threads": threads, "file_bytes": len(bam), "inflated_bytes": u, "records": n_rec,
           "file": "tools/bench_bam_sort.py's: %d chunks of %d MB of SAM text as BAM, the library's own --bam layout" % (n_chunks, mb), "rounds": rounds,
           "a_fused_against_plain": {
               "sort_device_wall_s": [round(t, 4) for t in times["sort_device"]], "sort_index_device_wall_s": [round(t, 4) for t in times["sort_index_device"]],
               "sort_device_median_s": round(med["sort_device"], 4), "sort_device_spread_ms": round(1e3 * (max(times["sort_device"]) - min(times["sort_device"])), 2),
               "sort_index_device_median_s": round(med["sort_index_device"], 4), "added_ms": round(1e3 * added, 2),
               "added_share_of_the_call": round(added / med["sort_index_device"], 4), "same_bytes_out": True, "bai_bytes": len(last["bai"])},
           "b_stages": {
               "index_kernels_device_ms_median": round(statistics.median(s[5] for s in index_stages), 3),
               "index_stages_wall_ms_median": round(statistics.median(s[2] for s in index_stages), 3),
               "serialisation_wall_ms_median": round(statistics.median(s[3] for s in index_stages), 3),
               "sort_walk_wall_ms_median": round(statistics.median(s[1] for s in sort_stages), 3),
               "sort_sort_wall_ms_median": round(statistics.median(s[2] for s in sort_stages), 3),
               "sort_gather_kernels_device_ms_median": round(statistics.median(s[5] for s in sort_stages), 3)}}
    # (c) the stand-alone calls on the sorted file
    z = out2.raw[:sizes["sort_index_device"]]
    got = {}

    def index_with(fn):
        p, n, why = C.c_void_p(), C.c_size_t(0), C.c_int(-1)
        r = fn(z, len(z), C.byref(p), C.byref(n), C.byref(why))
        assert r == n_rec and why.value == 0, (r, why.value)
        return taken(p, n)
    alone = {"index_device": lib.mi355x_bam_index_dev, "index_host": lib.mi355x_bam_index}
    for name, fn in alone.items():
        got[name] = index_with(fn)
    assert got["index_device"] == got["index_host"] == last["bai"]
    res["all_three_indexes_are_the_same_bytes"] = True
    c_times = {k: [] for k in alone}
    alone_stages = []
    for _ in range(min(rounds, 3)):
        for name, fn in alone.items():
            c0, t0 = time.process_time(), time.perf_counter()
            index_with(fn)
            c_times[name].append((time.perf_counter() - t0, time.process_time() - c0))
            if name == "index_device":
                ix = (C.c_double * 8)()
                lib.mi355x_bam_index_dev_stage_ms(ix)
                alone_stages.append(list(ix))
    res["c_stand_alone_on_the_sorted_file"] = {
        name: {"wall_s": [round(w, 4) for w, _ in v], "wall_s_median": round(statistics.median(w for w, _ in v), 4),
               "process_cpu_s_per_call_median": round(statistics.median(c for _, c in v), 3)} for name, v in c_times.items()}
    keys = ("inflate", "walk", "index", "serialisation", "whole_call", "index_kernels_device")
    res["c_stand_alone_on_the_sorted_file"]["index_device_stage_ms_median"] = {k: round(statistics.median(s[i] for s in alone_stages), 3) for i, k in enumerate(keys)}
    c = (C.c_uint64 * 8)()
    lib.mi355x_bam_index_dev_counts(c)
    res["index_device_counts"] = dict(zip(("calls", "records", "calls_walked_by_the_host", "runs_before_the_join", "chunks_written", "linear_windows", "bai_bytes",
                                           "calls_refused_for_memory"), list(c)))
    lib.mi355x_finalize()
    path = opt("--out", os.path.join(ROOT, "profiles", "bam_index_dev.json"), str)
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
