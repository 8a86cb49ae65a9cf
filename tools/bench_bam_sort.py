"""The device BAM sort against the host path of the same library on the same file -> profiles/bam_sort_dev.json
(or --out FILE).

  python tools/bench_bam_sort.py [--mb 270] [--gb 2] [--rounds 3] [--threads 16] [--out FILE]

The file is what `mpibwa_gpu --bam --device-bgzf` writes for chunks of tools/bench_bgzf.py's text (the example reads with their real
qualities laid out as SAM records at random places on chr1 .. chr22, --mb of it per chunk, every chunk with places of its own): the
binary header, then chunk after chunk from mi355x_bam_compress_dev until the inflated stream has --gb GB, then the empty end block.
The library's own layout: the device walks the records.  Two legs take turns, --rounds times after one warm-up call each:
mi355x_bam_sort_dev and mi355x_bam_sort at level 3 on --threads host threads (MPIBWA_SAMPOST_THREADS).  Per call: wall seconds (a host clock round a call that ends synchronised),
records/s and GB/s of inflated BAM, the CPU-seconds of this process (all threads).  Once, after the warm-up calls, both legs' files are inflated and compared.  The device leg also gives the wall time of each
stage of its last call (mi355x_bam_sort_dev_stage_ms).  The record gather kernel is timed in one more device call under
MPIBWA_BAM_SORT_GATHER_ALONE (device events round every gather launch, the other stream drained first) and set against a
device-to-device hipMemcpyAsync of the same number of bytes, timed by device events in the same run: both move every byte once in and
once out.  A measurement needs an MI355X; without one the device call ends the process."""
import ctypes as C
import hashlib
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
from bench_bam import contigs  # noqa: E402
from bench_bgzf import chunk_text  # noqa: E402

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def make_file(lib, mb, gb):
    bns, _keep = contigs()
    head_text = b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (bns.anns[i].name, bns.anns[i].len) for i in range(bns.n_seqs))
    raw = C.create_string_buffer(len(head_text) + 4096)
    n = lib.mi355x_bam_header(head_text, len(head_text), C.byref(bns), raw, len(raw))
    z = C.create_string_buffer(lib.mi355x_bgzf_bound(n))
    hn = lib.mi355x_bgzf_compress(raw.raw[:n], n, 3, z, len(z))
    assert n > 0 and hn > 0
    parts, records, u, k = [z.raw[:hn]], 0, n, 0
    while u < gb * 1e9:   # chunk after chunk, each with places of its own: no two records of the file are the same
        text = chunk_text(mb, seed=9 + k)
        cap = lib.mi355x_bgzf_bound(lib.mi355x_bam_bound(len(text)))
        out = C.create_string_buffer(cap)
        c0, c1 = (C.c_uint64 * 6)(), (C.c_uint64 * 6)()
        lib.mi355x_bam_dev_counts(c0)
        size = lib.mi355x_bam_compress_dev(text, len(text), C.byref(bns), out, cap)
        assert size > 0
        lib.mi355x_bam_dev_counts(c1)
        parts.append(out.raw[:size])
        records += c1[0] - c0[0]
        u += c1[3] - c0[3]
        k += 1
    return b"".join(parts) + EOF_BLOCK, records, u, k


def memcpy_ms(n_bytes, reps=5):
    """device-to-device hipMemcpyAsync of n_bytes, by device events: the median of reps after one warm-up"""
    hip = api._hip()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    a, b, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(a), n_bytes) == 0 and hip.hipMalloc(C.byref(b), n_bytes) == 0
    assert hip.hipMemset(a, 1, n_bytes) == 0 and hip.hipMemset(b, 2, n_bytes) == 0
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    ms = []
    for _ in range(reps + 1):
        assert hip.hipEventRecord(e0, None) == 0
        assert hip.hipMemcpyAsync(b, a, n_bytes, 3, None) == 0   # hipMemcpyDeviceToDevice
        assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
        ms.append(t.value)
    hip.hipFree(a)
    hip.hipFree(b)
    return statistics.median(ms[1:])


def main():
    args = sys.argv[1:]

    def opt(name, default, kind):
        return kind(args[args.index(name) + 1]) if name in args else default
    mb, gb, rounds, threads = opt("--mb", 270, int), opt("--gb", 2.0, float), opt("--rounds", 3, int), opt("--threads", 16, int)
    os.environ["MPIBWA_SAMPOST_THREADS"] = str(threads)
    lib = api.load_library()
    bam, n_rec, u, n_chunks = make_file(lib, mb, gb)
    cap = lib.mi355x_bam_sort_bound(bam, len(bam))
    assert cap > 0
    out = C.create_string_buffer(cap)
    legs = {"sort_device": lambda: lib.mi355x_bam_sort_dev(bam, len(bam), out, cap),
            "sort_host_level_3": lambda: lib.mi355x_bam_sort(bam, len(bam), 3, out, cap)}
    res = {"box": platform.node(), "cores": int(lib.mi355x_host_cpus()), "host_threads": threads, "file_bytes": len(bam), "inflated_bytes": u, "records": n_rec,
           "file": "example reads (real qualities) as BAM records at random places, the library's own --bam layout: %d chunks of %d MB of SAM text, each with places of its own" % (n_chunks, mb),
           "rounds": rounds, "legs": {}}
    sizes = {}
    text, digests = C.create_string_buffer(u + 64), {}
    for name, f in legs.items():   # warm-up: buffers, streams, threads, code objects; and what the leg's file inflates to
        sizes[name] = f()
        assert sizes[name] > 0, (name, sizes[name])
        n = lib.mi355x_bgzf_inflate(out, sizes[name], text, len(text))
        assert n > 0, (name, n)
        digests[name] = (n, hashlib.sha1(memoryview(text)[:n]).hexdigest())
    del text
    assert digests["sort_device"] == digests["sort_host_level_3"], digests   # both legs wrote the same header and records
    res["legs_inflate_to_the_same_bytes"] = True
    times = {k: [] for k in legs}
    stages = []
    for _ in range(rounds):        # alternating
        for name, f in legs.items():
            c0, t0 = time.process_time(), time.perf_counter()
            n = f()
            times[name].append((time.perf_counter() - t0, time.process_time() - c0))
            assert n == sizes[name]
            if name == "sort_device":
                ms = (C.c_double * 8)()
                lib.mi355x_bam_sort_dev_stage_ms(ms)
                stages.append(list(ms))
    for name in legs:
        wall = [w for w, _ in times[name]]
        cpu = [c for _, c in times[name]]
        med = statistics.median(wall)
        res["legs"][name] = {"output_bytes": sizes[name], "wall_s": [round(w, 4) for w in wall], "wall_s_median": round(med, 4),
                             "records_per_s_median": round(n_rec / med), "GB_per_s_of_inflated_bam_median": round(u / med / 1e9, 3),
                             "GB_per_s_of_inflated_bam_best": round(u / min(wall) / 1e9, 3), "process_cpu_s_per_call_median": round(statistics.median(cpu), 3)}
    keys = ("inflate", "walk", "sort", "emit", "whole_call")
    res["device_stage_wall_ms_median"] = {k: round(statistics.median(s[i] for s in stages), 2) for i, k in enumerate(keys)}
    # the gather kernel alone on the device, and the plain copy of as many bytes
    os.environ["MPIBWA_BAM_SORT_GATHER_ALONE"] = "1"
    assert legs["sort_device"]() == sizes["sort_device"]
    del os.environ["MPIBWA_BAM_SORT_GATHER_ALONE"]
    ms = (C.c_double * 8)()
    lib.mi355x_bam_sort_dev_stage_ms(ms)
    g_ms, g_bytes = ms[5], int(ms[6])
    lib.mi355x_finalize()   # the sort's buffers back, for the copy's two
    c_ms = memcpy_ms(g_bytes)
    res["gather_kernel"] = {"bytes": g_bytes, "device_ms_summed_over_pieces": round(g_ms, 3), "GB_per_s": round(g_bytes / g_ms / 1e6, 1),
                            "memcpy_d2d_ms": round(c_ms, 3), "memcpy_d2d_GB_per_s": round(g_bytes / c_ms / 1e6, 1), "gather_over_memcpy_rate": round(c_ms / g_ms, 3)}
    c = (C.c_uint64 * 8)()
    lib.mi355x_bam_sort_dev_counts(c)
    res["sort_device_counts"] = dict(zip(("calls", "records", "calls_walked_by_the_host", "inflated_bytes", "input_blocks", "output_blocks", "compressed_bytes",
                                          "calls_refused_for_memory"), list(c)))
    path = opt("--out", os.path.join(ROOT, "profiles", "bam_sort_dev.json"), str)
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
