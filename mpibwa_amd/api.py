"""ctypes binding of libmpibwa_amd.so — the host-side mirror of the reference's
operator interface (mem_opt_init / bwa_idx_load / mem_process_seqs)."""
import ctypes as C
import os

import numpy as np

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

libc = C.CDLL(None if os.environ.get("MPIBWA_SANITIZER_LIB") else "libc.so.6")   # (under tools/san_host.sh: the sanitizer's malloc / free)
libc.free.argtypes = [C.c_void_p]

EXPORTS = [
    "mem_process_seqs", "mem_opt_init", "bwa_fill_scmat", "bwa_idx_load_from_disk", "bwa_mem2idx", "bwa_idx_destroy",
    "mi355x_index_upload", "mi355x_index_alloc", "mi355x_index_buffers", "mi355x_index_d2d", "mi355x_index_commit",
    "mi355x_finalize", "mi355x_index_build", "mi355x_index_build_gpu",
    "mi355x_smem_batch", "mi355x_sa_batch", "mi355x_sa_batch2", "mi355x_sa_dense_info", "mi355x_extend_batch", "mi355x_extend_batch2", "mi355x_matesw_batch", "mi355x_matesw_batch_counts", "mi355x_chain_batch", "mi355x_c2a_batch", "mi355x_pair_batch", "mi355x_pair_maxreg", "mi355x_fastq_scan", "mi355x_fastq_chunks", "mi355x_fastq_fill", "mi355x_last_stats", "mi355x_host_cpus", "mi355x_collect_sam", "mi355x_collect_sam_into", "mi355x_host_ksw_align2",
    "bwa_set_rg", "bwa_insert_header", "bwa_idx2mem", "mi355x_write_map", "mi355x_init", "mi355x_rank_host_threads", "mi355x_index_checksums", "mi355x_init_bcast_seconds", "mi355x_global_batch", "mi355x_global_batch_counts", "mi355x_device_count", "mi355x_device_cus", "mi355x_device_memory", "mi355x_buffer_growths", "mi355x_prewarm", "mi355x_max_calls",
    "mi355x_sam_batch", "mi355x_sam_arena_bytes", "mi355x_se_batch", "mi355x_sam_se_batch", "mi355x_seed_batch", "mi355x_pair_wave_batch", "mi355x_pair_wave_maxreg",
    "mi355x_pair_wave_xa_batch", "mi355x_pair_wave_xa_cap", "mi355x_dedup_batch", "mi355x_dedup_maxreg", "mi355x_se_wave_batch",
    "mi355x_se_lines_cap", "mi355x_se_wave_lines_batch", "mi355x_sam_se_lines_batch", "mi355x_sam_lines_row", "mi355x_sam_lines_sa_stage",
    "mi355x_pair_wave_lines_batch", "mi355x_sam_pe_lines_batch", "mi355x_pair_stage_batch", "mi355x_pair_stage_room",
]


class mi355x_comm_t(C.Structure):
    """include/mpibwa_amd.h: the caller's transport for the RCCL bootstrap id"""
    BCAST = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
    _fields_ = [("rank", C.c_int), ("size", C.c_int), ("bcast", BCAST), ("user", C.c_void_p)]



def load_library(build_if_missing=True):
    """Load the product library.  Fails loudly if it is absent and cannot be built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = os.path.join(HERE, "libmpibwa_amd.so")
    # tools/san_host.sh: the library's HOST sources alone, built with AddressSanitizer / UBSan — no kernels and none of the entry points
    # that need the GPU; only the host-logic tests run on it
    host_only = os.environ.get("MPIBWA_SANITIZER_LIB")
    if host_only:
        path = host_only
    if not os.path.exists(path):
        if not build_if_missing or host_only:
            raise RuntimeError("%s is missing: run python -m mpibwa_amd.build" % path)
        from .build import build
        build()
    lib = C.CDLL(path)
    P = C.POINTER

    def sig(name, restype, argtypes):
        try:
            fn = getattr(lib, name)  # AttributeError here = the library does not export what include/mpibwa_amd.h declares
        except AttributeError:
            if host_only:
                return
            raise
        fn.restype = restype
        fn.argtypes = argtypes

    sig("mem_opt_init", P(abi.mem_opt_t), [])
    sig("bwa_idx_load_from_disk", P(abi.bwaidx_t), [C.c_char_p, C.c_int])
    sig("mi355x_index_build", C.c_int, [C.c_char_p, C.c_char_p])
    sig("mi355x_index_build_gpu", C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_char_p, P(C.c_double)])
    sig("mem_process_seqs", None, [P(abi.mem_opt_t), P(abi.bwt_t), P(abi.bntseq_t), P(C.c_uint8), C.c_int64, C.c_int,
                                   P(abi.bseq1_t), P(abi.mem_pestat_t)])
    sig("mi355x_index_upload", C.c_int, [C.c_int, P(abi.bwt_t), P(abi.bntseq_t), P(C.c_uint8)])
    sig("mi355x_index_alloc", C.c_int, [C.c_int, P(abi.bwt_t), P(abi.bntseq_t)])
    sig("mi355x_index_buffers", C.c_int, [P(C.c_void_p), P(C.c_size_t)] * 3)
    sig("mi355x_index_d2d", C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int])
    sig("mi355x_index_commit", C.c_int, [])
    sig("mi355x_smem_batch", C.c_int, [P(abi.mem_opt_t), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p, P(C.c_double), P(C.c_uint64)])
    sig("mi355x_sa_batch", C.c_int, [C.c_int, C.c_void_p, C.c_void_p, P(C.c_double), P(C.c_uint64)])
    sig("mi355x_sa_batch2", C.c_int, [C.c_int, C.c_void_p, C.c_void_p, P(C.c_double), C.c_int])
    sig("mi355x_sa_dense_info", C.c_double, [P(C.c_size_t)])
    sig("mi355x_extend_batch", C.c_int, [P(abi.mem_opt_t), C.c_int] + [C.c_void_p] * 8 + [P(C.c_double), P(C.c_uint64)])
    sig("mi355x_extend_batch2", C.c_int, [P(abi.mem_opt_t), C.c_int] + [C.c_void_p] * 11 + [P(C.c_double)])
    sig("mi355x_chain_batch", C.c_int64, [P(abi.mem_opt_t), C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int64, C.c_void_p])
    sig("mi355x_c2a_batch", C.c_int64, [P(abi.mem_opt_t), C.c_void_p, C.c_int] + [C.c_void_p] * 10 + [C.c_int] * 3 +
        [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p])
    sig("mi355x_fastq_scan", C.c_int64, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p])
    sig("mi355x_fastq_chunks", C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p])
    sig("mi355x_fastq_fill", C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p])
    sig("mi355x_matesw_batch", C.c_int, [P(abi.mem_opt_t), C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [P(C.c_double)])
    sig("mi355x_last_stats", None, [P(abi.mi355x_stats_t)])
    sig("mi355x_finalize", None, [])
    sig("mi355x_host_ksw_align2", None, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p])
    sig("mi355x_host_cpus", C.c_int, [])
    sig("mi355x_host_sort_dedup_patch", C.c_int, [P(abi.mem_opt_t), P(abi.bntseq_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])
    sig("mi355x_host_reg2sam_se", None, [P(abi.mem_opt_t), P(abi.bntseq_t), C.c_void_p, P(abi.bseq1_t), C.c_void_p, C.c_int, C.c_int64])
    sig("mi355x_host_pestat", None, [P(abi.mem_opt_t), C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])
    sig("mi355x_host_flt_chained_seeds", None, [P(abi.mem_opt_t), P(abi.bntseq_t), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
    sig("mi355x_host_sam_pe", C.c_int, [P(abi.mem_opt_t), P(abi.bntseq_t), C.c_void_p, C.c_void_p, C.c_uint64, P(abi.bseq1_t), C.c_void_p, C.c_int, C.c_void_p, C.c_int])
    sig("mi355x_collect_sam", C.c_void_p, [P(abi.bseq1_t), C.c_int, P(C.c_size_t)])
    sig("mi355x_fixmate_pair", C.c_int, [P(abi.bseq1_t), P(abi.bseq1_t), P(abi.bntseq_t)])
    sig("mi355x_fixmate", C.c_int64, [P(abi.bseq1_t), C.c_int, P(abi.bntseq_t)])
    sig("mi355x_bgzf_bound", C.c_size_t, [C.c_size_t])
    sig("mi355x_bgzf_compress", C.c_size_t, [C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t])
    sig("mi355x_bgzf_eof", C.c_size_t, [C.c_void_p])
    sig("mi355x_bgzf_compress_dev", C.c_size_t, [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t])
    sig("mi355x_bgzf_dev_counts", None, [P(C.c_uint64)])
    sig("mi355x_bgzf_find_block", C.c_int64, [C.c_char_p, C.c_int64, C.c_int])
    sig("mi355x_bgzf_scan", C.c_int64, [C.c_char_p, C.c_int64, C.c_int64, P(C.c_int64), P(C.c_int64)])
    sig("mi355x_bgzf_inflate", C.c_int64, [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t])
    sig("mi355x_bgzf_inflate_dev", C.c_int64, [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t])
    sig("mi355x_bgzf_inflate_dev_counts", None, [P(C.c_uint64)])
    sig("mi355x_bam_header", C.c_int64, [C.c_char_p, C.c_size_t, P(abi.bntseq_t), C.c_void_p, C.c_size_t])
    sig("mi355x_bam_bound", C.c_int64, [C.c_size_t])
    sig("mi355x_sam_to_bam", C.c_int64, [C.c_char_p, C.c_size_t, P(abi.bntseq_t), C.c_void_p, C.c_size_t, P(C.c_int64)])
    sig("mi355x_sam_to_bam_dev", C.c_int64, [C.c_char_p, C.c_size_t, P(abi.bntseq_t), C.c_void_p, C.c_size_t, P(C.c_int64)])
    sig("mi355x_bam_compress", C.c_int64, [C.c_char_p, C.c_size_t, P(abi.bntseq_t), C.c_int, C.c_void_p, C.c_size_t])
    sig("mi355x_bam_compress_dev", C.c_int64, [C.c_char_p, C.c_size_t, P(abi.bntseq_t), C.c_void_p, C.c_size_t])
    sig("mi355x_bam_dev_counts", None, [P(C.c_uint64)])
    sig("mi355x_bam_sort_bound", C.c_int64, [C.c_char_p, C.c_size_t])
    sig("mi355x_bam_sort", C.c_int64, [C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t])
    sig("mi355x_bam_sort_dev", C.c_int64, [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t])
    sig("mi355x_bam_sort_dev_counts", None, [P(C.c_uint64)])
    sig("mi355x_bam_sort_dev_stage_ms", None, [P(C.c_double)])
    sig("mi355x_bam_sort_dev_refused_need", C.c_uint64, [])
    sig("mi355x_bam_index", C.c_int64, [C.c_char_p, C.c_size_t, P(C.c_void_p), P(C.c_size_t), P(C.c_int)])
    sig("mi355x_bam_index_dev", C.c_int64, [C.c_char_p, C.c_size_t, P(C.c_void_p), P(C.c_size_t), P(C.c_int)])
    sig("mi355x_bam_sort_index_dev", C.c_int64, [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, P(C.c_void_p), P(C.c_size_t), P(C.c_int)])
    sig("mi355x_bam_index_dev_counts", None, [P(C.c_uint64)])
    sig("mi355x_bam_index_dev_stage_ms", None, [P(C.c_double)])
    sig("mi355x_route_by_chr", C.c_int64, [C.c_char_p, C.c_size_t, P(abi.bntseq_t), C.c_int, P(C.c_void_p), P(C.c_size_t)])
    sig("bwa_set_rg", C.c_void_p, [C.c_char_p])
    sig("bwa_insert_header", C.c_void_p, [C.c_char_p, C.c_void_p])
    sig("bwa_idx2mem", C.c_int, [P(abi.bwaidx_t)])
    sig("bwa_mem2idx", C.c_int, [C.c_int64, C.c_void_p, P(abi.bwaidx_t)])
    sig("bwa_idx_destroy", None, [P(abi.bwaidx_t)])
    sig("mi355x_write_map", C.c_int, [C.c_char_p, C.c_char_p])
    sig("mi355x_init", C.c_int, [C.c_int, P(abi.bwaidx_t), P(mi355x_comm_t)])
    sig("mi355x_init_bcast_seconds", C.c_double, [])
    sig("mi355x_index_checksums", C.c_int, [C.c_void_p])
    sig("mi355x_device_count", C.c_int, [])
    sig("mi355x_device_cus", C.c_int, [])
    sig("mi355x_device_memory", C.c_int, [P(C.c_size_t), P(C.c_size_t)])
    sig("mi355x_buffer_growths", C.c_ulonglong, [])
    sig("mi355x_pair_batch", C.c_int, [P(abi.mem_opt_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
    sig("mi355x_pair_stage_room", C.c_int, [C.c_int])
    sig("mi355x_pair_stage_batch", C.c_int, [P(abi.mem_opt_t), C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p])
    sig("mi355x_pair_wave_maxreg", C.c_int, [])
    sig("mi355x_pair_wave_batch", C.c_int, [P(abi.mem_opt_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 8)
    sig("mi355x_pair_wave_xa_cap", C.c_int, [])
    sig("mi355x_pair_wave_xa_batch", C.c_int, [P(abi.mem_opt_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 10)
    sig("mi355x_pair_wave_lines_batch", C.c_int, [P(abi.mem_opt_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 15)
    sig("mi355x_global_batch", C.c_int, [P(abi.mem_opt_t), C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7 +
        [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, P(C.c_double)])
    sig("mi355x_global_batch_counts", None, [P(C.c_uint64)])
    sig("mi355x_matesw_batch_counts", None, [P(C.c_uint64)])
    sig("mi355x_sam_arena_bytes", C.c_size_t, [C.c_int, C.c_int])
    sig("mi355x_sam_batch", C.c_int, [P(abi.mem_opt_t), C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_size_t, C.c_int] + [C.c_void_p] * 5)
    sig("mi355x_sam_se_batch", C.c_int, [P(abi.mem_opt_t), C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_size_t, C.c_int] + [C.c_void_p] * 5)
    sig("mi355x_se_batch", C.c_int, [P(abi.mem_opt_t), C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
    sig("mi355x_se_wave_batch", C.c_int, [P(abi.mem_opt_t), C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5)
    sig("mi355x_se_lines_cap", C.c_int, [])
    sig("mi355x_se_wave_lines_batch", C.c_int, [P(abi.mem_opt_t), C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 10)
    sig("mi355x_sam_lines_row", C.c_int, [])
    sig("mi355x_sam_lines_sa_stage", C.c_int, [])
    sig("mi355x_sam_se_lines_batch", C.c_int, [P(abi.mem_opt_t), C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 9 + [C.c_size_t, C.c_int] + [C.c_void_p] * 5)
    sig("mi355x_sam_pe_lines_batch", C.c_int, [P(abi.mem_opt_t), C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 9 + [C.c_size_t, C.c_int] + [C.c_void_p] * 5)
    sig("mi355x_dedup_maxreg", C.c_int, [])
    sig("mi355x_dedup_batch", C.c_int, [P(abi.mem_opt_t), C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [P(C.c_double)])
    sig("mi355x_seed_batch", C.c_int64, [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int64])
    _LIB = lib
    return lib


_HIP = None


def _hip():
    global _HIP
    if _HIP is None:
        _HIP = C.CDLL("libamdhip64.so")
        _HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _HIP


def build_index(fasta, prefix):
    lib = load_library()
    if lib.mi355x_index_build(fasta.encode(), prefix.encode()) != 0:
        raise RuntimeError("index build failed")


class Engine:
    """One rank = one GPU: loads a bwa index, uploads it to HBM and aligns batches."""

    def __init__(self, prefix, device=0, upload=True, dist=None, rank=0, map_path=None, comm=None):
        """dist given (torch.distributed, nccl = RCCL): rank 0 uploads the index from host memory, every other rank only
        allocates the device buffers and receives occ blocks, SA and pac by broadcast over xGMI.
        map_path given: the index is attached from mpiBWA's `.map` image (bwa_mem2idx) instead of the five bwa files.
        comm given (mi355x_comm_t): residency through mi355x_init(), i.e. the C-side RCCL broadcast."""
        self.lib = load_library()
        if map_path is not None:
            import numpy as np
            self._map = np.fromfile(map_path, dtype=np.uint8)          # writable: bwa_mem2idx rebuilds the pointers inside
            self._idx_obj = abi.bwaidx_t()
            self.lib.bwa_mem2idx(len(self._map), self._map.ctypes.data, C.byref(self._idx_obj))
            self.idx = C.pointer(self._idx_obj)
        else:
            self.idx = self.lib.bwa_idx_load_from_disk(prefix.encode(), 7)
        self.bwt = self.idx.contents.bwt
        self.bns = self.idx.contents.bns
        self.pac = self.idx.contents.pac
        self.uploaded = False
        self.bcast_seconds = None
        if upload and comm is not None:
            if self.lib.mi355x_init(device, self.idx, C.byref(comm)) != 0:
                raise RuntimeError("mi355x_init failed")
            self.uploaded = True
            self.bcast_seconds = self.lib.mi355x_init_bcast_seconds()
        elif upload and dist is None:
            if self.lib.mi355x_index_upload(device, self.bwt, self.bns, self.pac) != 0:
                raise RuntimeError("mi355x_index_upload failed")
            self.uploaded = True
        elif upload:
            self._upload_by_broadcast(device, dist, rank)

    def _upload_by_broadcast(self, device, dist, rank):
        """One collective per index array, in place: every rank allocates the three device arrays, rank 0 fills its own from
        host memory (one H2D), then torch.distributed.broadcast (nccl = RCCL over xGMI) runs directly on views of those
        arrays — no staging tensor, no device-to-device copy, no synchronisation between pieces (they are queued back to
        back on the collective's stream and pipeline along the ring); one synchronize at the end, then every rank expands
        its own dense SA and jump table."""
        import time
        import torch
        os.environ["MPIBWA_SA_DENSE"] = os.environ.get("MPIBWA_SA_DENSE", "1")
        if self.lib.mi355x_index_alloc(device, self.bwt, self.bns) != 0:
            raise RuntimeError("mi355x_index_alloc failed")
        pv = [C.c_void_p() for _ in range(3)]
        sv = [C.c_size_t() for _ in range(3)]
        self.lib.mi355x_index_buffers(C.byref(pv[0]), C.byref(sv[0]), C.byref(pv[1]), C.byref(sv[1]), C.byref(pv[2]), C.byref(sv[2]))
        if rank == 0:
            HIP = _hip()
            srcs = [(C.cast(self.bwt.contents.bwt, C.c_void_p), int(self.bwt.contents.bwt_size) * 4),
                    (C.cast(self.bwt.contents.sa, C.c_void_p), int(self.bwt.contents.n_sa) * 8),
                    (C.cast(self.pac, C.c_void_p), int(self.bns.contents.l_pac) // 4 + 1)]
            for which, (src, nbytes) in enumerate(srcs):
                if HIP.hipMemcpy(C.c_void_p(pv[which].value), src, C.c_size_t(nbytes), 1) != 0:   # hipMemcpyHostToDevice
                    raise RuntimeError("hipMemcpy H2D failed")

        class _DevView:   # zero-copy torch view of a raw device allocation
            def __init__(self, ptr, nbytes):
                self.__cuda_array_interface__ = {"data": (ptr, False), "shape": (nbytes,), "typestr": "|u1", "version": 2}
        t0 = time.time()
        piece = int(os.environ.get("MPIBWA_BCAST_PIECE_MB", "256")) << 20
        views = []
        for which in range(3):
            v = torch.as_tensor(_DevView(pv[which].value, sv[which].value), device="cuda:%d" % device)
            views.append(v)
            for off in range(0, sv[which].value, piece):
                dist.broadcast(v[off:off + piece], src=0)
        torch.cuda.synchronize(device)
        self.bcast_seconds = time.time() - t0
        del views
        # every rank hashes what it now holds on its device; rank 0's numbers go round; a rank that differs stops the run here
        mine = (C.c_uint64 * 3)()
        if self.lib.mi355x_index_checksums(mine) != 0:
            raise RuntimeError("mi355x_index_checksums failed")
        self.index_checksums = [int(x) for x in mine]
        objs = [self.index_checksums if rank == 0 else None]
        dist.broadcast_object_list(objs, src=0)
        if objs[0] != self.index_checksums:
            raise RuntimeError("rank %d received a damaged index by broadcast: checksums %s, rank 0 sent %s" % (rank, self.index_checksums, objs[0]))
        if self.lib.mi355x_index_commit() != 0:
            raise RuntimeError("mi355x_index_commit failed")
        self.uploaded = True

    def opt(self, **kw):
        o = self.lib.mem_opt_init()
        for k, v in kw.items():
            setattr(o.contents, k, v)
        return o

    def process(self, opt, reads, n_processed=0, pes0=None, with_qual=True, comment=None):
        batch = abi.SeqBatch(libc, reads, with_qual=with_qual, comment=comment)
        self.lib.mem_process_seqs(opt, self.bwt, self.bns, self.pac, n_processed, batch.n, batch.arr, pes0)
        return batch.take_sam()

    def prewarm(self, opt, n_reads, read_len=150, n_calls=1):
        """First-use cost of n_calls call contexts paid now (include/mpibwa_amd.h: mi355x_prewarm); seconds it took."""
        self.lib.mi355x_prewarm.restype = C.c_double
        self.lib.mi355x_prewarm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        as_p = lambda x: C.cast(x, C.c_void_p)
        return float(self.lib.mi355x_prewarm(as_p(opt), as_p(self.bwt), as_p(self.bns), as_p(self.pac), int(n_reads), int(read_len), int(n_calls)))

    def process_batch(self, opt, batch, n_processed=0, pes0=None):
        self.lib.mem_process_seqs(opt, self.bwt, self.bns, self.pac, n_processed, batch.n, batch.arr, pes0)

    def collect_sam(self, batch):
        """All SAM text of the batch as one bytes object (frees the per-read strings like mpiBWA's writer does)."""
        n = C.c_size_t(0)
        p = self.lib.mi355x_collect_sam(batch.arr, batch.n, C.byref(n))
        out = C.string_at(p, n.value)
        libc.free(C.c_void_p(p))
        return out

    def stats(self):
        st = abi.mi355x_stats_t()
        self.lib.mi355x_last_stats(C.byref(st))
        return {k: getattr(st, k) for k, _ in st._fields_}

    # ---- stage-level kernels ----
    def smem(self, opt, seqs, cap=256):
        """seqs: list of uint8 code arrays → list of (n_i,4) uint64 arrays sorted by info."""
        off = np.zeros(len(seqs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        flat = np.concatenate(seqs).astype(np.uint8) if len(seqs) else np.zeros(0, np.uint8)
        out = np.zeros((len(seqs), cap, 4), dtype=np.uint64)
        cnt = np.zeros(len(seqs), dtype=np.int32)
        ms = C.c_double(0)
        nbytes = C.c_uint64(0)
        rc = self.lib.mi355x_smem_batch(opt, len(seqs), flat.ctypes.data, off.ctypes.data, cap, out.ctypes.data,
                                        cnt.ctypes.data, C.byref(ms), C.byref(nbytes))
        if rc != 0:
            raise RuntimeError("mi355x_smem_batch overflowed cap=%d" % cap)
        return [out[i, :cnt[i]].copy() for i in range(len(seqs))], ms.value, nbytes.value

    def sa(self, ks):
        ks = np.ascontiguousarray(ks, dtype=np.uint64)
        out = np.zeros(len(ks), dtype=np.uint64)
        ms = C.c_double(0)
        nbytes = C.c_uint64(0)
        self.lib.mi355x_sa_batch(len(ks), ks.ctypes.data, out.ctypes.data, C.byref(ms), C.byref(nbytes))
        return out, ms.value, nbytes.value

    def sa_dense(self, ks):
        """Lookups through the dense SA table (None if the table was not expanded)."""
        ks = np.ascontiguousarray(ks, dtype=np.uint64)
        out = np.zeros(len(ks), dtype=np.uint64)
        ms = C.c_double(0)
        rc = self.lib.mi355x_sa_batch2(len(ks), ks.ctypes.data, out.ctypes.data, C.byref(ms), 1)
        return (out, ms.value) if rc == 0 else None

    def chains(self, opt, lens, l_rep, seeds_per_read, which):
        """Chaining stage for reads given by their seeds [(rbeg, qbeg, len), ...]; which = 0 device kernel, 1 host path.
        Returns per read None (device declines) or a list of chains (rid, far_beg, far_end, rmax0, rmax1, frac_bits, [(rbeg, qbeg, len)...])."""
        n = len(seeds_per_read)
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in seeds_per_read])
        S = int(off[n])
        rbeg = np.zeros(max(S, 1), dtype=np.uint64)
        ql = np.zeros(2 * max(S, 1), dtype=np.int32)
        k = 0
        for s in seeds_per_read:
            for rb, qb, ln in s:
                rbeg[k] = rb; ql[2 * k] = qb; ql[2 * k + 1] = ln
                k += 1
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        l_rep = np.ascontiguousarray(l_rep, dtype=np.int32)
        cap = n + 16 * S + 64 * n + 64
        out = np.zeros(cap, dtype=np.int64)
        out_off = np.zeros(n + 1, dtype=np.int64)
        rc = self.lib.mi355x_chain_batch(opt, C.cast(self.bns, C.c_void_p), n, lens.ctypes.data, l_rep.ctypes.data, off.ctypes.data, rbeg.ctypes.data,
                                         ql.ctypes.data, which, out.ctypes.data, cap, out_off.ctypes.data)
        assert rc >= 0
        res = []
        for r in range(n):
            p = int(out_off[r])
            nc = int(out[p]); p += 1
            if nc < 0:
                res.append(None)
                continue
            chs = []
            for _ in range(nc):
                rid, ns, fb, fe, r0, r1, fr = (int(x) for x in out[p:p + 7]); p += 7
                sd = [tuple(int(x) for x in out[p + 3 * j:p + 3 * j + 3]) for j in range(ns)]
                p += 3 * ns
                chs.append((rid, fb, fe, r0, r1, fr, sd))
            res.append(chs)
        return res

    C2A_FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep")

    def chain2aln(self, opt, reads, chains, heavy_t=8, early=1, layout=0):
        """Chain -> regions stage (mi355x_c2a_batch) on the resident index.  reads: nt4 code arrays; chains: per read a list of chains
        (rid, frac_rep, [(rbeg, qbeg, len, score), ...]) as mem_chain_t holds them after mem_chain_flt and mem_flt_chained_seeds.
        heavy_t: chain count above which a read goes through the chain groups (0: never); early: 0, 1 or 2; layout: 0 = slots of
        device-chained reads, 1 = of host-chained reads.  Returns (per read an int64 array (n_regs, 11) in C2A_FIELDS order, frac_rep as
        float bits; {"cells", "n_ext", "n_closed", "n_diff"}; units)."""
        n = len(reads)
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(r) for r in reads])
        flat = np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads]) if n else np.zeros(0, np.uint8)
        flat = np.ascontiguousarray(np.append(flat, np.zeros(1, np.uint8)))
        n_chains = np.array([len(c) for c in chains], dtype=np.int32)
        ch = [c for per in chains for c in per]
        rid = np.array([c[0] for c in ch] or [0], dtype=np.int32)
        frac = np.array([c[1] for c in ch] or [0], dtype=np.float32)
        nsd = np.array([len(c[2]) for c in ch] or [0], dtype=np.int32)
        sd = np.array([s for c in ch for s in c[2]] or [(0, 0, 0, 0)], dtype=np.int64).reshape(-1, 4)
        rbeg = np.ascontiguousarray(sd[:, 0])
        qbeg, ln, sc = (np.ascontiguousarray(sd[:, k], dtype=np.int32) for k in (1, 2, 3))
        cap = n + 11 * max(int(nsd.sum()), 1) + 64
        out = np.zeros(cap, dtype=np.int64)
        out_off = np.zeros(n + 1, dtype=np.int64)
        stat = np.zeros(4, dtype=np.uint64)
        units = C.c_int(0)
        rc = self.lib.mi355x_c2a_batch(opt, C.cast(self.bns, C.c_void_p), n, flat.ctypes.data, off.ctypes.data, n_chains.ctypes.data, rid.ctypes.data,
                                       frac.ctypes.data, nsd.ctypes.data, rbeg.ctypes.data, qbeg.ctypes.data, ln.ctypes.data, sc.ctypes.data,
                                       int(heavy_t), int(early), int(layout), out.ctypes.data, cap, out_off.ctypes.data, stat.ctypes.data, C.addressof(units))
        assert rc >= 0
        res = []
        for r in range(n):
            p = int(out_off[r])
            m = int(out[p])
            res.append(out[p + 1:p + 1 + 11 * m].reshape(m, 11).copy())
        st = dict(zip(("cells", "n_ext", "n_closed", "n_diff"), (int(x) for x in stat)))
        return res, st, units.value

    REG_DT = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("rid", "<i4"), ("score", "<i4"), ("truesc", "<i4"), ("w", "<i4"),
                       ("seedcov", "<i4"), ("seedlen0", "<i4"), ("frac_rep", "<f4"), ("pad", "<i4")])
    DESC_DT = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("req", "<i4"), ("rid", "<i4"), ("flag", "<i4"), ("mapq", "<i4"),
                        ("score", "<i4"), ("sub", "<i4")])
    AREQ_DT = np.dtype([("rb", "<i8"), ("re", "<i8"), ("read", "<i4"), ("qb", "<i4"), ("qe", "<i4"), ("w2", "<i4"), ("truesc", "<i4"), ("pad", "<i4")])

    def pairs(self, opt, pes, regs, n_regs, max_len=150, n_processed=0):
        """pair_simple_kernel on pairs given by their regions: regs (2 n_pairs, mi355x_pair_maxreg()) of REG_DT, n_regs (2 n_pairs).
        -> status (n_pairs,) uint8, desc (2 n_pairs,) DESC_DT, req (2 n_pairs,) AREQ_DT"""
        regs = np.ascontiguousarray(regs, dtype=self.REG_DT)
        assert regs.shape[1] == self.lib.mi355x_pair_maxreg()
        n_regs = np.ascontiguousarray(n_regs, dtype=np.int32)
        n_pairs = len(n_regs) // 2
        status = np.zeros(n_pairs, dtype=np.uint8)
        desc = np.zeros(2 * n_pairs, dtype=self.DESC_DT)
        req = np.zeros(2 * n_pairs, dtype=self.AREQ_DT)
        rc = self.lib.mi355x_pair_batch(opt, C.cast(self.bns, C.c_void_p), C.cast(pes, C.c_void_p), n_processed, n_pairs, regs.ctypes.data, n_regs.ctypes.data,
                                        max_len, status.ctypes.data, desc.ctypes.data, req.ctypes.data)
        if rc != 0:
            raise RuntimeError("mi355x_pair_batch: the kernel cannot use these insert-size statistics")
        return status, desc, req

    def pairs_stage(self, opt, pes, regs, n_regs, pair_ok=None, max_len=150, n_processed=0, fill=0xA5):
        """pairs() through mi355x_pair_stage_batch: pair_ok (n_pairs,) bytes, default all 1; the three arrays come back whole, with room
        for mi355x_pair_stage_room(n_pairs) pairs and every byte `fill` before the launch.
        -> status (room,) uint8, desc (2 room,) DESC_DT, req (2 room,) AREQ_DT"""
        regs = np.ascontiguousarray(regs, dtype=self.REG_DT)
        assert regs.ndim == 2 and regs.shape[1] == self.lib.mi355x_pair_maxreg()
        n_regs = np.ascontiguousarray(n_regs, dtype=np.int32)
        n_pairs = len(n_regs) // 2
        assert len(n_regs) == 2 * n_pairs and regs.shape[0] == 2 * n_pairs
        pair_ok = np.ones(n_pairs, dtype=np.uint8) if pair_ok is None else np.ascontiguousarray(pair_ok, dtype=np.uint8)
        assert len(pair_ok) == n_pairs
        room = int(self.lib.mi355x_pair_stage_room(n_pairs))
        status = np.zeros(room, dtype=np.uint8)
        desc = np.zeros(2 * room, dtype=self.DESC_DT)
        req = np.zeros(2 * room, dtype=self.AREQ_DT)
        rc = self.lib.mi355x_pair_stage_batch(opt, C.cast(self.bns, C.c_void_p), C.cast(pes, C.c_void_p), n_processed, n_pairs, regs.ctypes.data,
                                              n_regs.ctypes.data, pair_ok.ctypes.data, max_len, fill, status.ctypes.data, desc.ctypes.data, req.ctypes.data)
        if rc != 0:
            raise RuntimeError("mi355x_pair_stage_batch: the kernel cannot use these insert-size statistics")
        return status, desc, req

    PW_DECIDED_XA = 16

    def pairs_wave_xa(self, opt, pes, reads, regs, n_processed=0):
        """pairs_wave with the XA listing on (mi355x_pair_wave_xa_batch): status PW_DECIDED_XA = decided with an XA tag on a record.
        -> status, desc, req, xa_req (per read an AREQ_DT array of its XA entries' requests, pad = the entry's contig), alignments run.
        For sam_records the pair's requests are [req[2k], *xa_req[2k], req[2k + 1], *xa_req[2k + 1]]; desc already says so."""
        return self.pairs_wave(opt, pes, reads, regs, n_processed, xa=True)

    def pairs_wave(self, opt, pes, reads, regs, n_processed=0, xa=False):
        """pair_wave_kernel behind the pipeline's own rescue listing and mate-rescue kernel (mi355x_pair_wave_batch).  reads: 2 n_pairs nt4
        code arrays; regs: per read a REG_DT array of its regions after mem_sort_dedup_patch (at most mi355x_pair_wave_maxreg() are taken).
        -> status (n_pairs,) uint8, desc (2 n_pairs,) DESC_DT, req (2 n_pairs,) AREQ_DT, number of local alignments run"""
        n = len(reads)
        assert n % 2 == 0 and len(regs) == n
        n_pairs = n // 2
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(r) for r in reads])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads])) if n else np.zeros(1, dtype=np.uint8)
        reg_off = np.zeros(n + 1, dtype=np.int32)
        reg_off[1:] = np.cumsum([len(r) for r in regs])
        allregs = np.zeros(max(1, int(reg_off[-1])), dtype=self.REG_DT)
        for r, a in enumerate(regs):
            allregs[reg_off[r]:reg_off[r + 1]] = np.asarray(a, dtype=self.REG_DT)
        status = np.zeros(n_pairs, dtype=np.uint8)
        desc = np.zeros(n, dtype=self.DESC_DT)
        req = np.zeros(n, dtype=self.AREQ_DT)
        n_align = C.c_int(0)
        args = (opt, C.cast(self.bns, C.c_void_p), C.cast(self.pac, C.c_void_p), C.cast(pes, C.c_void_p), n_processed, n_pairs,
                flat.ctypes.data, off.ctypes.data, allregs.ctypes.data, reg_off.ctypes.data, status.ctypes.data,
                desc.ctypes.data, req.ctypes.data, C.cast(C.byref(n_align), C.c_void_p))
        if xa:
            cap = self.lib.mi355x_pair_wave_xa_cap()
            xa_req = np.zeros((max(n, 1), cap), dtype=self.AREQ_DT)
            xa_cnt = np.zeros(max(n, 1), dtype=np.uint8)
            rc = self.lib.mi355x_pair_wave_xa_batch(*args, xa_req.ctypes.data, xa_cnt.ctypes.data)
        else:
            rc = self.lib.mi355x_pair_wave_batch(*args)
        if rc != 0:
            raise RuntimeError("mi355x_pair_wave_batch: the kernel cannot use these insert-size statistics")
        if xa:
            return status, desc, req, [xa_req[r, :xa_cnt[r]].copy() for r in range(n)], n_align.value
        return status, desc, req, n_align.value

    PW_DECIDED_LINES = 17

    def pairs_wave_lines(self, opt, pes, reads, regs, n_processed=0, xa=True, lines=True):
        """pair_wave_kernel with its side arrays for the pairs mem_sam_pe reports end by end (mi355x_pair_wave_lines_batch); arguments as
        pairs_wave.  -> status, desc, req, xa_req as pairs_wave_xa returns them, n_lines (2 n_pairs,) uint8 — the lines of every read of a
        pair with status 17 (PW_DECIDED_LINES), 0: the unaligned record —, `lines`: per read a list of (desc, req, xa_req) per line in list
        order (a DESC_DT record, an AREQ_DT record and an AREQ_DT array), and the number of local alignments run.  For
        sam_records_pe_lines the pair's requests are [req, *xa_req] of read 2k's line 0, of its line 1, ..., then read 2k + 1's.
        xa=False: every XA listing off; lines=False: the side arrays are not handed over."""
        n = len(reads)
        assert n % 2 == 0 and len(regs) == n
        n_pairs = n // 2
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(r) for r in reads])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads])) if n else np.zeros(1, dtype=np.uint8)
        reg_off = np.zeros(n + 1, dtype=np.int32)
        reg_off[1:] = np.cumsum([len(r) for r in regs])
        allregs = np.zeros(max(1, int(reg_off[-1])), dtype=self.REG_DT)
        for r, a in enumerate(regs):
            if len(a):
                allregs[reg_off[r]:reg_off[r + 1]] = np.asarray(a, dtype=self.REG_DT)
        m = max(n, 1)
        cap, lcap = self.lib.mi355x_pair_wave_xa_cap(), self.lib.mi355x_se_lines_cap()
        status = np.zeros(max(n_pairs, 1), dtype=np.uint8)
        desc = np.zeros(m, dtype=self.DESC_DT)
        req = np.zeros(m, dtype=self.AREQ_DT)
        xa_req = np.zeros((m, cap), dtype=self.AREQ_DT)
        xa_cnt = np.zeros(m, dtype=np.uint8)
        n_lines = np.zeros(m, dtype=np.uint8)
        l_desc = np.zeros((m, lcap), dtype=self.DESC_DT)
        l_req = np.zeros((m, lcap), dtype=self.AREQ_DT)
        l_xc = np.zeros((m, lcap), dtype=np.uint8)
        l_xr = np.zeros((m, lcap, cap), dtype=self.AREQ_DT)
        n_align = C.c_int(0)
        ptr = lambda a, on: a.ctypes.data if on else None
        fn = self.lib.mi355x_pair_wave_lines_batch if lines else self.lib.mi355x_pair_wave_xa_batch if xa else self.lib.mi355x_pair_wave_batch
        args = (opt, C.cast(self.bns, C.c_void_p), C.cast(self.pac, C.c_void_p), C.cast(pes, C.c_void_p), n_processed, n_pairs,
                flat.ctypes.data, off.ctypes.data, allregs.ctypes.data, reg_off.ctypes.data, status.ctypes.data,
                desc.ctypes.data, req.ctypes.data, C.cast(C.byref(n_align), C.c_void_p))
        if lines:
            args += (ptr(xa_req, xa), ptr(xa_cnt, xa), n_lines.ctypes.data, l_desc.ctypes.data, l_req.ctypes.data, l_xc.ctypes.data, ptr(l_xr, xa))
        elif xa:
            args += (xa_req.ctypes.data, xa_cnt.ctypes.data)
        if fn(*args) != 0:
            raise RuntimeError("mi355x_pair_wave_lines_batch: the kernel cannot use these insert-size statistics")
        out = [[(l_desc[r, j].copy(), l_req[r, j].copy(), l_xr[r, j, :l_xc[r, j]].copy()) for j in range(int(n_lines[r]))] for r in range(n)]
        return status[:n_pairs], desc[:n], req[:n], [xa_req[r, :xa_cnt[r]].copy() for r in range(n)], n_lines[:n], out, n_align.value

    def singles(self, opt, regs, n_regs, max_len=150, n_processed=0):
        """se_simple_kernel on single-end reads given by their regions: regs (n_reads, mi355x_pair_maxreg()) of REG_DT, n_regs (n_reads).
        -> status (n_reads,) uint8, desc (n_reads,) DESC_DT, req (n_reads,) AREQ_DT"""
        regs = np.ascontiguousarray(regs, dtype=self.REG_DT)
        assert regs.shape[1] == self.lib.mi355x_pair_maxreg()
        n_regs = np.ascontiguousarray(n_regs, dtype=np.int32)
        n = len(n_regs)
        assert regs.shape[0] == n
        status = np.zeros(n, dtype=np.uint8)
        desc = np.zeros(n, dtype=self.DESC_DT)
        req = np.zeros(n, dtype=self.AREQ_DT)
        rc = self.lib.mi355x_se_batch(opt, C.cast(self.bns, C.c_void_p), n_processed, n, regs.ctypes.data, n_regs.ctypes.data, max_len,
                                      status.ctypes.data, desc.ctypes.data, req.ctypes.data)
        assert rc == 0
        return status, desc, req

    SE_DECIDED, SE_HOST_LENGTH, SE_HOST_ALT, SE_HOST_SUPP, SE_HOST_XA, SE_HOST_FULL, SE_HOST_TIE, SE_DECIDED_XA = 1, 5, 6, 10, 11, 13, 14, 16

    def singles_wave(self, opt, read_no, regs, max_len=150, n_processed=0, xa=True):
        """se_wave_kernel on single-end reads (mi355x_se_wave_batch).  read_no: the reads' numbers in the chunk (id = n_processed + number);
        regs: per read a REG_DT array of its regions after mem_sort_dedup_patch.  Everything comes back by work item.
        -> status (n,) uint8, desc (n,) DESC_DT, req (n,) AREQ_DT, xa_req (per read an AREQ_DT array of its XA entries' requests, pad = the
        entry's contig; empty with xa=False: the kernel then runs without the listing).  For sam_records_se the read's requests are
        [req[t], *xa_req[t]] (none for the unmapped record, desc.req = -3)."""
        n = len(regs)
        read_no = np.ascontiguousarray(read_no, dtype=np.int32)
        assert len(read_no) == n
        reg_off = np.zeros(n + 1, dtype=np.int32)
        reg_off[1:] = np.cumsum([len(r) for r in regs])
        allregs = np.zeros(max(1, int(reg_off[-1])), dtype=self.REG_DT)
        for r, a in enumerate(regs):
            if len(a):
                allregs[reg_off[r]:reg_off[r + 1]] = np.asarray(a, dtype=self.REG_DT)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        desc = np.zeros(max(n, 1), dtype=self.DESC_DT)
        req = np.zeros(max(n, 1), dtype=self.AREQ_DT)
        cap = self.lib.mi355x_pair_wave_xa_cap()
        xa_req = np.zeros((max(n, 1), cap), dtype=self.AREQ_DT)
        xa_cnt = np.zeros(max(n, 1), dtype=np.uint8)
        rc = self.lib.mi355x_se_wave_batch(opt, C.cast(self.bns, C.c_void_p), n_processed, n, read_no.ctypes.data, allregs.ctypes.data,
                                           reg_off.ctypes.data, max_len, status.ctypes.data, desc.ctypes.data, req.ctypes.data,
                                           xa_cnt.ctypes.data if xa else None, xa_req.ctypes.data if xa else None)
        assert rc == 0
        return status[:n], desc[:n], req[:n], [xa_req[t, :xa_cnt[t]].copy() for t in range(n)]

    SE_DECIDED_LINES = 17

    def singles_wave_lines(self, opt, read_no, regs, max_len=150, n_processed=0, xa=True, lines=True):
        """se_wave_kernel with its side arrays for reads of several lines (mi355x_se_wave_lines_batch); arguments as singles_wave.
        -> status, desc, req, xa_req as singles_wave returns them, and `lines`: per work item a list — empty unless status = 17
        (SE_DECIDED_LINES) — of (desc, req, xa_req) per line in list order: a DESC_DT record, an AREQ_DT record and an AREQ_DT array.
        For sam_records_se_lines the read's requests are [req, *xa_req] of line 0, then of line 1, ...  xa=False: both listings off;
        lines=False: the side arrays are not handed over and the call is singles_wave's."""
        n = len(regs)
        read_no = np.ascontiguousarray(read_no, dtype=np.int32)
        assert len(read_no) == n
        reg_off = np.zeros(n + 1, dtype=np.int32)
        reg_off[1:] = np.cumsum([len(r) for r in regs])
        allregs = np.zeros(max(1, int(reg_off[-1])), dtype=self.REG_DT)
        for r, a in enumerate(regs):
            if len(a):
                allregs[reg_off[r]:reg_off[r + 1]] = np.asarray(a, dtype=self.REG_DT)
        m = max(n, 1)
        cap, lcap = self.lib.mi355x_pair_wave_xa_cap(), self.lib.mi355x_se_lines_cap()
        status = np.zeros(m, dtype=np.uint8)
        desc = np.zeros(m, dtype=self.DESC_DT)
        req = np.zeros(m, dtype=self.AREQ_DT)
        xa_req = np.zeros((m, cap), dtype=self.AREQ_DT)
        xa_cnt = np.zeros(m, dtype=np.uint8)
        n_lines = np.zeros(m, dtype=np.uint8)
        l_desc = np.zeros((m, lcap), dtype=self.DESC_DT)
        l_req = np.zeros((m, lcap), dtype=self.AREQ_DT)
        l_xc = np.zeros((m, lcap), dtype=np.uint8)
        l_xr = np.zeros((m, lcap, cap), dtype=self.AREQ_DT)
        ptr = lambda a, on: a.ctypes.data if on else None
        rc = self.lib.mi355x_se_wave_lines_batch(opt, C.cast(self.bns, C.c_void_p), n_processed, n, read_no.ctypes.data, allregs.ctypes.data,
                                                 reg_off.ctypes.data, max_len, status.ctypes.data, desc.ctypes.data, req.ctypes.data,
                                                 ptr(xa_cnt, xa), ptr(xa_req, xa), ptr(n_lines, lines), ptr(l_desc, lines), ptr(l_req, lines),
                                                 ptr(l_xc, lines), ptr(l_xr, lines and xa))
        assert rc == 0
        out = [[(l_desc[t, j].copy(), l_req[t, j].copy(), l_xr[t, j, :l_xc[t, j]].copy()) for j in range(int(n_lines[t]))] for t in range(n)]
        return status[:n], desc[:n], req[:n], [xa_req[t, :xa_cnt[t]].copy() for t in range(n)], out

    DD_TAKEN, DD_HOST_MAXREG, DD_HOST_PATCH = 1, 3, 4
    DD_FILL = -0x5a5a5a5b

    def dedup(self, opt, lists, fill=DD_FILL):
        """The redundancy pass of mem_sort_dedup_patch on the device (mi355x_dedup_batch): lists = per read a REG_DT array of its raw regions.
        -> status (n,) uint8, m (n,) int32 (-1: declined), keep: per read an int32 array as long as its list — the first m entries are the
        places in the list of the regions the reference keeps, in its final order; the others still hold `fill`.
        self.last_dedup_ms is the kernels' time."""
        n = len(lists)
        reg_off = np.zeros(n + 1, dtype=np.int32)
        reg_off[1:] = np.cumsum([len(a) for a in lists])
        allregs = np.zeros(max(1, int(reg_off[-1])), dtype=self.REG_DT)
        for r, a in enumerate(lists):
            if len(a):
                allregs[reg_off[r]:reg_off[r + 1]] = np.asarray(a, dtype=self.REG_DT)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        m = np.full(max(n, 1), -1, dtype=np.int32)
        keep = np.full(max(1, int(reg_off[-1])), fill, dtype=np.int32)
        ms = C.c_double(0)
        rc = self.lib.mi355x_dedup_batch(opt, C.cast(self.bns, C.c_void_p), n, allregs.ctypes.data, reg_off.ctypes.data, status.ctypes.data,
                                         m.ctypes.data, keep.ctypes.data, C.byref(ms))
        assert rc == 0
        self.last_dedup_ms = ms.value
        return status[:n], m[:n], [keep[reg_off[r]:reg_off[r + 1]].copy() for r in range(n)]

    HDR_DT = np.dtype([("score", "<i4"), ("NM", "<i4"), ("n_cigar", "<i4"), ("md_len", "<i4"), ("pool_off", "<u4"), ("flags", "<i4")])
    SAM_GUARD = 4096
    SAM_GUARD_BYTE = 0xA5

    def sam_records_se(self, opt, reads, quals, names, desc, reqs, req_base, arena_bytes=0, grid_blocks=0):
        """sam_records for single-end descriptors (mi355x_sam_se_batch): n_reads reads, desc (n_reads,), req_base (n_reads + 1,)."""
        return self.sam_records(opt, reads, quals, names, desc, reqs, req_base, arena_bytes, grid_blocks, ends=1)

    def sam_records_se_lines(self, opt, reads, quals, names, n_lines, desc, reqs, req_base, arena_bytes=0, grid_blocks=0):
        """aln_kernel + sam_lines_kernel (mi355x_sam_se_lines_batch): n_reads single-end reads of n_lines[i] lines each (2 ..
        mi355x_se_lines_cap(); 0: not the device's), desc (n_reads, cap) DESC_DT with line j of read i at [i, j], reqs per read
        [line 0, its XA entries', line 1, ...] with read = i, req_base (n_reads + 1,).  -> sam_records' dict; out_len[i] covers all lines."""
        lcap = self.lib.mi355x_se_lines_cap()
        desc = np.ascontiguousarray(desc, dtype=self.DESC_DT).reshape(len(reads), lcap)
        n_lines = np.ascontiguousarray(n_lines, dtype=np.uint8)
        assert len(n_lines) == len(reads)
        return self.sam_records(opt, reads, quals, names, desc, reqs, req_base, arena_bytes, grid_blocks, ends=1, n_lines=n_lines)

    def sam_records_pe_lines(self, opt, reads, quals, names, n_lines, desc, reqs, req_base, arena_bytes=0, grid_blocks=0):
        """aln_kernel + the paired instantiation of sam_lines_kernel (mi355x_sam_pe_lines_batch): 2 n_pairs reads of n_lines[r] lines each
        (0 .. mi355x_se_lines_cap(); 0: the unaligned record), desc (2 n_pairs, cap) DESC_DT with line j of read r at [r, j], reqs per pair
        [read 2k: line 0, its XA entries', line 1, ...; read 2k + 1: ...] with read = 2k + e, req_base (n_pairs + 1,).
        -> sam_records' dict; out_len[r] covers all lines of read r."""
        lcap = self.lib.mi355x_se_lines_cap()
        desc = np.ascontiguousarray(desc, dtype=self.DESC_DT).reshape(len(reads), lcap)
        n_lines = np.ascontiguousarray(n_lines, dtype=np.uint8)
        assert len(n_lines) == len(reads)
        return self.sam_records(opt, reads, quals, names, desc, reqs, req_base, arena_bytes, grid_blocks, ends=2, n_lines=n_lines)

    def sam_records(self, opt, reads, quals, names, desc, reqs, req_base, arena_bytes=0, grid_blocks=0, ends=2, n_lines=None):
        """aln_kernel + sam_emit_kernel (mi355x_sam_batch) on chosen descriptors.  reads: 2 n_pairs nt4 code arrays; quals: as many byte
        strings or None; names: one byte string per read; desc (2 n_pairs,) DESC_DT; reqs AREQ_DT; req_base (n_pairs + 1,).
        -> dict: out_len, out_off, arena (arena_bytes of it), guard (the SAM_GUARD bytes behind it), arena_bytes, cursor, hdr (HDR_DT)"""
        n = len(reads)
        assert n % ends == 0 and len(names) == n and len(desc) == n and len(req_base) == n // ends + 1
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(r) for r in reads])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads]))
        fq = None
        if quals is not None:
            fq = np.frombuffer(b"".join(quals), dtype=np.uint8)
            assert len(fq) == len(flat)
        noff = np.zeros(n + 1, dtype=np.int32)
        noff[1:] = np.cumsum([len(x) for x in names])
        nm = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8)
        desc = np.ascontiguousarray(desc, dtype=self.DESC_DT)
        reqs = np.ascontiguousarray(reqs, dtype=self.AREQ_DT)
        req_base = np.ascontiguousarray(req_base, dtype=np.int32)
        assert int(req_base[-1]) == len(reqs)
        if not arena_bytes:
            arena_bytes = int(self.lib.mi355x_sam_arena_bytes(n, max(len(r) for r in reads)))
        out_len = np.zeros(n, dtype=np.int32)
        out_off = np.zeros(n, dtype=np.uint64)
        arena = np.zeros(arena_bytes + self.SAM_GUARD, dtype=np.uint8)
        cursor = np.zeros(1, dtype=np.uint64)
        hdr = np.zeros(max(len(reqs), 1), dtype=self.HDR_DT)
        fn = self.lib.mi355x_sam_batch if ends == 2 else self.lib.mi355x_sam_se_batch
        lines = ()
        if n_lines is not None:
            fn, lines = self.lib.mi355x_sam_se_lines_batch if ends == 1 else self.lib.mi355x_sam_pe_lines_batch, (n_lines.ctypes.data,)
        rc = fn(opt, C.cast(self.bns, C.c_void_p), C.cast(self.pac, C.c_void_p), n // ends, flat.ctypes.data, off.ctypes.data,
                                       fq.ctypes.data if fq is not None else None, nm.ctypes.data, noff.ctypes.data, *lines, desc.ctypes.data,
                                       reqs.ctypes.data if len(reqs) else None, req_base.ctypes.data, arena_bytes, int(grid_blocks), out_len.ctypes.data,
                                       out_off.ctypes.data, arena.ctypes.data, cursor.ctypes.data, hdr.ctypes.data)
        assert rc == 0
        return {"out_len": out_len, "out_off": out_off, "arena": arena[:arena_bytes], "guard": arena[arena_bytes:], "arena_bytes": arena_bytes,
                "cursor": int(cursor[0]), "hdr": hdr[:len(reqs)]}

    def seeds(self, intervals, cap, max_occ):
        """seed_prep_kernel + seed_enum_kernel (mi355x_seed_batch).  intervals: per read an (n_i, 4) uint64 array (x0, x1, size, info) in
        any order; a read with more than cap reports its true count and hands over the first cap.
        -> (sorted intervals per read, n_seeds, l_rep, per read (rows uint64 array, (n, 2) int32 array of qbeg, len))"""
        n = len(intervals)
        iv = np.zeros((n, cap, 4), dtype=np.uint64)
        cnt = np.zeros(n, dtype=np.int32)
        for r, a in enumerate(intervals):
            a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
            cnt[r] = len(a)
            iv[r, :min(len(a), cap)] = a[:cap]
        most = int(sum(min(int(s), max_occ) for r in range(n) for s in iv[r, :min(cnt[r], cap), 2]))
        n_seeds = np.zeros(n, dtype=np.int32)
        l_rep = np.zeros(n, dtype=np.int32)
        seed_off = np.zeros(n + 1, dtype=np.int64)
        rows = np.zeros(most + 1, dtype=np.uint64)
        qbl = np.zeros((most + 1, 2), dtype=np.int32)
        S = int(self.lib.mi355x_seed_batch(n, cap, max_occ, iv.ctypes.data, cnt.ctypes.data, n_seeds.ctypes.data, l_rep.ctypes.data,
                                           seed_off.ctypes.data, rows.ctypes.data, qbl.ctypes.data, most))
        if S < 0:
            raise RuntimeError("mi355x_seed_batch: the kernel counts %d seeds, the intervals allow %d" % (-1 - S, most))
        per = [(rows[seed_off[r]:seed_off[r + 1]].copy(), qbl[seed_off[r]:seed_off[r + 1]].copy()) for r in range(n)]
        return [iv[r, :min(cnt[r], cap)].copy() for r in range(n)], n_seeds, l_rep, per

    def matesw(self, opt, l_pac, pac, reads, rb, re, read, is_rev):
        """mem_matesw's ksw_align2 for windows of `pac`; returns (n_req x 8 int32, kernel ms)."""
        n = len(reads)
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in reads])
        flat = np.concatenate(reads).astype(np.uint8)
        rb = np.ascontiguousarray(rb, dtype=np.int64)
        re = np.ascontiguousarray(re, dtype=np.int64)
        read = np.ascontiguousarray(read, dtype=np.int32)
        is_rev = np.ascontiguousarray(is_rev, dtype=np.int32)
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        out = np.zeros((len(rb), 8), dtype=np.int32)
        ms = C.c_double(0)
        self.lib.mi355x_matesw_batch(opt, int(l_pac), pac.ctypes.data, n, flat.ctypes.data, off.ctypes.data, len(rb), rb.ctypes.data,
                                     re.ctypes.data, read.ctypes.data, is_rev.ctypes.data, out.ctypes.data, C.byref(ms))
        return out, ms.value

    def matesw_counts(self):
        """Of the last matesw(): what the second pass ran — quads of two alignments, of one, work items of a register launch, of the
        general launch."""
        c = (C.c_uint64 * 4)()
        self.lib.mi355x_matesw_batch_counts(c)
        return [int(x) for x in c]

    def global_align(self, opt, l_pac, pac, reads, rb, re, read, qb, qe, w, truesc, which=0, cigar_cap=128, md_cap=800):
        """mem_reg2aln's DP loop (CIGAR / MD / NM) for regions of `reads` against windows of `pac`, by aln_kernel.
        Returns (hdr (n,5) int32: score, NM, n_cigar, md_len, flags; list of cigar arrays; list of MD bytes; kernel ms)."""
        n = len(reads)
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in reads])
        flat = np.concatenate(reads).astype(np.uint8)
        arr = lambda x, t: np.ascontiguousarray(x, dtype=t)
        rb, re = arr(rb, np.int64), arr(re, np.int64)
        read, qb, qe, w, truesc = (arr(x, np.int32) for x in (read, qb, qe, w, truesc))
        pac = arr(pac, np.uint8)
        nr = len(rb)
        hdr = np.zeros((nr, 5), dtype=np.int32)
        cig = np.zeros((nr, cigar_cap), dtype=np.uint32)
        md = np.zeros((nr, md_cap), dtype=np.uint8)
        ms = C.c_double(0)
        rc = self.lib.mi355x_global_batch(opt, int(l_pac), pac.ctypes.data, n, flat.ctypes.data, off.ctypes.data, nr, rb.ctypes.data,
                                          re.ctypes.data, read.ctypes.data, qb.ctypes.data, qe.ctypes.data, w.ctypes.data,
                                          truesc.ctypes.data, which, hdr.ctypes.data, cig.ctypes.data, cigar_cap, md.ctypes.data, md_cap,
                                          C.byref(ms))
        if rc != 0:
            raise RuntimeError("mi355x_global_batch: result beyond cigar_cap / md_cap")
        cigs = [cig[i, :hdr[i, 2]].copy() for i in range(nr)]
        mds = [md[i, :hdr[i, 3]].tobytes() for i in range(nr)]
        return hdr, cigs, mds, ms.value

    def global_align_counts(self):
        """Of the last global_align(): the final lengths of aln_kernel's three request lists (no-DP, narrow band, full size) and
        the bytes of the result pool handed out."""
        c = (C.c_uint64 * 4)()
        self.lib.mi355x_global_batch_counts(c)
        return [int(x) for x in c]

    def extend(self, opt, qs, ts, w, h0, end_bonus):
        n = len(qs)
        qoff = np.zeros(n + 1, dtype=np.int64)
        qoff[1:] = np.cumsum([len(s) for s in qs])
        toff = np.zeros(n + 1, dtype=np.int64)
        toff[1:] = np.cumsum([len(s) for s in ts])
        qf = np.concatenate(qs).astype(np.uint8)
        tf = np.concatenate(ts).astype(np.uint8)
        w = np.ascontiguousarray(w, dtype=np.int32)
        h0 = np.ascontiguousarray(h0, dtype=np.int32)
        eb = np.ascontiguousarray(end_bonus, dtype=np.int32)
        out = np.zeros((n, 6), dtype=np.int32)
        ms = C.c_double(0)
        cells = C.c_uint64(0)
        self.lib.mi355x_extend_batch(opt, n, qf.ctypes.data, qoff.ctypes.data, tf.ctypes.data, toff.ctypes.data,
                                     w.ctypes.data, h0.ctypes.data, eb.ctypes.data, out.ctypes.data, C.byref(ms),
                                     C.byref(cells))
        return out, ms.value, cells.value

    def extend2(self, opt, qs, ts, w, h0, end_bonus, early, clip):
        """extend() through the row loop of the chain-to-region kernel: `early` (0 / 1) and `clip` per job (or one value for all);
        returns the six outputs per job, the kernel time and the cell count per job."""
        n = len(qs)
        qoff = np.zeros(n + 1, dtype=np.int64)
        qoff[1:] = np.cumsum([len(s) for s in qs])
        toff = np.zeros(n + 1, dtype=np.int64)
        toff[1:] = np.cumsum([len(s) for s in ts])
        qf = np.concatenate(qs).astype(np.uint8)
        tf = np.concatenate(ts).astype(np.uint8)
        w = np.ascontiguousarray(w, dtype=np.int32)
        h0 = np.ascontiguousarray(h0, dtype=np.int32)
        eb = np.ascontiguousarray(end_bonus, dtype=np.int32)
        early = np.ascontiguousarray(np.broadcast_to(np.asarray(early, dtype=np.int32), (n,)))
        clip = np.ascontiguousarray(np.broadcast_to(np.asarray(clip, dtype=np.int32), (n,)))
        out = np.zeros((n, 6), dtype=np.int32)
        cells = np.zeros(n, dtype=np.uint64)
        ms = C.c_double(0)
        self.lib.mi355x_extend_batch2(opt, n, qf.ctypes.data, qoff.ctypes.data, tf.ctypes.data, toff.ctypes.data,
                                      w.ctypes.data, h0.ctypes.data, eb.ctypes.data, early.ctypes.data, clip.ctypes.data,
                                      out.ctypes.data, cells.ctypes.data, C.byref(ms))
        return out, ms.value, cells
