// bam_sort_kernel.hip — the kernels of mi355x_bam_sort_dev (bam_sort_stage.hip): the record walk over the inflated stream, the order
// (hipCUB's stable radix sort over the key's bits) and the record gather that puts a piece's records back to back for the deflate.
// The hop, the validation and the key are bam_sort_util.h's.  DESIGN §8.5.
//
// The walk: a LANE per BGZF block.  The hop is a dependent chain of loads, a few hundred per block, and nothing in it can be shared
// among lanes: a wavefront per block would keep 63 lanes idle behind the one that hops, and a block staged in LDS first (64 KiB) would
// leave room for two blocks per CU.  With a lane per block every block of the file is in flight at once (a 3-GB stream has about 50 000
// blocks: 780 wavefronts), a pass costs one chain's latency, and the loads of a wavefront's 64 chains overlap.  Both passes walk the
// same chain: the first counts and validates, a scan gives every block its first record's index, the second writes offset, size and key.
//
// The gather: 16 lanes per record.  Sources are runs of a few hundred bytes at any byte alignment, the destination is dense.  A record's
// destination range is split at 16-byte boundaries of the piece buffer: the whole chunks between them are written as aligned dwordx4
// stores (16 lanes: 256 contiguous bytes per step), each assembled from five aligned source dwords (one dwordx4 and one dword load at a
// 4-byte boundary) by v_alignbyte with the record's byte shift; the at most 15 bytes in front of the first boundary and behind the last
// are single bytes, one lane each, because those chunks are shared with the neighbouring records.  No lane loops over bytes.
#include "hip_util.h"
#include "device.h"
#include "bam_sort_util.h"
#include <hipcub/hipcub.hpp>

namespace mbw {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) U32x4A4 { u32x4 v; };   // sixteen bytes at a 4-byte boundary: one global_load_dwordx4

// block b's part of the stream that holds records: from the header's end on
__device__ inline void block_range(const uint64_t *text_off, int b, uint64_t h_end, uint64_t &lo, uint64_t &hi)
{
	lo = text_off[b]; hi = text_off[b + 1];
	if (lo < h_end) lo = h_end;
}

// cnt[b] = the records of block b's chain; *bad = 1 when a chain meets a malformed record or does not end at its block's end
__global__ __launch_bounds__(64) void bam_walk_count_kernel(const uint8_t *__restrict__ u, const uint64_t *__restrict__ text_off, int n_blk, uint64_t h_end,
                                                            int32_t n_ref, uint32_t *__restrict__ cnt, uint32_t *__restrict__ bad)
{
	const int b = (int)(blockIdx.x * 64 + threadIdx.x);
	if (b > n_blk) return;
	if (b == n_blk) { cnt[b] = 0; return; }   // (the scan's last entry: the number of records)
	uint64_t at, hi;
	block_range(text_off, b, h_end, at, hi);
	uint32_t n = 0;
	bool ok = true;
	for (uint32_t step = 0; step < 0x10000 / 36 + 1 && at < hi; ++step) {   // (a hop is at least 36 bytes, a block at most 64 KiB)
		uint32_t size;
		uint64_t key;
		if (!bsort::record_at(u, at, hi, n_ref, &size, &key)) { ok = false; break; }
		at += size; ++n;
	}
	if (at < hi) ok = false;
	cnt[b] = ok ? n : 0;
	if (!ok) *bad = 1;
}

// the same chains again (they are well-formed: the host has read *bad): record first[b] + k gets its offset, size and key
__global__ __launch_bounds__(64) void bam_walk_write_kernel(const uint8_t *__restrict__ u, const uint64_t *__restrict__ text_off, int n_blk, uint64_t h_end,
                                                            int32_t n_ref, const uint32_t *__restrict__ first, uint64_t *__restrict__ off,
                                                            uint32_t *__restrict__ size_out, uint64_t *__restrict__ key_out)
{
	const int b = (int)(blockIdx.x * 64 + threadIdx.x);
	if (b >= n_blk) return;
	uint64_t at, hi;
	block_range(text_off, b, h_end, at, hi);
	uint32_t i = first[b];
	const uint32_t i_end = first[b + 1];   // (nothing is written beyond the block's own records, whatever the bytes say)
	for (; i < i_end && at < hi; ++i) {
		uint32_t size;
		uint64_t key;
		if (!bsort::record_at(u, at, hi, n_ref, &size, &key)) break;
		off[i] = at; size_out[i] = size; key_out[i] = key;
		at += size;
	}
}

__global__ __launch_bounds__(256) void bam_iota_kernel(uint32_t *__restrict__ idx, uint32_t n)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) idx[i] = i;
}

// ssize[i] = the size of the record that sorts to place i; ssize[n] = 0 (the scan's last entry: the stream's size)
__global__ __launch_bounds__(256) void bam_sorted_size_kernel(const uint32_t *__restrict__ size, const uint32_t *__restrict__ idx, uint32_t n,
                                                              uint32_t *__restrict__ ssize)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) { const uint32_t j = idx[i]; ssize[i] = j < n ? size[j] : 0; }
	else if (i == n) ssize[i] = 0;
}

struct Widen {
	__host__ __device__ uint64_t operator()(uint32_t v) const { return (uint64_t)v; }
};
typedef hipcub::TransformInputIterator<uint64_t, Widen, const uint32_t *> WideIn;

// Sorted records r0 .. r1 - 1, as far as they lie in [lo, hi) of the sorted stream, to piece[0 .. hi - lo): record r stands at dst[r] of
// the sorted stream and at off[idx[r]] of u.  piece may stand at any address (the 16-byte boundaries are those of the address, not of the
// offset); u has BAM_SORT_SLACK bytes behind its end.
__global__ __launch_bounds__(256) void bam_gather_kernel(const uint8_t *__restrict__ u, const uint64_t *__restrict__ off, const uint32_t *__restrict__ idx,
                                                         const uint64_t *__restrict__ dst, uint32_t n_rec, uint32_t r0, uint32_t r1, uint64_t lo, uint64_t hi,
                                                         uint8_t *__restrict__ piece)
{
	const uint32_t l = threadIdx.x & 15u;
	const uint32_t r = r0 + ((blockIdx.x * 256u + threadIdx.x) >> 4);
	if (r >= r1 || r >= n_rec) return;
	const uint64_t d0 = dst[r], d1 = dst[r + 1];
	const uint64_t a = d0 > lo ? d0 : lo, b = d1 < hi ? d1 : hi;
	if (a >= b) return;
	const uint32_t j = idx[r];
	if (j >= n_rec) return;
	const uint64_t src = off[j] + (a - d0);
	const uint32_t n = (uint32_t)(b - a);          // (at most the piece's size)
	const uint64_t o = a - lo;                      // where the bytes go in the piece
	const uint32_t to_edge = (16u - (uint32_t)((uintptr_t)(piece + o) & 15u)) & 15u, head = to_edge < n ? to_edge : n;
	if (l < head) piece[o + l] = u[src + l];
	const uint32_t n_chunks = (n - head) >> 4;
	const uint64_t s0 = src + head;
	const uint32_t sh = (uint32_t)(s0 & 3u);
	const uint8_t *s4 = u + (s0 - sh);              // (u is a device allocation's start: s4 is 4-byte aligned)
	u32x4 *o16 = (u32x4 *)(piece + o + head);
	for (uint32_t k = l; k < n_chunks; k += 16) {
		const u32x4 w = ((const U32x4A4 *)(s4 + 16ull * k))->v;
		const uint32_t w4 = *(const uint32_t *)(s4 + 16ull * k + 16);   // (at most 7 bytes beyond the record: the slack)
		u32x4 v;
		v.x = __builtin_amdgcn_alignbyte(w.y, w.x, sh);
		v.y = __builtin_amdgcn_alignbyte(w.z, w.y, sh);
		v.z = __builtin_amdgcn_alignbyte(w.w, w.z, sh);
		v.w = __builtin_amdgcn_alignbyte(w4, w.w, sh);
		o16[k] = v;
	}
	const uint32_t t0 = head + 16u * n_chunks;
	if (t0 + l < n) piece[o + t0 + l] = u[src + t0 + l];
}

} // namespace

void launch_bam_sort_count(void *stream, const uint8_t *d_u, const uint64_t *d_text_off, int n_blk, uint64_t h_end, int32_t n_ref, uint32_t *d_cnt, uint32_t *d_bad)
{
	hipLaunchKernelGGL(bam_walk_count_kernel, dim3((unsigned)(n_blk / 64 + 1)), dim3(64), 0, (hipStream_t)stream, d_u, d_text_off, n_blk, h_end, n_ref, d_cnt, d_bad);
	HIP_OK(hipGetLastError());
}

void launch_bam_sort_write(void *stream, const uint8_t *d_u, const uint64_t *d_text_off, int n_blk, uint64_t h_end, int32_t n_ref, const uint32_t *d_first,
                           uint64_t *d_off, uint32_t *d_size, uint64_t *d_key)
{
	if (n_blk <= 0) return;
	hipLaunchKernelGGL(bam_walk_write_kernel, dim3((unsigned)((n_blk + 63) / 64)), dim3(64), 0, (hipStream_t)stream, d_u, d_text_off, n_blk, h_end, n_ref, d_first,
	                   d_off, d_size, d_key);
	HIP_OK(hipGetLastError());
}

size_t bam_sort_temp_bytes(uint32_t n_rec, int n_blk)
{
	size_t a = 0, b = 0, c = 0;
	HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, a, (const uint32_t *)nullptr, (uint32_t *)nullptr, n_blk + 1));
	HIP_OK(hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n_rec));
	HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, c, WideIn((const uint32_t *)nullptr, Widen()), (uint64_t *)nullptr, (int)n_rec + 1));
	return std::max(a, std::max(b, c)) + 256;
}

void launch_bam_sort_scan(void *stream, void *d_tmp, size_t tmp_bytes, const uint32_t *d_cnt, uint32_t *d_first, int n_blk)
{
	HIP_OK(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_cnt, d_first, n_blk + 1, (hipStream_t)stream));
}

void launch_bam_sort_order(void *stream, void *d_tmp, size_t tmp_bytes, uint32_t n_rec, int bits, const uint64_t *d_key, uint64_t *d_key2, uint32_t *d_idx,
                           uint32_t *d_idx2, const uint32_t *d_size, uint32_t *d_ssize, uint64_t *d_dst)
{
	hipStream_t st = (hipStream_t)stream;
	const unsigned grid = (unsigned)(n_rec / 256 + 1);
	if (n_rec) {
		hipLaunchKernelGGL(bam_iota_kernel, dim3(grid), dim3(256), 0, st, d_idx, n_rec);
		HIP_OK(hipGetLastError());
		HIP_OK(hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, d_key, d_key2, (const uint32_t *)d_idx, d_idx2, (int)n_rec, 0, bits, st));
	}
	hipLaunchKernelGGL(bam_sorted_size_kernel, dim3(grid), dim3(256), 0, st, d_size, (const uint32_t *)d_idx2, n_rec, d_ssize);
	HIP_OK(hipGetLastError());
	HIP_OK(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, WideIn((const uint32_t *)d_ssize, Widen()), d_dst, (int)n_rec + 1, st));
}

void launch_bam_sort_gather(void *stream, const uint8_t *d_u, const uint64_t *d_off, const uint32_t *d_idx, const uint64_t *d_dst, uint32_t n_rec, uint32_t r0,
                            uint32_t r1, uint64_t lo, uint64_t hi, uint8_t *d_piece)
{
	if (r1 <= r0) return;
	hipLaunchKernelGGL(bam_gather_kernel, dim3((unsigned)((r1 - r0 + 15) / 16)), dim3(256), 0, (hipStream_t)stream, d_u, d_off, d_idx, d_dst, n_rec, r0, r1, lo, hi,
	                   d_piece);
	HIP_OK(hipGetLastError());
}

} // namespace mbw
