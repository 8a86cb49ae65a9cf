// bam_index_kernel.hip — the kernels of the BAI index for mi355x_bam_index_dev and mi355x_bam_sort_index_dev
// (bam_sort_stage.hip).  The rules are bam_index_util.h's.  Everything works in block-number space (block << 16 | offset in the block);
// the host translates to file offsets when it writes the bytes.
//
//   records   a lane per record in file order: the core fields and the CIGAR words (a short dependent loop), contig, interval, bin and
//             mapped; the block by a binary search in the cuts; the smallest stream offset of a record that ends beyond 2^29 or sorts
//             before its predecessor goes to *bad (an atomic only in a file that fails).
//   scans     an inclusive max-scan of ref << 32 | end, an exclusive sum of mapped, a head flag where (ref, bin) changes and hipCUB's
//             Flagged select of the heads' indices: the runs in file order.
//   contigs   a lane per contig: its records are [lower_bound(ref), lower_bound(ref + 1)) of the scanned maxima (the file is sorted),
//             so first v0, last v1, mapped, unmapped and n_intv need no atomics; an exclusive sum places the contigs' windows.
//   runs      the runs' keys, hipCUB's stable radix sort of (key, run) over ref_bits + 16 bits, their chunks gathered in that order.
//   windows   a lane per linear window: the first record whose scanned maximum exceeds ref << 32 | w << 14 is the first that ends behind
//             the window's start; it overlaps the window if it has that ref and begins before the window's end, else no record does
//             (later records begin later).  No contended atomic minimum per window.
#include "hip_util.h"
#include "device.h"
#include "bam_index_util.h"
#include <hipcub/hipcub.hpp>

namespace mbw {
namespace {

__global__ __launch_bounds__(256) void bai_record_kernel(const uint8_t *__restrict__ u, const uint64_t *__restrict__ off, const uint32_t *__restrict__ order,
                                                         const uint64_t *__restrict__ place, uint64_t place_base, const uint64_t *__restrict__ cut, uint64_t n_cut,
                                                         uint32_t n_rec, int32_t n_ref, const uint64_t *__restrict__ keys, uint64_t *__restrict__ rb,
                                                         uint64_t *__restrict__ v0, uint64_t *__restrict__ mx, uint32_t *__restrict__ beg, uint32_t *__restrict__ map,
                                                         unsigned long long *__restrict__ bad)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i > n_rec) return;
	if (i == n_rec) { map[i] = 0; return; }   // (the scan's last entry)
	const uint32_t j = order ? order[i] : i;
	if (j >= n_rec) return;
	const uint64_t at = off[j];
	const uint32_t size = bsort::load32(u, at) + 4;
	const bidx::Rec r = bidx::record_fields(u, at, size);
	bool fails = r.end > bidx::BAI_MAX_END;
	if (keys && i > 0 && keys[i] < keys[i - 1]) fails = true;
	if (fails) atomicMin(bad, (unsigned long long)at);
	const uint64_t end = r.end > bidx::BAI_MAX_END ? bidx::BAI_MAX_END + 1 : r.end;
	const uint32_t ref = r.ref < 0 ? (uint32_t)n_ref : (uint32_t)r.ref;
	rb[i] = bidx::run_key(r.ref, r.bin, n_ref);
	v0[i] = bidx::voffset_of(cut, n_cut, place_base + place[i]);
	mx[i] = (uint64_t)ref << 32 | end;
	beg[i] = r.beg;
	map[i] = r.mapped;
}

__global__ __launch_bounds__(256) void bai_head_kernel(const uint64_t *__restrict__ rb, uint32_t n_rec, uint8_t *__restrict__ head)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n_rec) head[i] = (i == 0 || rb[i] != rb[i - 1]) ? 1 : 0;
}

// the first i in [0, n) with a[i] >= x
__device__ inline uint32_t lower_bound64(const uint64_t *a, uint32_t n, uint64_t x)
{
	uint32_t lo = 0, hi = n;
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (a[mid] < x) lo = mid + 1; else hi = mid;
	}
	return lo;
}

// contig c < n_ref: stat[4 c ..] = v0 of its first record, v1 of its last, mapped, unmapped; n_intv[c].  c == n_ref: stat[4 c] = n_no_coor.
__global__ __launch_bounds__(256) void bai_contig_kernel(const uint64_t *__restrict__ mxs, const uint32_t *__restrict__ maps, const uint64_t *__restrict__ v0,
                                                         uint32_t n_rec, int32_t n_ref, uint64_t end_v, uint64_t *__restrict__ stat, uint32_t *__restrict__ n_intv)
{
	const uint32_t c = blockIdx.x * 256 + threadIdx.x;
	if (c > (uint32_t)n_ref) return;
	const uint32_t lo = lower_bound64(mxs, n_rec, (uint64_t)c << 32);
	if (c == (uint32_t)n_ref) {
		stat[4ull * c] = n_rec - lo; stat[4ull * c + 1] = 0; stat[4ull * c + 2] = 0; stat[4ull * c + 3] = 0;
		n_intv[c] = 0;
		return;
	}
	const uint32_t hi = lower_bound64(mxs, n_rec, ((uint64_t)c + 1) << 32);
	const uint32_t n = hi - lo, mapped = n ? maps[hi] - maps[lo] : 0;
	stat[4ull * c] = n ? v0[lo] : 0;
	stat[4ull * c + 1] = n ? (hi < n_rec ? v0[hi] : end_v) : 0;
	stat[4ull * c + 2] = mapped;
	stat[4ull * c + 3] = n - mapped;
	n_intv[c] = n ? (uint32_t)((((mxs[hi - 1] & 0xffffffffull) - 1) >> 14) + 1) : 0;
}

__global__ __launch_bounds__(256) void bai_run_key_kernel(const uint64_t *__restrict__ rb, const uint32_t *__restrict__ rs, uint32_t n_runs, uint32_t n_rec,
                                                          uint64_t *__restrict__ rk, uint32_t *__restrict__ ri)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r >= n_runs) return;
	const uint32_t i = rs[r];
	rk[r] = i < n_rec ? rb[i] : 0;
	ri[r] = r;
}

__global__ __launch_bounds__(256) void bai_run_chunk_kernel(const uint32_t *__restrict__ ri, const uint32_t *__restrict__ rs, const uint64_t *__restrict__ v0,
                                                            uint32_t n_runs, uint32_t n_rec, uint64_t end_v, uint64_t *__restrict__ rbeg, uint64_t *__restrict__ rend)
{
	const uint32_t q = blockIdx.x * 256 + threadIdx.x;
	if (q >= n_runs) return;
	const uint32_t r = ri[q];
	if (r >= n_runs) return;
	const uint32_t a = rs[r], b = r + 1 < n_runs ? rs[r + 1] : n_rec;
	rbeg[q] = a < n_rec ? v0[a] : end_v;
	rend[q] = b < n_rec ? v0[b] : end_v;
}

__global__ __launch_bounds__(256) void bai_window_kernel(const uint32_t *__restrict__ woff, int32_t n_ref, uint32_t n_win, const uint64_t *__restrict__ mxs,
                                                         const uint32_t *__restrict__ beg, const uint64_t *__restrict__ v0, uint32_t n_rec, uint64_t *__restrict__ io)
{
	const uint32_t g = blockIdx.x * 256 + threadIdx.x;
	if (g >= n_win) return;
	uint32_t lo = 0, hi = (uint32_t)n_ref;   // the last contig c with woff[c] <= g: woff[c + 1] > g, it has windows
	while (hi - lo > 1) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (woff[mid] <= g) lo = mid; else hi = mid;
	}
	const uint64_t c = lo, w = g - woff[lo];
	const uint32_t i = lower_bound64(mxs, n_rec, (c << 32 | w << 14) + 1);
	io[g] = (i < n_rec && (mxs[i] >> 32) == c && (uint64_t)beg[i] < (w + 1) << 14) ? v0[i] : bidx::BAI_NO_RECORD;
}

typedef hipcub::CountingInputIterator<uint32_t> Iota;

} // namespace

size_t bam_index_temp_bytes(uint32_t n_rec, int32_t n_ref, uint32_t n_runs)
{
	size_t a = 0, b = 0, c = 0, d = 0, e = 0;
	HIP_OK(hipcub::DeviceScan::InclusiveScan(nullptr, a, (const uint64_t *)nullptr, (uint64_t *)nullptr, hipcub::Max(), (int)n_rec));
	HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n_rec + 1));
	HIP_OK(hipcub::DeviceSelect::Flagged(nullptr, c, Iota(0), (const uint8_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)n_rec));
	HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, d, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n_ref + 1));
	HIP_OK(hipcub::DeviceRadixSort::SortPairs(nullptr, e, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n_runs));
	return std::max(std::max(a, b), std::max(c, std::max(d, e))) + 256;
}

void launch_bam_index_records(void *stream, const BamIndexBufs &B)
{
	hipStream_t st = (hipStream_t)stream;
	size_t tb = B.tmp_bytes;
	hipLaunchKernelGGL(bai_record_kernel, dim3(B.n_rec / 256 + 1), dim3(256), 0, st, B.u, B.off, B.order, B.place, B.place_base, B.cut, B.n_cut, B.n_rec, B.n_ref,
	                   B.keys, B.rb, B.v0, B.mx, B.beg, B.map, B.bad);
	HIP_OK(hipGetLastError());
	if (B.n_rec) {
		HIP_OK(hipcub::DeviceScan::InclusiveScan(B.tmp, tb, (const uint64_t *)B.mx, B.mxs, hipcub::Max(), (int)B.n_rec, st));
		hipLaunchKernelGGL(bai_head_kernel, dim3(B.n_rec / 256 + 1), dim3(256), 0, st, (const uint64_t *)B.rb, B.n_rec, B.head);
		HIP_OK(hipGetLastError());
		HIP_OK(hipcub::DeviceSelect::Flagged(B.tmp, tb, Iota(0), (const uint8_t *)B.head, B.rs, B.n_sel, (int)B.n_rec, st));
	} else
		HIP_OK(hipMemsetAsync(B.n_sel, 0, sizeof(uint32_t), st));
	HIP_OK(hipcub::DeviceScan::ExclusiveSum(B.tmp, tb, (const uint32_t *)B.map, B.maps, (int)B.n_rec + 1, st));
	hipLaunchKernelGGL(bai_contig_kernel, dim3((uint32_t)B.n_ref / 256 + 1), dim3(256), 0, st, (const uint64_t *)B.mxs, (const uint32_t *)B.maps, (const uint64_t *)B.v0,
	                   B.n_rec, B.n_ref, B.end_v, B.stat, B.n_intv);
	HIP_OK(hipGetLastError());
	HIP_OK(hipcub::DeviceScan::ExclusiveSum(B.tmp, tb, (const uint32_t *)B.n_intv, B.woff, (int)B.n_ref + 1, st));
}

void launch_bam_index_runs(void *stream, const BamIndexBufs &B, uint32_t n_runs, uint32_t n_win)
{
	hipStream_t st = (hipStream_t)stream;
	size_t tb = B.tmp_bytes;
	if (n_runs) {
		const unsigned grid = (n_runs + 255) / 256;
		hipLaunchKernelGGL(bai_run_key_kernel, dim3(grid), dim3(256), 0, st, (const uint64_t *)B.rb, (const uint32_t *)B.rs, n_runs, B.n_rec, B.rk, B.ri);
		HIP_OK(hipGetLastError());
		HIP_OK(hipcub::DeviceRadixSort::SortPairs(B.tmp, tb, (const uint64_t *)B.rk, B.rk2, (const uint32_t *)B.ri, B.ri2, (int)n_runs, 0,
		                                          (int)bidx::run_key_bits(B.n_ref), st));
		hipLaunchKernelGGL(bai_run_chunk_kernel, dim3(grid), dim3(256), 0, st, (const uint32_t *)B.ri2, (const uint32_t *)B.rs, (const uint64_t *)B.v0, n_runs, B.n_rec,
		                   B.end_v, B.rbeg, B.rend);
		HIP_OK(hipGetLastError());
	}
	if (n_win) {
		hipLaunchKernelGGL(bai_window_kernel, dim3((n_win + 255) / 256), dim3(256), 0, st, (const uint32_t *)B.woff, B.n_ref, n_win, (const uint64_t *)B.mxs,
		                   (const uint32_t *)B.beg, (const uint64_t *)B.v0, B.n_rec, B.io);
		HIP_OK(hipGetLastError());
	}
}

} // namespace mbw
