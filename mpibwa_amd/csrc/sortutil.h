// sortutil.h — the reference's sort is UNSTABLE and its tie order is visible in the SAM output (chains, regions, pair tables), so the
// exact comparison / swap sequence of ks_introsort (src/ksort.h:176-226) is restated here, ONCE, for the host and for every kernel:
// median-of-3 quicksort with an explicit stack, ranges of <= 16 left for a final insertion sort, comb sort of the range in hand when
// the depth budget 2 * ceil(log2 n) runs out.
//
// The functions are written over an ACCESSOR: at(i) returns a reference to element i (a T* on the host, an order array in LDS or in
// registers, a strided byte column of a lane's LDS on the device), lt(x, y) compares two element VALUES, indices are int.
//   ks_introsort_at        the sort, any n
//   ks_small_introsort_at  the sort for n <= 16, where it is one partition of the whole range and the insertion sort: no sub-range is
//                          long enough to be pushed, the depth budget (>= 4) cannot run out — no frame stack, no comb sort
//   ks_introsort           the host's form over a T*
// The frame stack is the caller's, three separate arrays handed over as three pointers (KsFramesAt, by value): a kernel keeps private
// arrays in registers that way, or puts them in LDS; one array or a struct of arrays by reference sends private frames to scratch.
// Only ranges of more than 16 elements are pushed and the smaller side is worked first, so with k frames on the stack the range in hand
// is at most n / 2^k elements and must be 18 or more for another push: n <= 16 << FRAMES never needs more than FRAMES frames.  Every
// device call site asserts that inequality against its largest n.
// Plain C++ for the host compilers (no HIP header); __host__ __device__ in a HIP translation unit.
#ifndef MBW_SORTUTIL_H
#define MBW_SORTUTIL_H
#include <cassert>
#include <climits>
#include <cstddef>

#ifdef __HIP__
#include <hip/hip_runtime.h>
#define KS_FN __host__ __device__ __forceinline__
#else
#define KS_FN inline
#endif

namespace mbw {

struct KsFramesAt { int *s, *t, *d; };   // left end, right end, depth budget of every pushed range

template <class At>
KS_FN void ks_swap_at(At at, int i, int j)
{
	const auto x = at(i);
	at(i) = at(j);
	at(j) = x;
}

template <class At, class Less>
KS_FN void ks_insertion_at(At at, int s, int t, Less lt)   // [s, t)
{
	for (int i = s + 1; i < t; ++i)
		for (int j = i; j > s && lt(at(j), at(j - 1)); --j) ks_swap_at(at, j, j - 1);
}

template <class At, class Less>
KS_FN void ks_comb_at(At at, int a, int n, Less lt)   // [a, a + n)
{
	const double shrink = 1.2473309501039786540366528676643;
	int gap = n;
	bool swapped;
	do {
		if (gap > 2) {
			gap = (int)((double)gap / shrink);
			if (gap == 9 || gap == 10) gap = 11;
		}
		swapped = false;
		for (int i = a; i < a + n - gap; ++i) {
			const int j = i + gap;
			if (lt(at(j), at(i))) { ks_swap_at(at, i, j); swapped = true; }
		}
	} while (swapped || gap > 2);
	if (gap != 1) ks_insertion_at(at, a, a + n, lt);
}

// one partition of [s, t], s < t: the median of the first, the middle and the last element goes to t as the pivot -> its final place
template <class At, class Less>
KS_FN int ks_partition_at(At at, int s, int t, Less lt)
{
	int i = s, j = t, k = i + ((j - i) >> 1) + 1;
	if (lt(at(k), at(i))) {
		if (lt(at(k), at(j))) k = j;
	} else k = lt(at(j), at(i)) ? i : j;
	const auto pivot = at(k);
	if (k != t) ks_swap_at(at, k, t);
	for (;;) {
		do ++i; while (lt(at(i), pivot));
		do --j; while (i <= j && lt(pivot, at(j)));
		if (j <= i) break;
		ks_swap_at(at, i, j);
	}
	ks_swap_at(at, i, t);
	return i;
}

template <class At, class Less>
KS_FN void ks_introsort_at(int n, At at, KsFramesAt f, Less lt)
{
	if (n < 2) return;
	if (n == 2) {
		if (lt(at(1), at(0))) ks_swap_at(at, 0, 1);
		return;
	}
	int d = 2;
	while ((1 << d) < n) ++d;
	int s = 0, t = n - 1, sp = 0;
	d <<= 1;
	for (;;) {
		if (s < t) {
			if (--d == 0) {
				ks_comb_at(at, s, t - s + 1, lt);
				t = s;
				continue;
			}
			const int i = ks_partition_at(at, s, t, lt);
			if (i - s > t - i) {
				if (i - s > 16) { f.s[sp] = s; f.t[sp] = i - 1; f.d[sp] = d; ++sp; }
				s = t - i > 16 ? i + 1 : t;
			} else {
				if (t - i > 16) { f.s[sp] = i + 1; f.t[sp] = t; f.d[sp] = d; ++sp; }
				t = i - s > 16 ? i - 1 : s;
			}
		} else {
			if (sp == 0) {
				ks_insertion_at(at, 0, n, lt);
				return;
			}
			--sp;
			s = f.s[sp]; t = f.t[sp]; d = f.d[sp];
		}
	}
}

template <class At, class Less>
KS_FN void ks_small_introsort_at(int n, At at, Less lt)   // n <= 16
{
	if (n < 2) return;
	if (n == 2) {
		if (lt(at(1), at(0))) ks_swap_at(at, 0, 1);
		return;
	}
	ks_partition_at(at, 0, n - 1, lt);
	ks_insertion_at(at, 0, n, lt);
}

// the host's form (the reference mallocs a stack of 8 d + 2 frames; 64 cover any int n — no heap traffic per sort).  Indices are int:
// n <= INT_MAX, which every list of the alignment path is by orders of magnitude
template <class T, class Less>
inline void ks_introsort(size_t n, T *a, Less lt)
{
	assert(n <= (size_t)INT_MAX);
	int fs[64], ft[64], fd[64];
	ks_introsort_at((int)n, [a](int i) -> T & { return a[i]; }, KsFramesAt{fs, ft, fd}, lt);
}

} // namespace mbw
#endif
