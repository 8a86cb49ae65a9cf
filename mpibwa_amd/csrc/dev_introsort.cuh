// dev_introsort.cuh — ks_introsort (src/ksort.h:176-226) for the device, statement by statement, over an ORDER array: o[0, n) holds element
// numbers, lt(x, y) compares two of them.  The reference's sort is unstable and its order of equal keys is visible in the output, so the
// sequence of comparisons and swaps is the reference's: median-of-three quicksort with an explicit stack, ranges of <= 16 left to one final
// insertion sort, comb sort when the depth budget 2 * ceil(log2 n) runs out (sortutil.h is the host's statement of the same, ck_introsort
// in chain_kernel.hip the one over a StoreLds).  One lane runs it.  The frame stack is the caller's (3 * DSORT_FRAMES ints, in LDS: an
// indexed array of the function's own would live in scratch): only ranges of more than 16 elements are pushed and the smaller side is
// worked first, so a frame is at most half the range it was cut from and n <= 2^DSORT_FRAMES * 16 elements never need more.
#ifndef MBW_DEV_INTROSORT_CUH
#define MBW_DEV_INTROSORT_CUH
#include <hip/hip_runtime.h>

namespace mbw {

#define DSORT_FRAMES 16

template <class T, class LT>
__device__ __forceinline__ void dsort_insertion(T *o, int s, int t, LT lt)   // [s, t)
{
	for (int i = s + 1; i < t; ++i)
		for (int j = i; j > s && lt(o[j], o[j - 1]); --j) { const T x = o[j]; o[j] = o[j - 1]; o[j - 1] = x; }
}
template <class T, class LT>
__device__ __forceinline__ void dsort_comb(T *o, int a, int n, LT lt)
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
			if (lt(o[j], o[i])) { const T x = o[i]; o[i] = o[j]; o[j] = x; swapped = true; }
		}
	} while (swapped || gap > 2);
	if (gap != 1) dsort_insertion(o, a, a + n, lt);
}
template <class T, class LT>
__device__ __forceinline__ void dev_introsort(T *o, int n, int *stk, LT lt)
{
	if (n < 2) return;
	if (n == 2) {
		if (lt(o[1], o[0])) { const T x = o[0]; o[0] = o[1]; o[1] = x; }
		return;
	}
	int d = 2;
	while ((1 << d) < n) ++d;
	int *fs = stk, *ft = stk + DSORT_FRAMES, *fd = stk + 2 * DSORT_FRAMES, sp = 0;
	int s = 0, t = n - 1;
	d <<= 1;
	for (;;) {
		if (s < t) {
			if (--d == 0) {
				dsort_comb(o, s, t - s + 1, lt);
				t = s;
				continue;
			}
			int i = s, j = t, k = i + ((j - i) >> 1) + 1;
			if (lt(o[k], o[i])) { if (lt(o[k], o[j])) k = j; }
			else k = lt(o[j], o[i]) ? i : j;
			const T pivot = o[k];
			if (k != t) { const T x = o[k]; o[k] = o[t]; o[t] = x; }
			for (;;) {
				do ++i; while (lt(o[i], pivot));
				do --j; while (i <= j && lt(pivot, o[j]));
				if (j <= i) break;
				const T x = o[i]; o[i] = o[j]; o[j] = x;
			}
			{ const T x = o[i]; o[i] = o[t]; o[t] = x; }
			if (i - s > t - i) {
				if (i - s > 16) { fs[sp] = s; ft[sp] = i - 1; fd[sp] = d; ++sp; }
				s = t - i > 16 ? i + 1 : t;
			} else {
				if (t - i > 16) { fs[sp] = i + 1; ft[sp] = t; fd[sp] = d; ++sp; }
				t = i - s > 16 ? i - 1 : s;
			}
		} else {
			if (sp == 0) { dsort_insertion(o, 0, n, lt); return; }
			--sp;
			s = fs[sp]; t = ft[sp]; d = fd[sp];
		}
	}
}

} // namespace mbw
#endif
