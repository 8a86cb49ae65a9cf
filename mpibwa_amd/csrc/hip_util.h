// hip_util.h — what the .hip files share on the host side: the error check, an event timer and an owning device array;
// on the device side the LDS hand-over inside a wave.
// (.hip files only: it pulls in the HIP runtime header)
#ifndef MBW_HIP_UTIL_H
#define MBW_HIP_UTIL_H
#include <hip/hip_runtime.h>
#include "internal.h"

#define HIP_OK(call)                                                                                                    \
	do {                                                                                                                \
		hipError_t e_ = (call);                                                                                         \
		if (e_ != hipSuccess) ::mbw::die("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);    \
	} while (0)

namespace mbw {

// What the lanes of a wave stored to LDS becomes visible to the wave's other lanes (a workgroup of one wave: no s_barrier)
__device__ __forceinline__ void wave_lds_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct Timer {
	hipEvent_t a, b;
	Timer() { HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b)); }
	~Timer() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
	void start(hipStream_t s) { HIP_OK(hipEventRecord(a, s)); }
	double stop(hipStream_t s)
	{
		HIP_OK(hipEventRecord(b, s));
		HIP_OK(hipEventSynchronize(b));
		float ms = 0;
		HIP_OK(hipEventElapsedTime(&ms, a, b));
		return ms;
	}
};

// A device array that lives as long as its scope (the stage entries; the pipeline's work buffers are DevBuf / PinBuf).  All sizes are in
// BYTES, whatever T: the callers' paddings are byte counts.  Blocking calls on the null stream, like the hipMalloc / hipMemcpy they wrap.
template <class T> struct DevArr {
	T *p = nullptr;
	size_t bytes = 0;
	DevArr() = default;
	// `bytes` of device memory, not initialised; host given: its first `copy` bytes (default: all of them) uploaded.  A null host
	// pointer or a copy of zero bytes uploads nothing.
	explicit DevArr(size_t bytes_, const void *host = nullptr, size_t copy = ~(size_t)0) : bytes(bytes_)
	{
		HIP_OK(hipMalloc(&p, bytes));
		if (copy > bytes) copy = bytes;
		if (host && copy) HIP_OK(hipMemcpy(p, host, copy, hipMemcpyHostToDevice));
	}
	DevArr(DevArr &&o) : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
	DevArr &operator=(DevArr &&o)
	{
		if (this != &o) { if (p) (void)hipFree(p); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
		return *this;
	}
	DevArr(const DevArr &) = delete;
	DevArr &operator=(const DevArr &) = delete;
	~DevArr() { if (p) (void)hipFree(p); }
	operator T *() const { return p; }
	void fill(int byte, size_t n) { HIP_OK(hipMemset(p, byte, n)); }   // the first n bytes
	void fill(int byte) { fill(byte, bytes); }
	void zero() { fill(0); }
	void download(void *host, size_t n) const { HIP_OK(hipMemcpy(host, p, n, hipMemcpyDeviceToHost)); }
};

} // namespace mbw
#endif
