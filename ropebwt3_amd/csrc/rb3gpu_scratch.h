/*
 * rb3gpu_scratch.h -- the owner of what one call of a query driver allocates (host only): device buffers, page-locked host
 * buffers and events, given back when the owner goes, by whichever return the call leaves.  What outlives a call is not
 * for it: that is the handle's (dev_malloc, buf_ensure in rb3gpu.hip).  It synchronises nothing: a buffer that may be in
 * use is waited for by the caller before it is regrown.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>

struct Scratch {
	std::vector<void*> dv, hv; // device buffers, page-locked host buffers
	std::vector<hipEvent_t> ev;
	Scratch() = default;
	Scratch(const Scratch&) = delete;
	Scratch &operator=(const Scratch&) = delete;
	~Scratch()
	{
		for (void *p : dv) (void)hipFree(p);
		for (void *p : hv) (void)hipHostFree(p);
		for (hipEvent_t e : ev) (void)hipEventDestroy(e);
	}
	template<class T> hipError_t dev(T **p, size_t bytes)
	{
		const hipError_t e = hipMalloc((void**)p, bytes);
		if (e == hipSuccess) dv.push_back((void*)*p);
		return e;
	}
	template<class T> hipError_t pinned(T **p, size_t bytes)
	{
		const hipError_t e = hipHostMalloc((void**)p, bytes, hipHostMallocDefault);
		if (e == hipSuccess) hv.push_back((void*)*p);
		return e;
	}
	hipError_t event(hipEvent_t *e)
	{
		const hipError_t r = hipEventCreate(e);
		if (r == hipSuccess) ev.push_back(*e);
		return r;
	}
	static void forget(std::vector<void*> &v, void *p) { v.erase(std::remove(v.begin(), v.end(), p), v.end()); }
	/* a device buffer and its page-locked twin on the host, both of `bytes` bytes, in place of the ones there are (either
	 * of d and h may be null: that side is left out) */
	template<class D, class H> hipError_t regrow(D **d, H **h, size_t bytes)
	{
		hipError_t e = hipSuccess;
		if (d && *d) {
			forget(dv, (void*)*d);
			e = hipFree((void*)*d), *d = nullptr;
		}
		if (e == hipSuccess && h && *h) {
			forget(hv, (void*)*h);
			e = hipHostFree((void*)*h), *h = nullptr;
		}
		if (e == hipSuccess && d) e = dev(d, bytes);
		if (e == hipSuccess && h) e = pinned(h, bytes);
		return e;
	}
};
