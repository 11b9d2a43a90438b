/*
 * rb3gpu_kount.hip -- the exclusive scan of the kept-children counts of a kount frontier (rocPRIM; kept out of rb3gpu.hip,
 * whose kernels and driver are in rb3gpu_kount.h and rb3gpu_kount there).
 */
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <stdint.h>

/* off[q] = cnt[0] + ... + cnt[q - 1] for q < n.  tmp NULL: *tmp_bytes = the scratch a scan of n entries needs */
extern "C" int rb3kount_scan(void *tmp, size_t *tmp_bytes, const uint32_t *cnt, int64_t *off, int64_t n, hipStream_t st)
{
	const hipError_t e = rocprim::exclusive_scan(tmp, *tmp_bytes, cnt, off, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), st);
	if (e != hipSuccess) { (void)hipGetLastError(); return e == hipErrorOutOfMemory ? -2 : -1; }
	return 0;
}
