/*
 * rb3gpu_kount.hip -- the exclusive scan of the kept-children counts of a kount frontier (rocPRIM; kept out of rb3gpu.hip,
 * whose kernels and driver are in rb3gpu_kount.h and rb3gpu_kount there), which the other query drivers share, and the sort of the pieces of
 * rb3gpu_retrieve_pieces.
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

/* (kout, vout) = the n pairs (kin, vin) by ascending key, bits [0, end_bit) of it (the pieces of rb3gpu_retrieve_pieces by string and distance).  tmp NULL:
 * *tmp_bytes = the scratch a sort of n pairs needs */
extern "C" int rb3kount_sort_pairs(void *tmp, size_t *tmp_bytes, const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, int64_t n, int end_bit, hipStream_t st)
{
	const hipError_t e = rocprim::radix_sort_pairs(tmp, *tmp_bytes, kin, kout, vin, vout, (size_t)n, 0u, (unsigned int)end_bit, st);
	if (e != hipSuccess) { (void)hipGetLastError(); return e == hipErrorOutOfMemory ? -2 : -1; }
	return 0;
}
