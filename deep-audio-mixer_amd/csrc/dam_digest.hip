// dam_digest.hip -- order-independent 64-bit digest of a device buffer's bit patterns.
//
// The data-parallel ModelTrainer (model_trainer.py) digests the flat parameter buffer of every replica after each training
// epoch and compares the digests over the process group: one read of the buffer and one 16-byte collective instead of an
// all-gather of 12.6 MB.  The reference is single-device and has no such check.
//
// Element i (index_base + i in the digest's index space) with 32-bit pattern b contributes
//     mix64(b + idx * GOLDEN)            (mix64 = splitmix64's finaliser, a bijection of uint64)
// and the contributions are ADDED modulo 2^64.  Addition with wrap-around is associative and commutative, so the result does
// not depend on the launch geometry or on the order in which blocks finish, and a buffer digested in pieces (each with its
// index_base, accumulate=1) gives the same value as in one launch.  Changing any bit of one element changes exactly one term,
// hence the sum.  Bit patterns are hashed as they are: NaN payloads, -0.0 and denormals are distinct values.
#include "dam_common.h"

namespace dam {
namespace {

constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr int DIGEST_THREADS = 256;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

__global__ __launch_bounds__(DIGEST_THREADS) void digest64_kernel(const uint32_t* __restrict__ x, int64_t n, uint64_t base,
                                                                  unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[DIGEST_THREADS];
    uint64_t acc = 0;
    for (int64_t i = blockIdx.x * (int64_t)DIGEST_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * DIGEST_THREADS)
        acc += mix64((uint64_t)x[i] + ((uint64_t)i + base) * GOLDEN);
    part[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int s = DIGEST_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    // one 64-bit global atomic per block (a vector-memory instruction): blocks may finish in any order
    if (threadIdx.x == 0) atomicAdd(out, part[0]);
}

}  // namespace
}  // namespace dam

extern "C" int dam_digest64_u32(const uint32_t* x, int64_t n, int64_t index_base, int max_blocks, int accumulate,
                                uint64_t* out, void* stream) {
    using namespace dam;
    if (!out || n < 0 || index_base < 0 || max_blocks < 0 || (n > 0 && !x)) return DAM_ERR_BAD_ARG;
    if ((uintptr_t)out & 7) return DAM_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (!accumulate && hipMemsetAsync(out, 0, sizeof(uint64_t), st) != hipSuccess) return DAM_ERR_LAUNCH;
    if (n == 0) return DAM_OK;
    int64_t blocks = cdiv(n, DIGEST_THREADS);
    const int64_t cap = max_blocks > 0 ? max_blocks : 4 * (int64_t)device_cus();
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(digest64_kernel, dim3((unsigned)blocks), dim3(DIGEST_THREADS), 0, st, x, n, (uint64_t)index_base,
                       (unsigned long long*)out);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}
