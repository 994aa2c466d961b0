// history_pack.hip -- the slots of a recorded ladder packed into the history's prefix layout.
//
// A ladder's samples are written by whichever workgroup held ladder level 0 in the round, each into a
// slot of S cells at a place that depends on the round alone (chain_dev.h RecDesc): sample i of the call
// at cell slot0 + i S of every component array, n_i = ncells[base + i] <= S of them used.  After the
// launch this kernel moves sample i left by i S - (n_0 + ... + n_{i-1}), onto the end of sample i - 1,
// and writes the offsets off[base + 1 .. base + count]: the layout every td_history_* consumer reads.
//   The moves overlap -- a destination may cover the (already moved) slots of several earlier samples
// and the head of its own source -- so their order is the design: one workgroup per component array (the
// four are independent), samples ascending, chunks of kPackChunk cells ascending, each chunk loaded into
// registers by the whole block, a barrier, then stored, a barrier.  A chunk's destination ends at or
// before its own source's end (every move is to the left), so it covers only cells that were read
// before: earlier chunks, earlier samples.  A sample already in place (no gap before it) is skipped.
#include <hip/hip_runtime.h>

#include "history.h"

namespace tdstar {

namespace {

constexpr int kPackThreads = 256;
constexpr int kPackU = 4;  // cells per thread per chunk
static_assert(kPackChunk == kPackThreads * kPackU, "history.h names the chunk for the tests");

__global__ __launch_bounds__(kPackThreads) void k_history_pack(double *__restrict__ cells, long long stride,
                                                                long long slot0, long long S,
                                                                const int *__restrict__ ncells, long long count,
                                                                long long *__restrict__ off) {
    double *a = cells + (long long)blockIdx.x * stride;  // this workgroup's component
    const int tid = threadIdx.x;
    long long dst = slot0;  // where the next sample goes: the running prefix (the same in every thread)
    for (long long i = 0; i < count; ++i) {
        const long long n = ncells[i], src = slot0 + i * S;
        if (dst != src) {
            for (long long c = 0; c < n; c += kPackChunk) {
                double v[kPackU];
#pragma unroll
                for (int u = 0; u < kPackU; ++u) {
                    const long long j = c + tid + u * kPackThreads;
                    v[u] = j < n ? a[src + j] : 0.0;
                }
                __syncthreads();  // the chunk is read
#pragma unroll
                for (int u = 0; u < kPackU; ++u) {
                    const long long j = c + tid + u * kPackThreads;
                    if (j < n) a[dst + j] = v[u];
                }
                __syncthreads();  // and written, before the next chunk's reads
            }
        }
        dst += n;
        if (blockIdx.x == 0 && tid == 0) off[i + 1] = dst;
    }
}

}  // namespace

hipError_t launch_history_pack(double *cells, long long stride, long long slot0, long long S, const int *ncells,
                               long long count, long long *off, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_history_pack, dim3(4), dim3(kPackThreads), 0, s, cells, stride, slot0, S, ncells, count,
                       off);
    return hipGetLastError();
}

}  // namespace tdstar
