// salt_amd/csrc/salt_inflate.hip -- BGZF members in device memory -> their text in device memory (blocked-gzip FASTQ input,
// salt_gpu_ws_inflate_bgzf / salt_gpu_bgzf_inflate).
//
//   k_bgzf_inflate  one workgroup per member: the member's bytes and its text both in LDS, one lane decodes, all lanes stage, check the
//                   CRC-32 and copy out (salt_inflate_block.h).  138 KiB of LDS: one member per CU at a time; a launch of more members than
//                   CUs runs them in waves of 256, which is why a 32-MiB chunk (about 520 members) is two to three members deep per CU.
// A member's text goes to its own range of the output and nowhere else; a bad member leaves its range untouched and a reason in status[].
#include <hip/hip_runtime.h>
#include "salt_kernels.h"
#include "salt_inflate_block.h"

namespace salt {

using namespace bgzf;

__global__ __launch_bounds__(INFL_THREADS) void k_bgzf_inflate(const uint8_t *members, const unsigned long long *c_off, const unsigned long long *u_off,
                                                                uint8_t *text, uint32_t *status)
{
    __shared__ InflateLds s;
    const unsigned long long c0 = c_off[blockIdx.x], c1 = c_off[blockIdx.x + 1], u0 = u_off[blockIdx.x], u1 = u_off[blockIdx.x + 1];
    // sizes that are no member's (offsets out of order included) become 0xFFFFFFFF: inflate_block refuses them before it reads a byte
    const uint32_t csize = c1 >= c0 && c1 - c0 <= INFL_MAX ? (uint32_t)(c1 - c0) : 0xFFFFFFFFu;
    const uint32_t usize = u1 >= u0 && u1 - u0 <= INFL_MAX ? (uint32_t)(u1 - u0) : 0xFFFFFFFFu;
    inflate_block(s, members + c0, csize, text + u0, usize, status + blockIdx.x, threadIdx.x);
}

hipError_t launch_bgzf_inflate(const uint8_t *members, const unsigned long long *c_off, const unsigned long long *u_off, uint32_t n_blocks,
                               uint8_t *text, uint32_t *status, hipStream_t st)
{
    if (n_blocks == 0) return hipSuccess;
    if (n_blocks > 0x7FFFFFFFu) return hipErrorInvalidValue;
    k_bgzf_inflate<<<n_blocks, INFL_THREADS, 0, st>>>(members, c_off, u_off, text, status);
    return hipGetLastError();
}

} // namespace salt
