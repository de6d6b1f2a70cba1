// k_bf_train.hip — translation unit of BruteForceRabitqIndex::train on the GPU (rbq_bf_train_device, reference
// src/brute_force.rs:214-285): the flat-output instantiations of k_encode (encode_vec.hpp) and the packer of the crate's
// ex_code_packed.  Rotation and the per-vector rescale factor are k_build.hip's k_rotate_rows and k_rescale.hip's k_rescale,
// reached through their launchers.  gfx950 only.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "encode_vec.hpp"

namespace rbq {

// raw ex codes [row][D] u8 (k_encode's pass B) -> ex_code_packed [row][D * EX / 8], the layout pack_ex2 / pack_ex6 of
// rbq_build.cpp write and bf_ex_code<EX> (bf.hpp) reads.  One lane per 16-dimension unit: unit u of the chunk is bytes
// [16 u, 16 u + 16) of the raw codes and bytes [4 u, 4 u + 4) (2-bit) or [12 u, 12 u + 12) (6-bit) of the packed ones, across
// row boundaries too (D % 16 == 0), so the D / 16 lanes of a vector — and the vectors of a wave — read and write one
// contiguous run.
//   2-bit: word = OR over g, i of (c[4g + i] & 3) << (8i + 2g)
//   6-bit: 8-byte word, byte i = (c[i] & 15) | (c[8 + i] & 15) << 4; then the 2-bit word of c >> 4
// The four dwords of a raw unit hold c[4g + i] in byte i of dword g, so every field moves as four bytes at once.
template <int EX>
__global__ __launch_bounds__(256) void k_bf_pack_ex(const uint4* __restrict__ raw, uint64_t nunits, uint32_t* __restrict__ out) {
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= nunits) return;
    const uint4 x = raw[u];
    const uint32_t sh = EX == 6 ? 4u : 0u; // where the top two bits of a code sit
    const uint32_t top = ((x.x >> sh) & 0x03030303u) | (((x.y >> sh) & 0x03030303u) << 2) | (((x.z >> sh) & 0x03030303u) << 4) |
                         (((x.w >> sh) & 0x03030303u) << 6);
    if (EX == 2) {
        out[u] = top;
    } else {
        uint32_t* o = out + 3 * u;
        o[0] = (x.x & 0x0f0f0f0fu) | ((x.z & 0x0f0f0f0fu) << 4);
        o[1] = (x.y & 0x0f0f0f0fu) | ((x.w & 0x0f0f0f0fu) << 4);
        o[2] = top;
    }
}

hipError_t launch_bf_encode(const EncodeParams& P, hipStream_t s) {
    if (!P.nslots) return hipSuccess;
    const dim3 grid((P.nslots + kEncThreads - 1) / kEncThreads);
    if (P.t_row) hipLaunchKernelGGL((k_encode<false, true, true>), grid, dim3(kEncThreads), 0, s, P);
    else hipLaunchKernelGGL((k_encode<false, false, true>), grid, dim3(kEncThreads), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_bf_pack_ex(const uint8_t* raw, uint64_t nrows, uint32_t D, uint32_t ex_bits, uint8_t* ex, hipStream_t s) {
    const uint64_t nunits = nrows * (D / 16);
    if (!nunits) return hipSuccess;
    if (ex_bits != 2 && ex_bits != 6) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((nunits + 255) / 256));
    if (ex_bits == 6) hipLaunchKernelGGL(k_bf_pack_ex<6>, grid, dim3(256), 0, s, (const uint4*)raw, nunits, (uint32_t*)ex);
    else hipLaunchKernelGGL(k_bf_pack_ex<2>, grid, dim3(256), 0, s, (const uint4*)raw, nunits, (uint32_t*)ex);
    return hipGetLastError();
}

} // namespace rbq
