// rbq_scan_limits.hpp — the limits and the LDS arithmetic of the scan that BOTH sides read: the kernels (through device/types.hpp,
// which includes this file) and the host's routing plan (rbq_search_plan.hpp, which the CPU tests build without HIP).  One
// definition of each; plain C++ — under hipcc the functions are __host__ __device__, under a host compiler plain inline.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RBQ_HOST_DEVICE __host__ __device__
#else
#define RBQ_HOST_DEVICE
#endif

namespace rbq {

#ifndef RBQ_NSCAN
#define RBQ_NSCAN 3         // scanner waves per workgroup (3 + replay wave = 256 threads: 4 workgroups per CU)
#endif
#ifndef RBQ_FILL_K
#define RBQ_FILL_K 2
#endif
constexpr int kNScan = RBQ_NSCAN;
constexpr int kScanThreads = (kNScan + 1) * 64; // scanner waves + 1 replay wave
constexpr int kTileBlocks = 2 * kNScan;         // 32-vector blocks per tile (one per scanner half-wave)
constexpr int kTileCand = kTileBlocks * 32;     // candidates per tile
constexpr int kFillK = RBQ_FILL_K;                 // stream entries per scanner lane and fill step
constexpr int kWindow = kNScan * 64 * kFillK;      // largest fill window
constexpr int kQueueCap = kTileBlocks - 1 + kWindow <= 512 ? 512 : 1024; // live-block FIFO (>= kTileBlocks - 1 + kWindow)

constexpr uint32_t kTopKRegMax = 256;             // largest top_k that lives in the replay wave's registers
constexpr uint32_t kNprobeMax = 8192;             // largest nprobe of the MFMA-shortlist selector (2 x nprobe u64 keys in LDS); above it the
                                                  // exact all-pairs ranking with its key window in global memory serves the call
constexpr uint32_t kTopKMax = 16384;              // largest top_k whose exact heap (top_k + 1 entries) fits the LDS; above it the heap of
                                                  // each query lives in global memory (ScanParams::heap_ws)
constexpr uint32_t kTopKHardMax = 1u << 20;       // largest top_k at all
constexpr size_t kLdsPerWorkgroupMax = 160 * 1024; // LDS of one compute unit (gfx950)

// Device layout of the ex codes ("lane-major"): per vector 16 lanes x W4 units of 16 B, stored [unit][lane][16 B].
// Lane l holds the codes of dims 16t+l (t = 0..D/16-1); unit j packs codes t = j*CPU .. j*CPU+CPU-1 as a
// little-endian 128-bit string, ex bits each, with no code straddling two units (CPU = 128/ex: 21 for 6-bit,
// 64 for 2-bit).  Unused code slots are zero.
RBQ_HOST_DEVICE constexpr uint32_t ex_cpu(uint32_t ex_bits) { return ex_bits ? 128u / ex_bits : 1u; }
RBQ_HOST_DEVICE constexpr uint32_t ex_w4(uint32_t D, uint32_t ex_bits) { // 16-byte units per lane
    return ex_bits ? (D / 16 + ex_cpu(ex_bits) - 1) / ex_cpu(ex_bits) : 0u;
}
RBQ_HOST_DEVICE inline uint32_t ex_bytes_dev(uint32_t D, uint32_t ex_bits) { return ex_w4(D, ex_bits) * 256u; }
// length of the zero-padded rotated query in LDS: every code slot of every unit has a (zero) partner
RBQ_HOST_DEVICE inline uint32_t ex_qlen(uint32_t D, uint32_t ex_bits) {
    const uint32_t n = ex_w4(D, ex_bits) * ex_cpu(ex_bits) * 16u;
    return n > D ? n : D;
}
// LDS carve-up of k_scan (dynamic only, LUT at byte 0):
//   lut[4Dc] u8 | qrot[D] f32 | heap_d[k+1] f32 | heap_s[k+1] u32 | q_slot,q_lb,q_ip,q_gadd,q_d [2][kTileCand] |
//   list[kTileCand] u32 | mask[2][kTileBlocks] u32 | queue[kQueueCap] WorkItem | fmask[kNScan] u64 |
//   T, len, nskip, nbatch | batch[kScanThreads/16] u32
// (heap_in_lds = false: the heap lives in global memory, ScanParams::heap_ws)
// nb = scan_nb(DT) of the instantiation that will run
RBQ_HOST_DEVICE inline size_t scan_lds_bytes(uint32_t Dc, uint32_t D, uint32_t ex_bits, uint32_t top_k, bool heap_in_lds = true, int nb = 1) {
    return (size_t)Dc * 4 + (size_t)ex_qlen(D, ex_bits) * 4 + (heap_in_lds ? (size_t)(top_k + 1) * 8 : (size_t)0) + (size_t)nb * kTileCand * 2 * 20 +
           (size_t)nb * kTileCand * 4 + 2 * (size_t)nb * kTileBlocks * 4 + kQueueCap * 8 + kNScan * kFillK * 8 + 32 + (kScanThreads / 16) * 8;
}

} // namespace rbq
