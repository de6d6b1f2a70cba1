// bf_index.hpp — the brute-force handle (rbq_bf_index) and what the units that serve it share: api_bf.hip (create, train, RBF1,
// search) and api_bf_mutate.hip (append, remove, fetch).  Internal, like api.hpp.
#pragma once
#include "api.hpp"

#pragma GCC visibility push(hidden)

namespace rbq_api {
struct BfWorkspace { // what one search call holds: a stream and its buffers, from the handle's pool
    hipStream_t stream = nullptr;
    DevBuf q, rot, lut, consts, dist, heap_d, heap_s, heap_len, filter, ids, scores, counts, stats;
    BfWorkspace() = default;
    BfWorkspace(const BfWorkspace&) = delete;
    ~BfWorkspace() { if (stream) (void)hipStreamDestroy(stream); } // (deleted under the index's DeviceGuard)
};
} // namespace rbq_api

struct rbq_bf_index : rbq_api::Geometry {
    int device = 0;
    rbq_header hdr;                    // rotator_blob -> blob below
    std::vector<uint8_t> blob;         // host copy of the rotator (RBF1 writer)
    uint64_t ex_len = 0;               // bytes of ex code per vector as the index holds them (rbq_bf_view::ex_len)
    rbq_api::Arr rot_blob, bin, ex, f[8]; // f: delta, vl, f_add, f_rescale, f_error, residual_norm, f_add_ex, f_rescale_ex
    std::mutex mu;
    std::vector<rbq_api::BfWorkspace*> pool;
    std::atomic<uint64_t> pushes{0}, tie_pushes{0};
};

namespace rbq_api {
// api_bf.hip
void bf_free(rbq_bf_index* ix);
struct BfOwner { // frees a half-built index on an early return
    rbq_bf_index* ix;
    ~BfOwner() { if (ix) bf_free(ix); }
    rbq_bf_index* release() { rbq_bf_index* r = ix; ix = nullptr; return r; }
};
// A handle of n vectors with the header and rotator of `hdr` on device `dev` (the caller has switched to it): rot_blob uploaded,
// bin / ex / f allocated for n rows and not written; ex_len as given.
int bf_new_index(const rbq_header* hdr, uint64_t n, uint64_t ex_len, int dev, BfOwner& own);
// The encoder chain of BruteForceRabitqIndex::train over `count` rows of `data` ([count][dim] f32, host or device memory, detected),
// a chunk at a time: k_rotate_rows -> k_rescale (opt) -> k_encode's flat mode against the zero centroid -> k_bf_pack_ex, written
// into rows row0 .. row0 + count - 1 of ix's arrays.  rbq_bf_train_device (row0 = 0) and rbq_bf_append (row0 = the old length).
int bf_encode_rows(rbq_bf_index* ix, const float* data, uint64_t count, uint64_t row0, bool opt, float t_const, uint64_t max_chunk_rows);
} // namespace rbq_api

#pragma GCC visibility pop
