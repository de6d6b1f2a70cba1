// topk.hpp — the top-k containers of the scan and brute-force kernels (gfx950, wave64) and the steps k_scan and k_scanw both take on
// them.  All of them reproduce the reference's BinaryHeap top-k (src/ivf.rs:904-931, :2116-2126) bit for bit:
//   LdsHeap                      Rust's std BinaryHeap on LDS (or global) arrays, one lane              (k_scan, k_scanw, k_bf_select)
//   HeapOps, RegHeap             the same heap in a wave's registers
//   RankRun, SortedRun           the tie-free fast path on the same registers: a sorted run
//   ParHeap, tie_log_replay      the heap with lane-parallel primitives; a tied query's replay of its log (k_scan)
//   replay_sorted, replay_heap   the reference's prune / push / pop loop over one refined batch (k_scan; k_scanw's own loop calls
//                                SortedRun::may_enter / ::offer)
//   lazy_tie_final               the final look of the lazy-tie rule (the rule and its proof: scanw.hpp, at `amb_min`)
//   run_distance_bits, spill_heap_sorted   a finished top-k -> ascending distances
#pragma once
#include "kernels.hpp"

namespace rbq {

// ---- Rust std BinaryHeap<HeapEntry> on LDS arrays (max-heap on total_cmp(distance)) -----------------------
struct LdsHeap {
    float* d;
    uint32_t* s;
    uint32_t len;
    __device__ __forceinline__ void sift_up(uint32_t pos, float ed, uint32_t es) {
        const int ke = total_key(ed);
        while (pos > 0) {
            const uint32_t parent = (pos - 1) >> 1;
            if (ke <= total_key(d[parent])) break;
            d[pos] = d[parent];
            s[pos] = s[parent];
            pos = parent;
        }
        d[pos] = ed;
        s[pos] = es;
    }
    __device__ __forceinline__ void push(float dist, uint32_t slot) { sift_up(len++, dist, slot); }
    __device__ __forceinline__ void pop() { // last -> root, sift_down_to_bottom(0), sift_up
        --len;
        if (len == 0) return;
        const float ed = d[len];
        const uint32_t es = s[len];
        const uint32_t end = len;
        uint32_t p = 0, child = 1;
        while (end >= 2 && child <= end - 2) {
            child += (total_key(d[child]) <= total_key(d[child + 1])) ? 1u : 0u;
            d[p] = d[child];
            s[p] = s[child];
            p = child;
            child = 2 * p + 1;
        }
        if (child == end - 1) {
            d[p] = d[child];
            s[p] = s[child];
            p = child;
        }
        sift_up(p, ed, es);
    }
    __device__ __forceinline__ void into_sorted() { // into_sorted_vec: swap(0,end); sift_down_range(0,end)
        uint32_t end = len;
        while (end > 1) {
            --end;
            const float ed = d[end];
            const uint32_t es = s[end];
            d[end] = d[0];
            s[end] = s[0];
            const int ke = total_key(ed);
            uint32_t p = 0, child = 1;
            bool placed = false;
            while (end >= 2 && child <= end - 2) {
                child += (total_key(d[child]) <= total_key(d[child + 1])) ? 1u : 0u;
                if (ke >= total_key(d[child])) { placed = true; break; }
                d[p] = d[child];
                s[p] = s[child];
                p = child;
                child = 2 * p + 1;
            }
            if (!placed && child == end - 1 && ke < total_key(d[child])) {
                d[p] = d[child];
                s[p] = s[child];
                p = child;
            }
            d[p] = ed;
            s[p] = es;
        }
    }
};

// ---- the same BinaryHeap held in the replay wave's registers ------------------------------------------------
// Entry i lives in lane i % 64 of register i / 64; TR registers hold 64*TR entries (the heap is one entry over top_k
// between a push and the pop that follows, so top_k <= 64*TR - 1: 63 with one register, 255 with four).
// All indices and values are wave-uniform, so every access is a v_readlane/v_writelane (a few cycles)
// instead of a dependent LDS round trip.  Register 0 is the pair (hd, hs); registers 1..TR-1 are elements of two
// vector values (element 0 unused) — vector elements with compile-time indices stay in VGPRs, a plain array ended up
// in scratch.  The sorted run (SortedRun below) is a second view of the same registers; only one is live at a time.
struct HeapOps {
    // every index is wave-uniform; readfirstlane makes that explicit so that hipcc emits a plain v_readlane instead of
    // a waterfall loop
    static __device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
    static __device__ __forceinline__ int key(int bits) { return bits ^ (int)(((uint32_t)(bits >> 31)) >> 1); }
};
template <int TR>
struct RegHeap : HeapOps {
    typedef int VI __attribute__((ext_vector_type(TR)));
    typedef uint32_t VU __attribute__((ext_vector_type(TR)));
    int hd;      // distance bits of entry `lane`
    uint32_t hs; // slot of entry `lane`
    VI xd;       // entries 64r + lane, r = 1..TR-1
    VU xs;
    uint32_t len;
    __device__ __forceinline__ int d_at(uint32_t i) const {
        const uint32_t r = uni(i >> 6);
        int v = hd;
#pragma unroll
        for (int k = 1; k < TR; ++k) v = r == (uint32_t)k ? xd[k] : v;
        return __builtin_amdgcn_readlane(v, (int)uni(i & 63u));
    }
    __device__ __forceinline__ uint32_t s_at(uint32_t i) const {
        const uint32_t r = uni(i >> 6);
        uint32_t v = hs;
#pragma unroll
        for (int k = 1; k < TR; ++k) v = r == (uint32_t)k ? xs[k] : v;
        return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)uni(i & 63u));
    }
    __device__ __forceinline__ void set(uint32_t i, int d, uint32_t s) { // v_writelane as compare+select
        const uint32_t r = uni(i >> 6);
        const bool me = (__lane_id() == uni(i & 63u));
        const bool m0 = me && r == 0u;
        hd = m0 ? d : hd;
        hs = m0 ? s : hs;
#pragma unroll
        for (int k = 1; k < TR; ++k) {
            const bool mk = me && r == (uint32_t)k;
            xd[k] = mk ? d : xd[k];
            xs[k] = mk ? s : xs[k];
        }
    }
    __device__ __forceinline__ void sift_up(uint32_t pos, int ed, uint32_t es) {
        const int ke = key(ed);
        pos = uni(pos);
        while (pos > 0) {
            const uint32_t parent = uni((pos - 1) >> 1);
            const int pd = d_at(parent);
            if (ke <= key(pd)) break;
            set(pos, pd, s_at(parent));
            pos = parent;
        }
        set(pos, ed, es);
    }
    __device__ __forceinline__ void push(int dbits, uint32_t slot) {
        const uint32_t p = uni(len);
        len = p + 1;
        sift_up(p, dbits, slot);
    }
    __device__ __forceinline__ void pop() {
        len = uni(len - 1);
        if (len == 0) return;
        const int ed = d_at(len);
        const uint32_t es = s_at(len);
        const uint32_t end = len;
        uint32_t p = 0, child = 1;
        while (end >= 2 && child <= end - 2) {
            const int c0 = d_at(child), c1 = d_at(child + 1);
            const bool right = key(c0) <= key(c1);
            child = uni(child + (right ? 1u : 0u));
            set(p, right ? c1 : c0, s_at(child));
            p = child;
            child = uni(2 * p + 1);
        }
        if (child == end - 1) {
            set(p, d_at(child), s_at(child));
            p = child;
        }
        sift_up(p, ed, es);
    }
};

// ---- tie-free fast path of the same top-k --------------------------------------------------------------------
// As long as no two distances in the heap are bit-identical, the reference's result does not depend on the
// layout of its BinaryHeap: pop evicts THE maximum and into_sorted_vec has one possible order.  Any equality the
// fast path meets reports a tie; the query is then re-run from its first block with the exact BinaryHeap emulation
// (RegHeap while top_k < 64*TR, LdsHeap above).
//
// RankRun (TR > 1: 64 <= top_k <= 256, the reference's own benchmark setting is 100): the top-k is a SORTED RUN of
// KEYS (HeapOps::key of the distance bits: a signed-integer image of total_cmp, its own inverse) in the RegHeap's
// registers, entry i in lane i % 64 of register i / 64, empty lanes = kHigh.  A whole refine batch (up to 64 candidates
// in stream order, lane j = candidate j) is merged in ONE data-parallel step instead of one candidate after the other —
// at top_k = 100 most evaluated candidates enter the top-k, and a serial insertion per candidate (~700 cycles of
// dependent scalar/DPP work each on a SIMD shared with the refining waves) was two thirds of the kernel.
//
// The reference's loop over the batch is, with U_j = run + candidates accepted before j and t_j = k-th smallest of U_j
// (+inf while |U_j| < k):   skip j if lb_j >= t_j;  drop j if d_j is not finite;  accept j iff d_j < t_j (then the
// maximum leaves when |U| > k).  Its final top-k F is the k smallest of run + A (A = accepted candidates).
// Claim: F = F' := the k smallest of  run + C,  C = ALL finite candidates of the batch, provided every candidate o in F'
// with lb_o >= d_o ("odd": lower bound not below the refined distance) has lb_o < m' := max F'.
// Proof (|run + C| >= k; otherwise every threshold is +inf, nothing is skipped, rejected or evicted, and F = F' = all):
// U_j is a subset of run + C, so its k-th smallest is not below that of run + C:  t_j >= m'  for every j.  Take a
// candidate s in F': d_s <= m' <= t_s.  If s is not odd, lb_s < d_s <= t_s: the reference evaluates it; if it is odd,
// lb_s < m' <= t_s by the proviso: evaluated as well.  It then accepts s unless d_s == t_s — an equal key inside
// run + C, reported as a tie (below).  So F' is a subset of run + A, which is a subset of run + C; being the k smallest of
// the larger set, F' is also the k smallest of run + A, i.e. F.  No acceptance decision, no thresholds — one merge:
//     G(u) = #{elements of run + candidates above u}:  run entries: position from the top + #{candidates > u};
//     candidates: #{run entries > x} + #{candidates > x};  with E = max(0, |run| + |candidates| - k), u stays iff
//     G(u) >= E, and its new position from the top is G(u) - E.  One scatter through LDS.
// When the proviso fails (or diagnostics want the exact c_skip/c_ext/c_est, which need the thresholds themselves) the
// batch is decided by the serial simulation below and merged the same way.
// Ties (the reference's result then depends on the layout of its heap; any of these reports a tie): two candidates with
// equal keys get the same G and are scattered to the same position, which leaves another position unwritten (lds_k is
// pre-filled with kHigh); a candidate equal to a run key lands next to it (neighbour check after the reload); an element
// that leaves with the same key as the new maximum (checked against the old registers).  Equal keys that both leave do
// not matter to the reference either.
template <int TR>
struct RankRun {
    typedef RegHeap<TR> H;
    static constexpr int kHigh = 0x7fffffff; // key of a NaN pattern: never inserted (non-finite distances are dropped)
    static constexpr int kLow = (int)0x80000000;
    static __device__ __forceinline__ void clear(H& h) { h.hd = kHigh; h.hs = 0u; h.xd = kHigh; h.xs = 0u; h.len = 0u; }
    static __device__ __forceinline__ int wave_max(int m) {
        int t;
        t = __builtin_amdgcn_update_dpp(kLow, m, 0x111, 0xf, 0xf, false); m = t > m ? t : m;
        t = __builtin_amdgcn_update_dpp(kLow, m, 0x112, 0xf, 0xf, false); m = t > m ? t : m;
        t = __builtin_amdgcn_update_dpp(kLow, m, 0x114, 0xf, 0xf, false); m = t > m ? t : m;
        t = __builtin_amdgcn_update_dpp(kLow, m, 0x118, 0xf, 0xf, false); m = t > m ? t : m;
        t = __builtin_amdgcn_update_dpp(kLow, m, 0x142, 0xa, 0xf, false); m = t > m ? t : m;
        t = __builtin_amdgcn_update_dpp(kLow, m, 0x143, 0xc, 0xf, false); m = t > m ? t : m;
        return __builtin_amdgcn_readlane(m, 63);
    }
    // Merge the batch `mt` (lane j: lower-bound bits v_lb, refined distance bits v_d, slot v_s) into the run.  `serial`
    // forces the serial decision (exact c_skip/c_ext/c_est: diagnostics).  dk_bits <- bits of the k-th distance once the
    // run is full.  lds_k/lds_s: scratch for top_k entries.  Returns true if an equal key was met.
    // amb_min: LAZY TIES.  Equal keys do not end the fast path on the spot: they are ordered by a fixed rule (run
    // entries below candidates, candidates by lane) and merged like any others; what is recorded is the one thing that can make
    // the reference's RESULT depend on the layout of its heap later on — an element that LEAVES (or is turned away) with the key of
    // the maximum that stays: amb_min = the smallest such key.  See k_scanw's final check for why that, plus a look at the final
    // run for equal neighbours, decides exactly the queries that need the BinaryHeap emulation.
    // mst: cycle stamps of the three phases (k_scan's RBQ_STAMPS == 4 build only; unused and null otherwise).
#if RBQ_STAMPS == 4
#define MSTAMP(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); mst[i] += t_ - mst[3]; mst[3] = t_; } while (0)
#else
#define MSTAMP(i)
#endif
    static __device__ __forceinline__ bool merge_batch(H& h, uint32_t top_k, unsigned long long mt, int v_lb, int v_d, uint32_t v_s,
                                                       uint32_t lane, bool serial, int* lds_k, uint32_t* lds_s, uint32_t& c_skip,
                                                       uint32_t& c_ext, uint32_t& c_est, int& dk_bits, int& amb_min,
                                                       unsigned long long* mst = nullptr) {
#if RBQ_STAMPS == 4
        mst[3] = __builtin_amdgcn_s_memtime();
#endif
        const uint32_t len = HeapOps::uni(h.len);
        const bool taken = (mt >> lane) & 1ull;
        const bool fin = taken && ((v_d & 0x7f800000) != 0x7f800000);
        const int x = fin ? HeapOps::key(v_d) : kHigh;
        const unsigned long long finm = __ballot(fin);
        const bool odd = fin && !(__int_as_float(v_lb) < __int_as_float(v_d)); // lower bound not below the refined distance
        const unsigned long long oddm = __ballot(odd);
        // ---- one pass over the finite candidates i (s = its key): Q = #{candidates > own key} for run entries and
        //      candidates; the same compare, counted over the wave, is #{run entries < s} for lane i (empty lanes hold
        //      kHigh: never below s)
        int Q[TR];
#pragma unroll
        for (int r = 0; r < TR; ++r) Q[r] = 0;
        int QA = 0;
        uint32_t cB = 0;
        for (unsigned long long todo = finm; todo; todo &= todo - 1ull) {
            const uint32_t i = (uint32_t)__builtin_ctzll(todo);
            const int s = __builtin_amdgcn_readlane(x, (int)i);
            uint32_t cnt = 0;
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const int kr = r == 0 ? h.hd : h.xd[r];
                const bool gt = s >= kr; // (a candidate sits ABOVE the run entries of its key; empty lanes hold kHigh)
                Q[r] += gt ? 1 : 0;
                cnt += (uint32_t)__popcll(__ballot(gt));
            }
            QA += (s > x || (s == x && i > lane)) ? 1 : 0; // (equal candidates in lane order)
            cB = lane == i ? cnt : cB;
        }
        MSTAMP(0);
        bool tie = false;
        unsigned long long accm = finm; // candidates merged
        const uint32_t nfin = (uint32_t)__popcll(finm);
        if (!serial && oddm && len + nfin > top_k) {
            // the proviso: odd candidates that stay must have lb < t_end' = the element with exactly E elements above it
            const int E = (int)(len + nfin - top_k);
            int tkey = kHigh;
            bool found = false;
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const uint32_t idx = (uint32_t)r * 64u + lane;
                const unsigned long long mm = __ballot(idx < len && (int)len - 1 - (int)idx + Q[r] == E);
                if (mm) { tkey = __builtin_amdgcn_readlane(r == 0 ? h.hd : h.xd[r], __builtin_ctzll(mm)); found = true; }
            }
            {
                const unsigned long long mm = __ballot(fin && (int)len - (int)cB + QA == E);
                if (mm) { tkey = __builtin_amdgcn_readlane(x, __builtin_ctzll(mm)); found = true; }
            }
            const float tf = __int_as_float(HeapOps::key(tkey));
            serial = !found || __ballot(odd && (int)len - (int)cB + QA >= E && !(__int_as_float(v_lb) < tf)) != 0ull;
        }
        if (serial) { // the reference's loop itself, on the run's top entries and the accepted candidates still alive
            uint32_t p = 0, size = len; // p: run entries that left (from the top)
            unsigned long long alive = 0ull;
            accm = 0ull;
            for (unsigned long long todo = mt; todo; todo &= todo - 1ull) {
                const uint32_t j = (uint32_t)__builtin_ctzll(todo);
                const bool full = size == top_k;
                int tk = kHigh, bt = kLow, am = kLow;
                if (full) {
                    bt = p < len ? h.d_at(len - 1u - p) : kLow;
                    am = wave_max(((alive >> lane) & 1ull) ? x : kLow);
                    tk = bt > am ? bt : am;
                }
                const float tf = full ? __int_as_float(HeapOps::key(tk)) : INFINITY;
                const float lb = __int_as_float(__builtin_amdgcn_readlane(v_lb, (int)j));
                if (!(lb < tf)) { ++c_skip; continue; }
                ++c_ext;
                if (!((finm >> j) & 1ull)) continue;
                ++c_est;
                const int ke = __builtin_amdgcn_readlane(x, (int)j);
                if (full) {
                    if (ke > tk) continue;
                    if (ke == tk) { // turned away with the key of the maximum: which of the two the reference keeps depends on its heap
                        amb_min = amb_min < tk ? amb_min : tk;
                        continue;
                    }
                    if (bt >= am) ++p;
                    else alive &= ~(1ull << (uint32_t)__builtin_ctzll(__ballot(((alive >> lane) & 1ull) && x == am)));
                } else ++size;
                alive |= 1ull << j;
                accm |= 1ull << j;
            }
            // a candidate skipped by its lower bound may be smaller than elements that stay: count the accepted only
#pragma unroll
            for (int r = 0; r < TR; ++r) Q[r] = 0;
            QA = 0;
            for (unsigned long long todo = accm; todo; todo &= todo - 1ull) {
                const uint32_t i = (uint32_t)__builtin_ctzll(todo);
                const int s = __builtin_amdgcn_readlane(x, (int)i);
#pragma unroll
                for (int r = 0; r < TR; ++r) {
                    const int kr = r == 0 ? h.hd : h.xd[r];
                    Q[r] += s >= kr ? 1 : 0;
                }
                QA += (s > x || (s == x && i > lane)) ? 1 : 0;
            }
        }
        MSTAMP(1);
        // ---- merge: an element stays iff G = #{elements of run + merged candidates above it} >= E
        const uint32_t macc = (uint32_t)__popcll(accm);
        if (macc) {
            const uint32_t total = len + macc;
            const uint32_t evict = total > top_k ? total - top_k : 0u, nlen = total - evict;
#pragma unroll
            for (int r = 0; r < TR; ++r)
                if ((uint32_t)r * 64u + lane < nlen) lds_k[r * 64 + lane] = kHigh;
            int G[TR];
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const uint32_t idx = (uint32_t)r * 64u + lane;
                G[r] = idx < len ? (int)len - 1 - (int)idx + Q[r] : -1;
                if (G[r] >= (int)evict) {
                    const uint32_t pos = nlen - 1u - (uint32_t)(G[r] - (int)evict);
                    lds_k[pos] = r == 0 ? h.hd : h.xd[r];
                    lds_s[pos] = r == 0 ? h.hs : h.xs[r];
                }
            }
            // (a run entry equal to x counts as above it: the pair lands side by side)
            const int GA = ((accm >> lane) & 1ull) ? (int)len - (int)cB + QA : -1;
            if (GA >= (int)evict) {
                const uint32_t pos = nlen - 1u - (uint32_t)(GA - (int)evict);
                lds_k[pos] = x;
                lds_s[pos] = v_s;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (evict) {
                // an element that leaves with the key of the new maximum: which of the two the reference keeps depends on
                // the layout of its heap
                const int newmax = lds_k[nlen - 1u];
                bool twin = GA >= 0 && GA < (int)evict && x == newmax;
#pragma unroll
                for (int r = 0; r < TR; ++r) twin |= G[r] >= 0 && G[r] < (int)evict && (r == 0 ? h.hd : h.xd[r]) == newmax;
                if (__ballot(twin) != 0ull) amb_min = amb_min < newmax ? amb_min : newmax;
            }
            bool bad = false; // an unwritten position, or a key not above its lower neighbour
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const uint32_t idx = (uint32_t)r * 64u + lane;
                const int kv = idx < nlen ? lds_k[idx] : kHigh;
                const uint32_t sv = idx < nlen ? lds_s[idx] : 0u;
                int below = __builtin_amdgcn_update_dpp(kLow, kv, 0x138, 0xf, 0xf, false); // wave_shr:1
                if (r > 0) {
                    const int carry = __builtin_amdgcn_readlane(r == 1 ? h.hd : h.xd[r - 1], 63);
                    below = lane == 0 ? carry : below;
                }
                bad |= idx < nlen && (kv == kHigh || below > kv); // (equal neighbours are in order)
                if (r == 0) { h.hd = kv; h.hs = sv; } else { h.xd[r] = kv; h.xs[r] = sv; }
            }
            tie |= __ballot(bad) != 0ull;
            h.len = nlen;
            if (nlen == top_k) dk_bits = HeapOps::key(h.d_at(top_k - 1u));
        }
        MSTAMP(2);
        return tie;
    }
    // merge_batch for a kernel's running state: n_skip / n_ext / n_est are added to, bag_dk is the k-th distance kept between batches.
    // (The merge counts from zero in locals and works on a copy of bag_dk, as both kernels' call sites did.)
    static __device__ __forceinline__ bool replay(H& h, uint32_t top_k, unsigned long long mt, int v_lb, int v_d, uint32_t v_s, uint32_t lane,
                                                  bool serial, int* lds_k, uint32_t* lds_s, uint32_t& n_skip, uint32_t& n_ext,
                                                  uint32_t& n_est, int& bag_dk, int& amb_min, unsigned long long* mst = nullptr) {
        uint32_t c_skip = 0, c_ext = 0, c_est = 0;
        int dk = bag_dk;
        const bool tie = merge_batch(h, top_k, mt, v_lb, v_d, v_s, lane, serial, lds_k, lds_s, c_skip, c_ext, c_est, dk, amb_min, mst);
        bag_dk = dk;
        n_skip += c_skip; n_ext += c_ext; n_est += c_est;
        return tie;
    }
};

// One register per lane (top_k <= 64): a SORTED RUN, entry i in lane i — one ballot pair and one DPP shift per
// insertion, the k-th distance is a readlane.  (With several registers the bag above is cheaper.)
template <int TR>
struct SortedRun {
    typedef int VI __attribute__((ext_vector_type(TR)));
    typedef uint32_t VU __attribute__((ext_vector_type(TR)));
    // k-th smallest distance (bits) of a run of `len` entries, +inf while the run is not full
    static __device__ __forceinline__ int kth(int d0, const VI& xd, uint32_t len, uint32_t top_k) {
        if (len < top_k) return 0x7f800000;
        const uint32_t kr = (top_k - 1u) >> 6;
        int v = d0;
#pragma unroll
        for (int r = 1; r < TR; ++r) v = kr == (uint32_t)r ? xd[r] : v; // kernel-uniform
        return __builtin_amdgcn_readlane(v, (int)HeapOps::uni((top_k - 1u) & 63u));
    }
    // insert (dbits, slot) into the run of `len` entries, above the entries of smaller keys (lazy ties: equal keys side by side)
    static __device__ __forceinline__ void insert(int& d0, uint32_t& s0, VI& xd, VU& xs, uint32_t len, int dbits, uint32_t slot,
                                                  uint32_t lane) {
        const int ke = HeapOps::key(dbits);
        uint32_t ipos = 0;
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            if (TR == 1 || (uint32_t)r * 64u < len) { // uniform: registers above the run hold nothing
                const int k = HeapOps::key(r == 0 ? d0 : xd[r]);
                const bool in = (uint32_t)r * 64u + lane < len;
                ipos += (uint32_t)__popcll(__ballot(in && k < ke)); // sorted: the smaller keys are a prefix
            }
        }
        const uint32_t rp = ipos >> 6, lp = ipos & 63u;
        // carries first (register r-1's OLD lane 63 enters register r at lane 0), then every register shifts
        VI cd = xd;
        VU cs = xs;
#pragma unroll
        for (int r = 1; r < TR; ++r) {
            cd[r] = __builtin_amdgcn_readlane(r == 1 ? d0 : xd[r - 1], 63);
            cs[r] = (uint32_t)__builtin_amdgcn_readlane((int)(r == 1 ? s0 : xs[r - 1]), 63);
        }
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            const int od = r == 0 ? d0 : xd[r];
            const uint32_t os = r == 0 ? s0 : xs[r];
            const int sd = __builtin_amdgcn_update_dpp(0, od, 0x138, 0xf, 0xf, false);      // wave_shr:1
            const int ss = __builtin_amdgcn_update_dpp(0, (int)os, 0x138, 0xf, 0xf, false);
            int nd = od;
            uint32_t ns = os;
            if (r > 0 && (uint32_t)r > rp) { // uniform
                nd = lane == 0 ? cd[r] : sd;
                ns = lane == 0 ? cs[r] : (uint32_t)ss;
            } else if ((uint32_t)r == rp) {
                nd = lane == lp ? dbits : (lane > lp ? sd : od);
                ns = lane == lp ? slot : (lane > lp ? (uint32_t)ss : os);
            }
            if (r == 0) { d0 = nd; s0 = ns; } else { xd[r] = nd; xs[r] = ns; }
        }
    }
    // The candidates of a batch (lane j = candidate j: taken lanes mt, lower-bound bits v_lb, distance bits v_d) that can still pass a
    // FULL run whose k-th distance is dk: the threshold only falls inside the batch, so a candidate whose lower bound or whose
    // distance is not below the threshold at the START of the batch is skipped or rejected by the reference as well (an EQUAL
    // distance stays in: the serial loop must record the tie).  Once the run is full most of a batch ends here.
    static __device__ __forceinline__ unsigned long long may_enter(unsigned long long mt, int v_lb, int v_d, int dk, uint32_t lane) {
        const int kk0 = HeapOps::key(dk);
        const bool pass = ((mt >> lane) & 1ull) && __int_as_float(v_lb) < __int_as_float(dk) && (v_d & 0x7f800000) != 0x7f800000 &&
                          HeapOps::key(v_d) <= kk0;
        return __ballot(pass);
    }
    // One evaluated candidate with a finite distance against the run (len entries, k-th distance dk: both kept up to date), by the
    // lazy-tie rule: equal keys are kept side by side, amb_min records the smallest key with which an element left (or was turned away)
    // while its twin stayed.
    static __device__ __forceinline__ void offer(RegHeap<TR>& rh, uint32_t& len, int& dk, uint32_t top_k, int dbits, uint32_t slot,
                                                 uint32_t lane, int& amb_min) {
        const int ke = HeapOps::key(dbits);
        const bool was_full = len == top_k;
        const int kk = HeapOps::key(dk);
        if (was_full) {
            if (ke > kk) return;                                     // pushed and popped again: no change
            if (ke == kk) { amb_min = amb_min < kk ? amb_min : kk; return; } // turned away with the maximum's key: which of the equal maxima leaves depends on the heap layout
        }
        insert(rh.hd, rh.hs, rh.xd, rh.xs, len, dbits, slot, lane);
        len = len < top_k ? len + 1u : len; // a full run drops its (new) entry top_k
        dk = kth(rh.hd, rh.xd, len, top_k);
        if (was_full && HeapOps::key(dk) == kk) amb_min = amb_min < kk ? amb_min : kk; // the old maximum left, its twin stays
    }
};

// ---- the same BinaryHeap with LANE-PARALLEL primitives -------------------------------------------------------------------------
// RegHeap walks a sift level by level through v_readlane / compare-and-select (every hop a VALU -> SGPR -> VALU round trip:
// ~2-3 k cycles per push + pop at top_k = 100).  ParHeap holds the same array (entry g in lane g % 64 of register g / 64, raw
// distance bits) and gets the same result — Rust's std BinaryHeap, operation for operation — from what the operations DO to the array:
//   push(x)  sift_up moves x up its fixed ancestor chain while x > parent: the ancestors with key < x (a bottom prefix of the chain,
//            by the heap property) each move to their path child, x takes the topmost one's place.  One parallel step: every slot on
//            the chain looks at its parent.
//   pop()    the last element e replaces the root, sift_down_to_bottom takes the larger child at every level (`<=`: the right one on
//            equal keys) down to a leaf, sift_up brings e back up while e > parent.  Net effect: along that larger-child path the
//            nodes p_1 .. p_m with key >= e (a top prefix: keys fall along the path) move up one level, e lands in p_m's place, and
//            everything below is put back where it was.  So: every slot computes its larger child in parallel (children fetched with
//            ds_bpermute), a short scalar chain follows the path while key >= e, one parallel step applies it.
// ~4x fewer cycles per real heap operation; used by the tie log's replay (own function, own register allocation).
template <int TR>
struct ParHeap {
    int kd[TR];      // KEY (HeapOps::key of the distance bits: plain signed compares; its own inverse) of entry 64 r + lane
    uint32_t ks[TR]; // slots
    uint32_t len;    // uniform
    static constexpr uint32_t kNone = 0xffffffffu;
    static __device__ __forceinline__ int key(int b) { return HeapOps::key(b); }
    // value of entry idx (per lane; idx < 64 TR) of an array held in TR registers; S0..S1: the source registers idx can lie in
    template <typename T>
    __device__ __forceinline__ T fetch(const T (&a)[TR], uint32_t idx, int s0, int s1) const {
        T v = a[0];
        const int addr = (int)((idx & 63u) << 2);
#pragma unroll
        for (int s = 0; s < TR; ++s)
            if (s >= s0 && s <= s1) {
                const T t = (T)__builtin_amdgcn_ds_bpermute(addr, (int)a[s]);
                v = (idx >> 6) == (uint32_t)s ? t : v;
            }
        return v;
    }
    template <typename T>
    __device__ __forceinline__ T at(const T (&a)[TR], uint32_t i) const { // uniform index
        const uint32_t r = HeapOps::uni(i >> 6);
        T v = a[0];
#pragma unroll
        for (int k = 1; k < TR; ++k) v = r == (uint32_t)k ? a[k] : v;
        return (T)__builtin_amdgcn_readlane((int)v, (int)HeapOps::uni(i & 63u));
    }
    // is g a proper ancestor of slot n in the implicit tree?
    static __device__ __forceinline__ bool is_anc(uint32_t g, uint32_t n) {
        const int t = (int)__builtin_clz(g + 1u) - (int)__builtin_clz(n + 1u);
        return g < n && t > 0 && ((n + 1u) >> t) == g + 1u;
    }
    __device__ __forceinline__ void push(int kx, uint32_t xs, uint32_t lane) { // kx: the KEY of the new distance
        const uint32_t n = HeapOps::uni(len);
        int nk[TR];
        uint32_t ns[TR];
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            const uint32_t g = (uint32_t)r * 64u + lane;
            const bool on_path = g == n || is_anc(g, n);
            const uint32_t par = g ? (g - 1u) >> 1 : 0u; // (lies in register <= r)
            const int pk = fetch(kd, par, (64 * r) / 128 > 0 ? (64 * r - 1) / 128 : 0, (64 * r + 62) / 128);
            const uint32_t ps = fetch(ks, par, (64 * r) / 128 > 0 ? (64 * r - 1) / 128 : 0, (64 * r + 62) / 128);
            const bool parent_moved = on_path && g > 0u && pk < kx;                 // the parent is an ancestor that x passes
            const bool takes_x = on_path && !parent_moved && (g == n || kd[r] < kx); // the top of the moved chain (or the slot itself)
            nk[r] = parent_moved ? pk : (takes_x ? kx : kd[r]);
            ns[r] = parent_moved ? ps : (takes_x ? xs : ks[r]);
        }
#pragma unroll
        for (int r = 0; r < TR; ++r) { kd[r] = nk[r]; ks[r] = ns[r]; }
        len = n + 1u;
    }
    __device__ __forceinline__ void pop(uint32_t lane) {
        const uint32_t n = HeapOps::uni(len) - 1u; // the last element's index = the new length
        len = n;
        if (n == 0u) return;
        const int ke = at(kd, n);
        const uint32_t es = at(ks, n);
        // every slot's larger child — if that child stays above e (`e <= parent` ends the closing sift_up), else none: the scalar
        // chain below then needs ONE readlane per level
        uint32_t big[TR];
        int bk[TR];
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            big[r] = kNone; bk[r] = 0;
            if (128 * r + 1 < 64 * TR) { // (slots of this register can have children inside the array)
                const uint32_t g = (uint32_t)r * 64u + lane, cl = 2u * g + 1u, cr = 2u * g + 2u;
                const int s0 = 2 * r, s1 = 2 * r + 2 < TR ? 2 * r + 2 : TR - 1;
                const int kl = fetch(kd, cl & (64u * TR - 1u), s0, s1), kr = fetch(kd, cr & (64u * TR - 1u), s0, s1);
                const bool hasl = cl < n, right = cr < n && kl <= kr; // `hole.get(child) <= hole.get(child + 1)`: the right one
                bk[r] = right ? kr : kl;
                big[r] = (hasl && bk[r] >= ke) ? (right ? cr : cl) : kNone;
            }
        }
        unsigned long long take[TR];
#pragma unroll
        for (int r = 0; r < TR; ++r) take[r] = 0ull;
        uint32_t p = 0;
        for (;;) { // the larger-child path from the root while its nodes stay above e
            const uint32_t c = at(big, p);
            if (c == kNone) break;
#pragma unroll
            for (int r = 0; r < TR; ++r) if ((p >> 6) == (uint32_t)r) take[r] |= 1ull << (p & 63u);
            p = c;
        }
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            const bool tk = (take[r] >> lane) & 1ull, isp = (uint32_t)r * 64u + lane == p;
            uint32_t bs = 0u;
            if (128 * r + 1 < 64 * TR) bs = fetch(ks, big[r] & (64u * TR - 1u), 2 * r, 2 * r + 2 < TR ? 2 * r + 2 : TR - 1); // (the slot moves with the key)
            kd[r] = tk ? bk[r] : (isp ? ke : kd[r]);
            ks[r] = tk ? bs : (isp ? es : ks[r]);
        }
    }
    // some node of the root-to-slot-K path equals its off-path child (heap full: len == K)
    __device__ __forceinline__ bool path_tie(uint32_t K, uint32_t lane) const {
        bool t = false;
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            if (128 * r + 1 < 64 * TR) {
                const uint32_t g = (uint32_t)r * 64u + lane, cl = 2u * g + 1u, cr = 2u * g + 2u;
                const int s0 = 2 * r, s1 = 2 * r + 2 < TR ? 2 * r + 2 : TR - 1;
                const int kl = fetch(kd, cl & (64u * TR - 1u), s0, s1), kr = fetch(kd, cr & (64u * TR - 1u), s0, s1);
                const bool anc = is_anc(g, K);
                const bool left_on_path = cl == K || is_anc(cl, K); // (else the right child is the path child)
                const uint32_t off = left_on_path ? cr : cl;
                t |= anc && off < K && kd[r] == (left_on_path ? kr : kl);
            }
        }
        return __ballot(t) != 0ull;
    }
};

// The reference's prune / push / pop loop (src/ivf.rs:2054-2126) over a query's logged candidates, with the BinaryHeap emulation: what a
// tied query runs instead of scanning its lists again (k_scan, `tie_log`).  One wave; the heap lives in registers (ParHeap) or, for
// top_k = 64 TR exactly, in LDS.  Returns the heap (everything by value: an argument passed by reference would pin the caller's top-k
// registers to memory for the whole kernel); `len` of the result is the heap's length in both cases.
template <int TR>
__device__ __attribute__((noinline)) RegHeap<TR> tie_log_replay(float* heap_d, uint32_t* heap_s, const uint32_t* tlog, uint32_t log_n,
                                                                uint32_t top_k, bool reg_heap, uint32_t lane, unsigned int* stats) {
    uint32_t n_real = 0;
    ParHeap<TR> ph;
#pragma unroll
    for (int r = 0; r < TR; ++r) { ph.kd[r] = 0; ph.ks[r] = 0u; }
    ph.len = 0u;
    LdsHeap lh{heap_d, heap_s, 0};
    // PUSH-THEN-POP IS THE IDENTITY.  Most evaluated candidates of a full heap lie above its root: the reference pushes them and pops
    // them again (src/ivf.rs:2116-2126).  With Rust's BinaryHeap (sift_up; pop = swap the last element into the root,
    // sift_down_to_bottom, sift_up) that pair leaves the array exactly as it was: the new key x > root climbs the path from slot k
    // to the root, shifting the path's elements down by one; pop removes the element now in slot k, puts it in the root, and the hole
    // walks back DOWN THE SAME PATH — at every path node the path child holds the node's own old value, which is >= the off-path
    // child — restoring every element, and the displaced one ends where it came from.  The only way off the path is a comparison
    // of EQUAL keys (`<=` picks the right child; the closing sift_up stops at `<=`), i.e. a path node whose old value equals its
    // off-path child's.  `ptie` = some node of the (fixed: top_k is) root-to-slot-k path equals its off-path child (conservative);
    // while it is false a candidate with key > root key is skipped in O(1); it is re-evaluated (lazily) after a real insertion.
    bool ptie = false, ptie_valid = true;
    auto lds_path_tie = [&]() -> bool {
        bool t = false;
        for (uint32_t c = top_k; c > 0;) {
            const uint32_t par = (c - 1u) >> 1, sib = (c & 1u) ? c + 1u : c - 1u;
            if (sib < top_k) t |= __float_as_int(heap_d[par]) == __float_as_int(heap_d[sib]);
            c = par;
        }
        return t;
    };
    for (uint32_t c0 = 0; c0 < log_n; c0 += 64u) {
        const uint32_t cn = log_n - c0 < 64u ? log_n - c0 : 64u;
        int e_lb = 0, e_d = 0;
        uint32_t e_s = 0;
        if (lane < cn) { const uint32_t* e = tlog + (size_t)(c0 + lane) * 3u; e_lb = (int)e[0]; e_d = (int)e[1]; e_s = e[2]; }
        for (uint32_t j = 0; j < cn; ++j) {
            const float lb = __int_as_float(__builtin_amdgcn_readlane(e_lb, (int)j));
            const int dbits = __builtin_amdgcn_readlane(e_d, (int)j);
            const uint32_t hlen = reg_heap ? HeapOps::uni(ph.len) : lh.len;
            const bool full = hlen == top_k;
            const int rootb = !full ? 0x7f800000 : (reg_heap ? HeapOps::key(__builtin_amdgcn_readlane(ph.kd[0], 0)) : __float_as_int(heap_d[0]));
            if (lb >= __int_as_float(rootb)) continue;                  // `lower_bound >= distk`: skipped
            if (!finite_f(__int_as_float(dbits))) continue;             // non-finite distance: dropped
            if (full && HeapOps::key(dbits) > HeapOps::key(rootb)) {    // pushed and popped again: the heap is unchanged ...
                if (!ptie_valid) { ptie = reg_heap ? ph.path_tie(top_k, lane) : lds_path_tie(); ptie_valid = true; }
                if (!ptie) continue;                                    // ... unless equal keys sit on the path
            }
            const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)e_s, (int)j);
            ++n_real;
            if (reg_heap) {
                ph.push(HeapOps::key(dbits), slot, lane);
                if (ph.len > top_k) ph.pop(lane);
            } else {
                if (lane == 0) {
                    lh.push(__int_as_float(dbits), slot);
                    if (lh.len > top_k) lh.pop();
                }
                lh.len = (uint32_t)__builtin_amdgcn_readfirstlane((int)lh.len);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            ptie_valid = false;
        }
    }
    if (stats && lane == 0) { atomicAdd(stats, 1u); atomicAdd(stats + 1, log_n); atomicAdd(stats + 2, n_real); }
    RegHeap<TR> rh;
    rh.hd = HeapOps::key(ph.kd[0]); rh.hs = ph.ks[0]; rh.xd = 0; rh.xs = 0u; // (keys back to distance bits)
#pragma unroll
    for (int r = 1; r < TR; ++r) { rh.xd[r] = HeapOps::key(ph.kd[r]); rh.xs[r] = ph.ks[r]; }
    rh.len = reg_heap ? ph.len : lh.len;
    return rh;
}

// ---- what k_scan's replay wave and k_scanw both do to the top-k ------------------------------------------------------------------
// A batch = the candidates a refine round took, lane j = candidate j in stream order: `mt` the taken lanes, v_lb / v_d the bits of the
// lower bound and of the refined distance, v_s the slot.  c_skip / c_ext / c_est count the reference's `lower_bound >= distk` skips, its
// evaluations and the finite ones among them.  Everything the loops decide on is wave-uniform (readlane / readfirstlane say so to the
// compiler): about a dozen scalar instructions per candidate that does not change the top-k.  A lower bound is never NaN here (the
// kernels turn a NaN bound into -inf), so `!(lb < distk)` is the reference's `lower_bound >= distk`.

// Register r of the fast run, as a key or as distance bits: SortedRun holds the bits, RankRun (`rank`) their keys; key() is its own inverse.
template <int TR>
__device__ __forceinline__ int run_key(const RegHeap<TR>& h, int r, bool rank) {
    const int v = r == 0 ? h.hd : h.xd[r];
    return rank ? v : HeapOps::key(v);
}
template <int TR>
__device__ __forceinline__ int run_distance_bits(const RegHeap<TR>& h, int r, bool rank) {
    const int v = r == 0 ? h.hd : h.xd[r];
    return rank ? HeapOps::key(v) : v;
}

// The reference's prune / push / pop loop over one batch, one taken candidate after the other, on the SORTED RUN (SortedRun::may_enter
// and ::offer hold the lazy-tie rule) ...
template <int TR>
__device__ __forceinline__ void replay_sorted(RegHeap<TR>& rh, uint32_t top_k, unsigned long long mt, int v_lb, int v_d, uint32_t v_s,
                                              uint32_t lane, bool count_skips, uint32_t& c_skip, uint32_t& c_ext, uint32_t& c_est,
                                              int& amb_min) {
    uint32_t len_s = HeapOps::uni(rh.len);
    int dk = SortedRun<TR>::kth(rh.hd, rh.xd, len_s, top_k);
    unsigned long long todo = mt;
    if (!count_skips && len_s == top_k) todo = SortedRun<TR>::may_enter(mt, v_lb, v_d, dk, lane); // (diagnostics count every decision)
    while (todo) {
        const uint32_t j = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const float lb = __int_as_float(__builtin_amdgcn_readlane(v_lb, (int)j));
        if (!(lb < __int_as_float(dk))) { ++c_skip; continue; }    // `lower_bound >= distk`: skipped
        ++c_ext;
        const int dbits = __builtin_amdgcn_readlane(v_d, (int)j);
        if ((dbits & 0x7f800000) == 0x7f800000) continue;           // non-finite distance: dropped
        ++c_est;
        SortedRun<TR>::offer(rh, len_s, dk, top_k, dbits, (uint32_t)__builtin_amdgcn_readlane((int)v_s, (int)j), lane, amb_min);
    }
    rh.len = len_s;
}
// ... and through the exact BinaryHeap in registers (RegHeap push / pop): what a query runs after a tie, or with `exact_heap`.
// (k_scanw has the two loops as ONE, inline, on its runtime `fast`, around the same SortedRun members: as calls to these two — or to
// one function of this shape — its top_k >= 64 instantiations, which sit at the scalar-register limit, spilled; see there.)
template <int TR>
__device__ __forceinline__ void replay_heap(RegHeap<TR>& rh, uint32_t top_k, unsigned long long mt, int v_lb, int v_d, uint32_t v_s,
                                            uint32_t& c_skip, uint32_t& c_ext, uint32_t& c_est) {
    unsigned long long todo = mt;
    while (todo) {
        const uint32_t j = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const float lb = __int_as_float(__builtin_amdgcn_readlane(v_lb, (int)j));
        const float distk = rh.len < top_k ? INFINITY : __int_as_float(rh.d_at(0));
        if (!(lb < distk)) { ++c_skip; continue; }                  // `lower_bound >= distk`: skipped
        ++c_ext;
        const int dbits = __builtin_amdgcn_readlane(v_d, (int)j);
        if ((dbits & 0x7f800000) == 0x7f800000) continue;           // non-finite distance: dropped
        ++c_est;
        rh.push(dbits, (uint32_t)__builtin_amdgcn_readlane((int)v_s, (int)j));
        if (rh.len > top_k) rh.pop();
    }
}

// The final look of the lazy-tie rule at the fast run (the rule and its proof: scanw.hpp, at `amb_min`): true if the query must be
// re-run with the BinaryHeap emulation — two equal neighbours in the run, or a full run whose maximum is amb_min.  (The run by value,
// here and in spill_heap_sorted: by reference k_scanw's top_k >= 64 instantiations came out up to 32 instructions away from the inline
// text and 1.2 % slower at top_k = 100, by value within 2 and as fast: profiles/scan_topk_fold.)
template <int TR>
__device__ __forceinline__ bool lazy_tie_final(RegHeap<TR> rh, bool rank, uint32_t top_k, int amb_min, uint32_t lane) {
    const uint32_t lenf = HeapOps::uni(rh.len);
    bool eq = false;
    int maxkey = (int)0x80000000;
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        const uint32_t i = (uint32_t)r * 64u + lane;
        const int kv = run_key(rh, r, rank);
        int below = __builtin_amdgcn_update_dpp((int)0x80000000, kv, 0x138, 0xf, 0xf, false); // wave_shr:1
        if (r > 0) {
            const int carry = __builtin_amdgcn_readlane(run_key(rh, r - 1, rank), 63);
            below = lane == 0 ? carry : below;
        }
        eq |= i >= 1u && i < lenf && kv == below;
        if (lenf && (lenf - 1u) >> 6 == (uint32_t)r) maxkey = __builtin_amdgcn_readlane(kv, (int)((lenf - 1u) & 63u));
    }
    return __ballot(eq) != 0ull || (lenf == top_k && maxkey == amb_min);
}

// The exact heap's way out: the `len` entries of the register heap go to heap_d / heap_s (`spill`; k_scan's heap of top_k = 64 TR is
// there already), one lane runs into_sorted_vec on them.  `sync` makes the wave's stores visible to that lane (each kernel passes
// its own).
template <int TR, typename Sync>
__device__ __forceinline__ void spill_heap_sorted(RegHeap<TR> rh, bool spill, uint32_t len, float* heap_d, uint32_t* heap_s,
                                                  uint32_t lane, Sync sync) {
    if (spill) {
#pragma unroll
        for (int r = 0; r < TR; ++r)
            if ((uint32_t)r * 64u + lane < len) {
                heap_d[r * 64 + lane] = __int_as_float(r == 0 ? rh.hd : rh.xd[r]);
                heap_s[r * 64 + lane] = r == 0 ? rh.hs : rh.xs[r];
            }
        sync();
    }
    if (lane == 0) {
        LdsHeap lh{heap_d, heap_s, len};
        lh.into_sorted();
    }
}

} // namespace rbq
