/* rbq_rng.h — the project's seeded RNG: splitmix64-seeded xoshiro256**.  Shared by the CPU builder (rbq_build.cpp) and the
 * device k-means driver (k_kmeans.hip), whose reseed draws and shuffles must be the same stream. */
#ifndef RBQ_RNG_H
#define RBQ_RNG_H
#include <cmath>
#include <cstdint>

namespace rbq_host {

struct Rng {
    uint64_t s[4];
    explicit Rng(uint64_t seed) {
        uint64_t z = seed;
        for (int i = 0; i < 4; ++i) {
            z += 0x9e3779b97f4a7c15ULL;
            uint64_t x = z;
            x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
            x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
            s[i] = x ^ (x >> 31);
        }
    }
    static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    uint64_t next() {
        uint64_t r = rotl(s[1] * 5, 7) * 9, t = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t; s[3] = rotl(s[3], 45);
        return r;
    }
    double uniform() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    bool have = false; double spare = 0;
    double normal() {
        if (have) { have = false; return spare; }
        double u, v, r;
        do { u = 2 * uniform() - 1; v = 2 * uniform() - 1; r = u * u + v * v; } while (r >= 1 || r == 0);
        double f = std::sqrt(-2 * std::log(r) / r);
        spare = v * f; have = true;
        return u * f;
    }
};

} // namespace rbq_host

#endif
