// planarslam_amd/csrc/glibc_rand.h — glibc's rand() after srand(seed) (stdlib/random_r.c, TYPE_3: the additive feedback generator x^31 + x^3 + 1 over a ring of
// 31 words, seeded by the Lehmer sequence 16807 * x mod (2^31 - 1), first 310 outputs discarded), on a ring the caller owns: 31 words that ONE thread walks (LDS on
// the device, where a thread-private array under a running index would go to scratch).  line3d.hip keeps the same stream on the lanes of a wave; this is the
// single-thread form for hornransac.hip and the CPU build of horn_arith.h.  Word i of the sequence lives in ring[i % 31]: r_i = r_(i-31) + r_(i-3), output r_i >> 1.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GLIBC_RAND_HD __host__ __device__ __forceinline__
#else
#define GLIBC_RAND_HD static inline
#endif

namespace planar {

struct GlibcRand {
    uint32_t* ring;   // [31]
    int i;            // index of the next word
};

GLIBC_RAND_HD GlibcRand glibc_srand(uint32_t* ring, uint32_t seed) {
    if (seed == 0) seed = 1;
    int32_t w = (int32_t)seed;
    ring[0] = (uint32_t)w;
    for (int i = 1; i < 31; i++) {
        const int32_t hi = w / 127773, lo = w % 127773;
        w = 16807 * lo - 2836 * hi;
        if (w < 0) w += 2147483647;
        ring[i] = (uint32_t)w;
    }
    for (int i = 34; i < 344; i++) ring[i % 31] += ring[(i - 3) % 31];
    return GlibcRand{ring, 344};
}

GLIBC_RAND_HD int glibc_rand(GlibcRand& g) {   // in [0, RAND_MAX = 2^31 - 1]
    const int at = g.i % 31;
    g.ring[at] += g.ring[(g.i - 3) % 31];
    g.i++;
    if (g.i >= 31 * 1024) g.i -= 31 * 1000;   // the same place in the ring, kept small
    return (int)(g.ring[at] >> 1);
}

}  // namespace planar
