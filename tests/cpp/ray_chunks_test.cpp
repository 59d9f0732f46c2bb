// for_ray_chunks (optrace_amd/csrc/ot_host.hpp), compiled without HIP: the pieces handed to the callback are contiguous,
// do not overlap, cover [first, first + count), none is longer than the limit, and there is none for count == 0.
#define OT_HOST_CHUNKS_ONLY
#include "ot_host.hpp"

#include <cstdio>

static int check(int64_t first, int64_t count) {
    int64_t next = first, pieces = 0;
    int bad = 0;
    for_ray_chunks(first, count, [&](int64_t base, uint32_t n) {
        if (base != next || n == 0 || (int64_t)n > OT_RAY_CHUNK || base + (int64_t)n > first + count) bad++;
        next = base + (int64_t)n;
        pieces++;
    });
    if (next != first + count) bad++;
    if (pieces != (count + OT_RAY_CHUNK - 1) / OT_RAY_CHUNK) bad++;  // (so none at all for count == 0)
    if (bad) std::printf("first %lld count %lld: %d violations, %lld pieces, end %lld\n", (long long)first, (long long)count, bad,
                         (long long)pieces, (long long)next);
    return bad;
}

int main() {
    static_assert(OT_RAY_CHUNK == (int64_t)1 << 28, "lanes address their ray with 32-bit byte offsets: 2^28 rays per launch");
    const int64_t L = (int64_t)1 << 28;
    const int64_t counts[] = {0, 1, L - 1, L, L + 1, 3 * L + 5}, firsts[] = {0, 63};
    int bad = 0, n = 0;
    for (int64_t count : counts)
        for (int64_t first : firsts) {
            bad += check(first, count);
            n++;
        }
    if (bad) return 1;
    std::printf("ok %d cases\n", n);
    return 0;
}
