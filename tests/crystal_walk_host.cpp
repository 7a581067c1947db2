// Host driver of the image walk of csrc/crystal_dev.h (crystal_walk, crystal_walk_chunks, crystal_walk_index, crystal_walk_narrow)
// for tests/test_crystal_walk_cpu.py: no HIP, no device.  Every (j, m) the walks hand out is compared with plain 64-bit e / M, e % M,
// on both sides of the switch between 32-bit and 64-bit index arithmetic.  Prints "ok <checks>" and returns 0, or the first
// failures and returns 1.
#include <stdio.h>

#include <vector>

#include "../arreau_amd/csrc/crystal_dev.h"

typedef unsigned long long u64;

static long checks = 0, failures = 0;

static void expect(bool ok, const char* what, u64 span, unsigned M, unsigned stride, u64 e) {
    ++checks;
    if (ok) return;
    if (++failures <= 10) printf("FAILED %s: span %llu M %u stride %u e %llu\n", what, span, M, stride, e);
}

// the strided walk from `start`: e = start, start + stride, ... < span, in that order
static void strided(u64 span, unsigned M, u64 start, unsigned stride, std::vector<unsigned char>* seen) {
    u64 e = start;
    crystal_walk(span, M, start, stride, [&](unsigned j, unsigned m) {
        expect(e < span && j == e / M && m == e % M, "crystal_walk", span, M, stride, e);
        if (seen && e < span) ++(*seen)[e];
        e += stride;
    });
    expect(e >= span && (e < span + stride || e == start), "crystal_walk's end", span, M, stride, e);
}

// the chunked walk of one lane: every round is handed out, valid or not, so that all lanes make the same number of calls
static void chunked(u64 span, unsigned M, unsigned lane, unsigned width, std::vector<unsigned char>& seen) {
    u64 base = 0;
    crystal_walk_chunks(span, M, lane, width, [&](bool valid, unsigned j, unsigned m) {
        const u64 e = base + lane;
        expect(base < span && valid == (e < span), "crystal_walk_chunks' valid", span, M, width, e);
        if (valid) {
            expect(j == e / M && m == e % M, "crystal_walk_chunks", span, M, width, e);
            ++seen[e];
        }
        base += width;
    });
    expect(base == (span + width - 1) / width * width, "crystal_walk_chunks' rounds", span, M, width, base);
}

int main() {
    const unsigned strides[2] = {64, 256}, images[3] = {27, 125, 4913};  // M of 1, 2 and 8 shells
    for (unsigned stride : strides)
        for (unsigned M : images) {
            // ---- small spans, walked whole by every lane: each e is met exactly once
            const u64 small[] = {0, 1, stride - 1, stride, stride + 1, 3ull * M + 5, 7ull * M, 40ull * M + stride - 1};
            for (u64 span : small) {
                expect(crystal_walk_narrow(span, stride), "narrow", span, M, stride, 0);
                std::vector<unsigned char> a(span, 0), b(span, 0);
                for (unsigned lane = 0; lane < stride; ++lane) {
                    strided(span, M, lane, stride, &a);
                    chunked(span, M, lane, stride, b);
                }
                for (u64 e = 0; e < span; ++e) expect(a[e] == 1 && b[e] == 1, "coverage", span, M, stride, e);
            }
            // ---- the last narrow span, the first wide one, and a span above 2^32: the last thousand entries
            const u64 last_narrow = 0xffffffffull - stride;
            const u64 large[] = {last_narrow, last_narrow + 1, 900000ull * 4913ull};
            expect(crystal_walk_narrow(large[0], stride) && !crystal_walk_narrow(large[1], stride) && !crystal_walk_narrow(large[2], stride),
                   "the narrow/wide switch", last_narrow, M, stride, 0);
            for (u64 span : large)
                for (unsigned lane = 0; lane < stride; ++lane) strided(span, M, span - 1000 - lane, stride, nullptr);
            // ---- the index arithmetic of either width over its whole range, sampled
            for (u64 e = 0; e <= 0xffffffffull; e += 16777619ull) {
                unsigned j, m;
                crystal_walk_index((unsigned)e, M, j, m);
                expect(j == e / M && m == e % M, "crystal_walk_index, 32 bits", 0, M, stride, e);
            }
            for (u64 e = 0xfff00000ull; e < (0xffffffffull + 1) * M; e += 16777619ull * (M / 2)) {  // j up to 2^32 - 1
                unsigned j, m;
                crystal_walk_index(e, M, j, m);
                expect(j == e / M && m == e % M, "crystal_walk_index, 64 bits", 0, M, stride, e);
            }
        }
    if (failures) {
        printf("%ld of %ld checks failed\n", failures, checks);
        return 1;
    }
    printf("ok %ld\n", checks);
    return 0;
}
