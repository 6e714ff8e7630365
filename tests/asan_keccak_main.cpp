// Stand-alone program for the sanitizer run of the Keccak hasher's host code (make asan-keccak-test): keccak256 at every length around
// the block edges, the digest encoding both ways, hash_or_noop at every width up to three blocks, two_to_one, the challenger's
// permutation, and the word filter on streams that are short, exact and full of words at or above p.  Exit status 0 = consistent.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../starky_bls12_381_amd/csrc/keccak.h"

using namespace starkhip;

int main() {
    int bad = 0;
    // keccak256("") and ("abc")
    static const uint8_t EMPTY[4] = {0xc5, 0xd2, 0x46, 0x01}, ABC[4] = {0x4e, 0x03, 0x65, 0x7a};
    uint8_t out[32];
    keccak256_host(nullptr, 0, out);
    bad += memcmp(out, EMPTY, 4) != 0;
    keccak256_host((const uint8_t*)"abc", 3, out);
    bad += memcmp(out, ABC, 4) != 0;
    // every length up to two blocks and a bit, from a buffer of exactly that length (an over-read is the sanitizer's to find)
    for (size_t len = 0; len <= 300; len++) {
        std::vector<uint8_t> m(len);
        for (size_t i = 0; i < len; i++) m[i] = (uint8_t)(i * 7 + len);
        keccak256_host(m.data(), len, out);
    }
    // hash_or_noop over exactly-sized inputs against keccak256 of their bytes, and the digest encoding's round trip
    for (size_t w = 1; w <= 52; w++) {
        std::vector<gl_t> in(w);
        for (size_t i = 0; i < w; i++) in[i] = (0x9E3779B97F4A7C15ULL * (i + w)) % GL_P;
        gl_t d[4], want[4];
        keccak_hash_or_noop(in.data(), w, 1, d);
        if (w > 3) {
            keccak256_host((const uint8_t*)in.data(), 8 * w, out);  // little-endian host
            uint64_t o[4];
            memcpy(o, out, 32);
            keccak_digest_words(o[0], o[1], o[2], o[3], want);
            bad += memcmp(d, want, sizeof d) != 0;
        }
        bad += !keccak_digest_in_range(d);
        uint64_t lanes[4];
        keccak_digest_lanes(d, lanes);
        keccak_digest_words(lanes[0], lanes[1], lanes[2], lanes[3], want);
        bad += memcmp(d, want, sizeof d) != 0;
        gl_t t[4];
        keccak_two_to_one(d, d, t);
        bad += !keccak_digest_in_range(t);
    }
    // the permutation and the filter
    gl_t s[12];
    for (int i = 0; i < 12; i++) s[i] = GL_P - 1;
    for (int k = 0; k < 100; k++) keccak_permute_host(s);
    for (int i = 0; i < 12; i++) bad += s[i] >= GL_P;
    for (size_t n = 0; n <= 40; n++) {
        std::vector<uint64_t> words(n);
        for (size_t i = 0; i < n; i++) words[i] = i % 3 == 0 ? GL_P + i : i;
        gl_t st[12] = {0};
        int used = 0;
        const int have = keccak_take_words(words.data(), (int)n, st, 0, &used);
        bad += have > 12 || used > (int)n || (have == 12) != (n >= 18);
    }
    printf("keccak host code: %d inconsistencies\n", bad);
    return bad != 0;
}
